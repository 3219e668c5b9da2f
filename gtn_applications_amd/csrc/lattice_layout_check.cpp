// Prints the alpha / beta tail layout of lattice_layout.h for a grid of descriptors (host only; `make layout_check`).
//   case B T shared max_states total_states
//   A|B <field> <bytes per element> <first byte> <one past the last byte>      (from the buffer's start)
//   end <floats>   total <floats>
// tests/test_lattice_layout_host.py reads it: order, disjointness, alignment, the total against its restatement.
#include <cstdio>
#include <initializer_list>

#include "lattice_layout.h"

using wfl::AbTail;

static void field(char buf, const char* name, int unit, const AbTail& l, int64_t first, int64_t count) {
  const long long lo = 4 * (long long)l.tail + unit * (long long)first;
  std::printf("%c %s %d %lld %lld\n", buf, name, unit, lo, lo + unit * (long long)count);
}

static void print_case(const wfl_lattice_desc& d, int T) {
  const AbTail l = wfl::ab_tail(d, T);
  const int B = d.B;
  std::printf("case %d %d %d %d %lld\n", B, T, d.shared, d.max_states, (long long)d.total_states);
  for (const char buf : {'A', 'B'}) {
    field(buf, "offs", 8, l, l.offs(0), l.offs(B) - l.offs(0));
    field(buf, "z", 8, l, l.z(0), l.z(B) - l.z(0));
    if (buf == 'A') {
      field(buf, "fmt", 4, l, l.fmt(0), l.fmt(B) - l.fmt(0));
      field(buf, "wref", 4, l, l.wref(0), l.wref(B) - l.wref(0));
    } else {
      field(buf, "verdict", 8, l, l.verdict(0), l.verdict(B) - l.verdict(0));
    }
    field(buf, "dump", 8, l, l.dump(), wfl::kDumpDoubles);
    field(buf, "prog", 8, l, l.prog(0), l.prog(B) - l.prog(0));
    field(buf, "bad", 4, l, l.bad(0), l.bad(B) - l.bad(0));
    if (buf == 'B') continue;
    field(buf, "nx", 4, l, l.nx(), 8);  // (the dimensions of OccHeader's arrays)
    field(buf, "next", 4, l, l.next(), 8);
    field(buf, "list", 4, l, l.list(), 8 * (int64_t)B);
    field(buf, "busy", 4, l, l.busy(), 8 * 256);
    field(buf, "meta", 4, l, l.meta(), 2);
    field(buf, "next_base", 4, l, l.next_base(), 8);
    field(buf, "based", 4, l, l.based(), (int64_t)B * l.live_tiles());
  }
  std::printf("end %lld\ntotal %lld\n", (long long)l.end_floats(), (long long)l.total_floats());
}

int main() {
  for (const int B : {1, 2, 7, 8, 255, 256})
    for (const int T : {0, 1, 15, 16, 31, 32, 33, 320, 1000})
      for (const int shared : {0, 1})
        for (const int max_states : {1, 64, 263}) {
          wfl_lattice_desc d = {};
          d.B = B, d.shared = shared, d.max_states = max_states;
          d.total_states = shared ? max_states : (int64_t)B * max_states;
          print_case(d, T);
        }
  return 0;
}
