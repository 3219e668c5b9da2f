// wfl_lexicon_lookahead_check and wfl_lexicon_marked_lookahead_check (include/wfl.h) on good and bad
// inputs in exact-size heap arrays: a stand-alone host program for AddressSanitizer and UBSan -- an index the check
// reads past the end of an array, or before it has checked the range it comes from, is a report.  No device is used:
// the checks are host code.  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude \
//     -Igtn_applications_amd/csrc scripts/lexicon_lookahead_check_asan.cpp gtn_applications_amd/csrc/beam_kernels.hip \
//     gtn_applications_amd/csrc/graph.cpp -o scripts/_build/lexicon_lookahead_check_asan && scripts/_build/lexicon_lookahead_check_asan
// It prints one line per input and exits 0 if the good ones pass with the expected ranges and every bad one is refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "wfl.h"

namespace {

struct Pack {
  std::vector<int32_t> arc_ptr, arc_label, arc_next, node_word;  // node_word empty: an end-marked lexicon
  std::vector<double> look;
  int V;
};

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // a heap block of exactly the array's size
  std::unique_ptr<T[]> a(new T[v.size()]);
  if (!v.empty()) std::memcpy(a.get(), v.data(), v.size() * sizeof(T));
  return a;
}

int run(const Pack& p, wfl_lexicon_lookahead* out, bool null_look = false) {
  const auto ptr = exact(p.arc_ptr), label = exact(p.arc_label), next = exact(p.arc_next), word = exact(p.node_word);
  const auto look = exact(p.look);
  const std::vector<int32_t> none(1, -1);
  const auto start = exact(none);  // (the look-ahead checks do not read start_node: one element, which a read beyond reports)
  const double nan = std::numeric_limits<double>::quiet_NaN();
  *out = wfl_lexicon_lookahead{null_look ? nullptr : look.get(), nan, nan, nan, nan, nan, nan};
  wfl_lexicon_marked m;
  m.trie.num_nodes = (int32_t)p.arc_ptr.size() - 1, m.trie.num_arcs = (int32_t)p.arc_label.size();
  m.trie.num_words = p.V, m.trie.reserved = 0;
  m.trie.arc_ptr = ptr.get(), m.trie.arc_label = label.get(), m.trie.arc_next = next.get();
  m.node_word = word.get(), m.start_node = start.get();
  return p.node_word.empty() ? wfl_lexicon_lookahead_check(&m.trie, out) : wfl_lexicon_marked_lookahead_check(&m, out);
}

// tests/test_lexicon_host.py's five words (1 5), (1 2 5), (2 5), (3), (2 2 4) with the scores -1, -2, -3, -4, -0.5
Pack end_marked() {
  return {{0, 3, 5, 7, 8, 9}, {1, 2, 3, 2, 5, 2, 5, 5, 4}, {1, 2, -4, 3, -1, 4, -3, -2, -5}, {}, {0.0, -1.0, -0.5, -2.0, -0.5}, 5};
}
// tests/test_lexicon_marked_host.py's "_a", "_a n", "_a n t", "_the", "_the re", "_an" with the same scores
Pack start_marked() {
  return {{0, 3, 4, 5, 5, 6, 6, 6}, {0, 1, 6, 2, 4, 3}, {1, 2, 3, 4, 5, 6}, {-1, 0, 3, 1, 1, 4, 2},
          {0.0, -1.0, -0.5, -2.0, -2.0, -0.5, -3.0}, 5};
}

}  // namespace

int main() {
  int failures = 0;
  wfl_lexicon_lookahead k;
  auto expect = [&](const char* what, int rc, bool ok) {
    const bool pass = (rc == WFL_OK) == ok;
    std::printf("%-52s %s%s%s\n", what, rc == WFL_OK ? "accepted" : "refused: ", rc == WFL_OK ? "" : wfl_last_error(),
                pass ? "" : "   <-- UNEXPECTED");
    failures += pass ? 0 : 1;
  };
  auto ranges = [&](const char* what, double a0, double a1, double e0, double e1, double s0, double s1) {
    const bool pass = k.arc_min == a0 && k.arc_max == a1 && k.end_min == e0 && k.end_max == e1 && k.start_min == s0 && k.start_max == s1;
    std::printf("%-52s arcs [%g, %g] ends [%g, %g] starts [%g, %g]%s\n", what, k.arc_min, k.arc_max, k.end_min, k.end_max,
                k.start_min, k.start_max, pass ? "" : "   <-- UNEXPECTED");
    failures += pass ? 0 : 1;
  };
  for (int marked = 0; marked < 2; ++marked) {
    const auto good = marked ? start_marked : end_marked;
    const char* tag = marked ? "start-marked: " : "end-marked: ";
    auto name = [&](const char* what) {
      static char buf[128];
      std::snprintf(buf, sizeof buf, "%s%s", tag, what);
      return (const char*)buf;
    };
    expect(name("the good look-ahead"), run(good(), &k), true);
    if (marked)
      ranges(name("its ranges"), -2.0, 0.0, -3.0, -0.5, -2.0, -0.5);
    else
      ranges(name("its ranges"), -1.0, 0.0, -2.0, 0.0, 0.0, 0.0);
    Pack p = good();
    for (size_t n = 1; n < p.look.size(); ++n) p.look[n] = (double)n;
    expect(name("any finite array with a zero root"), run(p, &k), true);
    p = good(), p.look[1] = std::numeric_limits<double>::quiet_NaN();
    expect(name("a NaN entry"), run(p, &k), false);
    p = good(), p.look.back() = std::numeric_limits<double>::infinity();
    expect(name("a +inf entry in the last node"), run(p, &k), false);
    p = good(), p.look[2] = -std::numeric_limits<double>::infinity();
    expect(name("a -inf entry"), run(p, &k), false);
    p = good(), p.look[0] = -0.25;
    expect(name("a root that is not 0"), run(p, &k), false);
    expect(name("a NULL node_look"), run(good(), &k, true), false);
    // a lexicon the pack check would have refused must not lead the look-ahead's check outside its arrays
    p = good(), p.arc_ptr[0] = 1;
    expect(name("arc_ptr does not start at 0"), run(p, &k), false);
    p = good(), p.arc_ptr[2] = 1000;
    expect(name("arc_ptr leaves the arcs"), run(p, &k), false);
    p = good(), p.arc_ptr[2] = 1;
    expect(name("arc_ptr descends"), run(p, &k), false);
    p = good(), p.arc_next[3] = 1000;
    expect(name("an arc to a node that is not there"), run(p, &k), false);
    if (marked) {
      p = good(), p.arc_next[3] = -3;
      expect(name("an end-marked word arc"), run(p, &k), false);
    }
    p = good(), p.V = 0;
    expect(name("no words"), run(p, &k), false);
  }
  {  // the smallest lexicons there are: one word of one label
    expect("end-marked: one word of one label", run({{0, 1}, {0}, {-1}, {}, {0.0}, 1}, &k), true);
    ranges("its ranges: no inner arc", 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
    expect("start-marked: one word of one label", run({{0, 1, 1}, {0}, {1}, {-1, 0}, {0.0, -1.5}, 1}, &k), true);
    ranges("its ranges", -1.5, -1.5, -1.5, -1.5, -1.5, -1.5);
  }
  expect("a NULL lexicon", wfl_lexicon_lookahead_check(nullptr, &k), false);
  expect("a NULL start-marked lexicon", wfl_lexicon_marked_lookahead_check(nullptr, &k), false);
  {
    const Pack p = end_marked();
    const auto ptr = exact(p.arc_ptr), label = exact(p.arc_label), next = exact(p.arc_next);
    const wfl_lexicon lex{5, 9, 5, 0, ptr.get(), label.get(), next.get()};
    expect("a NULL look-ahead struct", wfl_lexicon_lookahead_check(&lex, nullptr), false);
  }
  std::printf("%d unexpected\n", failures);
  return failures ? 1 : 0;
}
