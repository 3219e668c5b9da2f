// wfl_lexicon_marked_check (include/wfl.h) on good and bad packs in exact-size heap arrays: a
// stand-alone host program for AddressSanitizer and UBSan -- an index the check reads past the end of an array, or
// before it has checked the range it comes from, is a report.  No device is used: the check is host code.  Build and
// run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude \
//     -Igtn_applications_amd/csrc scripts/lexicon_marked_check_asan.cpp gtn_applications_amd/csrc/beam_kernels.hip \
//     gtn_applications_amd/csrc/graph.cpp -o scripts/_build/lexicon_marked_check_asan && scripts/_build/lexicon_marked_check_asan
// It prints one line per pack and exits 0 if the good packs pass and every bad one is refused.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "wfl.h"

namespace {

struct Pack {
  std::vector<int32_t> arc_ptr, arc_label, arc_next, node_word, start_node;
  int V, C, blank;
};

// every array copied into a heap block of exactly its size, so that the sanitizer sees the first element behind it
int run(const Pack& p, int num_nodes = -1, int num_arcs = -1) {
  auto exact = [](const std::vector<int32_t>& v) {
    std::unique_ptr<int32_t[]> a(new int32_t[v.size()]);
    if (!v.empty()) std::memcpy(a.get(), v.data(), v.size() * sizeof(int32_t));
    return a;
  };
  const auto ptr = exact(p.arc_ptr), label = exact(p.arc_label), next = exact(p.arc_next), word = exact(p.node_word),
             start = exact(p.start_node);
  wfl_lexicon_marked m;
  m.trie.num_nodes = num_nodes >= 0 ? num_nodes : (int32_t)p.arc_ptr.size() - 1;
  m.trie.num_arcs = num_arcs >= 0 ? num_arcs : (int32_t)p.arc_label.size();
  m.trie.num_words = p.V, m.trie.reserved = 0;
  m.trie.arc_ptr = ptr.get(), m.trie.arc_label = label.get(), m.trie.arc_next = next.get();
  m.node_word = word.get(), m.start_node = start.get();
  return wfl_lexicon_marked_check(&m, p.C, p.blank);
}

// "_a", "_a n", "_a n t", "_the", "_the re" and "_an" as a second spelling of "_a n"; classes 0 "_a", 1 "_the", 2 "n",
// 3 "t", 4 "re", 5 the blank, 6 "_an"
Pack good() {
  return {{0, 3, 4, 5, 5, 6, 6, 6}, {0, 1, 6, 2, 4, 3}, {1, 2, 3, 4, 5, 6}, {-1, 0, 3, 1, 1, 4, 2}, {1, 2, -1, -1, -1, -1, 3}, 5, 7, 5};
}

}  // namespace

int main() {
  int failures = 0;
  auto expect = [&](const char* what, int rc, bool ok) {
    const bool pass = (rc == WFL_OK) == ok;
    std::printf("%-44s %s%s%s\n", what, rc == WFL_OK ? "accepted" : "refused: ", rc == WFL_OK ? "" : wfl_last_error(),
                pass ? "" : "   <-- UNEXPECTED");
    failures += pass ? 0 : 1;
  };
  expect("the good pack", run(good()), true);
  {  // one word, one label: the smallest pack there is
    expect("one word of one label", run({{0, 1, 1}, {0}, {1}, {-1, 0}, {1, -1}, 1, 2, 1}), true);
  }
  Pack p = good();
  p.arc_ptr[0] = 1;
  expect("arc_ptr does not start at 0", run(p), false);
  p = good(), p.arc_ptr[2] = 2;
  expect("arc_ptr descends", run(p), false);
  p = good(), p.arc_ptr[3] = 1000;
  expect("arc_ptr leaves the arcs", run(p), false);
  p = good(), p.arc_ptr[7] = 1000;
  expect("arc_ptr ends behind the arcs", run(p), false);
  p = good(), p.arc_next[5] = 0;
  expect("an arc back to the root", run(p), false);
  p = good(), p.arc_next[5] = 1000;
  expect("an arc to a node that is not there", run(p), false);
  p = good(), p.arc_next[5] = -3;
  expect("an end-marked word arc", run(p), false);
  p = good(), p.arc_next[4] = 4;
  expect("a node entered twice", run(p), false);
  p = good(), p.arc_ptr = {0, 3, 4, 4, 4, 4, 5, 6}, p.arc_next = {1, 2, 3, 4, 6, 5};
  expect("a cycle apart from the root", run(p), false);
  p = good(), p.arc_label[5] = 1000;
  expect("a label outside the classes", run(p), false);
  p = good(), p.arc_label[5] = -1000;
  expect("a negative label", run(p), false);
  p = good(), p.arc_label[5] = 5;
  expect("the blank as a label", run(p), false);
  p = good(), p.arc_label[0] = 1, p.arc_label[1] = 0;
  expect("labels that do not ascend", run(p), false);
  p = good(), p.node_word[3] = -1;
  expect("a node without arcs that ends no word", run(p), false);
  p = good(), p.node_word[0] = 0;
  expect("a terminal root", run(p), false);
  p = good(), p.node_word[5] = 1000;
  expect("a word id that is not there", run(p), false);
  p = good(), p.node_word[5] = -1000;
  expect("a word id below -1", run(p), false);
  p = good(), p.node_word[5] = 3;
  expect("a word without a node", run(p), false);
  p = good(), p.start_node[6] = -1;
  expect("start_node misses a root arc", run(p), false);
  p = good(), p.start_node[2] = 4;
  expect("start_node names a deeper node", run(p), false);
  p = good(), p.start_node[2] = 1000;
  expect("start_node names no node", run(p), false);
  p = good(), p.arc_label[5] = 1;
  expect("a start class inside a word", run(p), false);
  p = good(), p.V = 0;
  expect("no words", run(p), false);
  p = good(), p.blank = 7;
  expect("a blank outside the classes", run(p), false);
  expect("a NULL pack", wfl_lexicon_marked_check(nullptr, 7, 5), false);
  std::printf("%d unexpected\n", failures);
  return failures ? 1 : 0;
}
