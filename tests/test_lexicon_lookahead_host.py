"""CPU tests (-m "not gpu") of the word-LM look-ahead on the host (gtn_applications_amd/lexicon.py: Lexicon.lookahead,
Lexicon.unigram_lookahead, LexiconLookahead; lm.py: NGramLM.unigram_scores; include/wfl.h: wfl_lexicon_lookahead,
wfl_lexicon_lookahead_check, wfl_lexicon_marked_lookahead_check): node_look of the five-word
lexicons of the other host tests, literally, for both boundaries; the unigram scores of tests/golden/lm_small.arpa
against the file's numbers; the -inf substitution; every ValueError; a bad look-ahead for every clause of the check; the
ranges the prune bound is formed from, literally."""
import ctypes
import math
import os

import numpy as np
import pytest

from gtn_applications_amd import _native as N
from gtn_applications_amd.lexicon import Lexicon, LexiconLookahead, check_lookahead
from gtn_applications_amd.lm import NGramLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN10 = math.log(10.0)

# tests/test_lexicon_host.py's five words over classes 1..5 of C = 6 with the blank 0
FIVE = [(1, 5), (1, 2, 5), (2, 5), (3,), (2, 2, 4)]
# tests/test_lexicon_marked_host.py's: 0 "_a", 1 "_the", 2 "n", 3 "t", 4 "re", 5 the blank, 6 "_an"
SPELLINGS = [(0,), (0, 2), (0, 2, 3), (1,), (1, 4), (6,)]
WORD_OF = [0, 1, 2, 3, 4, 1]
U = [-1.0, -2.0, -3.0, -4.0, -0.5]


def end_marked():
    return Lexicon(FIVE, 6, 0)


def start_marked():
    return Lexicon(SPELLINGS, 7, 5, boundary="start", word_of=WORD_OF)


def test_node_look_of_the_end_marked_lexicon_literally():
    lex = end_marked()
    # nodes: 0 root; 1 "1"; 2 "2"; 3 "1 2"; 4 "2 2".  Below "1": words 0 and 1; below "2": words 2 and 4.
    look = lex.lookahead(U)
    assert isinstance(look, LexiconLookahead) and look.lexicon is lex
    assert look.node_look.dtype == np.float64 and look.node_look.tolist() == [0.0, -1.0, -0.5, -2.0, -0.5]
    # the ranges, literally: inner arcs 0->1 (-1), 0->2 (-0.5), 1->3 (-1), 2->4 (0); a word completes at every node,
    # the root included (word 3 has one label)
    assert (look.arc_min, look.arc_max) == (-1.0, 0.0)
    assert (look.end_min, look.end_max) == (-2.0, 0.0)
    assert (look.start_min, look.start_max) == (0.0, 0.0)
    # the root is 0 whatever the scores, and a positive score is a score like any other
    assert lex.lookahead([3.0, 1.0, 2.0, 9.0, 0.0]).node_look.tolist() == [0.0, 3.0, 2.0, 1.0, 0.0]


def test_node_look_of_the_start_marked_lexicon_literally():
    lex = start_marked()
    # nodes: 0 root; 1 "_a" (word 0); 2 "_the" (3); 3 "_an" (1); 4 "_a n" (1); 5 "_the re" (4); 6 "_a n t" (2): a terminal
    # node counts its own word and everything below it
    look = lex.lookahead(U)
    assert look.node_look.tolist() == [0.0, -1.0, -0.5, -2.0, -2.0, -0.5, -3.0]
    # arcs 0->1 (-1), 0->2 (-0.5), 0->3 (-2), 1->4 (-1), 2->5 (0), 4->6 (-1); every node but the root is terminal; the
    # root's children are 1, 2, 3
    assert (look.arc_min, look.arc_max) == (-2.0, 0.0)
    assert (look.end_min, look.end_max) == (-3.0, -0.5)
    assert (look.start_min, look.start_max) == (-2.0, -0.5)


def test_unigram_scores_of_the_golden_file():
    words = ["wood", "cindy", "pittsburgh", "jean"]
    lm = NGramLM.from_arpa(os.path.join(ROOT, "tests", "golden", "lm_small.arpa"), words, blank=4)
    u = lm.unigram_scores()
    assert u.dtype == np.float64 and u.shape == (5,)
    assert u[:4].tolist() == [-0.6990 * LN10] * 4 and u[4] == -math.inf  # (the blank's entry)
    # entry v is step(base, v)[0] from the state without a back-off; the start state <s> backs off to it, uncounted
    base = lm.start
    while lm.bo_next[base] >= 0:
        base = int(lm.bo_next[base])
    assert base != lm.start and all(u[v] == lm.step(base, v)[0] for v in range(4))
    assert lm.step(lm.start, 0)[0] == (-0.3064 + -0.6990) * LN10 != u[0]
    # a word the file does not name takes <unk>'s unigram; the blank elsewhere
    lm = NGramLM.from_arpa(os.path.join(ROOT, "tests", "golden", "lm_small.arpa"), ["zebra", "jean"], blank=0)
    assert lm.unigram_scores().tolist() == [-math.inf, -1.0 * LN10, -0.6990 * LN10]


def word_lm(tmp_path, log10, name="u.arpa"):
    """a unigram word LM over w0 .. with the given log10 probabilities ("-inf": a word of probability 0)"""
    words = [f"w{v}" for v in range(len(log10))]
    lines = ["\\data\\", f"ngram 1={len(words) + 2}", "", "\\1-grams:", "-1.0\t<s>", "-1.0\t</s>"]
    lines += [f"{p}\t{w}" for p, w in zip(log10, words)]
    path = tmp_path / name
    path.write_text("\n".join(lines + ["", "\\end\\", ""]))
    return NGramLM.from_arpa(str(path), words, blank=len(words))


def test_unigram_lookahead_substitutes_and_is_built_once(tmp_path):
    lex = end_marked()
    lm = word_lm(tmp_path, [-1.0, "-inf", -3.0, -0.25, -2.0])
    assert lm.unigram_scores()[1] == -math.inf
    look = lex.unigram_lookahead(lm)
    # word 1 takes the smallest finite entry, word 2's: below "1 2" only word 1, below "1" words 0 and 1
    assert look.node_look.tolist() == [0.0, -1.0 * LN10, -2.0 * LN10, -3.0 * LN10, -2.0 * LN10]
    # once per (lexicon, lm) pair: the same object again, through every door
    assert lex.unigram_lookahead(lm) is look and check_lookahead("unigram", lex, lm, False, "t") is look
    other = word_lm(tmp_path, [-1.0, -1.0, -1.0, -1.0, -1.0], "v.arpa")
    assert lex.unigram_lookahead(other) is not look and lex.unigram_lookahead(other) is lex.unigram_lookahead(other)
    with pytest.raises(ValueError, match="finite unigram score for none"):
        lex.unigram_lookahead(word_lm(tmp_path, ["-inf"] * 5, "z.arpa"))
    with pytest.raises(ValueError, match="word LM over its 5 words"):
        lex.unigram_lookahead(word_lm(tmp_path, [-1.0] * 4, "four.arpa"))


def test_check_lookahead_and_every_value_error(tmp_path):
    lex, marked = end_marked(), start_marked()
    lm = word_lm(tmp_path, [-1.0, -2.0, -3.0, -0.25, -2.0])
    assert check_lookahead(None, None, None, False, "t") is None
    explicit = check_lookahead(np.array(U, np.float32), lex, lm, False, "t")
    assert explicit.node_look.tolist() == [0.0, -1.0, -0.5, -2.0, -0.5]
    prepared = marked.lookahead(U)
    assert check_lookahead(prepared, marked, lm, False, "t") is prepared
    for bad, message in (([0.0] * 4, "one score per word"), ([[0.0] * 5], "one score per word"), ([0.0] * 6, "one score per word"),
                         ([0.0, math.nan, 0.0, 0.0, 0.0], "word 1 is nan"), ([0.0, 0.0, 0.0, 0.0, -math.inf], "word 4 is -inf"),
                         ([0.0, 0.0, math.inf, 0.0, 0.0], "word 2 is inf"), ("bigram", "neither None, 'unigram'"),
                         (["a"] * 5, "must be numbers"), (prepared, "another lexicon")):
        with pytest.raises(ValueError, match=message):
            check_lookahead(bad, lex, lm, False, "t")
    for lx, m in ((None, lm), (lex, None), (None, None)):
        with pytest.raises(ValueError, match="lookahead needs a lexicon and its word lm"):
            check_lookahead("unigram", lx, m, False, "t")
    with pytest.raises(ValueError, match="merge_spellings"):
        check_lookahead("unigram", lex, lm, True, "t")
    with pytest.raises(ValueError, match="word LM over its 5 words"):
        check_lookahead(U, lex, word_lm(tmp_path, [-1.0] * 3, "three.arpa"), False, "t")


def _check(lex, node_look, marked=False):
    arr = None if node_look is None else np.ascontiguousarray(node_look, np.float64)
    desc = N.LexiconLookahead(None if arr is None else arr.ctypes.data, *([math.nan] * 6))
    if marked:
        d = lex.marked_desc()
        rc = N.lib.wfl_lexicon_marked_lookahead_check(ctypes.byref(d), ctypes.byref(desc))
    else:
        d = N.Lexicon(lex.num_nodes, lex.num_arcs, lex.num_words, 0, lex.arc_ptr.ctypes.data, lex.arc_label.ctypes.data,
                      lex.arc_next.ctypes.data)
        rc = N.lib.wfl_lexicon_lookahead_check(ctypes.byref(d), ctypes.byref(desc))
    return rc, N.last_error(), desc


@pytest.mark.parametrize("marked", [False, True], ids=["end", "start"])
def test_a_bad_lookahead_per_clause_of_the_check(marked):
    lex = start_marked() if marked else end_marked()
    good = lex.lookahead(U).node_look
    rc, _, desc = _check(lex, good, marked)
    assert rc == N.WFL_OK and (desc.arc_min, desc.arc_max) == ((-2.0, 0.0) if marked else (-1.0, 0.0))  # (NaN overwritten)
    for n, v in ((1, math.nan), (lex.num_nodes - 1, math.inf), (2, -math.inf)):
        bad = good.copy()
        bad[n] = v
        rc, message, _ = _check(lex, bad, marked)
        assert rc == N.ERR_INVALID and f"node_look[{n}] is not finite" in message
        with pytest.raises(ValueError, match="is not finite"):
            LexiconLookahead(lex, bad)
    bad = good.copy()
    bad[0] = -0.25
    rc, message, _ = _check(lex, bad, marked)
    assert rc == N.ERR_INVALID and "the root's look-ahead is 0" in message
    with pytest.raises(ValueError, match="the root's look-ahead is 0"):
        LexiconLookahead(lex, bad)
    # a wrong length is refused before the library reads anything; a NULL array by the library
    for wrong in (good[:-1], np.append(good, 0.0), good.reshape(1, -1)):
        with pytest.raises(ValueError, match="one entry per node"):
            LexiconLookahead(lex, wrong)
    rc, message, _ = _check(lex, None, marked)
    assert rc == N.ERR_INVALID and "NULL" in message
    with pytest.raises(ValueError, match="must be a lexicon.Lexicon"):
        LexiconLookahead(None, good)
    # any finite array with a zero root passes: the totals telescope whatever it holds
    assert _check(lex, np.arange(lex.num_nodes, dtype=np.float64), marked)[0] == N.WFL_OK


def test_the_ranges_of_a_small_trie_literally():
    # two words (1, 2, 4) and (1, 3, 4) over C = 5, blank 0: nodes 0 root, 1 "1", 2 "1 2", 3 "1 3"
    lex = Lexicon([(1, 2, 4), (1, 3, 4)], 5, 0)
    look = lex.lookahead([-2.0, -0.25])
    assert look.node_look.tolist() == [0.0, -0.25, -2.0, -0.25]
    assert (look.arc_min, look.arc_max) == (-1.75, 0.0)  # 0->1: -0.25, 1->2: -1.75, 1->3: 0
    assert (look.end_min, look.end_max) == (-2.0, -0.25)  # words complete at nodes 2 and 3
    assert (look.start_min, look.start_max) == (0.0, 0.0)
    # a lexicon of one-label words has no inner arc: [0, 0]
    flat = Lexicon([(1,), (2,)], 4, 0).lookahead([-1.0, -2.0])
    assert flat.node_look.tolist() == [0.0] and (flat.arc_min, flat.arc_max, flat.end_min, flat.end_max) == (0.0, 0.0, 0.0, 0.0)
    # start-marked: the same two words begun by class 1, and a one-label word 3
    marked = Lexicon([(1, 2, 4), (1, 3, 4), (1,)], 5, 0, boundary="start").lookahead([-2.0, -0.25, -1.0])
    assert marked.node_look.tolist() == [0.0, -0.25, -2.0, -0.25, -2.0, -0.25]
    assert (marked.arc_min, marked.arc_max) == (-1.75, 0.0)
    assert (marked.end_min, marked.end_max) == (-2.0, -0.25)  # terminal: node 1 (-0.25) and the two leaves
    assert (marked.start_min, marked.start_max) == (-0.25, -0.25)
