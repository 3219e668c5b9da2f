"""CPU tests (-m "not gpu") of the start-marked lexicon on the host (gtn_applications_amd/lexicon.py, boundary="start";
include/wfl.h: wfl_lexicon_marked, wfl_lexicon_marked_check): the packed arrays of a small
vocabulary that is not prefix-free, literally; walk() and words() by rule 5; every ValueError; a bad pack for every
clause of the pack check; the end-marked class unchanged; and from_words over the word pieces of
benchmarks/word_pieces_tokens_1000.txt."""
import ctypes
import os

import numpy as np
import pytest

from gtn_applications_amd import _native as N
from gtn_applications_amd.lexicon import Lexicon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# classes: 0 "_a", 1 "_the", 2 "n", 3 "t", 4 "re", 5 the blank, 6 "_an"
A_, THE, n_, t_, RE, BLANK, AN = range(7)
WORDS = ["_a", "_an", "_ant", "_the", "_there"]
SPELLINGS = [(A_,), (A_, n_), (A_, n_, t_), (THE,), (THE, RE), (AN,)]  # "_an" also as the one piece "_an"
WORD_OF = [0, 1, 2, 3, 4, 1]


def small():
    return Lexicon(SPELLINGS, 7, BLANK, words=WORDS, boundary="start", word_of=WORD_OF)


def test_packed_arrays_literally():
    L = small()
    # breadth first, children in label order: 0 root; 1 "_a", 2 "_the", 3 "_an"; 4 "_a n"; 5 "_the re"; 6 "_a n t"
    assert L.boundary == "start"
    assert (L.num_nodes, L.num_arcs, L.num_words) == (7, 6, 5)
    assert L.arc_ptr.tolist() == [0, 3, 4, 5, 5, 6, 6, 6]
    assert L.arc_label.tolist() == [A_, THE, AN, n_, RE, t_]
    assert L.arc_next.tolist() == [1, 2, 3, 4, 5, 6]  # (every target a node >= 1: leaves are stored)
    assert L.node_word.tolist() == [-1, 0, 3, 1, 1, 4, 2]  # (word 1 on two nodes: its two spellings)
    assert L.start_node.tolist() == [1, 2, -1, -1, -1, -1, 3]
    for a in (L.arc_ptr, L.arc_label, L.arc_next, L.node_word, L.start_node):
        assert a.dtype == np.int32


def test_walk_and_words_follow_rule_5():
    L = small()
    assert L.walk([]) == ([], 0)
    assert L.walk([A_]) == ([0], 1)  # a terminal inner node: the pending word counts
    assert L.walk([A_, n_]) == ([1], 4)
    assert L.walk([A_, A_, n_, t_]) == ([0, 2], 6)
    assert L.walk([THE, RE, AN, THE]) == ([4, 1, 3], 2)
    assert L.walk([n_]) is None  # no word begins with "n"
    assert L.walk([A_, RE]) is None  # "_a re" is no prefix of a spelling
    assert L.walk([BLANK]) is None
    assert L.words([A_, n_, THE]) == [1, 3]
    assert L.words([AN, A_, n_]) == [1, 1]  # the two spellings of one word
    with pytest.raises(ValueError, match="leave the lexicon"):
        L.words([A_, t_])
    # a lexicon with a non-terminal inner node: "_a n t" alone
    M = Lexicon([(A_, n_, t_)], 7, BLANK, boundary="start")
    assert M.walk([A_, n_]) == ([], 2)  # it ends inside the word
    with pytest.raises(ValueError, match="end inside a word"):
        M.words([A_, n_])
    assert M.walk([A_, n_, A_]) is None  # a new word behind an unfinished one
    assert M.words([A_, n_, t_, A_, n_, t_]) == [0, 0]


def test_value_errors():
    def bad(match, spellings, C=7, blank=BLANK, **kw):
        with pytest.raises(ValueError, match=match):
            Lexicon(spellings, C, blank, boundary="start", **kw)

    bad("no words", [])
    bad("'_an' has an empty spelling", [(A_,), ()], words=["_a", "_an"])
    bad("word 1 is spelled with the blank 5", [(A_,), (A_, BLANK)])
    bad(r"word 0 is spelled with class 7, outside \[0, 7\)", [(A_, 7)])
    bad(r"word 0 is spelled with class -1", [(-1,)])
    bad("'_a' and '_b' have the same spelling", [(A_,), (A_,)], words=["_a", "_b"])
    bad("same spelling twice", [(A_,), (A_,)], word_of=[0, 0])
    bad("'_c' has no spelling", [(A_,), (THE,)], words=["_a", "_b", "_c"], word_of=[0, 1])
    bad(r"word 1 has no spelling", [(A_,), (THE,)], word_of=[0, 2])
    bad("one word per spelling", [(A_,), (THE,)], word_of=[0])
    bad(r"outside \[0, 1\)", [(A_,), (THE,)], words=["_a"], word_of=[0, 1])
    # a class that both begins a word and occurs inside one, with the two words that show it
    bad("class 1 begins '_the' and occurs inside '_athe'", [(THE,), (A_, THE)], words=["_the", "_athe"])
    bad("class 0 begins word 0 and occurs inside word 0", [(A_, A_)])
    bad("7 classes, blank 7", [(A_,)], blank=7)
    with pytest.raises(ValueError, match="neither 'end' nor 'start'"):
        Lexicon([(A_,)], 7, BLANK, boundary="middle")


def pack(arc_ptr, arc_label, arc_next, node_word, start_node, V, N_=None, A=None):
    """a wfl_lexicon_marked over exact-size arrays and what keeps them alive"""
    arrays = [np.asarray(a, dtype=np.int32) for a in (arc_ptr, arc_label, arc_next, node_word, start_node)]
    trie = N.Lexicon(len(arc_ptr) - 1 if N_ is None else N_, len(arc_label) if A is None else A, V, 0,
                     arrays[0].ctypes.data, arrays[1].ctypes.data, arrays[2].ctypes.data)
    return N.LexiconMarked(trie, arrays[3].ctypes.data, arrays[4].ctypes.data), arrays


GOOD = dict(arc_ptr=[0, 3, 4, 5, 5, 6, 6, 6], arc_label=[0, 1, 6, 2, 4, 3], arc_next=[1, 2, 3, 4, 5, 6],
            node_word=[-1, 0, 3, 1, 1, 4, 2], start_node=[1, 2, -1, -1, -1, -1, 3], V=5)


def check(C=7, blank=BLANK, **change):
    desc, keep = pack(**{**GOOD, **change})
    rc = N.lib.wfl_lexicon_marked_check(ctypes.byref(desc), C, blank)
    return rc, N.last_error()


def test_pack_check_accepts_the_good_pack():
    assert check()[0] == N.WFL_OK


@pytest.mark.parametrize("change, message", [
    (dict(arc_ptr=[1, 3, 4, 5, 5, 6, 6, 6]), "arc_ptr runs from 1 to 6"),
    (dict(arc_ptr=[0, 3, 2, 5, 5, 6, 6, 6]), "arc_ptr descends or leaves"),
    (dict(arc_next=[1, 2, 3, 4, 5, 0]), "leads to node 0"),  # a tree rooted at 0: nothing leads back to the root
    (dict(arc_next=[1, 2, 3, 4, 5, 7]), "leads to node 7"),
    (dict(arc_next=[1, 2, 3, 4, 4, 6]), "node 4 is the target of more than one arc"),
    # nodes 5 and 6 point at each other, away from the root: every node entered once, yet no tree
    (dict(arc_ptr=[0, 3, 4, 4, 4, 4, 5, 6], arc_next=[1, 2, 3, 4, 6, 5], node_word=[-1, 0, 3, 1, 1, 4, 2]),
     "nodes are reached from the root"),
    (dict(arc_label=[0, 1, 6, 2, 4, 7]), "has label 7"),
    (dict(arc_label=[0, 1, 6, 2, 4, -1]), "has label -1"),
    (dict(arc_label=[0, 1, 6, 2, 4, 5]), "never the blank 5"),
    (dict(arc_label=[1, 0, 6, 2, 4, 3]), "not strictly ascending"),
    (dict(node_word=[-1, 0, 3, -1, 1, 4, 2]), "node 3 has no arc and ends no word"),  # an arc-less node is terminal
    (dict(node_word=[0, 0, 3, 1, 1, 4, 2]), "the root ends word 0"),
    (dict(node_word=[-1, 0, 3, 1, 1, 5, 2]), "node 5 ends word 5 of 5"),
    (dict(node_word=[-1, 0, 3, 1, 1, 3, 2]), "word 4 ends at no node"),  # every word id on at least one node
    (dict(start_node=[1, 2, -1, -1, -1, -1, -1]), r"start_node\[6\] is -1, the root's child by class 6 is 3"),
    (dict(start_node=[1, 2, 4, -1, -1, -1, 3]), r"start_node\[2\] is 4, the root's child by class 2 is -1"),
    (dict(arc_label=[0, 1, 6, 2, 4, 1]), "class 1 starts a word and is the label of arc 5 of node 4 inside one"),
    (dict(V=0), "0 words"),
])
def test_pack_check_refuses_every_clause(change, message):
    import re

    rc, err = check(**change)
    assert rc == N.ERR_INVALID
    assert re.search(message, err), err


def test_pack_check_refuses_null_arrays_and_bad_classes():
    assert N.lib.wfl_lexicon_marked_check(None, 7, BLANK) == N.ERR_INVALID
    desc, keep = pack(**GOOD)
    for field in ("node_word", "start_node"):
        d = N.LexiconMarked(desc.trie, desc.node_word, desc.start_node)
        setattr(d, field, None)
        assert N.lib.wfl_lexicon_marked_check(ctypes.byref(d), 7, BLANK) == N.ERR_INVALID
        assert "NULL" in N.last_error()
    assert check(C=7, blank=7)[0] == N.ERR_INVALID


def test_end_marked_objects_are_unchanged():
    # the same calls as before the second convention: the same arrays, no new ones, the same errors
    L = Lexicon([(0, 1, 3), (0, 2, 3), (1, 3)], 5, 4)
    assert L.boundary == "end"
    assert L.arc_ptr.tolist() == [0, 2, 4, 5, 6, 7]
    assert L.arc_label.tolist() == [0, 1, 1, 2, 3, 3, 3]
    assert L.arc_next.tolist() == [1, 2, 3, 4, -3, -1, -2]
    assert not hasattr(L, "node_word") and not hasattr(L, "start_node")
    assert L.walk([0, 1, 3, 1]) == ([0], 2) and L.words([1, 3, 0, 2, 3]) == [2, 1]
    with pytest.raises(ValueError, match="the spelling of 'a' is a proper prefix of that of 'ab': the lexicon is not "
                                         "prefix-free; spellings that end in a separator class"):
        Lexicon([(0,), (0, 1)], 3, 2, words=["a", "ab"])
    with pytest.raises(ValueError, match="the spelling of word 1 is a proper prefix of that of word 0"):
        Lexicon([(0, 1), (0,)], 3, 2)
    with pytest.raises(ValueError, match="word_of needs boundary='start'"):
        Lexicon([(0,), (1,)], 3, 2, word_of=[0, 1])
    # (the very vocabulary of this file is what the end-marked class refuses)
    with pytest.raises(ValueError, match="not prefix-free"):
        Lexicon(SPELLINGS[:5], 7, BLANK, words=WORDS)


def word_pieces():
    with open(os.path.join(ROOT, "benchmarks", "word_pieces_tokens_1000.txt"), encoding="utf-8") as f:
        return [line.rstrip("\n") for line in f if line.rstrip("\n")]


def synthesised_words(tokens, count=200, seed=0):
    """about `count` words over the word pieces, each one start piece joined with 0 - 2 plain pieces, with every word's
    shorter forms among them: not prefix-free by construction.  {word: its pieces}"""
    rs = np.random.RandomState(seed)
    first = [t for t in tokens if t.startswith("▁") and len(t) > 1]
    plain = [t for t in tokens if not t.startswith("▁")]
    words = {}
    while len(words) < count:
        pieces = [first[rs.randint(len(first))]] + [plain[rs.randint(len(plain))] for _ in range(rs.randint(3))]
        for k in range(1, len(pieces) + 1):  # the word and what it begins with
            words.setdefault("".join(pieces[:k]), pieces[:k])
    return words


def test_from_words_over_the_word_piece_file():
    tokens = word_pieces()
    assert len(tokens) == 1000 and "▁" in tokens and "▁the" in tokens
    words = synthesised_words(tokens)
    names = sorted(words)
    assert any(a != b and b.startswith(a) for a in names for b in names[names.index(a) + 1:names.index(a) + 3])
    blank = len(tokens)
    with pytest.raises(ValueError, match="not prefix-free"):
        Lexicon.from_words(names, tokens, blank, split=lambda w: words[w])
    L = Lexicon.from_words(names, tokens, blank, split=lambda w: words[w], boundary="start")
    assert (L.num_classes, L.blank, L.num_words, L.boundary) == (1001, 1000, len(names), "start")
    label = {t: i for i, t in enumerate(tokens)}
    for v, w in enumerate(names[:50]):
        assert L.words([label[p] for p in words[w]]) == [v]
    two = [label[p] for p in words[names[3]]] + [label[p] for p in words[names[7]]]
    assert L.words(two) == [3, 7]
    # several decompositions of a word: splits
    w = next(w for w in names if len(words[w]) == 1 and len(w) > 2 and all(ch in label for ch in w[1:]) and
             "▁" + w[1] in label)
    alt = ["▁" + w[1]] + list(w[2:])
    S = Lexicon.from_words([w], tokens, blank, boundary="start", splits=lambda x: [words[x], alt])
    assert S.num_words == 1 and len(S.spellings) == 2
    assert S.words([label[p] for p in alt]) == [0] and S.words([label[w]]) == [0]
    with pytest.raises(ValueError, match="no wordsep"):
        Lexicon.from_words(names, tokens, blank, wordsep="▁", boundary="start")
    with pytest.raises(ValueError, match="splits .* needs boundary='start'"):
        Lexicon.from_words(names, tokens, blank, splits=lambda x: [words[x]])
    with pytest.raises(ValueError, match="give one of them"):
        Lexicon.from_words(names, tokens, blank, boundary="start", split=lambda x: words[x], splits=lambda x: [words[x]])
    with pytest.raises(ValueError, match="is not one of the model's tokens"):
        Lexicon.from_words(["▁qqq"], tokens, blank, boundary="start", split=lambda x: ["▁qqq"])
