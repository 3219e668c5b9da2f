"""CPU tests (-m "not gpu") of the ASG beam search with a lexicon and a word-level LM (csrc/beam_kernels.hip:
wfl_asg_beam_search_lexicon, include/wfl.h): the header declares the new entry and libwfl.so
exports it, every bad argument is refused before a launch, engine.AsgLexiconBeamPlan and the module check their
arguments without a device, ASG.lexicon spells words as the criterion packs its targets, ASG.words reads a result back
-- and the Python restatement the GPU tests compare against (tests/asg_beam_lexicon_reference.py) is itself pinned to a
brute-force enumeration of all C^T frame paths, kept where they walk the lexicon (garbage transparent) back to a word
end and re-scored by rule 6, where nothing is pruned.  No device compute here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import asg_beam_lexicon_reference as AX
import asg_beam_reference as AR
import beam_lm_reference as LR
from gtn_applications_amd import _native as N
from gtn_applications_amd import engine as E
from gtn_applications_amd.criterions.asg import ASG, pack_replabels, unpack_replabels
from gtn_applications_amd.lexicon import Lexicon
from gtn_applications_amd.lm import NGramLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = AR.NEG


def test_header_declares_and_library_exports_the_entry_point():
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(wfl_[a-z0-9_]+)\s*\(", code))
    fresh = ctypes.CDLL(N.LIB_PATH)  # (a handle of its own: what the library exports, not what the table declared)
    name = "wfl_asg_beam_search_lexicon"
    assert name in declared and hasattr(fresh, name) and name in N.EXPORTED_SYMBOLS
    from gtn_applications_amd import metrics as M

    assert callable(E.asg_beam_search_lexicon) and callable(M.asg_beam_search_lexicon_errors)
    assert callable(ASG.lexicon) and callable(ASG.words)
    for fn in ("asg_beam_search_lexicon", "asg_beam_search_lexicon_errors", "AsgLexiconPlan"):
        assert hasattr(N.ops, fn), fn
    # the plans the existing searches are pinned to stay what they were
    assert E.AsgBeamPlan._fields == ("C", "beam", "classes_per_frame", "nbest") and len(E.BeamPlan._fields) == 11


# (B, T, C, beam, classes_per_frame, nbest, drop, num_replabels, garbage) around a good call
GOOD = dict(B=2, T=5, C=7, beam=4, K=3, nbest=2, drop=6, R=1, garbage=6)
BAD = [dict(B=0), dict(B=-1), dict(T=0), dict(C=0), dict(beam=0), dict(beam=65), dict(K=0), dict(K=8), dict(C=100, K=65),
       dict(nbest=0), dict(nbest=5), dict(beam=64, nbest=65), dict(R=-1), dict(drop=-2), dict(drop=7), dict(garbage=-2),
       dict(garbage=7), dict(garbage=100)]


def _search(a, null=None, lex_change=None, lm_change=None, weight=0.8, word=0.3, bonus=0.5, no_lex=False, with_lm=True,
            capacity=None):
    """wfl_asg_beam_search_lexicon with host addresses that are never touched: every case here is refused before a
    launch"""
    n = max(1, a["B"] * a["nbest"])
    bufs = dict(x=np.zeros(8, np.float32), Wt=np.zeros(8, np.float32), logz=np.zeros(8, np.float32), ws=np.zeros(8, np.int64),
                out=np.zeros(8, np.int32), offs=np.zeros(n + 1, np.int64), scores=np.zeros(n, np.float64))
    p = {k: (None if k == null else v.ctypes.data) for k, v in bufs.items()}
    larrays = dict(arc_ptr=np.array([0, 1], np.int32), arc_label=np.array([1], np.int32), arc_next=np.array([-1], np.int32))
    lf = dict(num_nodes=1, num_arcs=1, num_words=1, reserved=0, **{k: v.ctypes.data for k, v in larrays.items()})
    lf.update(lex_change or {})
    lex = N.Lexicon(*(lf[k] for k in ("num_nodes", "num_arcs", "num_words", "reserved", "arc_ptr", "arc_label", "arc_next")))
    arrays = dict(arc_ptr=np.zeros(2, np.int32), arc_label=np.zeros(1, np.int32), arc_next=np.zeros(1, np.int32),
                  arc_w=np.zeros(1, np.float64), bo_next=np.zeros(1, np.int32), bo_w=np.zeros(1, np.float64))
    f = dict(num_states=1, num_arcs=0, start=0, reserved=0, step_min=-1.0, step_max=0.0,
             **{k: v.ctypes.data for k, v in arrays.items()})
    f.update(lm_change or {})
    lm = N.NgramLm(*(f[k] for k in ("num_states", "num_arcs", "start", "reserved", "step_min", "step_max", "arc_ptr",
                                    "arc_label", "arc_next", "arc_w", "bo_next", "bo_w")))
    cap = a["B"] * a["nbest"] * a["T"] * max(1, a["R"]) if capacity is None else capacity
    return N.lib.wfl_asg_beam_search_lexicon(p["x"], p["Wt"], p["logz"], a["B"], a["T"], a["C"], a["beam"], a["K"], a["nbest"],
                                             a["drop"], a["R"], a["garbage"], None if no_lex else ctypes.byref(lex),
                                             ctypes.byref(lm) if with_lm else None, weight, word, bonus, 1, p["ws"], p["out"],
                                             cap, p["offs"], p["scores"], None)


@pytest.mark.parametrize("with_lm", [True, False])
@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_search_arguments_are_refused_without_a_device(change, with_lm):
    a = dict(GOOD, **change)
    if "C" in change:
        a["drop"] = a["garbage"] = -1
    assert _search(a, with_lm=with_lm) == N.ERR_INVALID
    assert "asg_beam_search_lexicon" in N.last_error()


@pytest.mark.parametrize("null", ["x", "Wt", "ws", "out", "offs", "scores"])
def test_null_pointers_are_refused(null):
    assert _search(GOOD, null=null) == N.ERR_INVALID
    assert _search(GOOD, null=null, with_lm=False) == N.ERR_INVALID


@pytest.mark.parametrize("change", [dict(num_nodes=0), dict(num_arcs=0), dict(num_words=0), dict(num_nodes=-1),
                                    dict(num_words=2 ** 31 - 1), dict(arc_ptr=None), dict(arc_label=None), dict(arc_next=None)],
                         ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_a_bad_lexicon_struct_is_refused(change):
    assert _search(GOOD, lex_change=change) == N.ERR_INVALID
    assert "lexicon" in N.last_error()
    assert _search(GOOD, lex_change=change, with_lm=False) == N.ERR_INVALID


@pytest.mark.parametrize("change", [dict(num_states=0), dict(num_arcs=-1), dict(start=-1), dict(start=1), dict(arc_ptr=None),
                                    dict(arc_label=None), dict(arc_next=None), dict(arc_w=None), dict(bo_next=None),
                                    dict(bo_w=None), dict(step_min=math.nan), dict(step_max=math.nan)],
                         ids=lambda c: ",".join(c))
def test_a_bad_word_lm_struct_is_refused(change):
    assert _search(GOOD, lm_change=change) == N.ERR_INVALID


def test_null_lexicon_weights_that_are_not_finite_small_capacity_and_too_many_classes():
    assert _search(GOOD, no_lex=True) == N.ERR_INVALID
    for w, o, b in ((math.nan, 0.0, 0.0), (math.inf, 0.0, 0.0), (1.0, math.nan, 0.0), (1.0, -math.inf, 0.0),
                    (1.0, 0.0, math.nan), (1.0, 0.0, math.inf)):
        for with_lm in (True, False):
            assert _search(GOOD, weight=w, word=o, bonus=b, with_lm=with_lm) == N.ERR_INVALID
            assert "finite" in N.last_error()
    a = dict(GOOD, R=3)
    assert _search(a, capacity=2 * 2 * 5 * 3 - 1) == N.ERR_INVALID
    assert "out holds" in N.last_error()
    assert _search(dict(GOOD, C=16385, drop=-1, garbage=-1)) == N.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------
# the host side: ASG.lexicon, ASG.words, the plan and the module's refusals
# ------------------------------------------------------------------------------------------------------------------
TOKENS = ["a", "b", "c", "|"]
WORDS = ["ab", "aab", "baaa", "c", "bcc"]  # (a doubled letter at the start and at the end, a tripled one)
# rule 1, written out: token i is class i + R, replabel k is class k
SPELLED = {1: [(1, 2, 4), (1, 0, 2, 4), (2, 1, 0, 1, 4), (3, 4), (2, 3, 0, 4)],
           2: [(2, 3, 5), (2, 0, 3, 5), (3, 2, 1, 5), (4, 5), (3, 4, 0, 5)]}


@pytest.mark.parametrize("garbage", [True, False])
@pytest.mark.parametrize("R", [1, 2])
def test_asg_lexicon_spells_words_as_the_criterion_packs_targets(R, garbage):
    crit = ASG(len(TOKENS), num_replabels=R, use_garbage=garbage)
    lex = crit.lexicon(WORDS, TOKENS, wordsep="|")
    assert isinstance(lex, Lexicon) and lex.spellings == SPELLED[R] and lex.word_names == WORDS
    n = len(TOKENS) + R + int(garbage)
    assert n == crit.N
    assert (lex.num_classes, lex.blank) == ((n, n - 1) if garbage else (n + 1, n))
    if garbage:
        assert lex.blank == crit.garbage_idx and all(crit.garbage_idx not in s for s in lex.spellings)
    for v, w in enumerate(WORDS):
        toks = [TOKENS.index(ch) for ch in w] + [3]
        assert list(lex.spellings[v]) == pack_replabels(toks, R)
        assert unpack_replabels(list(lex.spellings[v]), R) == toks
        assert crit.words(lex, toks) == [v]
        assert crit.words(lex, torch.tensor(toks)) == [v]
    # a sentence packed as a whole is its words packed one by one: no word ends in a token a word starts with
    sentence = [1, 4, 3, 2, 0]
    toks = [t for v in sentence for t in [TOKENS.index(ch) for ch in WORDS[v]] + [3]]
    assert pack_replabels(toks, R) == [c for v in sentence for c in lex.spellings[v]]
    assert crit.words(lex, toks) == sentence and crit.words(lex, []) == []
    with pytest.raises(ValueError):
        crit.words(lex, toks[:-1])  # (it ends inside a word)
    with pytest.raises(ValueError):
        crit.words(lex, [2, 2, 2, 2, 3])  # (no such word)
    # a splitter instead of characters; without a separator
    pieces = ASG(3, num_replabels=R, use_garbage=garbage).lexicon(["ab", "aab"], ["a", "b", "c"], split=lambda w: list(w))
    assert pieces.spellings == [(R, R + 1), (R, 0, R + 1)]


def test_asg_lexicon_refuses_what_it_cannot_spell():
    crit = ASG(len(TOKENS), num_replabels=1)
    with pytest.raises(ValueError, match="'ab'.*'ba'|'ba'.*'ab'"):
        crit.lexicon(["ab", "ba"], TOKENS)  # (b ends one and starts the other)
    with pytest.raises(ValueError, match="separator"):
        crit.lexicon(["ca", "ab"], TOKENS)
    with pytest.raises(ValueError, match="'aa'"):
        crit.lexicon(["aa"], TOKENS)  # (the word behind itself)
    with pytest.raises(ValueError, match="'[|]c'"):
        crit.lexicon(["ab", "|c"], TOKENS, wordsep="|")  # (a word that starts with the separator)
    crit.lexicon(["ab", "cb"], TOKENS)  # (b ends both words and starts none)
    for kw in (dict(words=["ad"], tokens=TOKENS), dict(words=["ab"], tokens=TOKENS[:3]), dict(words=["ab"], tokens=list("aabc")),
               dict(words=["ab"], tokens=TOKENS, wordsep="#"), dict(words=[], tokens=TOKENS), dict(words=[""], tokens=TOKENS),
               dict(words=["ab", "abc"], tokens=TOKENS), dict(words=["ab", "ab"], tokens=TOKENS, wordsep="|")):
        with pytest.raises(ValueError):
            crit.lexicon(**kw)


def _word_lm(words, tmp_path, blank=None, eos=True, seed=3):
    p = tmp_path / f"words{len(words)}_{blank}_{eos}.arpa"
    p.write_text(LR.random_arpa(np.random.RandomState(seed), words, 2, 0.5, eos=eos))
    return NGramLM.from_arpa(str(p), words, len(words) if blank is None else blank)


def test_plan_refuses_what_it_should(tmp_path):
    with_g, without = ASG(4, 1, True), ASG(4, 1, False)
    lg, ln = with_g.lexicon(WORDS, TOKENS, wordsep="|"), without.lexicon(WORDS, TOKENS, wordsep="|")
    lm = _word_lm(WORDS, tmp_path)
    P = E.AsgLexiconBeamPlan
    assert P._fields == ("C", "beam", "classes_per_frame", "nbest", "garbage", "lexicon", "lm", "lm_weight", "word_bonus",
                         "length_bonus", "lm_eos")
    assert P.checked(6, 16, None, 1, 5, lg, None, 1.0, 0.0, 0.0, True, "t") == (6, 16, 6, 1, 5, lg, None, 1.0, 0.0, 0.0, True)
    assert P.checked(5, np.int64(4), 3, 2, None, ln, lm, 0.5, np.float64(-1), 2, False, "t") == \
        (5, 4, 3, 2, None, ln, lm, 0.5, -1.0, 2.0, False)
    good = dict(C=6, beam_size=4, classes_per_frame=None, nbest=1, garbage=5, lexicon=lg, lm=None, lm_weight=1.0, word_bonus=0.0,
                length_bonus=0.0, lm_eos=True)
    bad = (dict(beam_size=0), dict(beam_size=65), dict(beam_size=True), dict(classes_per_frame=7), dict(nbest=5), dict(C=0),
           dict(garbage=6), dict(garbage=-1), dict(garbage=True), dict(garbage=4), dict(garbage=None), dict(lexicon=None),
           dict(lexicon="words.txt"), dict(C=7, garbage=6), dict(C=5, garbage=None, lexicon=ASG(4, 2, False).lexicon(WORDS, TOKENS, wordsep="|")),
           dict(lm="lm.arpa"), dict(lm=_word_lm(WORDS + ["w"], tmp_path)), dict(lm=_word_lm(WORDS, tmp_path, blank=1)),
           dict(lm_weight=0.5), dict(lm_eos=False), dict(lm=lm, lm_weight=math.nan), dict(lm=lm, lm_weight="1"),
           dict(word_bonus=math.inf), dict(word_bonus=True), dict(length_bonus=math.nan), dict(lm=lm, lm_eos=1))
    for change in bad:
        with pytest.raises(ValueError, match="^t: "):
            P.checked(**dict(good, **change), what="t")
    # without a frame and without a device
    hyps, scores = P.checked(**dict(good, nbest=2, word_bonus=3.0), what="t").no_frames(2)
    assert [[h.tolist() for h in u] for u in hyps] == [[[], []]] * 2 and scores.tolist() == [[0.0, -math.inf]] * 2
    hyps, scores = E.asg_beam_search_lexicon(torch.zeros(2, 0, 6), torch.zeros(7, 6), lg, garbage=5, nbest=2, lm=lm, lm_weight=0.5)
    assert scores.tolist() == [[0.5 * lm.step(lm.start, len(WORDS) + 1)[0], -math.inf]] * 2
    for kw in (dict(num_replabels=-1), dict(num_replabels=True), dict(drop=6), dict(garbage=None)):
        with pytest.raises(ValueError):
            E.asg_beam_search_lexicon(torch.zeros(2, 0, 6), torch.zeros(7, 6), lg, **dict(dict(garbage=5), **kw))
    with pytest.raises(ValueError):
        E.asg_beam_search_lexicon(torch.zeros(2, 0, 6), torch.zeros(6, 6), lg, garbage=5)


@pytest.mark.parametrize("garbage", [True, False])
def test_module_refuses_bad_lexicon_arguments_before_a_device_is_needed(tmp_path, garbage):
    crit = ASG(len(TOKENS), num_replabels=1, use_garbage=garbage)
    x = torch.zeros(2, 5, crit.N)
    lex = crit.lexicon(WORDS, TOKENS, wordsep="|")
    lm = _word_lm(WORDS, tmp_path)
    token_lm = _word_lm([f"t{i}" for i in range(crit.N - 1)], tmp_path, blank=0)
    bad = (dict(lexicon="words.txt"), dict(lexicon=object()), dict(lexicon=[(1, 4)]),
           dict(lexicon=ASG(5, 1, garbage).lexicon(WORDS, TOKENS + ["d"], wordsep="|")), dict(lexicon=ASG(4, 2, garbage).lexicon(WORDS, TOKENS, wordsep="|")),
           dict(lm=lm), dict(lm_weight=0.5), dict(length_bonus=0.5), dict(word_bonus=0.5), dict(word_bonus=-1), dict(lm_eos=False),
           dict(lm_weight="1"), dict(lexicon=lex, word_bonus=math.nan), dict(lexicon=lex, word_bonus=math.inf),
           dict(lexicon=lex, word_bonus="1"), dict(lexicon=lex, word_bonus=True), dict(lexicon=lex, lm=token_lm),
           dict(lexicon=lex, lm=_word_lm(WORDS + ["w5"], tmp_path)), dict(lexicon=lex, lm=_word_lm(WORDS, tmp_path, blank=1)),
           dict(lexicon=lex, lm="lm.arpa"), dict(lexicon=lex, lm_weight=0.5), dict(lexicon=lex, lm_eos=False),
           dict(lexicon=lex, lm=lm, lm_weight=math.nan), dict(lexicon=lex, length_bonus=math.inf),
           dict(lexicon=lex, lm=lm, lm_eos=1), dict(lexicon=lex, beam_size=65), dict(lexicon=lex, nbest=17))
    for kw in bad:
        with pytest.raises(ValueError):
            crit.beam_search(x, **kw)
        if "nbest" not in kw:
            with pytest.raises(ValueError):
                crit.errors(x, [[1], [2]], None, **dict(dict(beam_size=4), **kw))
    with pytest.raises(ValueError):
        crit.beam_search(torch.zeros(2, 5, crit.N + 1), lexicon=lex)
    for kw in (dict(lexicon=lex), dict(lexicon=lex, lm=lm), dict(word_bonus=0.5), dict(lm=lm), dict(lm_eos=False)):
        with pytest.raises(ValueError):  # (they belong to errors()' beam search)
            crit.errors(x, [[1], [2]], None, **kw)
    # no frame and no device: the empty sequence (no word either), scored by </s> alone where there is an LM
    empty = [[[], []]] * 2
    none = torch.zeros(2, 0, crit.N)
    hyps, scores = crit.beam_search(none, nbest=2, return_scores=True, lexicon=lex, word_bonus=3.0, length_bonus=1.0)
    assert [[h.tolist() for h in u] for u in hyps] == empty and scores.tolist() == [[0.0, -math.inf]] * 2
    hyps, scores = crit.beam_search(none, nbest=2, return_scores=True, lexicon=lex, lm=lm, lm_weight=0.5, word_bonus=3.0)
    assert [[h.tolist() for h in u] for u in hyps] == empty
    assert scores.tolist() == [[0.5 * lm.step(lm.start, len(WORDS) + 1)[0], -math.inf]] * 2 and math.isfinite(scores[0, 0])
    _, scores = crit.beam_search(none, return_scores=True, lexicon=lex, lm=lm, lm_eos=False)
    assert scores.tolist() == [[0.0]] * 2
    mute = _word_lm(WORDS, tmp_path, eos=False, seed=4)
    assert mute.score([]) == -math.inf
    for w in (0.0, -1.0, 0.5):
        _, scores = crit.beam_search(none, nbest=2, return_scores=True, lexicon=lex, lm=mute, lm_weight=w)
        assert scores.tolist() == [[-math.inf, -math.inf]] * 2
    assert crit.beam_search(torch.zeros(0, 5, crit.N), lexicon=lex, lm=lm) == []
    # without a lexicon the call is what it was
    hyps, scores = crit.beam_search(none, nbest=2, return_scores=True)
    assert [[h.tolist() for h in u] for u in hyps] == empty and scores.tolist() == [[0.0, 0.0]] * 2


# ------------------------------------------------------------------------------------------------------------------
# the reference against all frame paths, walked through the lexicon and re-scored by rule 6
# ------------------------------------------------------------------------------------------------------------------
# (C, T, garbage, {raw spelling: word id}): C^T frame paths can be enumerated, and few enough raw sequences walk the
# lexicon that W = 64 drops none (checked per case against a search that cannot drop any)
SETUPS = [
    (4, 5, 3, {(1, 2): 0, (2,): 1, (1, 0): 2}),          # r0, a, b, G: "ab", "b", "aa"
    (4, 6, None, {(1, 3): 0, (2, 0, 3): 1, (2, 3): 2}),  # r0, a, b, |: "a|", "bb|", "b|"
    (4, 5, 3, {(2,): 0, (1, 0, 2): 1}),                  # a one-label word beside a doubled letter
    (3, 7, 2, {(1, 0): 0}),                              # r0, a, G: "aa" alone
    (3, 8, None, {(1, 2): 0, (2, 0): 1}),                # r0, a, b: "ab", "bb"
    (3, 7, 2, {(1,): 0}),                                # a single one-label word around the garbage
]
CONSTANTS = [(0.7, 1.3, -0.4), (-0.5, -0.8, 0.6), (1.0, 0.0, 0.0)]


@pytest.mark.parametrize("eos", [True, False])
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("setup", range(len(SETUPS)))
def test_reference_equals_rescored_brute_force_when_nothing_is_pruned(setup, order, eos):
    C, T, garbage, lexicon = SETUPS[setup]
    V = len(lexicon)
    words = [f"w{v}" for v in range(V)]
    for k, (alpha, omega, beta) in enumerate(CONSTANTS):
        rs = np.random.RandomState(24000 + 100 * setup + 10 * order + 2 * k + int(eos))
        x = (rs.randn(T, C) * (1.0, 3.0)[k % 2]).astype(np.float32)
        Wt = (0.5 * rs.randn(C + 1, C)).astype(np.float32)
        lm = LR.ArpaLM(LR.random_arpa(rs, words, order, 0.6), words, V) if order else None
        want = AX.brute_force(x, Wt, lexicon, garbage, lm, alpha, omega, beta, eos)
        assert len(want) >= 2
        hyps, margin, _ = AX.beam_search(x, Wt, 64, C, 3, lexicon, garbage, lm, alpha, omega, beta, eos)
        every, _, _ = AX.beam_search(x, Wt, 10 ** 6, C, 3, lexicon, garbage, lm, alpha, omega, beta, eos)
        assert hyps == every  # (nothing was pruned)
        assert margin > 1e-9
        for r, (seq, score) in enumerate(hyps):
            if r < len(want):
                assert seq == want[r][0], (r, hyps, want[:4])
                assert abs(score - want[r][1]) <= 1e-9, (r, score, want[r][1])
            else:
                assert (seq, score) == ((), NEG)
        logz = AR.denominator(x, Wt)
        norm, _, _ = AX.beam_search(x, Wt, 64, C, 3, lexicon, garbage, lm, alpha, omega, beta, eos, logz=logz)
        assert abs(norm[0][1] - (hyps[0][1] - logz)) <= 1e-12


def test_reference_without_a_constraint_is_the_asg_reference():
    """a lexicon of all one-label words over every class admits every raw sequence: with neither LM nor bonus the
    search with a lexicon is the plain ASG search; and the garbage is transparent: with it taken out of the lexicon the
    same sequences come back"""
    rs = np.random.RandomState(79)
    C = 5
    full = {(c,): c for c in range(C)}
    rest = {(c,): c for c in range(C - 1)}
    for _ in range(6):
        x = rs.randn(20, C).astype(np.float32)
        Wt = (0.5 * rs.randn(C + 1, C)).astype(np.float32)
        plain, _, _ = AR.beam_search(x, Wt, 8, 3, 4)
        for lexicon, garbage in ((full, None), (rest, C - 1)):
            got, _, _ = AX.beam_search(x, Wt, 8, 3, 4, lexicon, garbage, None, 1.0, 0.0, 0.0, True)
            assert [h for h, _ in got] == [h for h, _ in plain]
            assert all(abs(a - b) <= 1e-12 for (_, a), (_, b) in zip(got, plain))
    # no frame: the empty sequence with </s> alone
    assert AX.beam_search(np.zeros((0, C), np.float32), np.zeros((C + 1, C), np.float32), 4, 3, 2, full, None, None, 0.5, 9.0,
                          9.0, True)[0] == [((), 0.0), ((), NEG)]
    assert AX.raw_lexicon([[0, 0, 3], [1, 0, 0, 0, 3]], 1) == {(1, 0, 4): 0, (2, 1, 0, 1, 4): 1}
    assert AX.raw_lexicon([[0, 0, 3], [1, 0, 0, 0, 3]], 2) == {(2, 0, 5): 0, (3, 2, 1, 5): 1}
