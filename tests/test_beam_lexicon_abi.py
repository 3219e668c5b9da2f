"""CPU tests (-m "not gpu") of the CTC beam search with a lexicon and a word-level LM (csrc/beam_kernels.hip:
wfl_ctc_beam_search_lexicon, include/wfl.h): the header declares the new entry points and libwfl.so exports them, every
bad argument is refused before a launch, the module checks its lexicon arguments without a device -- and the Python
restatement the GPU tests compare against (tests/beam_lexicon_reference.py) is itself pinned to a brute-force
enumeration of all alignments, kept where they segment into words and re-scored by the word LM and the two bonuses,
where nothing is pruned.  No device compute here."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import beam_lexicon_reference as XR
import beam_lm_reference as LR
import beam_reference as R
from gtn_applications_amd import _native as N
from gtn_applications_amd.lexicon import Lexicon
from gtn_applications_amd.lm import NGramLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wfl_lexicon_check", "wfl_ctc_beam_search_lexicon")


def test_header_declares_and_library_exports_the_lexicon_entry_points():
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(wfl_[a-z0-9_]+)\s*\(", code))
    fresh = ctypes.CDLL(N.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(fresh, name), name
        assert name in N.EXPORTED_SYMBOLS, name
    assert "typedef struct wfl_lexicon" in code
    struct = code[code.index("typedef struct wfl_lexicon"):code.index("} wfl_lexicon;")]
    assert re.findall(r"\b(\w+)\s*[;,]", struct) == ["num_nodes", "num_arcs", "num_words", "reserved", "arc_ptr", "arc_label",
                                                      "arc_next"]
    assert [n for n, _ in N.Lexicon._fields_] == ["num_nodes", "num_arcs", "num_words", "reserved", "arc_ptr", "arc_label",
                                                 "arc_next"]
    # the operators of the search take the lexicon in their plan: a DeviceLexicon or None
    assert hasattr(N.ops, "DeviceLexicon")
    assert "lexicon: " in N.ops.BeamPlan.__init__.__doc__ and "word_bonus: " in N.ops.BeamPlan.__init__.__doc__
    for fn in ("ctc_beam_search", "ctc_beam_search_errors"):
        assert "plan: " in getattr(N.ops, fn).__doc__, fn


GOOD = dict(B=2, T=5, C=7, blank=0, beam=4, K=3, nbest=2)
BAD = [dict(B=0), dict(T=0), dict(C=0), dict(blank=-1), dict(blank=7), dict(beam=0), dict(beam=65), dict(K=0), dict(K=8),
       dict(nbest=0), dict(nbest=5)]


def _search(a, null=None, lex_change=None, lm_change=None, weight=0.8, word=0.3, bonus=0.5, no_lex=False, with_lm=True,
            capacity=None):
    """wfl_ctc_beam_search_lexicon with host addresses that are never touched: every case here is refused before a
    launch"""
    n = max(1, a["B"] * a["nbest"])
    bufs = dict(x=np.zeros(8, np.float32), ws=np.zeros(8, np.int64), out=np.zeros(8, np.int32),
                offs=np.zeros(n + 1, np.int64), scores=np.zeros(n, np.float64))
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
    cap = a["B"] * a["nbest"] * a["T"] if capacity is None else capacity
    return N.lib.wfl_ctc_beam_search_lexicon(p["x"], None, a["B"], a["T"], a["C"], a["blank"], a["beam"], a["K"], a["nbest"], 1,
                                             None if no_lex else ctypes.byref(lex), ctypes.byref(lm) if with_lm else None,
                                             weight, word, bonus, 1, p["ws"], p["out"], cap, p["offs"], p["scores"], None)


@pytest.mark.parametrize("with_lm", [True, False])
@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_search_arguments_are_refused_without_a_device(change, with_lm):
    assert _search(dict(GOOD, **change), with_lm=with_lm) == N.ERR_INVALID
    assert "ctc_beam_search_lexicon" in N.last_error()


@pytest.mark.parametrize("null", ["x", "ws", "out", "offs", "scores"])
def test_null_pointers_are_refused(null):
    assert _search(GOOD, null=null) == N.ERR_INVALID
    assert _search(GOOD, null=null, with_lm=False) == N.ERR_INVALID


@pytest.mark.parametrize("change", [dict(num_nodes=0), dict(num_arcs=0), dict(num_words=0), dict(num_nodes=-1),
                                    dict(num_words=2 ** 31 - 1),
                                    dict(arc_ptr=None), dict(arc_label=None), dict(arc_next=None)], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
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
    assert _search(GOOD, capacity=GOOD["B"] * GOOD["nbest"] * GOOD["T"] - 1) == N.ERR_INVALID
    assert _search(dict(GOOD, C=16385)) == N.ERR_UNSUPPORTED


def _word_lm(words, tmp_path, blank=None, eos=True, seed=3):
    p = tmp_path / f"words{len(words)}_{blank}_{eos}.arpa"
    p.write_text(LR.random_arpa(np.random.RandomState(seed), words, 2, 0.5, eos=eos))
    return NGramLM.from_arpa(str(p), words, len(words) if blank is None else blank)


def test_module_refuses_bad_lexicon_arguments_before_a_device_is_needed(tmp_path):
    from gtn_applications_amd.criterions.ctc import CTC

    crit = CTC(blank=0, use_pt=False)
    x = torch.zeros(2, 5, 7)
    words = ["w0", "w1", "w2"]
    lex = Lexicon([(1, 6), (2, 3, 6), (2, 2, 6)], 7, 0, words=words)
    lm = _word_lm(words, tmp_path)
    token_lm = _word_lm([f"t{i}" for i in range(6)], tmp_path, blank=0)  # (an LM over the emissions' classes)
    bad = (dict(lexicon="words.txt"), dict(lexicon=object()), dict(lexicon=[(1, 6)]),
           dict(lexicon=Lexicon([(1, 5)], 6, 0)), dict(lexicon=Lexicon([(1, 5)], 7, 6)),
           dict(word_bonus=0.5), dict(word_bonus=-1), dict(lexicon=lex, word_bonus=math.nan), dict(lexicon=lex, word_bonus=math.inf),
           dict(lexicon=lex, word_bonus="1"), dict(lexicon=lex, word_bonus=True), dict(lexicon=lex, lm=token_lm),
           dict(lexicon=lex, lm=_word_lm(words + ["w3"], tmp_path)), dict(lexicon=lex, lm=_word_lm(words, tmp_path, blank=1)),
           dict(lexicon=lex, lm="lm.arpa"), dict(lexicon=lex, lm_weight=0.5), dict(lexicon=lex, lm_eos=False),
           dict(lexicon=lex, lm=lm, lm_weight=math.nan), dict(lexicon=lex, length_bonus=math.inf),
           dict(lexicon=lex, lm=lm, lm_eos=1), dict(lexicon=lex, beam_size=65), dict(lexicon=lex, nbest=17))
    for kw in bad:
        with pytest.raises(ValueError):
            crit.beam_search(x, **kw)
        if "nbest" not in kw:
            with pytest.raises(ValueError):
                crit.errors(x, [[1], [2]], None, **dict(dict(beam_size=4), **kw))
    for kw in (dict(lexicon=lex), dict(lexicon=lex, lm=lm), dict(word_bonus=0.5)):  # they belong to errors()' beam search
        with pytest.raises(ValueError):
            crit.errors(x, [[1], [2]], None, **kw)
    # no frame and no device: the empty sequence (no word either), scored by </s> alone where there is an LM
    empty = [[[], []]] * 2
    hyps, scores = crit.beam_search(torch.zeros(2, 0, 7), nbest=2, return_scores=True, lexicon=lex, word_bonus=3.0, length_bonus=1.0)
    assert [[h.tolist() for h in u] for u in hyps] == empty and scores.tolist() == [[0.0, -math.inf]] * 2
    hyps, scores = crit.beam_search(torch.zeros(2, 0, 7), nbest=2, return_scores=True, lexicon=lex, lm=lm, lm_weight=0.5,
                                    word_bonus=3.0)
    assert [[h.tolist() for h in u] for u in hyps] == empty
    assert scores.tolist() == [[0.5 * lm.step(lm.start, 4)[0], -math.inf]] * 2 and math.isfinite(scores[0, 0])
    _, scores = crit.beam_search(torch.zeros(2, 0, 7), return_scores=True, lexicon=lex, lm=lm, lm_eos=False)
    assert scores.tolist() == [[0.0]] * 2
    mute = _word_lm(words, tmp_path, eos=False, seed=4)
    assert mute.score([]) == -math.inf
    for w in (0.0, -1.0, 0.5):
        _, scores = crit.beam_search(torch.zeros(2, 0, 7), nbest=2, return_scores=True, lexicon=lex, lm=mute, lm_weight=w)
        assert scores.tolist() == [[-math.inf, -math.inf]] * 2
    assert crit.beam_search(torch.zeros(0, 5, 7), lexicon=lex, lm=lm) == []


# ------------------------------------------------------------------------------------------------------------------
# the reference against all alignments, segmented into words and re-scored
# ------------------------------------------------------------------------------------------------------------------
# (C, T, words, longest spelling without the separator, whether the last non-blank class is a separator): small enough to enumerate C^T alignments, and with fewer
# than 64 label sequences inside the lexicon (asserted per case), so that W = 64 drops none of them
SIZES = [(4, 4, 3, 2, True), (3, 5, 2, 3, False), (4, 3, 5, 3, False), (4, 6, 2, 1, True), (3, 5, 2, 2, False), (4, 3, 4, 2, False)]
CASES = [(order, alpha, omega, beta, eos) for order in (0, 1, 2) for alpha in (0.7, -0.5)
         for omega, beta in ((0.0, 0.0), (1.3, -0.4), (-0.8, 0.6)) for eos in (True, False)]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("order,alpha,omega,beta,eos", CASES)
def test_reference_equals_rescored_brute_force_when_nothing_is_pruned(order, alpha, omega, beta, eos, seed):
    n = CASES.index((order, alpha, omega, beta, eos))
    C, T, V, longest, sep = SIZES[(n + 3 * seed) % len(SIZES)]
    blank = (n + seed) % C
    sep = max(c for c in range(C) if c != blank) if sep else None
    rs = np.random.RandomState(20000 + 2 * n + seed)
    x = (rs.randn(T, C) * (1.0, 3.0)[seed]).astype(np.float32)
    lexicon = XR.random_lexicon(rs, C, blank, V, longest, sep)
    assert XR.is_prefix_free(lexicon) and len(lexicon) == V
    letters = [c for c in range(C) if c != blank]
    reachable = sum(1 for k in range(T + 1) for s in itertools.product(letters, repeat=k) if XR.segment(lexicon, s) is not None)
    assert reachable <= 64
    words = [f"w{v}" for v in range(V)]
    lm = LR.ArpaLM(LR.random_arpa(rs, words, order, 0.6), words, V) if order else None
    want = []
    for seq, mass in R.brute_force(x, blank):
        at = XR.segment(lexicon, seq)
        if at is None or at[1]:
            continue  # (outside the lexicon, or it ends inside a word)
        l = (lm.score(at[0], eos=eos) if lm else 0.0)
        if l != R.NEG:
            want.append((mass + alpha * l + omega * len(at[0]) + beta * len(seq), seq))
    want.sort(key=lambda e: (-e[0], e[1]))
    hyps, margin, _ = XR.beam_search(x, blank, 64, C, 64, lexicon, lm, alpha, omega, beta, eos)
    assert margin > 1e-9
    assert len(want) >= 2
    for r, (seq, score) in enumerate(hyps):
        if r < len(want):
            assert seq == want[r][1], (r, hyps[:4], want[:4])
            assert abs(score - want[r][0]) <= 1e-9, (r, score, want[r][0])
        else:
            assert (seq, score) == ((), R.NEG)
    lse = sum(R.row_lse(R.clean(row)) for row in x)
    norm, _, _ = XR.beam_search(x, blank, 64, C, 64, lexicon, lm, alpha, omega, beta, eos, normalize=True)
    assert abs(norm[0][1] - (hyps[0][1] - lse)) <= 1e-12


def test_reference_with_every_sequence_a_word_sequence_is_the_lm_reference():
    """a lexicon of all one-label words admits every label sequence, word v = the v-th non-blank class: the lexicon
    search with a word LM is then the token LM search, and with neither LM nor bonus the plain one"""
    rs = np.random.RandomState(78)
    C, blank = 5, 2
    classes = [c for c in range(C) if c != blank]
    lexicon = {(c,): v for v, c in enumerate(classes)}
    tokens = [f"t{i}" for i in range(C - 1)]
    text = LR.random_arpa(rs, tokens, 3, 0.8)
    token_lm, word_lm = LR.ArpaLM(text, tokens, blank), LR.ArpaLM(text, tokens, C - 1)
    for _ in range(6):
        x = rs.randn(20, C).astype(np.float32)
        plain, _, _ = R.beam_search(x, blank, 8, 3, 4)
        off, _, _ = XR.beam_search(x, blank, 8, 3, 4, lexicon, None, 1.0, 0.0, 0.0, True)
        assert [h for h, _ in off] == [h for h, _ in plain]
        assert all(abs(a - b) <= 1e-12 for (_, a), (_, b) in zip(off, plain))
        want, _, _ = LR.beam_search(x, blank, 8, 3, 4, token_lm, 0.8, 0.5, True)
        got, _, _ = XR.beam_search(x, blank, 8, 3, 4, lexicon, word_lm, 0.8, 0.2, 0.3, True)  # (0.2 + 0.3 per label)
        assert [h for h, _ in got] == [h for h, _ in want]
        assert all(abs(a - b) <= 1e-12 for (_, a), (_, b) in zip(got, want))
    # no frame: the empty sequence with </s> alone
    assert XR.beam_search(np.zeros((0, C), np.float32), blank, 4, 3, 2, lexicon, word_lm, 0.5, 9.0, 9.0, True)[0] == \
        [((), 0.5 * word_lm.score((), eos=True)), ((), R.NEG)]
    assert XR.beam_search(np.zeros((0, C), np.float32), blank, 4, 3, 2, lexicon, None, 0.5, 9.0, 9.0, True)[0] == \
        [((), 0.0), ((), R.NEG)]
