"""CPU tests (-m "not gpu") of the CTC beam search with an n-gram LM (csrc/beam_kernels.hip: wfl_ctc_beam_search_lm,
include/wfl.h): the header declares the new entry points and libwfl.so exports them, every bad argument is refused
before a launch, the module checks its LM arguments without a device -- and the Python restatement the GPU tests compare
against (tests/beam_lm_reference.py) is itself pinned to a brute-force enumeration of all alignments, re-scored by the
LM and the length bonus, where nothing is pruned.  No device compute here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import beam_lm_reference as LR
import beam_reference as R
from gtn_applications_amd import _native as N
from gtn_applications_amd.lm import NGramLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wfl_ngram_lm_check", "wfl_ctc_beam_search_lm")


def test_header_declares_and_library_exports_the_lm_entry_points():
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(wfl_[a-z0-9_]+)\s*\(", code))
    fresh = ctypes.CDLL(N.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(fresh, name), name
        assert name in N.EXPORTED_SYMBOLS, name
    assert "typedef struct wfl_ngram_lm" in code and "WFL_NGRAM_LM_MAX_BACKOFF 8" in code
    assert ctypes.sizeof(N.NgramLm) == 16 + 16 + 6 * ctypes.sizeof(ctypes.c_void_p)
    # the operators of the search take the model in their plan: a DeviceLm or None
    assert hasattr(N.ops, "DeviceLm")
    assert all(f"{arg}: " in N.ops.BeamPlan.__init__.__doc__ for arg in ("lm", "lm_weight", "length_bonus", "score_eos"))
    for fn in ("ctc_beam_search", "ctc_beam_search_errors"):
        assert hasattr(N.ops, fn), fn
        assert "plan: " in getattr(N.ops, fn).__doc__, fn


GOOD = dict(B=2, T=5, C=7, blank=0, beam=4, K=3, nbest=2)
BAD = [dict(B=0), dict(T=0), dict(C=0), dict(blank=-1), dict(blank=7), dict(beam=0), dict(beam=65), dict(K=0), dict(K=8),
       dict(nbest=0), dict(nbest=5)]


def _search(a, null=None, lm_change=None, weight=0.8, bonus=0.5, no_lm=False, capacity=None):
    """wfl_ctc_beam_search_lm with host addresses that are never touched: every case here is refused before a launch"""
    n = max(1, a["B"] * a["nbest"])
    bufs = dict(x=np.zeros(8, np.float32), ws=np.zeros(8, np.int64), out=np.zeros(8, np.int32),
                offs=np.zeros(n + 1, np.int64), scores=np.zeros(n, np.float64))
    p = {k: (None if k == null else v.ctypes.data) for k, v in bufs.items()}
    arrays = dict(arc_ptr=np.zeros(2, np.int32), arc_label=np.zeros(1, np.int32), arc_next=np.zeros(1, np.int32),
                  arc_w=np.zeros(1, np.float64), bo_next=np.zeros(1, np.int32), bo_w=np.zeros(1, np.float64))
    f = dict(num_states=1, num_arcs=0, start=0, reserved=0, step_min=-1.0, step_max=0.0,
             **{k: v.ctypes.data for k, v in arrays.items()})
    f.update(lm_change or {})
    lm = N.NgramLm(*(f[k] for k in ("num_states", "num_arcs", "start", "reserved", "step_min", "step_max", "arc_ptr",
                                    "arc_label", "arc_next", "arc_w", "bo_next", "bo_w")))
    cap = a["B"] * a["nbest"] * a["T"] if capacity is None else capacity
    return N.lib.wfl_ctc_beam_search_lm(p["x"], None, a["B"], a["T"], a["C"], a["blank"], a["beam"], a["K"], a["nbest"], 1,
                                        None if no_lm else ctypes.byref(lm), weight, bonus, 1, p["ws"], p["out"], cap,
                                        p["offs"], p["scores"], None)


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_search_arguments_are_refused_without_a_device(change):
    assert _search(dict(GOOD, **change)) == N.ERR_INVALID
    assert "ctc_beam_search_lm" in N.last_error()


@pytest.mark.parametrize("null", ["x", "ws", "out", "offs", "scores"])
def test_null_pointers_are_refused(null):
    assert _search(GOOD, null=null) == N.ERR_INVALID


@pytest.mark.parametrize("change", [dict(num_states=0), dict(num_arcs=-1), dict(start=-1), dict(start=1), dict(arc_ptr=None),
                                    dict(arc_label=None), dict(arc_next=None), dict(arc_w=None), dict(bo_next=None),
                                    dict(bo_w=None), dict(step_min=math.nan), dict(step_max=math.nan)],
                         ids=lambda c: ",".join(c))
def test_a_bad_lm_struct_is_refused(change):
    assert _search(GOOD, lm_change=change) == N.ERR_INVALID


def test_null_lm_weights_that_are_not_finite_small_capacity_and_too_many_classes():
    assert _search(GOOD, no_lm=True) == N.ERR_INVALID
    for w, b in ((math.nan, 0.0), (math.inf, 0.0), (-math.inf, 0.0), (1.0, math.nan), (1.0, math.inf)):
        assert _search(GOOD, weight=w, bonus=b) == N.ERR_INVALID
        assert "finite" in N.last_error()
    assert _search(GOOD, capacity=GOOD["B"] * GOOD["nbest"] * GOOD["T"] - 1) == N.ERR_INVALID
    assert _search(dict(GOOD, C=16385)) == N.ERR_UNSUPPORTED


def _small_lm(C, blank, tmp_path):
    tokens = [f"t{i}" for i in range(C - 1)]
    p = tmp_path / "small.arpa"
    p.write_text(LR.random_arpa(np.random.RandomState(3), tokens, 2, 0.5))
    return NGramLM.from_arpa(str(p), tokens, blank)


def test_module_refuses_bad_lm_arguments_before_a_device_is_needed(tmp_path):
    from gtn_applications_amd import engine as E
    from gtn_applications_amd.criterions.ctc import CTC

    crit = CTC(blank=0, use_pt=False)
    x = torch.zeros(2, 5, 7)
    lm = _small_lm(7, 0, tmp_path)
    bad = (dict(lm="lm.arpa"), dict(lm=object()), dict(lm=_small_lm(6, 0, tmp_path)), dict(lm=_small_lm(7, 6, tmp_path)),
           dict(lm=lm, lm_weight=math.nan), dict(lm=lm, lm_weight=math.inf), dict(lm=lm, length_bonus=-math.inf),
           dict(lm=lm, lm_weight="1"), dict(lm=lm, lm_eos=1), dict(lm_weight=0.5), dict(length_bonus=0.1),
           dict(lm_eos=False), dict(lm=lm, beam_size=65), dict(lm=lm, nbest=17))
    for kw in bad:
        with pytest.raises(ValueError):
            crit.beam_search(x, **kw)
        if "nbest" not in kw:
            with pytest.raises(ValueError):
                crit.errors(x, [[1], [2]], None, **dict(dict(beam_size=4), **kw))
    with pytest.raises(ValueError):  # the LM arguments of errors() belong to its beam search
        crit.errors(x, [[1], [2]], None, lm=lm)
    # the defaults without an lm are today's call: accepted by the check, like every finite pair with one
    def lm_fields(lm, lm_weight, length_bonus, lm_eos):
        plan = E.BeamPlan.checked(7, 0, 4, None, 1, lm, lm_weight, length_bonus, lm_eos, None, 0.0, "t")
        return plan.lm, plan.lm_weight, plan.length_bonus, plan.lm_eos

    assert lm_fields(None, 1.0, 0.0, True) == (None, 1.0, 0.0, True)
    assert lm_fields(lm, 0, -3, False) == (lm, 0.0, -3.0, False)
    # numpy numbers and one-element tensors are numbers too (a sweep over weights); strings and bools are not
    got = lm_fields(lm, np.float32(0.5), torch.tensor(-1.5), np.bool_(False))
    assert got == (lm, 0.5, -1.5, False) and all(type(v) is t for v, t in zip(got[1:], (float, float, bool)))
    for kw in (dict(lm_weight=np.float64(math.nan)), dict(length_bonus=torch.tensor(math.inf)), dict(lm_weight=True),
               dict(lm_weight=np.ones(2)), dict(length_bonus=b"1")):
        with pytest.raises(ValueError):
            crit.beam_search(x, lm=lm, **kw)
    # no frame and no device: the empty sequence, scored by </s> alone
    hyps, scores = crit.beam_search(torch.zeros(2, 0, 7), nbest=2, return_scores=True, lm=lm, lm_weight=0.5)
    assert [[h.tolist() for h in u] for u in hyps] == [[[], []]] * 2
    assert scores.tolist() == [[0.5 * lm.score([]), -math.inf]] * 2
    # an LM without </s> from the start state: that rank is dropped whatever the weight (never 0 * -inf or -w * -inf)
    p = tmp_path / "no_eos.arpa"
    p.write_text(LR.random_arpa(np.random.RandomState(4), [f"t{i}" for i in range(6)], 2, 0.5, eos=False))
    mute = NGramLM.from_arpa(str(p), [f"t{i}" for i in range(6)], 0)
    assert mute.score([]) == -math.inf
    for w in (0.0, -1.0, 0.5):
        hyps, scores = crit.beam_search(torch.zeros(2, 0, 7), nbest=2, return_scores=True, lm=mute, lm_weight=w)
        assert [[h.tolist() for h in u] for u in hyps] == [[[], []]] * 2
        assert scores.tolist() == [[-math.inf, -math.inf]] * 2
    _, scores = crit.beam_search(torch.zeros(2, 0, 7), return_scores=True, lm=mute, lm_weight=0.0, lm_eos=False)
    assert scores.tolist() == [[0.0]] * 2


# ------------------------------------------------------------------------------------------------------------------
# the reference against all alignments, re-scored
# ------------------------------------------------------------------------------------------------------------------
# (C, T) at which fewer than 64 label sequences exist -- 1 + (C-1) + ... + (C-1)^T -- so that W = 64 drops none of them
SIZES = [(2, 6), (3, 5), (4, 3), (3, 4), (4, 2), (2, 3)]
CASES = [(order, alpha, beta, eos) for order in (2, 3) for alpha in (0.0, 0.7, 2.0) for beta in (0.0, 1.1, -0.5)
         for eos in (True, False)]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("order,alpha,beta,eos", CASES)
def test_reference_equals_rescored_brute_force_when_nothing_is_pruned(order, alpha, beta, eos, seed):
    n = CASES.index((order, alpha, beta, eos))
    C, T = SIZES[(n + 3 * seed) % len(SIZES)]
    assert sum((C - 1) ** k for k in range(T + 1)) <= 64
    blank = (n + seed) % C
    rs = np.random.RandomState(10000 + 2 * n + seed)
    x = (rs.randn(T, C) * (1.0, 3.0)[seed]).astype(np.float32)
    tokens = [f"t{i}" for i in range(C - 1)]
    lm = LR.ArpaLM(LR.random_arpa(rs, tokens, order, 0.6), tokens, blank)
    want = []
    for seq, mass in R.brute_force(x, blank):
        l = lm.score(seq, eos=eos)
        if l != R.NEG:
            want.append((mass + alpha * l + beta * len(seq), seq))
    want.sort(key=lambda e: (-e[0], e[1]))
    hyps, margin, _ = LR.beam_search(x, blank, 64, C, 64, lm, alpha, beta, eos)
    assert margin > 1e-9
    assert len(want) >= 2
    for r, (seq, score) in enumerate(hyps):
        if r < len(want):
            assert seq == want[r][1], (r, hyps[:4], want[:4])
            assert abs(score - want[r][0]) <= 1e-12, (r, score, want[r][0])
        else:
            assert (seq, score) == ((), R.NEG)
    lse = sum(R.row_lse(R.clean(row)) for row in x)
    norm, _, _ = LR.beam_search(x, blank, 64, C, 64, lm, alpha, beta, eos, normalize=True)
    assert abs(norm[0][1] - (hyps[0][1] - lse)) <= 1e-12


def test_reference_without_lm_terms_is_the_plain_reference_and_the_lm_changes_the_best():
    rs = np.random.RandomState(77)
    C, blank = 5, 2
    tokens = [f"t{i}" for i in range(C - 1)]
    lm = LR.ArpaLM(LR.random_arpa(rs, tokens, 3, 1.0), tokens, blank)  # (every gram: no token is ever impossible)
    changed = 0
    for _ in range(10):
        x = rs.randn(20, C).astype(np.float32)
        plain, _, _ = R.beam_search(x, blank, 8, 3, 4)
        off, _, _ = LR.beam_search(x, blank, 8, 3, 4, lm, 0.0, 0.0, False)
        assert [h for h, _ in off] == [h for h, _ in plain]
        assert all(abs(a - b) <= 1e-12 for (_, a), (_, b) in zip(off, plain))
        on, _, _ = LR.beam_search(x, blank, 8, 3, 4, lm, 0.8, 0.5, True)
        changed += on[0][0] != plain[0][0]
    assert changed >= 5
    # no frame: the empty sequence with </s> alone
    assert LR.beam_search(np.zeros((0, C), np.float32), blank, 4, 3, 2, lm, 0.5, 9.0, True)[0] == \
        [((), 0.5 * lm.score((), eos=True)), ((), R.NEG)]
    assert LR.beam_search(np.zeros((0, C), np.float32), blank, 4, 3, 2, lm, 0.5, 9.0, False)[0] == [((), 0.0), ((), R.NEG)]
