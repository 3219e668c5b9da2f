"""CPU tests (-m "not gpu") of the CTC prefix beam search (csrc/beam_kernels.hip, include/wfl.h): the header declares
the entry points and libwfl.so exports them, every bad argument is refused before a device is needed, the workspace grows
with its arguments -- and the Python restatement the GPU tests compare against (tests/beam_reference.py) is itself pinned
to a brute-force enumeration of all alignments where nothing is pruned.  No device compute here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import beam_reference as R
from gtn_applications_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wfl_ctc_beam_workspace", "wfl_ctc_beam_search")


def test_header_declares_and_library_exports_the_beam_entry_points():
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(wfl_[a-z0-9_]+)\s*\(", code))
    fresh = ctypes.CDLL(N.LIB_PATH)  # (a handle of its own: what the library exports, not what the table declared)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(fresh, name), name
        assert name in N.EXPORTED_SYMBOLS, name
    from gtn_applications_amd import engine as E
    from gtn_applications_amd import metrics as M

    assert callable(E.ctc_beam_search) and callable(M.beam_search_errors)
    for fn in ("ctc_beam_search", "ctc_beam_search_errors"):
        assert hasattr(N.ops, fn), fn


def _workspace(B, T, C, W, K, nbest):
    cap, ws = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = N.lib.wfl_ctc_beam_workspace(B, T, C, W, K, nbest, ctypes.byref(cap), ctypes.byref(ws))
    return rc, cap.value, ws.value


# (B, T, C, blank, beam, classes_per_frame, nbest) around a good call
GOOD = dict(B=2, T=5, C=7, blank=0, beam=4, K=3, nbest=2)
BAD = [dict(B=0), dict(B=-1), dict(T=0), dict(C=0), dict(blank=-1), dict(blank=7), dict(beam=0), dict(beam=65),
       dict(K=0), dict(K=8), dict(C=100, K=65), dict(nbest=0), dict(nbest=5), dict(beam=64, nbest=65)]


def _search(a, null=None, capacity=None):
    """wfl_ctc_beam_search with host addresses that are never touched: every case here is refused before a launch"""
    n = max(1, a["B"] * a["nbest"])
    bufs = dict(x=np.zeros(8, np.float32), ws=np.zeros(8, np.int64), out=np.zeros(8, np.int32),
                offs=np.zeros(n + 1, np.int64), scores=np.zeros(n, np.float64))
    p = {k: (None if k == null else v.ctypes.data) for k, v in bufs.items()}
    cap = a["B"] * a["nbest"] * a["T"] if capacity is None else capacity
    return N.lib.wfl_ctc_beam_search(p["x"], None, a["B"], a["T"], a["C"], a["blank"], a["beam"], a["K"], a["nbest"], 1,
                                     p["ws"], p["out"], cap, p["offs"], p["scores"], None)


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_arguments_are_refused_without_a_device(change):
    a = dict(GOOD, **change)
    assert _search(a) == N.ERR_INVALID
    assert N.last_error()
    if "blank" not in change:  # (the workspace call takes everything but the blank)
        assert _workspace(a["B"], a["T"], a["C"], a["beam"], a["K"], a["nbest"])[0] == N.ERR_INVALID


@pytest.mark.parametrize("null", ["x", "ws", "out", "offs", "scores"])
def test_null_pointers_are_refused(null):
    assert _search(GOOD, null=null) == N.ERR_INVALID


def test_small_capacity_null_results_and_too_many_classes():
    need = GOOD["B"] * GOOD["nbest"] * GOOD["T"]
    assert _workspace(2, 5, 7, 4, 3, 2)[:2] == (N.WFL_OK, need)
    assert _search(GOOD, capacity=need - 1) == N.ERR_INVALID
    ws = ctypes.c_int64()
    assert N.lib.wfl_ctc_beam_workspace(2, 5, 7, 4, 3, 2, None, ctypes.byref(ws)) == N.ERR_INVALID
    assert N.lib.wfl_ctc_beam_workspace(2, 5, 7, 4, 3, 2, ctypes.byref(ws), None) == N.ERR_INVALID
    assert _workspace(1, 2, 16384, 4, 64, 1)[0] == N.WFL_OK
    assert _workspace(1, 2, 16385, 4, 64, 1)[0] == N.ERR_UNSUPPORTED
    assert _search(dict(GOOD, C=16385)) == N.ERR_UNSUPPORTED


def test_workspace_grows_with_every_argument():
    base = dict(B=3, T=40, W=8, K=6)
    size = lambda **kw: _workspace(kw["B"], kw["T"], 100, kw["W"], kw["K"], 1)
    for name, values in (("B", (1, 2, 3, 50, 128)), ("T", (1, 2, 39, 40, 1000)), ("W", (1, 2, 8, 63, 64)),
                         ("K", (1, 2, 6, 63, 64))):
        got = [size(**dict(base, **{name: v})) for v in values]
        assert all(rc == N.WFL_OK for rc, _, _ in got), (name, got)
        sizes = [ws for _, _, ws in got]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (name, sizes)
        assert all(ws % 16 == 0 for ws in sizes)
    # the arena [T W] records and the candidates [T (K+1)] of every utterance fit
    rc, cap, ws = _workspace(128, 1000, 100, 64, 64, 64)
    assert rc == N.WFL_OK and cap == 128 * 64 * 1000
    assert ws >= 128 * 1000 * (64 * 8 + 65 * 8 + 4)


def test_module_refuses_bad_arguments_before_a_device_is_needed():
    from gtn_applications_amd.criterions.ctc import CTC

    crit = CTC(blank=0, use_pt=False)
    x = torch.zeros(2, 5, 7)
    for kw in (dict(beam_size=0), dict(beam_size=65), dict(beam_size=2.0), dict(classes_per_frame=0),
               dict(classes_per_frame=8), dict(nbest=0), dict(beam_size=4, nbest=5), dict(input_lengths=[1]),
               dict(input_lengths=[0, 5]), dict(input_lengths=[1, 6])):
        with pytest.raises(ValueError):
            crit.beam_search(x, **kw)
    with pytest.raises(ValueError):
        CTC(blank=7, use_pt=False).beam_search(x)
    with pytest.raises(ValueError):
        crit.beam_search(torch.zeros(2, 5, 7, dtype=torch.int64))
    with pytest.raises(ValueError):
        crit.beam_search(torch.zeros(5, 7))
    with pytest.raises(ValueError):
        crit.errors(x, [[1], [2]], None, beam_size=65)


# ------------------------------------------------------------------------------------------------------------------
# the reference against all alignments
# ------------------------------------------------------------------------------------------------------------------
CASES = [(T, blank, seed) for T in (1, 2, 3, 4, 5) for blank in (0, 1, 2) for seed in (0, 1)]


@pytest.mark.parametrize("T,blank,seed", CASES)
def test_reference_equals_brute_force_when_nothing_is_pruned(T, blank, seed):
    """C = 3, W = 64, K = C: at most 1 + 2 + ... + 2^5 = 63 prefixes exist, none is dropped, so the 3-best of the search
    are the 3 label sequences of largest total mass over all 3^T alignments"""
    rs = np.random.RandomState(1000 * T + 10 * blank + seed)
    x = (rs.randn(T, 3) * (1.0, 3.0)[seed]).astype(np.float32)
    want = R.brute_force(x, blank)
    hyps, margin, _ = R.beam_search(x, blank, 64, 3, 3)
    assert margin > 1e-9  # (no entry is ever dropped; what is left is the distance between the returned ranks)
    assert len(hyps) == 3
    for r, (seq, score) in enumerate(hyps):
        if r < len(want):
            assert seq == want[r][0], (r, hyps, want[:4])
            assert abs(score - want[r][1]) <= 1e-9, (r, score, want[r][1])
        else:
            assert (seq, score) == ((), R.NEG)
    total = R.NEG
    for _, s in want:
        total = R.lae(total, s)
    lse = sum(R.row_lse(R.clean(row)) for row in x)
    assert abs(total - lse) <= 1e-9  # (the masses of all sequences add up to the normaliser)
    norm, _, _ = R.beam_search(x, blank, 64, 3, 3, normalize=True)
    assert abs(norm[0][1] - (hyps[0][1] - lse)) <= 1e-12


def test_reference_merges_and_degenerate_frames():
    rs = np.random.RandomState(5)
    x = rs.randn(30, 4).astype(np.float32)
    _, _, merges = R.beam_search(x, 0, 8, 2, 3)
    assert merges >= 20
    # a frame without a finite score: nothing survives
    x[7] = -np.inf
    hyps, _, _ = R.beam_search(x, 0, 8, 2, 3)
    assert hyps == [((), R.NEG)] * 3
    # NaN counts as -inf; a last frame where only the blank is finite keeps every prefix and adds its score
    y = rs.randn(6, 4).astype(np.float32)
    z = np.concatenate([y, np.array([[np.nan, -np.inf, 0.5, np.nan]], np.float32)])
    a, _, _ = R.beam_search(y, 2, 8, 4, 3)
    b, _, _ = R.beam_search(z, 2, 8, 4, 3)
    assert [s for s, _ in a] == [s for s, _ in b]
    assert all(abs(sa + 0.5 - sb) <= 1e-12 for (_, sa), (_, sb) in zip(a, b))
    assert R.beam_search(np.zeros((0, 4), np.float32), 0, 4, 4, 2)[0] == [((), 0.0), ((), R.NEG)]
