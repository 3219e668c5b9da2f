"""CPU tests (-m "not gpu") of the Transducer prefix beam search (csrc/beam_kernels.hip, include/wfl.h, DESIGN.md
section 22): the header declares the two entry points and libwfl.so exports them, every bad argument is refused before a
device is needed, the workspace grows with its arguments, engine.TransducerBeamPlan refuses what it should, the module
refuses the ambiguous token graphs and the transition models it has no dense operands for and answers batches without
a frame on the host -- and the Python restatement the GPU tests compare against (tests/transducer_beam_reference.py) is
itself pinned to an enumeration of all C^T frame paths where nothing is pruned, and to the oracle's loss.  No device
compute here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import transducer_beam_reference as R
from gtn_applications_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wfl_transducer_beam_workspace", "wfl_transducer_beam_search")
NEG = R.NEG


def test_header_declares_and_library_exports_the_transducer_beam_entry_points():
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
    from gtn_applications_amd.criterions.transducer import Transducer

    assert callable(E.transducer_beam_search) and callable(M.transducer_beam_search_errors) and callable(Transducer.beam_search)
    for fn in ("transducer_beam_search", "transducer_beam_search_errors"):
        assert hasattr(N.ops, fn), fn


def _workspace(B, T, C, W, K, nbest):
    cap, ws = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = N.lib.wfl_transducer_beam_workspace(B, T, C, W, K, nbest, ctypes.byref(cap), ctypes.byref(ws))
    return rc, cap.value, ws.value


# (B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize) around a good call
GOOD = dict(B=2, T=5, C=7, blank=6, forced=1, beam=4, K=3, nbest=2, normalize=1)
BAD = [dict(B=0), dict(B=-1), dict(T=0), dict(C=0), dict(beam=0), dict(beam=65), dict(K=0), dict(K=8),
       dict(C=100, K=65), dict(nbest=0), dict(nbest=5), dict(beam=64, nbest=65), dict(blank=-1), dict(blank=7),
       dict(forced=2), dict(forced=-1)]


def _search(a, null=None, capacity=None):
    """wfl_transducer_beam_search with host addresses that are never touched: every case here is refused before a launch"""
    n = max(1, a["B"] * a["nbest"])
    bufs = dict(x=np.zeros(8, np.float32), Wt=np.zeros(8, np.float32), logz=np.zeros(8, np.float32), ws=np.zeros(8, np.int64),
                out=np.zeros(8, np.int32), offs=np.zeros(n + 1, np.int64), scores=np.zeros(n, np.float64))
    p = {k: (None if k == null else v.ctypes.data) for k, v in bufs.items()}
    cap = a["B"] * a["nbest"] * a["T"] if capacity is None else capacity
    return N.lib.wfl_transducer_beam_search(p["x"], p["Wt"], p["logz"], a["B"], a["T"], a["C"], a["blank"], a["forced"], a["beam"],
                                            a["K"], a["nbest"], a["normalize"], p["ws"], p["out"], cap, p["offs"], p["scores"], None)


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_arguments_are_refused_without_a_device(change):
    a = dict(GOOD, **change)
    if "C" in change and "blank" not in change:
        a["blank"] = 0
    assert _search(a) == N.ERR_INVALID
    assert N.last_error()
    if "blank" not in change and "forced" not in change:  # (the workspace call takes everything but these two)
        assert _workspace(a["B"], a["T"], a["C"], a["beam"], a["K"], a["nbest"])[0] == N.ERR_INVALID


@pytest.mark.parametrize("null", ["x", "ws", "out", "offs", "scores"])
def test_null_pointers_are_refused(null):
    assert _search(GOOD, null=null) == N.ERR_INVALID
    assert _search(dict(GOOD, forced=0), null=null) == N.ERR_INVALID


def test_the_normaliser_belongs_to_the_transitions():
    assert _search(GOOD, null="logz") == N.ERR_INVALID  # (transitions and normalize, but no logz)
    assert _search(GOOD, null="Wt") == N.ERR_INVALID    # (logz without transitions)


def test_small_capacity_null_results_and_too_many_classes():
    assert _workspace(2, 5, 7, 4, 3, 2)[:2] == (N.WFL_OK, 2 * 2 * 5)
    assert _search(GOOD, capacity=2 * 2 * 5 - 1) == N.ERR_INVALID
    ws = ctypes.c_int64()
    assert N.lib.wfl_transducer_beam_workspace(2, 5, 7, 4, 3, 2, None, ctypes.byref(ws)) == N.ERR_INVALID
    assert N.lib.wfl_transducer_beam_workspace(2, 5, 7, 4, 3, 2, ctypes.byref(ws), None) == N.ERR_INVALID
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
    rc, cap, ws = _workspace(128, 1000, 101, 64, 64, 64)
    assert rc == N.WFL_OK and cap == 128 * 64 * 1000
    assert ws >= 128 * 1000 * (64 * 8 + 65 * 8)
    # the search may be the CTC one: its workspace is enough
    cap2, ws2 = ctypes.c_int64(), ctypes.c_int64()
    assert N.lib.wfl_ctc_beam_workspace(128, 1000, 101, 64, 64, 64, ctypes.byref(cap2), ctypes.byref(ws2)) == N.WFL_OK
    assert ws >= ws2.value and cap == cap2.value


def test_plan_refuses_what_it_should():
    from gtn_applications_amd import engine as E

    P = E.TransducerBeamPlan
    assert P.checked(100, 99, False, 16, None, 1, "t") == (100, 99, False, 16, 32, 1)
    assert P.checked(7, np.int64(0), np.bool_(True), np.int64(4), np.int32(7), 4, "t") == (7, 0, True, 4, 7, 4)
    assert P.checked(16384, 5, 1, 64, 64, 64, "t") == (16384, 5, True, 64, 64, 64)
    assert P._fields == ("C", "blank", "forced", "beam", "classes_per_frame", "nbest")
    # what AsgBeamPlan refuses
    for args in ((7, 0, None, 1), (7, 65, None, 1), (7, 2.0, None, 1), (7, True, None, 1), (7, "4", None, 1), (7, None, None, 1),
                 (7, 4, 0, 1), (7, 4, 8, 1), (100, 4, 65, 1), (7, 4, True, 1), (7, 4, 3.0, 1),
                 (7, 4, None, 0), (7, 4, None, 5), (7, 4, None, True), (7, 4, None, 1.0),
                 (0, 4, None, 1), (16385, 4, None, 1)):
        with pytest.raises(ValueError):
            E.AsgBeamPlan.checked(*args, "t")
        with pytest.raises(ValueError):
            P.checked(args[0], 0, False, *args[1:], "t")
    # a bad blank, a bad forced
    for blank in (-1, 7, 1.0, True, None, "0"):
        with pytest.raises(ValueError):
            P.checked(7, blank, False, 4, None, 1, "t")
    for forced in (2, -1, None, "no", 1.0):
        with pytest.raises(ValueError):
            P.checked(7, 6, forced, 4, None, 1, "t")
    # BeamPlan and AsgBeamPlan stay what they were: this plan is a class of its own
    assert not issubclass(P, E.BeamPlan) and not issubclass(P, E.AsgBeamPlan)
    assert len(E.BeamPlan._fields) == 11 and E.AsgBeamPlan._fields == ("C", "beam", "classes_per_frame", "nbest")


TOKENS = ["a", "b", "c"]
G2I = {"a": 0, "b": 1, "c": 2}


def _crit(**kw):
    from gtn_applications_amd.criterions.transducer import Transducer

    return Transducer(TOKENS, G2I, **kw)


def test_module_refuses_the_ambiguous_token_graphs_and_general_transition_models():
    from gtn_applications_amd import graph as G
    from gtn_applications_amd import transitions_builder as TB

    x = torch.zeros(2, 5, 4)
    with pytest.raises(NotImplementedError, match="ambiguous"):
        _crit(blank="none").beam_search(torch.zeros(2, 5, 3))
    with pytest.raises(NotImplementedError, match="ambiguous"):
        _crit(blank="optional", allow_repeats=True).beam_search(x)
    with pytest.raises(NotImplementedError, match="ambiguous"):
        _crit(blank="optional", allow_repeats=True).errors(x, [[0], [1]], None, beam_size=4)
    crit = _crit(blank="optional", allow_repeats=False)
    g = G.Graph(False)  # a hand-made token graph: none of make_token_graph's four
    g.add_node(True, True)
    g.add_node(False, True)
    g.add_arc(0, 1, 0)
    g.add_arc(1, 0, 1)
    crit.tokens = g
    with pytest.raises(NotImplementedError, match="ambiguous"):
        crit.beam_search(x)
    # a back-off transition graph is neither the unigram nor the bigram model
    lines = [["a", "b", "a", "c"], ["b", "b", "c"], ["c", "a"]]
    trans = TB.build_transitions(lines, TOKENS, (0, 0), blank="optional", self_loops=True)
    for kw in (dict(blank="optional", allow_repeats=False), dict(blank="forced")):
        with pytest.raises(NotImplementedError, match="transition model"):
            _crit(transitions=trans, **kw).beam_search(x)
    # both searched graphs, every searched model: nothing raised before the device is asked for (T == 0: never)
    for kw in (dict(blank="optional", allow_repeats=False), dict(blank="forced")):
        for ngram in (0, 1, 2):
            assert len(_crit(ngram=ngram, **kw).beam_search(torch.zeros(2, 0, 4))) == 2


def test_module_refuses_bad_arguments_and_answers_no_frames_without_a_device():
    for kw0 in (dict(blank="optional", allow_repeats=False), dict(blank="forced")):
        crit = _crit(**kw0)  # 3 tokens + the blank
        x = torch.zeros(2, 5, 4)
        for kw in (dict(beam_size=0), dict(beam_size=65), dict(beam_size=2.0), dict(beam_size=True), dict(classes_per_frame=0),
                   dict(classes_per_frame=5), dict(nbest=0), dict(beam_size=4, nbest=5)):
            with pytest.raises(ValueError):
                crit.beam_search(x, **kw)
        with pytest.raises(ValueError):
            crit.beam_search(torch.zeros(2, 5, 3))  # (a wrong class count)
        with pytest.raises(ValueError):
            crit.beam_search(torch.zeros(2, 5, 5))
        with pytest.raises(ValueError):
            crit.beam_search(torch.zeros(2, 5, 4, dtype=torch.int64))
        with pytest.raises(ValueError):
            crit.beam_search(torch.zeros(5, 4))
        with pytest.raises(ValueError):
            crit.errors(x, [[1], [2]], None, beam_size=65)
        with pytest.raises(ValueError):
            crit.errors(x, [[1], [2]], None, classes_per_frame=3)  # (needs a beam_size)
        # no frames: on the host, in viterbi()'s dtype
        hyps = crit.beam_search(torch.zeros(3, 0, 4))
        assert len(hyps) == 3 and all(h.dtype == torch.int32 and h.numel() == 0 for h in hyps)
        hyps, scores = crit.beam_search(torch.zeros(3, 0, 4), beam_size=4, nbest=2, return_scores=True)
        assert [len(h) for h in hyps] == [2, 2, 2] and all(r.numel() == 0 for h in hyps for r in h)
        assert scores.dtype == torch.float64 and scores.shape == (3, 2) and bool((scores == 0).all())
        hyps, scores = crit.beam_search(torch.zeros(0, 5, 4), nbest=1, return_scores=True)
        assert hyps == [] and scores.shape == (0, 1)
    from gtn_applications_amd import engine as E

    hyps, scores = E.transducer_beam_search(torch.zeros(2, 0, 7), torch.zeros(8, 7), 6, True, nbest=3, beam_size=3)
    assert [len(h) for h in hyps] == [3, 3] and scores.shape == (2, 3) and bool((scores == 0).all())
    hyps, scores = E.transducer_beam_search(torch.zeros(2, 0, 7), None, 0)
    assert [len(h) for h in hyps] == [1, 1]
    with pytest.raises(ValueError):
        E.transducer_beam_search(torch.zeros(2, 0, 7), torch.zeros(7, 7), 6)
    with pytest.raises(ValueError):
        E.transducer_beam_search(torch.zeros(2, 0, 7), None, 7)


# ------------------------------------------------------------------------------------------------------------------
# the reference against all frame paths
# ------------------------------------------------------------------------------------------------------------------
CASES = ([(3, T, scale) for T in (1, 2, 3, 4, 5) for scale in (1.0, 3.0)] +
         [(2, T, 1.0) for T in range(1, 8)] + [(4, 4, 1.0), (4, 4, 3.0)])


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
@pytest.mark.parametrize("with_Wt", [False, True], ids=["plain", "Wt"])
@pytest.mark.parametrize("C,T,scale", CASES)
def test_reference_equals_brute_force_when_nothing_is_pruned(C, T, scale, with_Wt, forced):
    """W = 64, K = C, the blank at every position.  Nothing is pruned: every frame has at most 64 entries (C = 3, T = 5:
    the sequences over two tokens with an alignment in five frames), which the comparison of EVERY sequence's mass with
    the enumeration shows -- a pruned prefix would be missing from the result or short of mass."""
    for blank in range(C):
        rs = np.random.RandomState(100000 * C + 1000 * T + 100 * blank + 10 * int(scale) + int(with_Wt))
        x = (rs.randn(T, C) * scale).astype(np.float32)
        Wt = (0.5 * rs.randn(C + 1, C)).astype(np.float32) if with_Wt else None
        want = R.brute_force(x, Wt, blank, forced)
        hyps, margin, _ = R.beam_search(x, Wt, blank, forced, 64, C, 64)
        got = [(s, v) for s, v in hyps if v > NEG]
        assert len(got) == len(want) <= 64
        assert [s for s, _ in got] == [s for s, _ in want], (blank, got[:4], want[:4])
        for (s, v), (_, m) in zip(got, want):
            assert abs(v - m) <= 1e-9, (blank, s, v, m)
        assert all(hyps[r] == ((), NEG) for r in range(len(got), 64))
        assert margin > 1e-9  # (no entry is ever dropped: what is left is the distance between the returned ranks)
        # the masses of all sequences add up to the normaliser where every path is accepted
        norm = R.normaliser(x, Wt)
        total = NEG
        for _, m in want:
            total = R.lae(total, m)
        if not forced:
            assert abs(total - norm) <= 1e-9
        else:
            assert total <= norm + 1e-12
        normed, _, _ = R.beam_search(x, Wt, blank, forced, 64, C, 3, norm=norm)
        assert abs(normed[0][1] - (hyps[0][1] - norm)) <= 1e-12


def test_without_transitions_the_optional_topology_is_the_ctc_reference():
    import beam_reference as CR

    rs = np.random.RandomState(3)
    for T, C, W, K in ((30, 5, 4, 3), (20, 8, 8, 8), (1, 2, 1, 2)):
        for blank in (0, C - 1):
            x = rs.randn(T, C).astype(np.float32)
            assert R.beam_search(x, None, blank, False, W, K, min(3, W)) == CR.beam_search(x, blank, W, K, min(3, W))
            zero = np.zeros((C + 1, C), np.float32)
            assert R.beam_search(x, zero, blank, False, W, K, min(3, W)) == CR.beam_search(x, blank, W, K, min(3, W))


# ------------------------------------------------------------------------------------------------------------------
# the reference against the oracle's loss
# ------------------------------------------------------------------------------------------------------------------
def _operands(x, params, ngram):
    """(emissions, Wt or None) as the criterion's routes form them (_unigram_route, _bigram_dense_operands), float64"""
    C = x.shape[1]
    if ngram == 0:
        return x, None
    if ngram == 1:
        return x + params, None
    n1 = C + C * C
    Wt = np.concatenate([params[:C].reshape(1, C), params[C:n1].reshape(C, C).T], axis=0)
    xd = x.copy()
    xd[-1] += params[n1 + 1:]
    return xd, Wt


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_reference_scores_are_minus_the_oracles_loss(ngram, forced):
    from oracle import criteria as OC

    kw = dict(blank="forced") if forced else dict(blank="optional", allow_repeats=False)
    orc = OC.TransducerOracle(["a", "b"], {"a": 0, "b": 1}, ngram=ngram, **kw)
    rs = np.random.RandomState(10 * ngram + int(forced))
    worst, checked = 0.0, 0
    for T in (1, 3, 4, 5):
        x = rs.randn(T, 3)
        params = None
        if ngram > 0:
            params = 0.5 * rs.randn(len(orc.transition_params))
            orc.transition_params = params
        xe, Wt = _operands(x, params, ngram)
        norm = R.normaliser(xe, Wt)
        hyps, _, _ = R.beam_search(xe, Wt, 2, forced, 64, 3, 64, norm=norm)
        for seq, score in hyps:
            if not seq or score == NEG:
                continue
            want = -orc.loss(x[None], [list(seq)])[0]
            worst, checked = max(worst, abs(score - want)), checked + 1
            assert abs(score - want) <= 1e-9, (T, seq, score, want)
    print(f"ngram {ngram} forced {forced}: {checked} sequences, worst |score + loss| = {worst:.3g}")
    assert checked >= 10


# ------------------------------------------------------------------------------------------------------------------
# named cases of the rules
# ------------------------------------------------------------------------------------------------------------------
def test_forced_no_token_in_frame_zero():
    # class 0 towers in frame 0, the blank is 2: the optional topology starts with it, the forced one cannot
    x = np.array([[9.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], np.float32)
    opt, _, _ = R.beam_search(x, None, 2, False, 64, 3, 64)
    assert opt[0][0] == (0,)
    hyps, _, _ = R.beam_search(x, None, 2, True, 64, 3, 64)
    want = dict(R.brute_force(x, None, 2, True))
    got = {s: v for s, v in hyps if v > NEG}
    assert set(got) == set(want) == {(), (0,), (1,)}  # (three frames: blank, token or blank, blank)
    assert all(abs(got[s] - want[s]) <= 1e-12 for s in want)
    one, _, _ = R.beam_search(x[:1], None, 2, True, 64, 3, 3)
    assert one == [((), 0.0), ((), NEG), ((), NEG)]  # (a single frame: the blank alone)


def test_forced_a_hypothesis_that_ends_in_a_token_is_not_returned_and_the_ranks_close_up():
    # the last frame forbids the blank behind token 0 only: (0,) has pb = -inf at the end, (1,) and () remain
    x = np.zeros((3, 3), np.float32)
    x[1] = [1.0, 0.5, -1.0]
    Wt = np.zeros((4, 3), np.float32)
    Wt[1 + 2][0] = -np.inf  # 0 -> blank forbidden
    hyps, _, _ = R.beam_search(x, Wt, 2, True, 64, 3, 4)
    assert [s for s, v in hyps if v > NEG] == [(1,), ()]
    assert hyps[2:] == [((), NEG), ((), NEG)]
    assert hyps[0][1] == pytest.approx(0.5) and hyps[1][1] == pytest.approx(-1.0)
    # in the optional topology the same hypothesis counts through pnb and comes first
    opt, _, _ = R.beam_search(x, Wt, 2, False, 64, 3, 64)
    assert (0,) in [s for s, v in opt if v > NEG]


def test_a_forbidden_transition_drops_the_entries_that_cross_it():
    x = np.zeros((3, 3), np.float32)
    Wt = np.zeros((4, 3), np.float32)
    Wt[1 + 1][0] = -np.inf   # 0 -> 1 forbidden
    Wt[1 + 0][2] = np.nan    # blank -> 0 forbidden (a NaN counts as -inf): token 0 only from the start or behind 1
    for forced in (False, True):
        hyps, _, _ = R.beam_search(x, Wt, 2, forced, 64, 3, 64)
        want = dict(R.brute_force(x, Wt, 2, forced))
        got = {s: v for s, v in hyps if v > NEG}
        assert set(got) == set(want)
        assert all(abs(got[s] - want[s]) <= 1e-12 for s in want)
        assert (0, 0) not in got  # (a repeated token needs the blank between, and blank -> 0 is forbidden)
        if forced:
            assert all(0 not in s for s in got)  # (every token follows the blank)
        else:
            assert (0,) in got and (1, 0) in got
            assert abs(got[(0, 1)] - 0.0) <= 1e-12  # (0 -> 1 is forbidden: the one alignment is 0, blank, 1)


def test_frame_zero_uses_the_start_row_and_the_empty_prefix_the_blank_row_behind_it():
    x = np.zeros((2, 3), np.float32)
    Wt = np.zeros((4, 3), np.float32)
    Wt[0] = [1.0, 2.0, 4.0]       # start -> 0, 1, blank
    Wt[1 + 0][2] = 8.0            # blank -> 0
    Wt[1 + 2][2] = 16.0           # blank -> blank
    hyps, _, _ = R.beam_search(x, Wt, 2, False, 64, 3, 64)
    got = {s: v for s, v in hyps if v > NEG}
    assert got[()] == 4.0 + 16.0              # start -> blank, blank -> blank
    assert got[(1,)] == pytest.approx(R.lae(R.lae(2.0, 2.0), 4.0))  # 1 1 | 1 blank | blank 1
    assert got[(0,)] == pytest.approx(R.lae(R.lae(1.0, 1.0), 4.0 + 8.0))  # 0 0 | 0 blank | blank 0 (over the blank's row)
    one, _, _ = R.beam_search(x[:1], Wt, 2, False, 64, 3, 3)
    assert one == [((), 4.0), ((1,), 2.0), ((0,), 1.0)]  # (a single frame: row 0 alone)


def test_reference_merges_and_degenerate_frames():
    rs = np.random.RandomState(5)
    x = rs.randn(30, 4).astype(np.float32)
    Wt = (0.5 * rs.randn(5, 4)).astype(np.float32)
    for forced in (False, True):
        _, _, merges = R.beam_search(x, Wt, 3, forced, 8, 3, 3)
        assert merges >= 20
    # a frame without a finite score: nothing survives
    y = x.copy()
    y[7] = -np.inf
    assert R.beam_search(y, Wt, 3, False, 8, 3, 3)[0] == [((), NEG)] * 3
    y[7] = np.nan
    assert R.beam_search(y, Wt, 3, True, 8, 3, 3)[0] == [((), NEG)] * 3
    assert R.beam_search(np.zeros((0, 4), np.float32), Wt, 3, False, 4, 4, 2)[0] == [((), 0.0), ((), NEG)]
