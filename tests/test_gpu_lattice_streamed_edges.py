"""The streamed lattice sweeps at the limits their kernels are built around (-m gpu): csrc/lattice_streamed.h and its host
side in lattice_kernels.hip (stream_mode, lattice_forward_streamed, lattice_grad_streamed), driven through the engine layer
as tests/test_gpu_lattice_edges.py drives the tuned launches -- with that file's generator and harness (_lean_utt, _hub,
_with_arcs, _eps_case, _no_path_case, _inputs, _reference, _run, _grad_kernels, _viterbi, _first_arc_best_path), against
the float64 recurrences of oracle/recurrences.py and _maxplus_eps.

  A. acceptors that are streamed because of their size, at small T
     1. the dispatch boundary: two acceptors 900 arcs apart, the smaller on the tuned launches, the larger streamed
     2. state vectors in LDS (mode 1) and in the alpha / beta arrays (mode 2) on both sides of the 160 KiB crossing, state
        ids above 32 767 (bit 31 of the packed arc words), the documented maximum of 65 535 states, 65 536 refused
     3. relax_wave / relax_eps_wave: labelled in- and out-degree 32, 33, 64, 257 and 300, epsilon in- and out-degree 32, 33
        and 70 on closure levels of their own, a level with light and heavy states, tying tropical scores whose tying arcs
        sit in different lanes and in the first and the second trip of 256 arcs
     4. 1 001 labels (8 rows per chunk), a label with one arc and one with several hundred, the fused log-softmax gradient,
        accumulation; 520 and 700 labels (14 and 10 rows per chunk)
     5. mixed batches, a shared acceptor, utterances without a path, NaN / -inf inputs
     6. frame counts around the chunk, both semirings
  B. the streamed kernels forced onto small acceptors (WFL_LATTICE_STREAMED=1 / 2, one child process each): state counts
     around the thread count, epsilon cases, mixed batches, no path, the gradient's tile heights 1, 2, 3, 15 and 16 with a
     last partial tile (dx also against the tuned path's dx: close, atol 2e-6), twenty-one full chunks in both semirings,
     large row maxima (the first-frame shift of a chunk in mode 2)

Every case asserts that the launch it means to test ran: wfl_lattice_diagnostics out[8] rises by one per forward and one per
gradient call, out[9] by one per forward call whose state vectors lived in global memory -- the mode is restated here
(_stream_config) as _config restates chain_config.  Streamed sweeps are log-domain: lattice_formats says 0.

Bars: the project's own, through check() of tests/test_gpu_configs.py -- scores and dx at close()'s 1e-4 relative + 1e-5,
dW at 5e-5 absolute (scales S_X, S_W), Viterbi scores within 1e-5 |best| + 1e-4 and exact on integer scores.  Records:
lattice_streamed_edges_<family>_<quantity>.  Nothing here reads the reference project."""
import contextlib
import ctypes
import functools
import json
import os
import re
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_lattice_edges as ED  # noqa: E402
from lattice_workspace import tuned_workspace as _tuned_workspace  # noqa: E402
from test_gpu_configs import STATS, _gpu_and_stats, check  # noqa: E402,F401
from test_gpu_lattice_edges import (NEG, S_W, S_X, _degrees, _dW_want, _grad_kernels, _inputs, _lean_utt,  # noqa: E402
                                    _no_path_case, _pack, _reference, _run, _utt, _viterbi, _with_arcs)
from test_gpu_lattice_streamed import _workspace  # noqa: E402
from test_gpu_parity import close, dev  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
FORCED = os.environ.get("WFL_LATTICE_STREAMED")  # "1" / "2" in the children of part B


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


# =================================================================================================
# which launch ran
# =================================================================================================
def _counters():
    """wfl_lattice_diagnostics (out[8], out[9]): streamed launches (sweeps and gradients) and, of the sweeps, those whose
    state vectors lived in global memory, so far in this process"""
    from gtn_applications_amd import _native as N

    out = (ctypes.c_uint64 * 10)()
    N.check(N.lib.wfl_lattice_diagnostics(out, 10))
    return int(out[8]), int(out[9])


def _stream_config(d, T=0, B=1):
    """stream_rpc, stream_lds_bytes / stream_mode and the tile height of lattice_grad_streamed restated: (emission rows per
    chunk, 1: state vectors in LDS / 2: in the alpha / beta arrays, frames per gradient tile)"""
    K = max(1, d.max_labels)
    R = max(2, min(16, 1024 * 8 // K) & ~1)
    lds = 2 * R * d.max_labels * 4 + 256 + 16 * d.max_states
    mode = 1 if FORCED != "2" and lds <= 160 * 1024 else 2
    return R, mode, max(1, min(16, T * B // 512, 16384 // K))


@contextlib.contextmanager
def _launches(forwards, grads, desc=None, mode=None):
    """the calls inside were streamed: out[8] rises by forwards + grads; out[9] by the forward calls if the descriptor's
    mode (restated) is 2, else not at all; mode: what the case is about"""
    s0, g0 = _counters()
    holder = []
    yield holder
    torch.cuda.synchronize()
    s1, g1 = _counters()
    assert s1 - s0 == forwards + grads, (s1 - s0, forwards, grads)
    d = desc if desc is not None else holder[0]
    got_mode = _stream_config(d)[1]
    assert mode is None or got_mode == mode, (got_mode, mode, d.max_states, d.max_labels)
    assert g1 - g0 == (forwards if got_mode == 2 else 0), (g1 - g0, got_mode, forwards)


@contextlib.contextmanager
def _harness(fmt=0, tag=""):
    """test_gpu_lattice_edges' harness with this file's record names, and with the format it asserts where a case does not
    say one (0: streamed sweeps are log-domain)"""
    pre = "lattice_streamed_edges_" + (f"forced{FORCED}_" if FORCED else "") + tag
    old = ED._rec, ED.FMT
    ED._rec = lambda name, what: pre + re.sub(r"(_\d+)+$", "", name) + "_" + what
    ED.FMT = fmt
    try:
        yield
    finally:
        ED._rec, ED.FMT = old


def _streamed(name, utts, T, C, seed, mode=None, **kw):
    """_run with fmt=0, and the proof that its forward and gradient calls were streamed launches"""
    grads = 2 if kw.get("nopath") else 1  # (_run accumulates onto a seed as well beside utterances without a path)
    with _harness(), _launches(1, grads, mode=mode) as h:
        r = _run(name, utts, T, C, seed, fmt=0, **kw)
        h.append(r.pack.desc)
    return r


def _streamed_viterbi(utts, x, W, wids, mode=None, **kw):
    d = _pack(utts, x.shape[2], wids).desc
    with _launches(1, 0, desc=d, mode=mode):
        _viterbi(utts, x, W, wids, **kw)


# =================================================================================================
# the acceptors of part A (generated once)
# =================================================================================================
C12 = 12


@functools.lru_cache(maxsize=None)
def _case(which, C=C12, accept_near_starts=False):
    """a: 3 000 states, in-degree 8, mixed labels (23 972 arcs); b: 10 200 states, in-degree up to 3; c: 40 000 states,
    in-degree 2; d: 65 535 states, in-degree 2; e: 2 500 states, in-degree 8, 1 001 labels -- one label on a single arc,
    one on several hundred"""
    rs = np.random.RandomState({"a": 101, "b": 102, "c": 103, "d": 104, "e": 105}[which] + 1000 * accept_near_starts + C)
    if which == "a":
        extra = [q for q in range(3000) if q % 50 <= 12] if accept_near_starts else ()
        return _lean_utt(rs, 3000, C, 8, 8, False, exact=True, accept_extra=extra)
    if which == "b":
        return _lean_utt(rs, 10200, C, 3, 8, False)
    if which == "c":
        return _lean_utt(rs, 40000, C, 2, 8, False, exact=True)
    if which == "d":
        return _lean_utt(rs, 65535, C, 2, 8, False, exact=True)
    u = _lean_utt(rs, 2500, 1001, 8, 8, False, exact=True, n_labels=1001)
    lab = u.lab.copy()
    lab[np.flatnonzero(lab == 5)[1:]] = 0      # label 5 keeps one arc
    lab[rs.permutation(np.flatnonzero((lab != 5) & (lab != 1000)))[:400]] = 0  # label 0: several hundred
    for k in np.flatnonzero(np.bincount(lab, minlength=1001) == 0):  # (a label that lost its last arc gets one back)
        lab[int(np.flatnonzero(lab == 0)[-1])] = k
    cnt = np.bincount(lab, minlength=1001)
    assert cnt.min() >= 1 and cnt[5] == 1 and cnt[0] >= 300, (cnt.min(), cnt[5], cnt[0])
    return _utt(u.Q, u.src, u.dst, lab, u.start, u.accept)


def _labelled_hubs(u, rs, C, in_deg=(), out_deg=(), first=300, step=250):
    """u with states of exactly the labelled in-degrees of in_deg (arcs from earlier states; the hub accepts) and of the
    out-degrees of out_deg (the mirror image: arcs from one state to that many distinct later states, none of them a
    hub; the state is a start state): (utterance, in-hubs, out-hubs)"""
    hubs_in = [first + step * i for i in range(len(in_deg))]
    hubs_out = [first + step // 2 + step * i for i in range(len(out_deg))]
    ind, outd = np.bincount(u.dst, minlength=u.Q), np.bincount(u.src, minlength=u.Q)
    src, dst = [], []
    for q, n in zip(hubs_in, in_deg):
        m = n - int(ind[q])
        src += rs.randint(0, q, size=m).tolist()
        dst += [q] * m
    special = set(hubs_in) | set(hubs_out)
    outd = outd + np.bincount(np.asarray(src, np.int64), minlength=u.Q)
    for p, n in zip(hubs_out, out_deg):
        m = n - int(outd[p])
        later = np.array([q for q in range(p + 1, u.Q) if q not in special])
        src += [p] * m
        dst += rs.permutation(later)[:m].tolist()
    lab = rs.randint(C, size=len(src))
    v = _with_arcs(u, src, dst, lab, start=sorted(set(u.start) | set(hubs_out)), accept=sorted(set(u.accept) | set(hubs_in)))
    ind, outd = np.bincount(v.dst, minlength=v.Q), np.bincount(v.src, minlength=v.Q)
    assert ind[hubs_in].tolist() == list(in_deg) and outd[hubs_out].tolist() == list(out_deg)
    return v, hubs_in, hubs_out


@functools.lru_cache(maxsize=None)
def _hub_case():
    """case a with hubs of 300 and 33 in-arcs"""
    return _labelled_hubs(_case("a"), np.random.RandomState(111), C12, in_deg=(300, 33))[0]


# =================================================================================================
# A1. the dispatch boundary
# =================================================================================================
def _boundary_pair():
    """600 states, 512 labels, 9 700 and 10 600 arcs.  chain_lds_bytes (lattice_kernels.hip) of such a descriptor is
    8 arcs + 82 804 B (16 rows of 512 labels twice over: 65 536 B; 28 B per state; the rest 468 B) against 163 840:
    9 700 arcs fit with 3 436 B to spare, 10 600 are 3 764 B over."""
    rs = np.random.RandomState(120)
    C = 520
    base = _lean_utt(rs, 600, C, 16, 20, False, window=24, exact=True, n_labels=512)
    assert 9000 <= len(base.src) <= 9700 and len(set(base.lab.tolist())) == 512

    def grown(n):
        m = n - len(base.src)
        d = rs.randint(30, 600, size=m)
        return _with_arcs(base, d - 1 - rs.randint(24, size=m), d, base.lab[rs.randint(len(base.lab), size=m)])
    return grown(9700), grown(10600), C


def test_dispatch_boundary():
    """The smaller acceptor keeps the tuned launches (counter unchanged, format 1, the tuned workspace), the larger one is
    streamed (counter + 1 per call, format 0, a larger workspace); both meet the oracle in logZ, dx and dW.  dx and dW
    come from a call each: the tuned grad_kernel has no room for both at once this close to the boundary (DESIGN 3.2.1:
    the window that stays refused), and the streamed one is asked the same way."""
    from gtn_applications_amd import engine as E

    small, large, C = _boundary_pair()
    T = 20
    for name, u, streamed in (("boundary_tuned", small, False), ("boundary_streamed", large, True)):
        rs = np.random.RandomState(121)
        x, W, wids, _ = _inputs(rs, [u], T, C)
        ref = _reference([u], x, W, wids)
        coef, coef_w = (0.5 + rs.rand(1)).astype(np.float32), (0.5 + rs.rand(1)).astype(np.float32)
        pack = _pack([u], C, wids)
        assert pack.desc.max_labels == 512 and pack.desc.max_arcs == len(u.src)
        before = _counters()
        xd, Wd = dev(x), dev(W)
        st = E.lattice_forward(xd, pack, weights=Wd)
        dx, dW = torch.full_like(xd, float("nan")), torch.zeros_like(Wd)
        E.lattice_grad(st, dev(coef), dx=dx)
        E.lattice_grad(st, dev(coef), coef_w=dev(coef_w), dW=dW)
        torch.cuda.synchronize()
        after = _counters()
        rec = "lattice_streamed_edges_" + name + "_"
        check(rec + "logz", st.logz.cpu().numpy(), [ref[0][0]], S_X)
        check(rec + "dx", dx.cpu().numpy()[0], coef[0] * ref[0][1], S_X)
        check(rec + "dW", dW.cpu().numpy(), _dW_want([u], wids, ref, coef_w, len(W)), S_W)
        ws, tuned = _workspace(pack, T), _tuned_workspace(pack.desc, T)
        if streamed:
            assert (after[0] - before[0], after[1] - before[1]) == (3, 0) and _stream_config(pack.desc)[1] == 1
            assert E.lattice_formats(st).tolist() == [0]
            assert ws[0] == tuned[0] and ws[1] > tuned[1], (ws, tuned)
        else:
            assert after == before
            assert E.lattice_formats(st).tolist() == [1]
            assert ws == tuned, (ws, tuned)


# =================================================================================================
# A2. state vectors in LDS and in global memory; state ids that need 16 bits
# =================================================================================================
@pytest.mark.parametrize("Q,mode", [(10100, 1), (10200, 2)])
def test_mode_boundary(Q, mode):
    """2 R Kmax 4 + 256 + 16 Qmax against 160 KiB: with 12 labels (R = 16) 10 128 states are the last that fit"""
    rs = np.random.RandomState(130 + mode)
    u = _case("b") if Q == 10200 else _lean_utt(rs, Q, C12, 3, 8, False)
    r = _streamed(f"mode{mode}_boundary", [u], 12, C12, 131, mode=mode)
    assert _stream_config(r.pack.desc)[:2] == (16, mode) and r.pack.desc.max_states == Q
    # and over three chunks: in mode 2 the second and the third start from a stored frame that keeps the offset of the
    # chunk before (sub, shift)
    _streamed(f"mode{mode}_chunks", [u], 33, C12, 135, mode=mode)


def test_state_ids_above_32767():
    """case c, 40 000 states: other | slot << 16 and src | dst << 16 with bit 15 of a state id set (bit 31 of the word)"""
    u = _case("c")
    assert int(u.dst.max()) > 32767
    r = _streamed("states_40000", [u], 12, C12, 132, mode=2)
    _streamed_viterbi([u], r.x, r.W, r.wids, mode=2)


def test_the_documented_maximum_of_states():
    """case d, 65 535 states (README): accepted, and right"""
    u = _case("d")
    assert u.Q == 65535 and int(u.dst.max()) == 65534
    _streamed("states_65535", [u], 6, C12, 133, mode=2)


def test_one_state_more_is_refused_before_any_launch():
    from gtn_applications_amd import _native as N
    from gtn_applications_amd import engine as E

    rs = np.random.RandomState(134)
    u = _lean_utt(rs, 65536, C12, 2, 8, False, exact=True)
    x, W, wids, _ = _inputs(rs, [u], 6, C12)
    before = _counters()
    with pytest.raises(N.WflError, match="lattice too large"):
        E.lattice_forward(dev(x), _pack([u], C12, wids), weights=dev(W))
    torch.cuda.synchronize()
    assert _counters() == before


# =================================================================================================
# A3. heavy states: relax_wave, relax_eps_wave
# =================================================================================================
DEGREES = (32, 33, 64, 257, 300)


def test_heavy_labelled_in_and_out_degrees():
    """kStreamHeavy = 32: 32 arcs stay with one thread, 33 go to a wave, 64 fill its lanes once, 257 and 300 need a second
    trip of 256 -- as in-degrees (the forward sweep) and, mirrored, as out-degrees (the backward sweep)"""
    rs = np.random.RandomState(140)
    u, hin, hout = _labelled_hubs(_case("a"), rs, C12, DEGREES, DEGREES)
    assert _degrees(u) == (300, 300, 0, 0)
    r = _streamed("heavy_labelled", [u], 20, C12, 141, mode=1)
    _streamed_viterbi([u], r.x, r.W, r.wids, mode=1)


def _eps_hubs():
    """Case a with epsilon arcs p -> q, p < q, from even to odd states, so that only the hubs named here sit above level
    0 as sources.  Even hubs: o1 (level 0; 33 out), l1 (level 1; 3 in: a light state), h1 (level 1; 33 in, 70 out), h2
    (level 2; 70 in, one from h1; 33 out), h3 (level 3; 32 in, one from h2; 32 out): five levels, every heavy degree on
    a level of its own, level 1 with a heavy state and light ones (l1 and the targets of o1)."""
    rs = np.random.RandomState(142)
    u = _case("a")
    o1, l1, h1, h2, h3 = 300, 600, 1000, 1400, 1800
    special = {o1, l1, h1, h2, h3}
    es, ed = [], []

    def into(h, n, also=()):
        pool = np.array([p for p in range(max(0, h - 600), h, 2) if p not in special])
        s = list(also) + rs.permutation(pool)[:n - len(also)].tolist()
        es.extend(s), ed.extend([h] * n)

    def out_of(p, n):
        pool = np.arange(p + 1, min(u.Q, p + 801))
        pool = pool[pool % 2 == 1]
        es.extend([p] * n), ed.extend(rs.permutation(pool)[:n].tolist())
    out_of(o1, 33)
    into(l1, 3)
    into(h1, 33), out_of(h1, 69)        # (its seventieth goes to h2)
    into(h2, 70, [h1]), out_of(h2, 32)  # (its thirty-third goes to h3)
    into(h3, 32, [h2]), out_of(h3, 32)
    v = _with_arcs(u, es, ed, [-1] * len(es), accept=sorted(set(u.accept) | {h1, h2, h3}))
    e = v.lab < 0
    ein, eout = np.bincount(v.dst[e], minlength=v.Q), np.bincount(v.src[e], minlength=v.Q)
    assert ein[[l1, h1, h2, h3]].tolist() == [3, 33, 70, 32] and eout[[o1, h1, h2, h3]].tolist() == [33, 70, 33, 32]
    assert _degrees(v)[2:] == (70, 70)
    return v


def test_heavy_epsilon_in_and_out_degrees():
    u = _eps_hubs()

    def expect(pack):
        assert pack.desc.max_levels == 5 and pack.desc.max_eps == int((u.lab < 0).sum())
    r = _streamed("heavy_eps", [u], 20, C12, 143, mode=1, expect=expect)
    _streamed_viterbi([u], r.x, r.W, r.wids, mode=1)


def _tying_arcs(x, u, w, hub):
    """positions, within the hub's in-arcs in the caller's order, of the arcs that tie for the best score into the hub
    at the last frame (max-plus recurrence, exact on small integers)"""
    a = np.full(u.Q, NEG)
    a[u.start] = 0.0
    for t in range(x.shape[0] - 1):
        n = np.full(u.Q, NEG)
        np.maximum.at(n, u.dst, a[u.src] + w + x[t, u.lab])
        a = n
    k = np.flatnonzero(u.dst == hub)
    v = a[u.src[k]] + w[k] + x[-1, u.lab[k]]
    assert np.isfinite(v.max())
    return np.flatnonzero(v == v.max()).tolist()


@pytest.mark.parametrize("deg", [33, 64, 257, 300])
def test_tying_scores_into_a_heavy_state(deg):
    """Small integers everywhere; the hub is the only accept state, so the best path ends with the arc relax_wave picks
    among the hub's deg in-arcs in the last frame.  Those arcs are parallel: one source, one label, no learnable weight,
    graph weights of -1, -2 and -3 -- but 0 on the arcs number deg / 3, deg / 2 + 1 and deg - 1, which tie for the best
    (the oracle is asked first that exactly these do): three lanes, and from 257 arcs on both trips of 256.  The path
    must be the one of the documented tie rule (_first_arc_best_path): through arc deg / 3."""
    rs = np.random.RandomState(150 + deg)
    C, T, hub = 5, 10, 1500
    u = _lean_utt(rs, 3000, C, 8, 8, False, exact=True)
    keep = u.dst != hub
    best = [deg // 3, deg // 2 + 1, deg - 1]
    gw = -1.0 - rs.randint(3, size=deg)
    gw[best] = 0.0
    n = int(keep.sum())
    u = _utt(u.Q, np.concatenate([u.src[keep], np.full(deg, hub - 7)]), np.concatenate([u.dst[keep], np.full(deg, hub)]),
             np.concatenate([u.lab[keep], np.full(deg, 2)]), u.start, [hub], np.concatenate([np.zeros(n), gw]))
    assert _degrees(u)[0] == deg and len({b % 64 for b in best}) == 3
    x, W, wids, _ = _inputs(rs, [u], T, C)
    x = rs.randint(-2, 3, size=x.shape).astype(np.float32)
    W = rs.randint(-1, 2, size=W.shape).astype(np.float32)
    wids[0][n:] = -1
    w = u.gw.astype(np.float64) + np.where(wids[0] >= 0, W.astype(np.float64)[np.maximum(wids[0], 0)], 0.0)
    assert _tying_arcs(x[0].astype(np.float64), u, w, hub) == best
    _streamed_viterbi([u], x, W, wids, mode=1, exact=True)


# =================================================================================================
# A4. many labels: fewer than 16 rows per chunk
# =================================================================================================
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_1001_labels_through_every_gradient_call(fused, accumulate):
    """case e: R = 8, C = 1 001 >= 512 (stream_grad_rows' other form), tiles of at most 16 384 / 1 004 frames; dx alone, dx
    with dW, dW alone, optionally through the fused log-softmax and onto a seed"""
    u = _case("e")
    d = _pack([u], 1001, [np.full(len(u.src), -1, np.int32)]).desc
    assert _stream_config(d, 20, 1) == (8, 1, 1) and d.max_labels == 1004
    with _harness(), _launches(1, 3, desc=d, mode=1):
        a, b = _grad_kernels("labels_1001", [u], 20, 1001, 160 + 2 * fused + accumulate, accumulate, fused)
    close(a, b, atol=2e-6)


@pytest.mark.parametrize("K,R", [(520, 14), (700, 10)])
def test_14_and_10_rows_per_chunk(K, R):
    """two full chunks and one frame"""
    rs = np.random.RandomState(170 + K)
    u = _lean_utt(rs, 2500, K, 8, 8, False, exact=True, n_labels=K)

    def expect(pack):
        assert _stream_config(pack.desc)[:2] == (R, 1) and pack.desc.max_labels == K
    r = _streamed(f"labels_{K}", [u], 2 * R + 1, K, 171, mode=1, expect=expect)
    _streamed_viterbi([u], r.x, r.W, r.wids, mode=1)


# =================================================================================================
# A5. batches
# =================================================================================================
def test_mixed_and_shared_batches():
    """40 states beside 3 000 beside a hub acceptor: the staged area and the heavy lists at a0, e0 and 2 (s0 + g) of
    every utterance; one shared acceptor for three utterances: one staged copy, g = 0"""
    rs = np.random.RandomState(180)
    utts = [_lean_utt(rs, 40, C12, 3, 8, True), _case("a"), _hub_case()]
    assert _degrees(utts[2])[0] == 300
    r = _streamed("batch_sizes", utts, 20, C12, 181, mode=1)
    _streamed_viterbi(utts, r.x, r.W, r.wids, mode=1)
    utts = [_hub_case(), _eps_hubs(), _lean_utt(rs, 40, C12, 3, 8, True)]
    _streamed("batch_eps", utts, 20, C12, 182, mode=1)
    _streamed("batch_shared", [_hub_case()], 20, C12, 183, mode=1, shared=True, B=3)


def test_no_accepting_path_beside_streamed_utterances():
    """no accept state, an accept state out of reach, cut by -inf weights -- beside case a: logz = -inf, dx rows exactly
    zero (exactly the seed when accumulating), nothing in their dW ids, no best path"""
    utts, C = _no_path_case()
    utts = utts + [_case("a")]
    r = _streamed("no_path", utts, 17, C, 184, mode=1, nopath=(1, 2, 3))
    _streamed_viterbi(utts, r.x, r.W, r.wids, mode=1, nopath=(1, 2, 3))


def test_non_finite_inputs():
    """NaN arc weights (learnable and the graph's own), NaN emissions and a -inf emission column: read as -inf"""
    rs = np.random.RandomState(185)
    a = _case("a")
    gw = np.where(rs.rand(len(a.src)) < 0.03, np.nan, 0.0)
    utts = [_lean_utt(rs, 257, C12, 4, 8, True), _utt(a.Q, a.src, a.dst, a.lab, a.start, a.accept, gw), _hub_case()]

    def edit(x, W, wids):
        W[rs.rand(len(W)) < 0.03] = np.nan
        x[rs.rand(*x.shape) < 0.01] = np.nan
        x[0, :, 5] = NEG
        x[2, :, 7] = NEG
    _streamed("non_finite", utts, 20, C12, 186, mode=1, edit=edit)


# =================================================================================================
# A6. frames
# =================================================================================================
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 31, 32, 33, 49])
def test_frame_counts_around_the_chunk(T):
    """T = 1, T < R, T = R, T = R +- 1, several chunks, in both semirings.  One or two frames reach few states: every state
    within twelve of a start state accepts there, and three classes keep the gradient from being mostly zero."""
    C = 3 if T <= 2 else C12
    u = _case("a", C, T <= 2)
    r = _streamed(f"frames_{T}", [u], T, C, 190 + T, mode=1)
    _streamed_viterbi([u], r.x, r.W, r.wids, mode=1)


@pytest.mark.parametrize("T", [7, 8, 9, 17])
def test_frame_counts_around_the_chunk_of_eight(T):
    u = _case("e")
    r = _streamed(f"frames8_{T}", [u], T, 1001, 290 + T, mode=1)
    _streamed_viterbi([u], r.x, r.W, r.wids, mode=1)


# =================================================================================================
# B. the streamed kernels forced onto small acceptors
# =================================================================================================
# (B, T, TS): TS = min(16, B T / 512), T one below, at and one above a multiple of it
TILE_CASES = [(8, 127, 1), (8, 128, 2), (8, 129, 2), (8, 191, 2), (8, 192, 3), (8, 193, 3), (64, 127, 15), (64, 128, 16),
              (64, 129, 16)]


def _tile_case(B, T):
    """B acceptors of about 300 states, uniform labels; returns the dx of the dx-with-dW call"""
    rs = np.random.RandomState(400 + B + T)
    utts = [_lean_utt(rs, 300 - b % 8, C12, 6, 8, True) for b in range(B)]
    return _grad_kernels(f"tiles_{B}_{T}", utts, T, C12, 401 + B + T, True, False)[1]


def _forced_run(fn, forwards, grads, *args):
    """a case of test_gpu_lattice_edges under its own descriptor checks, format 0 and the proof of the streamed launches"""
    s0, g0 = _counters()
    fn(*args)
    torch.cuda.synchronize()
    s1, g1 = _counters()
    assert s1 - s0 == forwards + grads and g1 - g0 == (forwards if FORCED == "2" else 0), (fn.__name__, args, s1 - s0, g1 - g0)


def _forced_cases(dx_file):
    """what a child runs under WFL_LATTICE_STREAMED=1 / 2: every launch streamed, the state vectors in LDS / in global
    memory"""
    assert FORCED in ("1", "2")
    with _harness():
        for Q in (1, 2, 63, 64, 65, 1023, 1024, 1025):  # q == tid in registers against the strided loop
            _forced_run(ED.test_state_counts_around_every_thread_count, 1, 1, Q)
        _forced_run(ED.test_epsilon_arcs_inside_and_outside_the_lean_limits, 1, 1, "lean")
        _forced_run(ED.test_epsilon_arcs_inside_and_outside_the_lean_limits, 1, 1, "nine")
        _forced_run(ED.test_mixed_batches, 4, 4)
        _forced_run(ED.test_no_accepting_path_beside_normal_utterances, 1, 2)
        _forced_run(ED.test_no_best_path_beside_normal_utterances, 1, 0)
        _forced_run(ED.test_twenty_one_full_chunks_in_both_semirings, 2, 1)
        # large row maxima, 30 |randn| on every row: the renormalisation shift of every chunk is far from 0 (mode 2 carries
        # it into the chunk's first frame: sub, shift).  Added to the whole row: within a row the scores stay 1.5 randn (at
        # 30 randn per entry the posteriors are one-hot, and the oracle's gradient mostly zero).
        rs = np.random.RandomState(410)
        utts = [_lean_utt(rs, 300, C12, 5, 8, True), _lean_utt(rs, 1025, C12, 5, 8, False)]

        def edit(x, W, wids):
            x += (30.0 * np.abs(rs.randn(*x.shape[:2], 1))).astype(np.float32)
            assert x[:, :48].max(axis=2).reshape(2, 3, 16).sum(axis=2).min() > 100  # every full chunk of 16 frames

        def shifts_are_large(ref):
            assert min(r[0] for r in ref) > 300
        _forced_run(lambda: _run("row_maxima", utts, 49, C12, 411, edit=edit, ref_check=shifts_are_large), 1, 1)
        dx = {}
        for B, T, TS in TILE_CASES:
            assert _stream_config(types.SimpleNamespace(max_labels=C12, max_states=300), T, B)[2] == TS
            assert T % TS == {127: (0 if TS == 1 else 7), 128: 0, 129: 1, 191: 1, 192: 0, 193: 1}[T]
            s0 = _counters()[0]
            dx[f"{B}_{T}"] = _tile_case(B, T)
            assert _counters()[0] - s0 == 4
        np.savez(dx_file, **dx)
    print("forced streamed cases ok " + json.dumps(STATS))


@pytest.fixture(scope="module")
def _tuned_tile_dx():
    """the tuned path's dx (grad_kernel) of the tile cases, on the same inputs as the children's"""
    before = _counters()
    with _harness(fmt=1, tag="tuned_"):
        out = {(B, T): _tile_case(B, T) for B, T, _ in TILE_CASES}
    assert _counters() == before
    return out


@pytest.mark.parametrize("mode", [1, 2])
def test_forced_streamed_kernels_on_small_acceptors(mode, _tuned_tile_dx):
    """WFL_LATTICE_STREAMED is read at a process's first launch: a fresh child process per mode"""
    with tempfile.TemporaryDirectory() as tmp:
        dx_file = os.path.join(tmp, "dx.npz")
        code = (f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_lattice_streamed_edges as m; "
                f"m._forced_cases({dx_file!r})")
        env = dict(os.environ, WFL_LATTICE_STREAMED=str(mode))
        try:
            r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=240, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.fail(f"WFL_LATTICE_STREAMED={mode}: no result within 240 s")
        marker = "forced streamed cases ok "
        assert r.returncode == 0 and marker in r.stdout, f"status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
        STATS.update(json.loads(r.stdout.rsplit(marker, 1)[1]))  # (the child's worst cases: lattice_streamed_edges_forced<mode>_*)
        dx = np.load(dx_file)
        for B, T, _ in TILE_CASES:
            close(dx[f"{B}_{T}"], _tuned_tile_dx[B, T], atol=2e-6)
