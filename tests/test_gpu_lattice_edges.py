"""The lattice engine at the limits its kernels are built around (-m gpu): csrc/lattice_kernels.hip, driven through the
engine layer (PackedLattice.from_graphs, lattice_forward, lattice_formats, lattice_grad, lattice_viterbi) on random
acceptors that no criterion builds.

  A. sweeps   the lean one-state-per-thread sweeps (run_chain_prob: uniform-label frame loops of 2, 4, 6 and 8 arc slots,
     mixed-label loops of class 2, 4 and 8, idle waves) at every thread count of chain_threads, in-degree 1 .. 8 and 9,
     out-degree 9, different degree classes in the waves of one workgroup, frame counts around the 16-frame chunk, fewer
     than 16 rows per chunk, the 192-thread launch, mixed batches, utterances without an accepting path, NaN / -inf
     inputs, epsilon arcs inside and outside the lean limits -- log Z, dx and dW against the float64 recurrences of
     oracle/recurrences.py
  B. gradients   occ_grad_kernel against grad_kernel on the same sweeps, the fused log-softmax backward, the row streaming
     at its C >= 512 switch, grad_kernel's chunks of 16 arcs per label, its tile sizes
  C. tropical sweep and back-trace   valid accepting paths whose score is the max-plus optimum, exact on tying scores
  D. the log-domain chain_kernel (WFL_LATTICE_DOMAIN=log, one child process) on a selection of A

Bars: scores and dx at the defaults of tests/test_gpu_parity.py::close (1e-4 relative + 1e-5), dW at 5e-5 absolute -- those
of test_general_probability_sweep_on_random_acceptors -- through check() of tests/test_gpu_configs.py, so the worst ratios
land in the parity JSON it writes (lattice_edges_*).  Every case asserts on the oracle's own output, before the device is
asked, that it is worth comparing against: finite scores, gradients that are not mostly zero.
Nothing here reads the reference project."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import recurrences as OR  # noqa: E402
# _gpu_and_stats: the module-level fixture of test_gpu_configs, registered for this module by the import -- it skips
# without a GPU and writes STATS (shared) when this module's tests are over
from test_gpu_configs import STATS, _gpu_and_stats, check  # noqa: E402,F401
from test_gpu_lattice_streamed import _maxplus_eps  # noqa: E402
from test_gpu_parity import RTOL, _random_acceptor, close, dev  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
NEG = float("-inf")
# what lattice_formats must say of a feasible utterance: 1 (fp64 probability domain); 0 in the child process of part D
FMT = 0 if os.environ.get("WFL_LATTICE_DOMAIN") == "log" else 1
# check() allows RTOL * |want| + 2e-5 * scale: these scales restate close()'s atol of 1e-5 and the dW bar of 5e-5
S_X, S_W = 0.5, 2.5


def _rec(name, what):
    """the record of check(): one per family of cases (the case's name without its numbers) and quantity"""
    return "lattice_edges_" + re.sub(r"(_\d+)+$", "", name) + ("_logdomain_" if FMT == 0 else "_") + what


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


# =================================================================================================
# the generator
# =================================================================================================
def _starts(Q):
    return [q for q in range(Q) if q % 50 == 0]


def _accepts(Q, extra=()):
    return sorted(set([q for q in range(Q) if q % 7 == 3] + [Q - 1] + [int(q) for q in extra if q < Q]))


def _utt(Q, src, dst, lab, start=None, accept=None, gw=None):
    """an utterance's acceptor: the Graph and, for the oracle, its arcs in insertion order (lab < 0: epsilon)"""
    from gtn_applications_amd import graph as G

    u = types.SimpleNamespace(Q=Q, src=np.asarray(src, np.int64), dst=np.asarray(dst, np.int64), lab=np.asarray(lab, np.int64))
    u.start = _starts(Q) if start is None else list(start)
    u.accept = _accepts(Q) if accept is None else list(accept)
    u.gw = np.zeros(len(u.src), np.float32) if gw is None else np.asarray(gw, np.float32)
    g = G.Graph(True)
    st, ac = np.zeros(Q, np.uint8), np.zeros(Q, np.uint8)
    st[u.start], ac[u.accept] = 1, 1
    g.add_nodes(st, ac)
    if len(u.src):
        g.add_arcs(u.src, u.dst, np.where(u.lab < 0, G.epsilon, u.lab), weight=u.gw)
    u.g = g
    return u


def _lean_arcs(rs, Q, C, din, dout, uniform, self_loops=True, window=12, n_labels=None, exact=False):
    """Arcs of _lean_acceptor.  din: an int or one per state; self_loops="starts": only the start states loop (the only
    reachable shape of in-degree 1); window: in-arcs come from [q - window, q); n_labels: that many distinct labels,
    every one of them used, the first and the last class among them; exact: every state gets din in-arcs if it can."""
    din_q = np.broadcast_to(np.asarray(din), (Q,))
    src, dst = [], []
    outdeg = np.zeros(Q, np.int64)
    for q in range(Q):
        d = int(din_q[q])  # (a state with a self-loop alone would be out of reach: at least one arc from elsewhere)
        want = d if (exact or q % 5 == 0) else int(rs.randint(min(2, d), d + 1))
        have = 0
        if self_loops is True or (self_loops == "starts" and q % 50 == 0):
            src.append(q), dst.append(q)
            outdeg[q] += 1
            have = 1
        for p in rs.permutation(np.arange(max(0, q - window), q)).tolist():
            if have >= want:
                break
            if outdeg[p] >= dout:
                continue
            src.append(p), dst.append(q)
            outdeg[p] += 1
            have += 1
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    K = C if n_labels is None else n_labels
    pool = rs.permutation(C)[:K]
    if K >= 2 and K < C:
        pool[:2] = [0, C - 1]
        pool[2:] = 1 + rs.permutation(C - 2)[:K - 2]
    if uniform:
        lab = pool[rs.permutation(Q) % K][dst]
    else:
        lab = pool[rs.permutation(len(src)) % K]
    return src, dst, lab


def _lean_acceptor(rs, Q, C, din, dout, uniform, self_loops=True, **kw):
    """(Graph, src, dst, lab) of an acceptor inside the lean sweeps' shape: a self-loop on every state and in-arcs from
    states in [q - 12, q) until the state has a drawn number of in-arcs of at most din (every fifth state exactly din; a
    source that already has dout out-arcs is skipped); uniform: every arc into q carries q's own label, otherwise each
    arc draws its own.  Start states: q % 50 == 0; accept states: q % 7 == 3 and Q - 1."""
    u = _lean_utt(rs, Q, C, din, dout, uniform, self_loops, **kw)
    return u.g, u.src, u.dst, u.lab


def _lean_utt(rs, Q, C, din, dout=8, uniform=True, self_loops=True, accept_extra=(), start=None, accept=None, **kw):
    src, dst, lab = _lean_arcs(rs, Q, C, din, dout, uniform, self_loops, **kw)
    return _utt(Q, src, dst, lab, start, _accepts(Q, accept_extra) if accept is None else accept)


def _degrees(u):
    """(largest labelled in-degree, out-degree, epsilon in-degree, epsilon out-degree) of an utterance"""
    l, e = u.lab >= 0, u.lab < 0
    cnt = lambda v: int(np.bincount(v, minlength=u.Q).max()) if len(v) else 0  # noqa: E731
    return cnt(u.dst[l]), cnt(u.src[l]), cnt(u.dst[e]), cnt(u.src[e])


def _with_arcs(u, src, dst, lab, **kw):
    """u with more arcs appended (epsilon arcs, a hub's)"""
    return _utt(u.Q, np.concatenate([u.src, src]), np.concatenate([u.dst, dst]), np.concatenate([u.lab, lab]),
                kw.get("start", u.start), kw.get("accept", u.accept))


# =================================================================================================
# inputs, the oracle and the conditions on its output
# =================================================================================================
def _inputs(rs, utts, T, C, nopath=(), shared=False, B=None):
    """emissions 1.5 randn, learnable weights 0.4 randn: about four ids per five arcs, so some are shared by several arcs
    (of any utterance), one arc in ten has no parameter (-1); the utterances of `nopath` get ids of their own"""
    B = len(utts) if B is None else B
    x = (1.5 * rs.randn(B, T, C)).astype(np.float32)
    n = [len(u.src) for u in utts]
    nW = max(1, int(0.8 * sum(n)))
    own = {b: nW + sum(n[k] for k in nopath if k < b) for b in nopath}
    wids = []
    for b, u in enumerate(utts):
        w = rs.randint(nW, size=n[b]).astype(np.int32)
        w[rs.rand(n[b]) < 0.1] = -1
        if b in own:
            w = (own[b] + np.arange(n[b])).astype(np.int32)
        wids.append(w)
    W = (0.4 * rs.randn(nW + sum(n[k] for k in nopath))).astype(np.float32)
    return x, W, wids, nW


def _oracle(u, xb, W, wid):
    w = u.gw.astype(np.float64) + np.where(wid >= 0, W.astype(np.float64)[np.maximum(wid, 0)], 0.0)
    fn = OR.lattice_forward_backward_eps if (u.lab < 0).any() else OR.lattice_forward_backward
    return fn(np.asarray(xb, np.float64), u.src, u.dst, u.lab, w, u.start, u.accept, u.Q)


def _reference(utts, x, W, wids, nopath=(), shared=False):
    """the oracle's (score, dx, darc) per utterance, held to the conditions every case asserts on it"""
    B = x.shape[0]
    C = x.shape[2]
    ref = []
    for b in range(B):
        u, wid = (utts[0], wids[0]) if shared else (utts[b], wids[b])
        score, gx, garc = _oracle(u, x[b], W, wid)
        if b in nopath:
            assert score == NEG and not gx.any() and not garc.any(), b
        else:
            assert np.isfinite(score), (b, score)
            if C >= 511:  # most columns carry no label: of those that do, half must see a gradient
                cols = np.unique(u.lab[u.lab >= 0])
                frac = float((np.abs(gx[:, cols]).max(axis=0) > 0).mean())
            else:
                frac = float((gx > 1e-6).mean())
            assert frac >= 0.5, (b, frac)
        ref.append((score, gx, garc))
    return ref


def _dW_want(utts, wids, ref, coef_w, n, shared=False):
    out = np.zeros(n)
    for b, (_, _, garc) in enumerate(ref):
        wid = wids[0] if shared else wids[b]
        m = wid >= 0
        np.add.at(out, wid[m], coef_w[b] * garc[m])
    return out


def _pack(utts, C, wids, shared=False, B=None):
    from gtn_applications_amd import engine as E

    return E.PackedLattice.from_graphs([u.g for u in utts], C, torch.device("cuda"), wids=wids, B=B, shared=shared)


def _run(name, utts, T, C, seed, nopath=(), shared=False, B=None, fmt=None, edit=None, expect=None, ref_check=None):
    """One batch through lattice_forward and lattice_grad (dx and dW: grad_kernel), against the oracle.  edit(x, W, wids):
    changes to the inputs (non-finite values) before either side sees them.  expect(pack): assertions on the descriptor.
    ref_check(ref): further conditions of a case on the oracle's output.
    Utterances of `nopath`: logz == -inf, dx rows exactly zero (exactly the seed when accumulating), nothing in dW."""
    from gtn_applications_amd import engine as E

    rs = np.random.RandomState(seed)
    x, W, wids, nW = _inputs(rs, utts, T, C, nopath, shared, B)
    if edit is not None:
        edit(x, W, wids)
    B = x.shape[0]
    ref = _reference(utts, x, W, wids, nopath, shared)
    if ref_check is not None:
        ref_check(ref)
    coef = (0.5 + rs.rand(B)).astype(np.float32)
    coef_w = (0.5 + rs.rand(B)).astype(np.float32)
    seedx = rs.randn(B, T, C).astype(np.float32)
    xd, Wd = dev(x), dev(W)
    pack = _pack(utts, C, wids, shared, B)
    if expect is not None:
        expect(pack)
    st = E.lattice_forward(xd, pack, weights=Wd)
    got_fmt = E.lattice_formats(st).tolist()
    want_fmt = FMT if fmt is None else fmt
    assert all(f == want_fmt for b, f in enumerate(got_fmt) if b not in nopath), (name, got_fmt)
    logz = st.logz.cpu().numpy().astype(np.float64)
    feas = [b for b in range(B) if b not in nopath]
    for b in nopath:
        assert logz[b] == NEG, (name, b, logz[b])
    check(_rec(name, "logz"), logz[feas], [ref[b][0] for b in feas], S_X)
    for accumulate in (False, True):
        dx = dev(seedx) if accumulate else torch.full_like(xd, float("nan"))
        dW = torch.zeros_like(Wd)
        E.lattice_grad(st, dev(coef), coef_w=dev(coef_w), dx=dx, accumulate=accumulate, dW=dW)
        dx, dW = dx.cpu().numpy(), dW.cpu().numpy()
        for b in nopath:
            assert np.array_equal(dx[b], seedx[b] if accumulate else np.zeros_like(dx[b])), (name, b, accumulate)
        for b in feas:
            want = coef[b] * ref[b][1] + (seedx[b].astype(np.float64) if accumulate else 0.0)
            check(_rec(name, "dx"), dx[b], want, S_X)
        check(_rec(name, "dW"), dW, _dW_want(utts, wids, ref, coef_w, len(W), shared), S_W)
        assert not dW[nW:].any(), name  # (the ids of the utterances without a path)
        if nopath == () and not accumulate:
            break  # (accumulation into a seed: with the utterances without a path, and in part B)
    return types.SimpleNamespace(x=x, W=W, wids=wids, ref=ref, pack=pack, st=st)


def _config(pack):
    """chain_config of csrc/lattice_kernels.hip restated: (threads of the sweep workgroups, rows per chunk)"""
    d = pack.desc
    nt = 128 if d.max_states <= 128 else 256 if d.max_states <= 256 else 512 if d.max_states <= 512 else 1024
    while nt < 256 and nt * 8 < 2 * d.max_labels:
        nt += 64
    return nt, max(2, min(16, nt * 8 // max(1, d.max_labels)) & ~1)


def _expect_config(nt, rpc):
    def expect(pack):
        assert _config(pack) == (nt, rpc), (_config(pack), pack.desc.max_states, pack.desc.max_labels)
    return expect


# =================================================================================================
# A. sweeps: log Z, dx, dW against the oracle
# =================================================================================================
QS = [1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025]


def _state_count_case(Q):
    """a uniform and a mixed-label acceptor of Q states (few classes for the tiny ones: half the columns must matter)"""
    rs = np.random.RandomState(1000 + Q)
    C = min(12, Q + 1)
    return [_lean_utt(rs, Q, C, 4, 8, True), _lean_utt(rs, Q, C, 5, 8, False)], C


@pytest.mark.parametrize("Q", QS)
def test_state_counts_around_every_thread_count(Q):
    """Q on both sides of every step of chain_threads (128, 256, 512, 1024 threads), the smallest acceptors, and 1025 states:
    more than the workgroup has threads, so not lean, but swept in the probability domain all the same"""
    utts, C = _state_count_case(Q)
    nt = 128 if Q <= 128 else 256 if Q <= 256 else 512 if Q <= 512 else 1024
    _run(f"states_{Q}", utts, 33, C, Q, expect=_expect_config(nt, 16))


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("din", [1, 2, 3, 4, 5, 6, 7, 8])
def test_in_degrees_reach_every_frame_loop(din, uniform):
    """the largest in-degree (and, the backward sweep, out-degree) from 1 to 8: the uniform-label loops of 2, 4, 6 and 8
    arc slots, the mixed-label loops of class 2, 4 and 8.  In-degree 1 leaves only trees below looping start states: every
    state accepts there, and three classes keep the gradient from being mostly zero."""
    rs = np.random.RandomState(2000 + 10 * din + uniform)
    if din == 1:
        C, T = 3, 17
        utts = [_lean_utt(rs, Q, C, 1, 8, uniform, "starts", accept_extra=range(Q)) for Q in (129, 256)]
    else:
        C, T = 12, 17
        utts = [_lean_utt(rs, Q, C, din, max(din, 2), uniform) for Q in (129, 256)]
    for u in utts:
        assert _degrees(u)[0] == din and _degrees(u)[1] <= 8
    _run(f"din_{din}_{int(uniform)}", utts, T, C, din)


def _degree_nine(rs, Q, C, out):
    """a lean acceptor with one more arc: into (out: out of) a state that has eight already"""
    u = _lean_utt(rs, Q, C, 8, 8, False)
    ind, outd = np.bincount(u.dst, minlength=Q), np.bincount(u.src, minlength=Q)
    if out:
        p = int(np.flatnonzero(outd[:Q - 40] == 8)[0])
        q = int(next(q for q in range(p + 13, Q) if ind[q] < 8))
    else:
        q = int(np.flatnonzero(ind == 8)[-1])
        p = int(next(p for p in range(q - 13, 0, -1) if outd[p] < 8))
    u = _with_arcs(u, [p], [q], [int(rs.randint(C))])
    assert _degrees(u)[:2] == ((8, 9) if out else (9, 8))
    return u


def test_degree_nine_falls_to_the_general_sweep():
    """one state of in-degree 9; one state of out-degree 9 with every in-degree at most 8 (prob_eligible tests both):
    the general probability sweep, each in a batch of its own"""
    rs = np.random.RandomState(9)
    for out in (False, True):
        _run(f"degree9_{int(out)}", [_degree_nine(rs, 200, 12, out)], 33, 12, 90 + out)


@pytest.mark.parametrize("uniform", [True, False])
def test_waves_of_one_workgroup_in_different_degree_classes(uniform):
    """256 states whose in-degree is at most 2 in the first wave, 4 in the second, 6 in the third and 8 in the fourth: four
    frame loops side by side on one barrier per frame; beside it 129 states: a wave of one state and an idle wave"""
    rs = np.random.RandomState(3000 + uniform)
    din = np.repeat([2, 4, 6, 8], 64)
    utts = [_lean_utt(rs, 256, 12, din, 8, uniform), _lean_utt(rs, 129, 12, din[:129], 8, uniform)]
    ind = np.bincount(utts[0].dst, minlength=256).reshape(4, 64).max(axis=1)
    assert ind.tolist() == [2, 4, 6, 8]
    _run(f"waves_{int(uniform)}", utts, 33, 12, 31 + uniform, expect=_expect_config(256, 16))


@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 31, 32, 33, 47, 64, 65])
def test_frame_counts_around_the_chunk(T):
    """no full 16-frame chunk, only full chunks, both -- at 128, 512 and 1024 threads (the last one has no straight-line
    chunks).  One or two frames reach few states: every state within twelve of a start state accepts there, and three
    classes keep the gradient from being mostly zero."""
    for Q in (65, 257, 1024):
        rs = np.random.RandomState(4000 + 7 * T + Q)
        C = 3 if T <= 2 else 12
        extra = [q for q in range(Q) if q % 50 <= 12] if T <= 2 else ()
        utts = [_lean_utt(rs, Q, C, 4, 8, True, accept_extra=extra), _lean_utt(rs, Q, C, 6, 8, False, accept_extra=extra)]
        _run(f"frames_{T}_{Q}", utts, T, C, T + Q)


@pytest.mark.parametrize("Q,K,nt,rpc", [(100, 100, 128, 10), (128, 300, 128, 2), (128, 600, 192, 2), (128, 800, 256, 2)])
def test_fewer_than_sixteen_rows_per_chunk(Q, K, nt, rpc):
    """many labels on few states: chain_config gives chunks of 10 and of 2 rows (no full chunk: every chunk is the loop
    form), the 192-thread launch (prob_chain_kernel<256>) and 256 threads at two rows"""
    rs = np.random.RandomState(5000 + K)
    C = 1027
    utts = [_lean_utt(rs, Q, C, 8, 8, False, exact=True, n_labels=K), _lean_utt(rs, Q - 3, C, 5, 8, True, n_labels=Q - 3)]
    assert len(set(utts[0].lab.tolist())) == K

    def expect(pack):
        assert pack.desc.max_labels == (K + 3) & ~3 and _config(pack) == (nt, rpc), (_config(pack), pack.desc.max_labels)
    _run(f"rows_{K}", utts, 19, C, K, expect=expect)


def _hub(rs, u, q, n, C):
    """u with n more arcs into q from earlier states"""
    return _with_arcs(u, rs.randint(0, q, size=n), np.full(n, q), rs.randint(C, size=n))


def test_mixed_batches():
    """descriptor maxima are the batch's, eligibility is the utterance's: 40 states beside 700, uniform beside mixed
    labels, lean beside a hub of 30 in-arcs, one shared acceptor for three utterances"""
    rs = np.random.RandomState(6)
    C = 12
    _run("mixed_sizes", [_lean_utt(rs, 40, C, 3, 8, True), _lean_utt(rs, 700, C, 5, 8, False)], 33, C, 61,
         expect=_expect_config(1024, 16))
    _run("mixed_labels", [_lean_utt(rs, 200, C, 4, 8, True), _lean_utt(rs, 200, C, 4, 8, False),
                          _lean_utt(rs, 180, C, 8, 8, True)], 33, C, 62)
    _run("mixed_hub", [_lean_utt(rs, 300, C, 4, 8, True), _hub(rs, _lean_utt(rs, 300, C, 4, 8, False), 150, 30, C)], 33, C, 63)
    _run("mixed_shared", [_lean_utt(rs, 257, C, 5, 8, False)], 33, C, 64, shared=True, B=3)


def _no_path_case():
    rs = np.random.RandomState(7)
    C = 12
    cut = _lean_utt(rs, 40, C, 4, 8, False, accept=[24, 31, 38, 39])
    gw = np.where((cut.src < 20) & (cut.dst >= 20), NEG, 0.0)
    utts = [_lean_utt(rs, 65, C, 4, 8, True),
            _lean_utt(rs, 40, C, 4, 8, True, accept=[]),                   # no accept state
            _lean_utt(rs, 257, C, 4, 8, False, start=[0], accept=[256]),   # 256 states away, twelve a frame at the most
            _utt(40, cut.src, cut.dst, cut.lab, cut.start, cut.accept, gw),  # cut in two by -inf arc weights
            _lean_utt(rs, 257, C, 5, 8, False)]
    return utts, C


def test_no_accepting_path_beside_normal_utterances():
    utts, C = _no_path_case()
    _run("no_path", utts, 17, C, 71, nopath=(1, 2, 3))


def test_non_finite_inputs():
    """NaN arc weights (learnable and the graph's own), NaN emissions and a -inf emission column: read as -inf"""
    rs = np.random.RandomState(8)
    C = 12
    a = _lean_utt(rs, 129, C, 5, 8, False)
    gw = np.where(rs.rand(len(a.src)) < 0.03, np.nan, 0.0)
    utts = [_lean_utt(rs, 257, C, 4, 8, True), _utt(a.Q, a.src, a.dst, a.lab, a.start, a.accept, gw),
            _hub(rs, _lean_utt(rs, 200, C, 4, 8, False), 100, 30, C)]

    def edit(x, W, wids):
        W[rs.rand(len(W)) < 0.03] = np.nan
        x[rs.rand(*x.shape) < 0.01] = np.nan
        x[0, :, 5] = NEG
        x[2, :, 7] = NEG
    _run("non_finite", utts, 33, C, 81, edit=edit)


def _eps_case(kind):
    """a lean mixed-label acceptor of 200 states with epsilon arcs p -> q, p < q: a chain of seven (eight closure levels),
    a state that collects four and one that sends four -- the lean limits (kEpsDeg, kProbMaxLev); "five": a fifth into the
    collecting state, "nine": an eighth arc on the chain -- both outside"""
    rs = np.random.RandomState({"lean": 1, "five": 2, "nine": 3}[kind])
    u = _lean_utt(rs, 200, 12, 4, 8, False)
    chain = list(range(20, 20 + 3 * (9 if kind == "nine" else 8), 3))
    es, ed = chain[:-1], chain[1:]
    nin = 5 if kind == "five" else 4
    es += [100 + 2 * i for i in range(nin)]
    ed += [120] * nin
    es += [140] * 4
    ed += [143, 147, 151, 155]
    u = _with_arcs(u, es, ed, [-1] * len(es))
    lev = 1 + int(max(0, len(chain) - 1))
    assert _degrees(u)[2:] == (nin, 4) and lev == (9 if kind == "nine" else 8)
    return u


@pytest.mark.parametrize("kind", ["lean", "five", "nine"])
def test_epsilon_arcs_inside_and_outside_the_lean_limits(kind):
    """against the epsilon-aware recurrence, the epsilon arcs' weight gradients included"""
    u = _eps_case(kind)
    rs = np.random.RandomState(11)

    def expect(pack):
        assert pack.desc.max_levels == (9 if kind == "nine" else 8) and pack.desc.max_eps == len(u.src) - int((u.lab >= 0).sum())
    _run(f"eps_{kind}", [u, _lean_utt(rs, 129, 12, 4, 8, True)], 33, 12, 12, expect=expect)


def test_host_side_guards():
    """what would send a kernel outside its arrays is rejected on the host: a label that is no class, a weight id beyond
    the learnable weights (the sweeps read there, the gradient adds there), fewer or more ids than arcs"""
    from gtn_applications_amd import _native as N
    from gtn_applications_amd import engine as E

    rs = np.random.RandomState(13)
    C, T = 12, 5
    u = _lean_utt(rs, 40, C, 3, 8, True)
    wid = np.arange(len(u.src), dtype=np.int32)
    for bad in (C, -2):
        lab = u.lab.copy()
        lab[7] = bad
        with pytest.raises(N.WflError, match="label"):
            E.PackedLattice.from_graphs([_raw_label_graph(u, lab)], C, torch.device("cuda"), wids=[wid])
    with pytest.raises(N.WflError, match="label"):
        _pack([u], int(u.lab.max()), [wid])  # (fewer classes than the labels need)
    with pytest.raises(ValueError, match="one entry per arc"):
        _pack([u], C, [wid[:-1]])
    pack = _pack([u], C, [wid])
    x = dev(rs.randn(1, T, C))
    with pytest.raises(ValueError, match="weight id"):
        E.lattice_forward(x, pack, weights=torch.zeros(len(wid) - 1, device="cuda"))
    W = torch.zeros(len(wid), device="cuda")
    st = E.lattice_forward(x, pack, weights=W)
    with pytest.raises(ValueError, match="weight id"):
        E.lattice_grad(st, torch.ones(1, device="cuda"), dx=torch.zeros_like(x), dW=torch.zeros(len(wid) - 1, device="cuda"))
    E.lattice_grad(st, torch.ones(1, device="cuda"), dx=torch.zeros_like(x), dW=torch.zeros_like(W))


def _raw_label_graph(u, lab):
    """u's graph with the labels as given (no translation of negative ones to epsilon)"""
    from gtn_applications_amd import graph as G

    g = G.Graph(True)
    st, ac = np.zeros(u.Q, np.uint8), np.zeros(u.Q, np.uint8)
    st[u.start], ac[u.accept] = 1, 1
    g.add_nodes(st, ac)
    g.add_arcs(u.src, u.dst, lab)
    return g


# =================================================================================================
# B. the three gradient kernels on the same sweeps
# =================================================================================================
def _softmax_rows(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _grad_kernels(name, utts, T, C, seed, accumulate, fused):
    """One forward pass, three gradient calls: dx alone (occ_grad_kernel where the acceptor is uniform), dx with dW
    (grad_kernel), dW alone -- per-utterance factors, an upstream scalar, optionally onto a seed and through the fused
    log-softmax.  Returns the two dx."""
    from gtn_applications_amd import engine as E

    rs = np.random.RandomState(seed)
    x, W, wids, _ = _inputs(rs, utts, T, C)
    B = len(utts)
    xin = x.astype(np.float64)
    if fused:  # the oracle sees log_softmax(x) in float64
        xin = xin - np.log(np.exp(xin - xin.max(axis=2, keepdims=True)).sum(axis=2, keepdims=True)) - xin.max(axis=2, keepdims=True)
    ref = _reference(utts, xin, W, wids)
    coef = (0.5 + rs.rand(B)).astype(np.float32)
    coef_w = (0.5 + rs.rand(B)).astype(np.float32)
    g0 = np.float32(0.37)
    seedx = rs.randn(B, T, C).astype(np.float32)
    xd, Wd = dev(x), dev(W)
    st = E.lattice_forward(xd, _pack(utts, C, wids), weights=Wd, log_softmax=fused)
    assert E.lattice_formats(st).tolist() == [FMT] * B
    check(_rec(name, "logz"), st.logz.cpu().numpy(), [r[0] for r in ref], S_X)
    want = np.zeros((B, T, C))
    for b in range(B):
        g = float(g0) * coef[b] * ref[b][1]
        if fused:  # g_t - softmax(x_t) sum_c g_t[c]
            g = g - _softmax_rows(x[b]) * g.sum(axis=1, keepdims=True)
        want[b] = g + (seedx[b] if accumulate else 0.0)
    want_dW = float(g0) * _dW_want(utts, wids, ref, coef_w, len(W))
    args = dict(gout=dev(np.array([g0])), accumulate=accumulate)
    out = []
    for with_dW in (False, True):
        dx = dev(seedx) if accumulate else torch.full_like(xd, float("nan"))
        dW = torch.zeros_like(Wd) if with_dW else None
        E.lattice_grad(st, dev(coef), coef_w=dev(coef_w) if with_dW else None, dx=dx, dW=dW, **args)
        check(_rec(name, ("fused_" if fused else "") + ("dx_grad" if with_dW else "dx_occ")), dx.cpu().numpy(), want, S_X)
        if with_dW:
            check(_rec(name, "dW"), dW.cpu().numpy(), want_dW, S_W)
        out.append(dx.cpu().numpy())
    dW = torch.zeros_like(Wd)
    E.lattice_grad(st, dev(coef), coef_w=dev(coef_w), dW=dW, **args)
    check(_rec(name, "dW"), dW.cpu().numpy(), want_dW, S_W)
    return out


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_occupancy_gradient_equals_the_general_gradient(accumulate, fused):
    """uniform acceptors (no parameter gradient asked for: occ_grad_kernel; asked for: grad_kernel) -- both meet the oracle
    and each other at the bar of test_banded_gradient_kernel_matches_the_general_kernel.  The mixed-label acceptor among
    them is not one for the occupancies (occ_eligible): grad_kernel serves it in both calls."""
    rs = np.random.RandomState(20 + accumulate)
    utts = [_lean_utt(rs, 257, 12, 5, 8, True), _lean_utt(rs, 65, 12, 8, 8, True), _lean_utt(rs, 200, 12, 3, 8, True),
            _lean_utt(rs, 129, 12, 5, 8, False)]
    occ, gen = _grad_kernels("occ_vs_grad", utts, 47, 12, 21 + accumulate, accumulate, fused)
    close(occ, gen, atol=2e-6)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("C", [3, 12, 511, 512, 513, 1027])
def test_class_counts_across_the_row_streaming_switch(C, fused):
    """stream_grad_rows changes its form at C >= 512; odd C leaves rows that are only four-byte aligned.  The labels
    include the first and the last class."""
    rs = np.random.RandomState(30 + C)
    K = min(C, 150)
    utts = [_lean_utt(rs, 257, C, 5, 8, True, n_labels=K), _lean_utt(rs, 200, C, 4, 8, True, n_labels=K)]
    for u in utts:
        assert {0, C - 1} <= set(u.lab.tolist())
    occ, gen = _grad_kernels(f"classes_{C}", utts, 21, C, C, False, fused)
    close(occ, gen, atol=2e-6)


PER_LABEL_SEEDS = {(15, 5): 2, (16, 4): 2, (17, 64): 4, (33, 65): 6, (16, 1): 1, (17, 1): 1}


@pytest.mark.parametrize("n_arcs,K", [(15, 5), (16, 4), (17, 64), (33, 65), (16, 1), (17, 1)])
def test_arcs_per_label_around_the_gradient_chunk(n_arcs, K):
    """grad_kernel sums a label's arcs in chunks of 16 (kChunk): one label on exactly 15, 16, 17 and 33 arcs of a mixed-label
    acceptor with 1, 4, 5, 64 and 65 distinct labels (K == 1: the whole acceptor has n_arcs arcs).  60 states with 65
    labels are past band_grad_kernel's limit.  The label sits on arcs near the start states, its class is favoured by
    the emissions, and the oracle must say of the arcs at the chunks' edges (the 1st, 16th, 17th and 33rd of the label
    in the packer's order: by destination, then as inserted) that they matter -- posteriors that sum to 4e-3 over the
    19 frames, so 2e-4 in some frame, twice what the bar lets pass on a gradient entry of 1 -- so that a chunk edge the
    kernel got wrong would show.  The seeds are the first at which the oracle says so (no kernel result enters)."""
    seed = PER_LABEL_SEEDS[n_arcs, K]
    rs = np.random.RandomState(seed)
    C = max(K, 2)  # (no class without a label: the oracle's gradient is not to be mostly zero)
    if K == 1:
        Q = 6
        src, dst, _ = _lean_arcs(rs, Q, C, 4, 8, True, window=3, exact=True)
        src, dst = src[:n_arcs], dst[:n_arcs]
        assert len(src) == n_arcs
        utts = [_utt(Q, src, dst, np.full(n_arcs, 1), [0], range(Q))]
    else:
        utts = []
        for Q in (60, 130):
            src, dst, _ = _lean_arcs(rs, Q, C, 8, 8, False)
            near = (dst % 50 <= 20) & (src != dst)  # (within reach of a start state in T frames)
            order = np.concatenate([rs.permutation(np.flatnonzero(near)), rs.permutation(np.flatnonzero(~near))])
            lab = np.empty(len(src), np.int64)
            lab[order[:n_arcs]] = C - 1  # the one label; every other class on the remaining arcs, as evenly as they go
            lab[order[n_arcs:]] = rs.permutation(K - 1)[np.arange(len(src) - n_arcs) % (K - 1)]
            assert len(set(lab.tolist())) == K and int((lab == C - 1).sum()) == n_arcs
            utts.append(_utt(Q, src, dst, lab))

    def expect(pack):
        assert pack.desc.max_labels == (K + 3) & ~3

    def edit(x, W, wids):
        x[:, :, C - 1] += 2.0

    def ref_check(ref):
        for u, (_, _, garc) in zip(utts, ref):
            arcs = np.flatnonzero(u.lab == (1 if K == 1 else C - 1))
            arcs = arcs[np.argsort(u.dst[arcs], kind="stable")]
            edges = [k for k in (0, 15, 16, 32) if k < n_arcs]
            assert garc[arcs[edges]].min() >= 4e-3, garc[arcs[edges]]
    _run(f"per_label_{n_arcs}_{K}", utts, 19, C, seed, expect=expect, edit=edit, ref_check=ref_check)


@pytest.mark.parametrize("T", [31, 32, 33, 65])
@pytest.mark.parametrize("Q", [40, 300, 1024])
def test_gradient_tile_sizes(Q, T):
    """the tiles of grad_kernel fall from 32 frames to one as the acceptor grows (40 KiB of LDS): frame counts around a
    tile, through both gradients"""
    rs = np.random.RandomState(50 + Q + T)
    utts = [_lean_utt(rs, Q, 12, 6, 8, True), _lean_utt(rs, Q - 1, 12, 6, 8, True)]
    occ, gen = _grad_kernels(f"tiles_{Q}_{T}", utts, T, 12, Q + T, True, False)
    close(occ, gen, atol=2e-6)


# =================================================================================================
# C. tropical sweep and back-trace
# =================================================================================================
def _first_arc_best_path(x, u, w):
    """The best path under the tie rule of DESIGN 4 ("Viterbi ties"), for an acceptor without epsilon arcs: of equal
    candidates into a state the first arc in the caller's arc order stays, of equal accept states the lowest."""
    T = x.shape[0]
    order = np.argsort(u.dst, kind="stable")
    a = np.full(u.Q, NEG)
    a[u.start] = 0.0
    bp = np.full((T, u.Q), -1, np.int64)
    for t in range(T):
        v = a[u.src] + w + x[t, u.lab].astype(np.float64)
        n = np.full(u.Q, NEG)
        for k in order.tolist():
            if v[k] > n[u.dst[k]]:
                n[u.dst[k]], bp[t, u.dst[k]] = v[k], k
        a = n
    acc = np.asarray(u.accept, np.int64)
    q = int(acc[np.argmax(a[acc])])
    path = []
    for t in range(T - 1, -1, -1):
        path.append(int(bp[t, q]))
        q = int(u.src[bp[t, q]])
    return path[::-1]


def _viterbi(utts, x, W, wids, nopath=(), exact=False):
    """lattice_viterbi on one batch: every path starts in a start state, connects, ends in an accept state, holds exactly
    T labelled arcs and scores the max-plus optimum, as does logz; exact (scores that are small integers): exactly, and
    without epsilon arcs the path is the one the documented tie rule picks"""
    from gtn_applications_amd import engine as E

    B, T, C = x.shape
    paths, logz = E.lattice_viterbi(dev(x), _pack(utts, C, wids), weights=dev(W))
    logz = logz.cpu().numpy()
    for b, u in enumerate(utts):
        w = u.gw.astype(np.float64) + np.where(wids[b] >= 0, W.astype(np.float64)[np.maximum(wids[b], 0)], 0.0)
        w = np.where(np.isnan(w), NEG, w)
        best = _maxplus_eps(x[b], u.src, u.dst, u.lab, w, np.asarray(u.start, np.int64), np.asarray(u.accept, np.int64), u.Q) \
            if len(u.accept) else NEG
        if b in nopath:
            assert best == NEG and paths[b] is None and logz[b] == NEG, (b, best, logz[b])
            continue
        assert np.isfinite(best) and paths[b] is not None, (b, best)
        p = np.asarray(paths[b], dtype=np.int64)
        assert u.src[p[0]] in u.start and u.dst[p[-1]] in u.accept, b
        assert (u.dst[p[:-1]] == u.src[p[1:]]).all(), b
        labelled = p[u.lab[p] >= 0]
        assert len(labelled) == T, (b, len(labelled))
        score = float(w[p].sum() + x[b, np.arange(T), u.lab[labelled]].astype(np.float64).sum())
        tol = 0.0 if exact else 1e-5 * abs(best) + 1e-4
        assert abs(score - best) <= tol, (b, score, best)
        assert abs(float(logz[b]) - best) <= tol, (b, float(logz[b]), best)
        if exact and not (u.lab < 0).any():
            assert p.tolist() == _first_arc_best_path(x[b], u, w), b


def _parity_acceptor(rs, Q, C, n_eps, hubs):
    g, src, dst, lab = _random_acceptor(rs, Q, C, n_eps, hubs)
    return _utt(Q, src, dst, lab, accept=[q for q in range(Q) if q % 7 == 3])


def _viterbi_batches():
    rs = np.random.RandomState(60)
    C = 12
    yield [_lean_utt(rs, 129, C, 4, 8, True), _lean_utt(rs, 100, C, 8, 8, False)], 33
    yield [_lean_utt(rs, 513, C, 6, 8, False), _hub(rs, _lean_utt(rs, 300, C, 4, 8, False), 150, 30, C)], 17
    yield [_eps_case("lean"), _eps_case("nine")], 33
    yield [_parity_acceptor(rs, 300, C, 25, [100, 150]), _lean_utt(rs, 257, C, 5, 8, True)], 33
    yield [_lean_utt(rs, 1025, C, 4, 8, False)], 16


def test_best_paths_on_lean_and_general_acceptors():
    for k, (utts, T) in enumerate(_viterbi_batches()):
        rs = np.random.RandomState(600 + k)
        x, W, wids, _ = _inputs(rs, utts, T, 12)
        _viterbi(utts, x, W, wids)


def test_best_path_on_tying_scores_is_a_best_path():
    """small integers everywhere: every path score is exact in float32, many paths tie, and the returned path's score is
    the optimum exactly; in-degrees up to 8: ties among the first four arcs of a state and among the later ones"""
    rs = np.random.RandomState(61)
    C, T = 5, 33
    utts = [_lean_utt(rs, 129, C, 8, 8, False), _lean_utt(rs, 257, C, 4, 8, True), _eps_case("lean")]
    utts[2] = _utt(utts[2].Q, utts[2].src, utts[2].dst, np.where(utts[2].lab >= C, utts[2].lab % C, utts[2].lab),
                   utts[2].start, utts[2].accept)
    x, W, wids, _ = _inputs(rs, utts, T, C)
    x = rs.randint(-2, 3, size=x.shape).astype(np.float32)
    W = rs.randint(-1, 2, size=W.shape).astype(np.float32)
    _viterbi(utts, x, W, wids, exact=True)


def test_no_best_path_beside_normal_utterances():
    utts, C = _no_path_case()
    rs = np.random.RandomState(62)
    x, W, wids, _ = _inputs(rs, utts, 17, C, nopath=(1, 2, 3))
    _viterbi(utts, x, W, wids, nopath=(1, 2, 3))


def test_twenty_one_full_chunks_in_both_semirings():
    """Q = 300, T = 336: the per-chunk offsets past a handful of chunks, log and tropical"""
    rs = np.random.RandomState(63)
    utts = [_lean_utt(rs, 300, 12, 5, 8, True), _lean_utt(rs, 300, 12, 5, 8, False)]
    r = _run("long", utts, 336, 12, 64)
    _viterbi(utts, r.x, r.W, r.wids)


# =================================================================================================
# D. the log-domain chain_kernel
# =================================================================================================
def _log_domain_cases():
    """what the child process runs under WFL_LATTICE_DOMAIN=log (FMT is 0 there): one case per thread count, an epsilon
    case, hubs, utterances without a path -- same oracle, same bars"""
    assert FMT == 0
    for Q in (128, 256, 512, 1024, 1025):
        test_state_counts_around_every_thread_count(Q)
    test_fewer_than_sixteen_rows_per_chunk(128, 600, 192, 2)
    test_epsilon_arcs_inside_and_outside_the_lean_limits("lean")
    test_degree_nine_falls_to_the_general_sweep()
    test_mixed_batches()
    test_no_accepting_path_beside_normal_utterances()
    print("log-domain cases ok " + json.dumps(STATS))


def test_log_domain_sweeps_on_the_same_acceptors():
    """WFL_LATTICE_DOMAIN is read at a process's first launch: a fresh child process"""
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_lattice_edges as m; m._log_domain_cases()"
    env = dict(os.environ, WFL_LATTICE_DOMAIN="log")
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=240, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail("WFL_LATTICE_DOMAIN=log: no result within 240 s")
    assert r.returncode == 0 and "log-domain cases ok " in r.stdout, f"status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
    STATS.update(json.loads(r.stdout.rsplit("log-domain cases ok ", 1)[1]))  # (the child's worst cases: lattice_edges_*_logdomain_*)
