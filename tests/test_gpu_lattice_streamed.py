"""GPU tests of the streamed lattice sweeps (csrc/lattice_streamed.h): acceptors whose arcs do not fit one CU's LDS.

1. Transducer loss, emission gradient and transition-parameter gradient under a pruned back-off bigram over the 1 000
   word pieces of tests/golden/word_pieces_tokens_1000.txt (built here from a seeded synthetic corpus: ~1 000 states,
   ~55 K arcs) against the float64 epsilon-aware recurrence; only the normaliser is streamed.
2. Viterbi under that model: valid accepting arc paths whose score is the max-plus optimum (recurrence below).
3. CTC with targets of 1 200 and 2 000 labels.
4. The streamed kernels forced onto graphs that fit LDS (WFL_LATTICE_STREAMED=1 and =2, each in a child process).
5. Graphs that fit LDS keep their launches: no streamed launch, the workspace query unchanged.
The bars are those of tests/test_gpu_configs.py and tests/test_gpu_ngram.py."""
import ctypes
import functools
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import recurrences as OR  # noqa: E402

from test_gpu_configs import check, STATS, RTOL, _word_piece_setup  # noqa: E402,F401
from lattice_workspace import tuned_workspace as _tuned_workspace  # noqa: E402
from test_gpu_ngram import check_dparams, _oracle, _run  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
GOLDEN = os.path.join(TESTS, "golden")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def _streamed_launches():
    """wfl_lattice_diagnostics out[8]: launches of the streamed sweeps and gradients so far in this process"""
    from gtn_applications_amd import _native as N

    out = (ctypes.c_uint64 * 9)()
    N.check(N.lib.wfl_lattice_diagnostics(out, 9))
    return int(out[8])


def _workspace(pack, T):
    from gtn_applications_amd import _native as N

    n_xg, n_ab = ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib.wfl_lattice_workspace(pack._desc_ref, T, ctypes.byref(n_xg), ctypes.byref(n_ab)))
    return n_xg.value, n_ab.value


@functools.lru_cache(maxsize=None)
def _backoff_word_piece_graph(n_lines=8000, seed=0):
    """build_transitions.py --blank optional --add_self_loops --prune 0 0 over a synthetic corpus: Zipf-distributed
    draws over the 1 000 word pieces, n_lines lines of 5 to 29 pieces"""
    from gtn_applications_amd import transitions_builder as TB

    tokens, g2i = _word_piece_setup()
    rs = np.random.RandomState(seed)
    order = rs.permutation(len(tokens))
    p = 1.0 / np.arange(1, len(tokens) + 1)
    p /= p.sum()
    lines = [[tokens[order[i]] for i in rs.choice(len(tokens), size=rs.randint(5, 30), p=p)] for _ in range(n_lines)]
    g = TB.build_transitions(lines, tokens, (0, 0), blank="optional", self_loops=True)
    return tokens, g2i, g


def _word_piece_batch(B, T, seed):
    from gtn_applications_amd.criterions import transducer as TR

    tokens, g2i, g = _backoff_word_piece_graph()
    C = len(tokens) + 1
    rs = np.random.RandomState(seed)
    random.seed(seed)
    targets = [[g2i[c] for wp in (random.choice(tokens) for _ in range(15)) for c in wp] for _ in range(B)]
    x = rs.randn(B, T, C).astype(np.float32)
    crit = TR.Transducer(tokens, g2i, blank="optional", allow_repeats=False, transitions=g, reduction="mean")
    params = (0.3 * rs.randn(crit.transition_params.numel())).astype(np.float32)
    return crit, g, x, targets, params


def _word_piece_loss_case(B, T, seed, name):
    """case 1: returns the number of streamed launches of the step"""
    from gtn_applications_amd.criterions import transducer as TR

    crit, g, x, targets, params = _word_piece_batch(B, T, seed)
    C = x.shape[2]
    want_loss, _, want_dx, want_dp, counts = _oracle(crit, x, targets, params)
    before = _streamed_launches()
    loss, dx, dp = _run(crit, x, targets, params)
    torch.cuda.synchronize()
    launches = _streamed_launches() - before
    check(name + "_loss", [loss], [want_loss], 0.0)
    scale = max(1.0 / len(t) for t in targets) / B
    check(name + "_dx", dx, want_dx, scale)
    check_dparams(name + "_dparams", dp, want_dp, counts, scale)
    if os.environ.get("WFL_LATTICE_STREAMED"):
        return launches
    # the normaliser is streamed, the numerator (the alignment graphs composed with the model: small) is not
    dev = torch.device("cuda")
    den = TR._transitions_pack(g, B, C, dev)
    assert den.desc.max_arcs > 40000
    assert _workspace(den, T)[1] > _tuned_workspace(den.desc, T)[1]
    _, entry = TR._pack_entry(targets, crit.tokens, crit.lexicon, g, C, dev, "mean")
    assert _workspace(entry[0], T) == _tuned_workspace(entry[0].desc, T)
    return launches


def test_backoff_word_pieces_loss_and_gradients():
    """case 1: B = 8, T = 250, 15 word pieces per target spelled in graphemes"""
    launches = _word_piece_loss_case(8, 250, 11, "streamed_wp")
    assert launches == 2  # the normaliser's sweeps and its gradient


def _eps_levels(src, dst, lab, Q):
    """level of every state in the acyclic epsilon subgraph (longest epsilon path into it)"""
    lev = np.zeros(Q, dtype=np.int64)
    e = np.flatnonzero(lab < 0)
    for _ in range(Q):
        new = lev.copy()
        np.maximum.at(new, dst[e], lev[src[e]] + 1)
        if (new == lev).all():
            break
        lev = new
    return lev


def _maxplus_eps(x, src, dst, lab, w, start, accept, Q):
    """max-plus recurrence of emissions x [T, C] o acceptor (lab < 0: epsilon arcs, followed after every frame and
    before the first, by levels): the best accepting path score, float64"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    il, ie = np.flatnonzero(lab >= 0), np.flatnonzero(lab < 0)
    lev = _eps_levels(src, dst, lab, Q)
    by_level = [ie[lev[src[ie]] == l] for l in range(int(lev.max()) + 1)] if len(ie) else []

    def closure(a):
        for arcs in by_level:
            np.maximum.at(a, dst[arcs], a[src[arcs]] + w[arcs])
        return a

    a = np.full(Q, -np.inf)
    a[start] = 0.0
    a = closure(a)
    for t in range(x.shape[0]):
        n = np.full(Q, -np.inf)
        np.maximum.at(n, dst[il], a[src[il]] + w[il] + x[t, lab[il]])
        a = closure(n)
    return float(a[accept].max())


def _viterbi_case(B, T, seed, crit, g, x, params):
    from gtn_applications_amd import engine as E
    from gtn_applications_amd.criterions import transducer as TR

    C = x.shape[2]
    dev = torch.device("cuda")
    ga = g.arrays()
    src, dst, lab, olab = (np.asarray(ga[k], dtype=np.int64) for k in ("src", "dst", "ilabel", "olabel"))
    start, accept = np.flatnonzero(ga["start"]), np.flatnonzero(ga["accept"])
    Q = len(ga["start"])
    xc = torch.from_numpy(x).to(dev)
    pc = torch.from_numpy(params).to(dev)
    paths, _ = E.lattice_viterbi(xc, TR._transitions_pack(g, B, C, dev), weights=pc)
    decoded = []
    for b in range(B):
        p = paths[b]
        assert p is not None and len(p) >= T
        p = np.asarray(p, dtype=np.int64)
        assert start.tolist().count(src[p[0]]) == 1 and dst[p[-1]] in set(accept.tolist())
        assert (dst[p[:-1]] == src[p[1:]]).all()
        labelled = p[lab[p] >= 0]
        assert len(labelled) == T
        score = float(np.sum(params[p].astype(np.float64)) + np.sum(x[b, np.arange(T), lab[labelled]].astype(np.float64)))
        best = _maxplus_eps(x[b], src, dst, lab, params, start, accept, Q)
        assert abs(score - best) <= 1e-5 * abs(best) + 1e-4, (b, score, best)
        frames = olab[p][olab[p] >= 0].tolist()
        decoded.append([k for k, _ in itertools.groupby(frames) if k != C - 1])
    with torch.no_grad():
        crit.transition_params.copy_(torch.from_numpy(params))
    got = crit.viterbi(xc)
    for b in range(B):
        assert got[b].tolist() == decoded[b], b


def test_backoff_word_pieces_viterbi():
    """case 2: E.lattice_viterbi on the normaliser's pack and Transducer.viterbi, B = 8, T = 250"""
    crit, g, x, _, params = _word_piece_batch(8, 250, 12)
    crit.cuda()
    before = _streamed_launches()
    _viterbi_case(8, 250, 12, crit, g, x, params)
    assert _streamed_launches() - before >= 1


def _no_repeat_targets(rs, lens, n_labels):
    out = []
    for L in lens:
        t = [int(rs.randint(n_labels))]
        while len(t) < L:
            v = int(rs.randint(n_labels))
            if v != t[-1]:
                t.append(v)
        out.append(t)
    return out


def _ctc_case(B, T, C, lens, seed, name):
    from gtn_applications_amd.criterions import ctc

    rs = np.random.RandomState(seed)
    x = torch.log_softmax(torch.from_numpy(rs.randn(B, T, C).astype(np.float32)), dim=2)
    targets = _no_repeat_targets(rs, lens, C - 1)
    for reduction in ("none", "mean"):
        want_loss, want_dx = OR.ctc_loss_grad(x.numpy(), targets, C - 1, reduction)
        xg = x.cuda().requires_grad_(True)
        loss = ctc.CTCLoss(xg, targets, C - 1, reduction)
        loss.backward()
        check(f"{name}_{reduction}_loss", [loss.item()], [want_loss], 0.0)
        scale = (1.0 if reduction == "none" else max(1.0 / L for L in lens)) / B
        check(f"{name}_{reduction}_dx", xg.grad.cpu().numpy(), want_dx, scale)


def test_ctc_long_targets():
    """case 3: B = 3, C = 32, T = 4 500, targets of 1 200, 2 000 and 2 000 labels (4 001 states)"""
    before = _streamed_launches()
    _ctc_case(3, 4500, 32, (1200, 2000, 2000), 21, "streamed_ctc_long")
    assert _streamed_launches() - before >= 4  # two steps, a sweep and a gradient each


# ---- case 4: the streamed kernels forced onto graphs that fit (child processes, WFL_LATTICE_STREAMED=1 / 2) ----------
def _forced_backoff_fixture():
    import test_gpu_ngram as NG

    before = _streamed_launches()
    NG.test_backoff_transitions_at_benchmark_length(GOLDEN)
    assert _streamed_launches() - before >= 4  # numerator and normaliser: sweeps and gradients


def _forced_bigram():
    import test_gpu_ngram as NG
    from gtn_applications_amd.criterions import transducer as TR

    TR._DENSE_NGRAM = False  # the normaliser and Viterbi through the lattice engine, not the dense short cut
    before = _streamed_launches()
    NG.test_ngram_transitions_at_the_reference_benchmark_size("ctc", 2)
    assert _streamed_launches() - before >= 5  # loss: 2 x (sweeps + gradient); Viterbi: sweeps


def _forced_ctc_300():
    before = _streamed_launches()
    _ctc_case(2, 700, 32, (300, 280), 31, "forced_ctc_300")
    assert _streamed_launches() - before >= 4


def _forced_word_pieces_global_states():
    assert _word_piece_loss_case(4, 250, 13, "forced_global_wp") == 4  # numerator and normaliser streamed


def _child(mode, fn, timeout):
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_lattice_streamed as m; m.{fn}()"
    env = dict(os.environ, WFL_LATTICE_STREAMED=str(mode))
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=timeout, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail(f"WFL_LATTICE_STREAMED={mode} {fn}: no result within {timeout} s")
    assert r.returncode == 0, f"WFL_LATTICE_STREAMED={mode} {fn}: status {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"


@pytest.mark.parametrize("mode", [1, 2])
def test_forced_streamed_path(mode):
    """case 4: every log / tropical sweep and gradient streamed (1: states in LDS, 2: states in global memory); a child
    that fails stops the test before the next one starts"""
    cases = [("_forced_backoff_fixture", 300), ("_forced_bigram", 300), ("_forced_ctc_300", 300)]
    if mode == 2:
        cases.append(("_forced_word_pieces_global_states", 300))
    for fn, timeout in cases:
        _child(mode, fn, timeout)


# ---- case 5: graphs that fit keep their launches ----------------------------------------------------------------------
def test_fitting_graphs_keep_their_path():
    """the cfg4 shape (B = 64, T = 800, 1 000 pieces, no transition model) and the 8-node back-off fixture: no streamed
    launch, and the workspace query answers what the tuned layout needs"""
    import json

    from gtn_applications_amd import graph as G
    from gtn_applications_amd.criterions import transducer as TR

    dev = torch.device("cuda")
    tokens, g2i = _word_piece_setup()
    B, T = 64, 800
    C = len(tokens) + 1
    random.seed(0)
    targets = [[g2i[c] for wp in (random.choice(tokens) for _ in range(15)) for c in wp] for _ in range(B)]
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(0))
    crit = TR.Transducer(tokens, g2i, blank="optional", allow_repeats=False, reduction="mean")
    before = _streamed_launches()
    xg = x.cuda().requires_grad_(True)
    crit(xg, [torch.tensor(t) for t in targets]).backward()
    torch.cuda.synchronize()
    assert np.isfinite(xg.grad.cpu().numpy()).all()
    _, entry = TR._pack_entry(targets, crit.tokens, crit.lexicon, None, C, dev, "mean")
    assert _workspace(entry[0], T) == _tuned_workspace(entry[0].desc, T)

    lit = json.load(open(os.path.join(GOLDEN, "reference_literals.json")))["backoff_transitions"]
    N, T2, B2 = lit["N"], 250, 16
    g = G.Graph(True)
    for n in range(8):
        g.add_node(n in lit["start"], n in lit["accept"])
    for a in lit["arcs"]:
        g.add_arc(*a)
    crit2 = TR.Transducer([(n,) for n in range(N)], {n: n for n in range(N)}, blank="optional", allow_repeats=False,
                          transitions=g, reduction="mean").cuda()
    rs = np.random.RandomState(5)
    x2 = torch.from_numpy(rs.randn(B2, T2, N + 1).astype(np.float32)).cuda().requires_grad_(True)
    targets2 = [rs.randint(0, N, size=rs.randint(20, 45)).tolist() for _ in range(B2)]
    crit2(x2, [torch.tensor(t) for t in targets2]).backward()
    crit2.viterbi(x2.detach())
    torch.cuda.synchronize()
    den = TR._transitions_pack(g, B2, N + 1, dev)
    assert _workspace(den, T2) == _tuned_workspace(den.desc, T2)
    assert _streamed_launches() == before
