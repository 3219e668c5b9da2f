"""The dense engine's GRADIENT launches across frame chunks and call forms (-m gpu): engine.dense_grad on
csrc/dense_kernels.hip (wfl_dense_grad / wfl_dense_grad_parts) and csrc/dense_wide.h, ASGLoss at the end.

A gradient launch cuts an utterance into chunks = max(1, min(T, ceil(512 / B))) workgroups of rows = ceil(T / chunks)
frames.  The bucket-by-bucket tests of tests/test_gpu_parity.py run at B <= 6, where every workgroup sees ONE frame: the
stage loops (TS = 8 / 16 frames, 2 TS with two register sets on the matrix cores), their ragged tails, the pair
alpha_{t_begin - 1} / beta_{t_begin} across a chunk edge and the all-zero partial of an empty chunk never run there.

  A  frame chunks: twelve (B, T) whose chunks are ragged, empty, exactly / one more than a stage, one per utterance; six
     class counts (one per kernel family); dx + dW, dx alone, dW alone
  B  call forms: per-utterance coef, coef_w beside it / absent, gout, accumulate, both addends, all of them together
  C  the log-domain gradient (a forbidden transition flags every utterance): NP = 4 / 16 / 40 / 64 (two and three
     passes), the emission-only launch beyond 101 classes
  D  mixed batches: clean, flagged (-inf emission) and dead (an impossible frame) utterances side by side
  E  beyond the on-chip class limit (csrc/dense_wide.h): the call forms only
  F  ASGLoss on leaves: the early gradient (addend = the numerator's, no gout), then a retained graph (gout, both addends)

Expectation, from include/wfl.h and engine.dense_grad's docstring:
    dx = (accumulate ? prior_dx : 0) + g addend    + g coef_b   post_x,b
    dW = (accumulate ? prior_dW : 0) + g dW_addend + g sum_b coef_w_b post_W,b          g = gout[0], or 1 without gout
with post_x / post_W the float64 posteriors of oracle/recurrences.py.  The posteriors of a whole batch come from the scaled
float64 matrix products of OR.asg_loss_grad_batched (_batched_posteriors below: the same products, with exact zeros where
a score is -inf); every case asserts them against OR.dense_forward_backward on four of its utterances -- the first, the
last, a flagged one where there is one -- to 1e-9 before the device is asked.  Bar: tests/test_gpu_configs.py::check,
|got - want| <= 1e-4 |want| + 2e-5 scale, scale = |g| max_b |coef_b| for dx and |g| max_b |coef_w_b| for dW (ONE
posterior's coefficient); priors and g * addends are drawn inside +-scale.  Output buffers are pre-filled with NaN (or the
prior), the buffer of the partial sums as well; every call runs twice and must repeat itself bit for
bit.  Worst ratios land in the parity JSON that tests/test_gpu_configs.py writes, under dense_grad_*."""

import collections
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import recurrences as OR  # noqa: E402
# _gpu_and_stats: the module-level fixture of test_gpu_configs, registered for this module too by the import -- skips
# without a GPU, and writes STATS (shared, so with every module's records so far) when this module's tests are over
from test_gpu_configs import _gpu_and_stats, check  # noqa: E402,F401

NEG = float("-inf")
CLASSES = [20, 50, 100, 128, 150, 192]  # padded to 32 / 64 / 104 / 128 (exact) / 160 / 192 (exact)
GOUT = -2.5


def _chunks(B, T):
    return max(1, min(T, -(-512 // B)))


# =================================================================================================
# the oracle
# =================================================================================================
def _batched_posteriors(x, W):
    """float64 posteriors of the fully connected graph for a whole batch: (log Z [B], state posteriors [B, T, C],
    dW(cw) -> sum_b cw_b * (start / transition posteriors of b) [(C+1), C]).  The products of OR.asg_loss_grad_batched;
    a score of -inf is an exact zero factor (no frame may be -inf throughout: the caller takes such an utterance out)."""
    x = np.asarray(x, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    x = np.where(np.isnan(x), NEG, x)
    W = np.where(np.isnan(W), NEG, W)
    B, T, C = x.shape
    M = W[1:]  # [cur, prev]
    mrow, m0 = M.max(), W[0].max()
    P = np.exp(M - mrow)
    xm = x.max(axis=2, keepdims=True)
    assert np.isfinite(xm).all() and np.isfinite(mrow) and np.isfinite(m0)
    ex = np.exp(x - xm)
    a, la = np.empty((B, T, C)), np.empty((B, T))
    v = ex[:, 0] * np.exp(W[0] - m0)
    s = v.sum(axis=1)
    a[:, 0], la[:, 0] = v / s[:, None], np.log(s) + xm[:, 0, 0] + m0
    for t in range(1, T):
        v = ex[:, t] * (a[:, t - 1] @ P.T)
        s = v.sum(axis=1)
        a[:, t], la[:, t] = v / s[:, None], la[:, t - 1] + np.log(s) + xm[:, t, 0] + mrow
    logz = la[:, T - 1]
    bt, lb = np.empty((B, T, C)), np.empty((B, T))
    bt[:, T - 1], lb[:, T - 1] = 1.0 / C, np.log(C)
    for t in range(T - 2, -1, -1):
        v = (bt[:, t + 1] * ex[:, t + 1]) @ P
        s = v.sum(axis=1)
        bt[:, t], lb[:, t] = v / s[:, None], lb[:, t + 1] + np.log(s) + xm[:, t + 1, 0] + mrow
    assert np.isfinite(logz).all() and np.isfinite(la).all() and np.isfinite(lb).all()
    post = a * bt * np.exp(la + lb - logz[:, None])[:, :, None]
    wgt = np.exp(la[:, :-1] + lb[:, 1:] + xm[:, 1:, 0] + mrow - logz[:, None])  # [B, T-1]
    cur = ex[:, 1:] * bt[:, 1:] * wgt[:, :, None]                               # [B, T-1, C]
    prev = a[:, :-1]

    def dW(cw):
        cw = np.asarray(cw, dtype=np.float64)
        out = np.zeros_like(W)
        out[1:] = P * ((cur * cw[:, None, None]).reshape(-1, C).T @ prev.reshape(-1, C))
        out[0] = (post[:, 0] * cw[:, None]).sum(axis=0)
        return out

    return logz, post, dW


Case = collections.namedtuple("Case", "x W logz post dW_ones dW_spread flagged dead")


def _spread(B, seed=0):
    """per-utterance coefficients over a decade (0.1 .. 1), one of them zero, one negative"""
    v = 10.0 ** (-np.random.RandomState(977 + B + seed).rand(B))
    v[1 % B] = 0.0
    v[2 % B] = -v[2 % B]
    return v.astype(np.float32)


def _make_case(x, W, dead=()):
    """The oracle's numbers for one input, asserted against OR.dense_forward_backward on four utterances.  `dead`:
    utterances with an impossible frame -- log Z = -inf, posteriors zero, no share in dW."""
    B, T, C = x.shape
    flagged = [bool(not np.isfinite(x[b]).all() or not np.isfinite(W).all()) for b in range(B)]
    xo = x.copy()
    for b in dead:
        xo[b] = 0.0
    logz, post, dW = _batched_posteriors(xo, W)
    alive = np.ones(B)
    for b in dead:
        logz[b], post[b], alive[b] = NEG, 0.0, 0.0
    probe = {0, B - 1, B // 2} | set(dead) | {next((b for b in range(B) if flagged[b] and b not in dead), 0)}
    for b in sorted(probe):
        lz, px, pW = OR.dense_forward_backward(np.where(np.isnan(x[b]), NEG, x[b]), W)
        one = np.zeros(B)
        one[b] = alive[b]
        if b in dead:
            assert lz == NEG
            px, pW = np.zeros_like(px), np.zeros_like(pW)
        else:
            assert abs(lz - logz[b]) <= 1e-9 * max(1.0, abs(lz)), (b, lz, logz[b])
            assert np.abs(px.sum(axis=1) - 1.0).max() <= 1e-9
        assert np.abs(np.nan_to_num(px) - post[b]).max() <= 1e-9, b
        assert np.abs(np.nan_to_num(pW) - dW(one)).max() <= 1e-9 * max(1, T), b
    return Case(x, W, logz, post, dW(alive), dW(alive * _spread(B)), flagged, tuple(dead))


def _scores(B, T, C):
    """well-conditioned emissions and transitions: nothing for the range check to flag"""
    rs = np.random.RandomState(100003 * B + 101 * T + C)
    return (2.0 * rs.randn(B, T, C)).astype(np.float32), rs.randn(C + 1, C).astype(np.float32)


@functools.lru_cache(maxsize=2)
def _clean_case(B, T, C):
    return _make_case(*_scores(B, T, C))


@functools.lru_cache(maxsize=2)
def _forbidden_case(B, T, C):
    """a forbidden transition: no utterance of the batch is served in the probability domain"""
    x, W = _scores(B, T, C)
    W[1 + 4, 7] = NEG
    return _make_case(x, W)


# =================================================================================================
# the device's numbers beside it
# =================================================================================================
# coef: a number (every utterance), "s" (_spread), "r" (another spread: differs from "s" utterance by utterance);
# coef_w: None (absent: 1), a number, "s"
Form = collections.namedtuple("Form", "name coef coef_w gout accumulate addend dW_addend outs")
PLAIN = Form("plain", 0.5, 0.5, None, False, False, False, "both")
FORMS = [
    Form("per_utterance_coef", "s", "s", None, False, False, False, "both"),
    Form("coef_w_differs", "s", 0.25, None, False, False, False, "both"),
    Form("coef_w_absent", "s", None, None, False, False, False, "both"),
    Form("gout", 0.5, "s", GOUT, False, False, False, "both"),
    Form("accumulate_dx_alone", "s", None, None, True, False, False, "dx"),
    Form("accumulate_both_gout", 0.5, "s", GOUT, True, False, False, "both"),
    Form("addends_gout", "s", 0.25, GOUT, False, True, True, "both"),
    Form("all_together", "r", "s", GOUT, True, True, True, "both"),
]
ALL = FORMS[-1]


def _coef_vector(spec, B):
    if spec is None:
        return np.ones(B, np.float32)
    if spec == "s":
        return _spread(B)
    if spec == "r":
        return (0.7 * _spread(B, seed=5)[::-1]).astype(np.float32)
    return np.full(B, spec, np.float32)


@functools.lru_cache(maxsize=2)
def _forward(kind, B, T, C):
    """the sweeps of one case, once for all its forms: (case, x, W, DenseState)"""
    from gtn_applications_amd import engine as E

    case = {"clean": _clean_case, "forbidden": _forbidden_case, "wide": _clean_case}[kind](B, T, C)
    xt, Wt = torch.from_numpy(case.x).cuda(), torch.from_numpy(case.W).cuda()
    return case, xt, Wt, E.dense_forward(xt, Wt, need_beta=True)


@contextlib.contextmanager
def _empty_means_nan():
    """engine.dense_grad takes the partial sums' buffer from torch.empty: while this is open that buffer starts as NaNs,
    so that a slice no workgroup wrote (an empty chunk's) shows in dW whatever the allocator would have handed out"""
    real = torch.empty

    def filled(*args, **kwargs):
        t = real(*args, **kwargs)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real


def _run_form(group, case, xt, Wt, st, form, zero_entry=None):
    """One call form against the formula, twice over: the second run must repeat the first bit for bit.  `zero_entry`: an
    entry of dW whose prior and addend are zero (a forbidden transition: the result must then be exactly 0.0).
    Returns (dx, dW) as numpy (None where the form leaves one out)."""
    from gtn_applications_amd import engine as E

    B, T, C = case.x.shape
    g = 1.0 if form.gout is None else form.gout
    cf, cw = _coef_vector(form.coef, B), _coef_vector(form.coef_w, B)
    sx, sw = abs(g) * float(np.abs(cf).max()), abs(g) * float(np.abs(cw).max())
    rs = np.random.RandomState(B + 7 * T + 13 * C + len(form.name))
    # priors inside +-scale, addends inside +-scale / |g| (they arrive scaled by g)
    prior_dx = (sx * (2 * rs.rand(B, T, C) - 1)).astype(np.float32)
    prior_dW = (sw * (2 * rs.rand(C + 1, C) - 1)).astype(np.float32)
    add_dx = (sx / abs(g) * (2 * rs.rand(B, T, C) - 1)).astype(np.float32)
    add_dW = (sw / abs(g) * (2 * rs.rand(C + 1, C) - 1)).astype(np.float32)
    if zero_entry is not None:
        prior_dW[zero_entry] = add_dW[zero_entry] = 0.0
    want_dx = form.outs in ("both", "dx")
    want_dW = form.outs in ("both", "dW")
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    coef = dev(cf)
    coef_w = None if form.coef_w is None else dev(cw)
    gout = None if form.gout is None else torch.tensor([form.gout], dtype=torch.float32, device="cuda")
    addend = dev(add_dx) if form.addend and want_dx else None
    dW_addend = dev(add_dW) if form.dW_addend and want_dW else None
    runs = []
    for _ in range(2):
        dx = dW = None
        if want_dx:
            dx = dev(prior_dx) if form.accumulate else torch.full_like(xt, float("nan"))
        if want_dW:
            dW = dev(prior_dW) if form.accumulate else torch.full_like(Wt, float("nan"))
        with _empty_means_nan():
            E.dense_grad(xt, Wt, st, coef, coef_w=coef_w, gout=gout, dx=dx, accumulate=form.accumulate, dW=dW,
                         addend=addend, dW_addend=dW_addend)
        runs.append((dx, dW))
    (dx, dW), (dx2, dW2) = runs
    tag = f"{group}_{form.name}_{form.outs}"
    out_dx = out_dW = None
    if want_dx:
        exp = g * cf.astype(np.float64)[:, None, None] * case.post
        if form.accumulate:
            exp = exp + prior_dx
        if form.addend:
            exp = exp + g * add_dx.astype(np.float64)
        out_dx = dx.cpu().numpy()
        check(f"dense_grad_{group}_C{C}_dx", out_dx, exp, sx)
        assert torch.equal(dx, dx2), f"{tag}: dx differs between two runs of the same call"
        for b in case.dead:
            if not form.accumulate and not form.addend:
                assert not out_dx[b].any(), (tag, b, float(np.abs(out_dx[b]).max()))
    if want_dW:
        if form.coef_w == "s":
            post_w = case.dW_spread
        else:
            post_w = case.dW_ones * (1.0 if form.coef_w is None else form.coef_w)
        exp = g * post_w
        if form.accumulate:
            exp = exp + prior_dW
        if form.dW_addend:
            exp = exp + g * add_dW.astype(np.float64)
        out_dW = dW.cpu().numpy()
        check(f"dense_grad_{group}_C{C}_dW", out_dW, exp, sw)
        assert torch.equal(dW, dW2), f"{tag}: dW differs between two runs of the same call (the reduction order is fixed)"
        if zero_entry is not None:
            assert out_dW[zero_entry] == 0.0, (tag, out_dW[zero_entry])
    return out_dx, out_dW


def _logz(group, case, st):
    got = st.logz.cpu().numpy().astype(np.float64)
    alive = np.array([b not in case.dead for b in range(len(got))])
    assert (got[~alive] == NEG).all(), (group, got[~alive])
    check(f"dense_grad_{group}_logz", got[alive], case.logz[alive], 0.0)


# =================================================================================================
# A. frame chunks
# =================================================================================================
# (B, T, chunks, rows per chunk, rows of the last chunk that has any, empty chunks)
CHUNK_ROWS = [
    (128, 9, 4, 3, 3, 1),       # an empty trailing chunk
    (128, 65, 4, 17, 14, 0),    # TS + 1 at TS = 16, 2 TS + 1 at TS = 8
    (171, 97, 3, 33, 31, 0),    # 2 TS + 1 in the matrix-core loop: X, Y, X again
    (256, 31, 2, 16, 15, 0),    # exactly TS, then TS - 1
    (511, 20, 2, 10, 10, 0),    # just below the one-chunk switch
    (512, 20, 1, 20, 20, 0),    # one chunk per utterance
    (513, 20, 1, 20, 20, 0),
    (40, 27, 13, 3, 3, 4),      # several empty chunks
    (8, 250, 64, 4, 2, 1),      # the training-batch pattern, scaled down
    (1, 600, 512, 2, 2, 212),   # one utterance, mostly empty grid
    (3, 1, 1, 1, 1, 0),         # only start posteriors
    (3, 2, 2, 1, 1, 0),
]


def _assert_chunking(B, T, C, chunks, rows=None, last=None, empty=None):
    """the grid this file's shapes were chosen for: a change of dense_chunks shows here, as shapes to choose anew"""
    from gtn_applications_amd import engine as E

    assert E._dense_sizes(B, T, C)[0] == B * chunks * (C + 1) * C, (B, T, C, chunks, E._dense_sizes(B, T, C)[0])
    assert chunks == _chunks(B, T)
    if rows is not None:
        used = -(-T // rows)
        assert rows == -(-T // chunks) and empty == chunks - used and last == T - (used - 1) * rows


@pytest.mark.parametrize("B,T,chunks,rows,last,empty,C", [r + (C,) for r in CHUNK_ROWS for C in CLASSES])
def test_gradient_across_frame_chunks(B, T, chunks, rows, last, empty, C):
    """Every chunk pattern of CHUNK_ROWS in every kernel family, nothing flagged: dx + dW, dx alone, dW alone (at 64 /
    104 / 128 padded classes: the matrix-core launch, the vector-pipe launch, the matrix-core launch without dx)."""
    from gtn_applications_amd import engine as E

    _assert_chunking(B, T, C, chunks, rows, last, empty)
    case, xt, Wt, st = _forward("clean", B, T, C)
    assert not E.dense_flagged(st).any()
    _logz("A_chunks", case, st)
    for outs in ("both", "dx", "dW"):
        _, dW = _run_form("A_chunks", case, xt, Wt, st, PLAIN._replace(outs=outs))
        if T == 1 and dW is not None:
            assert not dW[1:].any()  # no transition was taken


# =================================================================================================
# B. call forms
# =================================================================================================
FORM_SHAPES = [(40, 27, 13), (128, 65, 4)]


@pytest.mark.parametrize("B,T,chunks,C,form", [(B, T, k, C, f) for B, T, k in FORM_SHAPES for C in CLASSES for f in FORMS],
                         ids=lambda v: v.name if isinstance(v, Form) else str(v))
def test_gradient_call_forms(B, T, chunks, C, form):
    """wfl_dense_grad's arguments against the formula: with accumulate (and without dW) the 64 / 104 / 128 buckets leave
    the matrix-core launch for dense_fast_grad_kernel<64 / 104 / 128>."""
    from gtn_applications_amd import engine as E

    _assert_chunking(B, T, C, chunks)
    case, xt, Wt, st = _forward("clean", B, T, C)
    assert not E.dense_flagged(st).any()
    _run_form("B_forms", case, xt, Wt, st, form)


# =================================================================================================
# C. the log-domain gradient
# =================================================================================================
LOG_ROWS = [CHUNK_ROWS[0], CHUNK_ROWS[1], CHUNK_ROWS[5]]  # an empty chunk, ragged chunks of 17 frames, one chunk of 20
assert [r[:2] for r in LOG_ROWS] == [(128, 9), (128, 65), (512, 20)]
LOG_CASES = [(C, "both") for C in (20, 50, 100, 150, 192)] + [(150, "dx")]  # NP = 4, 16, 40, 64 x 2, 64 x 3; NP = 4 without dW


@pytest.mark.parametrize("B,T,chunks,C,outs", [r[:3] + c for r in LOG_ROWS for c in LOG_CASES])
def test_log_domain_gradient_variants(B, T, chunks, C, outs):
    """W[1+4, 7] = -inf: every utterance is flagged and dense_grad_kernel<NP> writes the whole gradient -- each NP, the
    several passes over the frames beyond 128 classes, the emission-only launch; the forbidden transition's gradient is
    exactly zero."""
    from gtn_applications_amd import engine as E

    _assert_chunking(B, T, C, chunks)
    case, xt, Wt, st = _forward("forbidden", B, T, C)
    assert all(case.flagged) and E.dense_flagged(st).all()
    _logz("C_log", case, st)
    for form in (PLAIN, ALL):
        _run_form("C_log", case, xt, Wt, st, form._replace(outs=outs), zero_entry=(1 + 4, 7))


# =================================================================================================
# D. mixed batches
# =================================================================================================
@pytest.mark.parametrize("B,T,chunks,C", [(B, T, k, C) for B, T, k in FORM_SHAPES for C in (50, 100, 150)])
def test_mixed_batch_clean_flagged_and_dead(B, T, chunks, C):
    """Every third utterance holds a -inf emission (flagged: the log-domain launches serve it), one utterance an
    impossible frame (dead: zero rows, no share in dW), the rest take the probability-domain launches -- one partial
    buffer, one reduction.  The dead utterance's neighbours do not notice it: bit for bit the rows they get beside a
    clean utterance in its place."""
    from gtn_applications_amd import engine as E

    _assert_chunking(B, T, C, chunks)
    rs = np.random.RandomState(B + T + C)
    x = (2.0 * rs.randn(B, T, C)).astype(np.float32)
    W = rs.randn(C + 1, C).astype(np.float32)
    for b in range(0, B, 3):
        x[b, (5 * b + 1) % T, (3 * b) % C] = NEG
    x[3, T - 1, 4] = np.nan  # (NaN counts as -inf; utterance 3 is flagged already)
    dead = B // 2 + (1 if (B // 2) % 3 == 0 else 0)
    assert dead % 3 != 0
    x_alive = x.copy()
    x[dead, T // 2, :] = NEG
    results = []
    for inp, dead_set in ((x, (dead,)), (x_alive, ())):
        case = _make_case(inp, W, dead=dead_set)
        assert case.flagged == [b % 3 == 0 or b in dead_set for b in range(B)]
        xt, Wt = torch.from_numpy(inp).cuda(), torch.from_numpy(W).cuda()
        st = E.dense_forward(xt, Wt, need_beta=True)
        assert E.dense_flagged(st).cpu().tolist() == case.flagged
        _logz("D_mixed", case, st)
        results.append(_run_form("D_mixed", case, xt, Wt, st, PLAIN))
    (dx_dead, _), (dx_alive, _) = results
    assert not dx_dead[dead].any()
    others = [b for b in range(B) if b != dead]
    assert np.array_equal(dx_dead[others], dx_alive[others])


# =================================================================================================
# E. beyond the on-chip limit
# =================================================================================================
@pytest.mark.parametrize("B,T,C", [(B, T, C) for C in (200, 321) for B, T in ((3, 12), (70, 9))])
def test_call_forms_beyond_the_on_chip_limit(B, T, C):
    """193 classes and more: csrc/dense_wide.h's gradient takes the same arguments (its class and length edges:
    tests/test_gpu_dense_wide.py)."""
    from gtn_applications_amd import engine as E

    case, xt, Wt, st = _forward("wide", B, T, C)
    assert not E.dense_flagged(st).any()
    _logz("E_wide", case, st)
    for form in (ALL, PLAIN._replace(outs="dx"), PLAIN._replace(outs="dW")):
        _run_form("E_wide", case, xt, Wt, st, form)


# =================================================================================================
# F. ASG end to end
# =================================================================================================
@pytest.mark.parametrize("B,T,C", [(40, 27, 28), (128, 65, 100), (8, 250, 100), (40, 27, 150), (128, 65, 150), (8, 250, 150)])
def test_asg_loss_over_chunked_gradients(B, T, C):
    """ASGLoss on leaf tensors: the gradient launched behind the forward sweeps (addend = the numerator's gradient, no
    gout), then on a retained graph a first pass scaled by -2.5 and a second, recomputed one (gout = 0.5, both addends)."""
    from gtn_applications_amd.criterions import asg

    rs = np.random.RandomState(31 * B + T + C)
    x = (2.0 * rs.randn(B, T, C)).astype(np.float32)
    W = rs.randn(C + 1, C).astype(np.float32)
    targets = [rs.randint(0, C, size=rs.randint(1, min(T, 12) + 1)).tolist() for _ in range(B)]
    losses, want_dx, want_dW = OR.asg_loss_grad_batched(x, W, targets)
    assert np.isfinite(losses).all()
    leaves = lambda: (torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(W).cuda().requires_grad_(True))  # noqa: E731
    name = f"dense_grad_F_asg_C{C}"
    xg, Wg = leaves()
    loss = asg.ASGLoss(xg, Wg, targets, "none")
    loss.backward()
    check(name + "_loss", np.array([loss.item()]), np.array([losses.mean()]), 0.0)
    check(name + "_dx", xg.grad.cpu().numpy(), want_dx, 1.0 / B)
    check(name + "_dW", Wg.grad.cpu().numpy(), want_dW, 1.0 / B)
    xg, Wg = leaves()
    loss = asg.ASGLoss(xg, Wg, targets, "none")
    (loss * GOUT).sum().backward(retain_graph=True)
    check(name + "_dx", xg.grad.cpu().numpy(), GOUT * want_dx, abs(GOUT) / B)
    check(name + "_dW", Wg.grad.cpu().numpy(), GOUT * want_dW, abs(GOUT) / B)
    xg.grad = Wg.grad = None
    (loss * 0.5).sum().backward()
    check(name + "_dx", xg.grad.cpu().numpy(), 0.5 * want_dx, 0.5 / B)
    check(name + "_dW", Wg.grad.cpu().numpy(), 0.5 * want_dW, 0.5 / B)
