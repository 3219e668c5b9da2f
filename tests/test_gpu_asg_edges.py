"""The ASG criterion end to end (criterions/asg.py, csrc/torch_ops.cpp::asg_forward, the force-aligned numerator of the
lattice engine with arcs that index W, the dense denominator) at its edges: targets as long as the input, longer, empty,
one label repeated; one and two frames; one class, the class counts where the dense launches change kernels; numerators
around 64 and 128 states beside a one-label utterance; the numerator on the streamed sweeps; one utterance and more
utterances than compute units; every call form; the module's replabel / garbage packing; utterances without an alignment
beside ones that have one.

Reference: oracle.recurrences.asg_loss_grad (float64) on the same float32 inputs, pinned here against the graph
restatement oracle.criteria.asg on two small cases.  Bars (tests/test_gpu_parity.py): loss 1e-4 relative, dx
1e-4 |want| + 1e-5, dW 1e-4 |want| + 2e-5, whatever grad_output scales the gradient by.

An utterance no alignment fits whatever the scores (L_b > T, L_b = 0): the loss is exactly +inf, its
rows of dx are exactly 0.0, and it has no share in dW.  The oracle does not say that -- its denominator term stays in
the row and in dW -- so `expectation()` builds it: the oracle on the live sub-batch, times B_live / B.

ASGLoss returns the batch mean under both reductions (asg.py:116-121): an utterance's own loss is that of a batch of one.
With WFL_WORST_CASES=<file> the worst error / tolerance of every case is written there
(profiles/asg_edges_parity_worst_cases.json)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import criteria as OC
from oracle import recurrences as OR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
RTOL, ATOL_DX, ATOL_DW = 1e-4, 1e-5, 2e-5
INF = float("inf")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _mods():
    from gtn_applications_amd import engine as E
    from gtn_applications_amd.criterions import asg

    return E, asg


# ---------------------------------------------------------------------------------------------------------------------
# record, bars
# ---------------------------------------------------------------------------------------------------------------------
def record(case, ratio=None, **notes):
    """the worst ratio to the bar per case (and figures that are reported, not asserted)"""
    rec = WORST.setdefault(case, {"max_err_over_tol": -1.0})
    changed = False
    if ratio is not None and ratio > rec["max_err_over_tol"]:
        rec["max_err_over_tol"], changed = float(ratio), True
    for k, v in notes.items():
        if rec.get(k) != v:
            rec[k], changed = v, True
    path = os.environ.get("WFL_WORST_CASES")
    if changed and path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        new = dict(old.get(case, {}), **rec)
        new["max_err_over_tol"] = max(rec["max_err_over_tol"], old.get(case, {}).get("max_err_over_tol", -1.0))
        old[case] = new
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def check(case, what, got, want, atol, rtol=RTOL):
    """|got - want| <= rtol |want| + atol, elementwise; the worst ratio goes to the record"""
    got = got.detach().cpu().double().numpy() if hasattr(got, "detach") else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (case, what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{case} {what}: not finite"
    err = np.abs(got - want)
    tol = rtol * np.abs(want) + atol
    ratio = err / tol
    k = int(np.argmax(ratio)) if ratio.size else 0
    worst = float(ratio.flat[k]) if ratio.size else 0.0
    print(f"{case} {what}: worst err/tol {worst:.4g}")
    record(case, worst)
    assert worst <= 1.0, (f"{case} {what}: |{got.flat[k]:.9g} - {want.flat[k]:.9g}| = {err.flat[k]:.3g} > {tol.flat[k]:.3g} "
                          f"at flat index {k}")


def check_loss(case, got, want):
    got = float(got)
    print(f"{case} loss: got {got!r} want {want!r}")
    if want == INF:
        assert got == INF, f"{case}: loss {got!r}, want +inf"
        return
    ratio = abs(got - want) / (RTOL * abs(want)) if want != 0.0 else (0.0 if got == 0.0 else INF)
    record(case, ratio)
    assert ratio <= 1.0, f"{case}: loss {got!r}, want {want!r} (err/tol {ratio:.3g})"


# ---------------------------------------------------------------------------------------------------------------------
# data, expectation, the step in its call forms
# ---------------------------------------------------------------------------------------------------------------------
def draw(seed, B, T, C):
    rs = np.random.RandomState(seed)
    return rs, rs.randn(B, T, C).astype(np.float32), (0.5 * rs.randn(C + 1, C)).astype(np.float32)


def is_dead(target, T):
    return len(target) == 0 or len(target) > T


_EXPECT = {}


def expectation(name, x, W, targets, reduction):
    """(loss, dx, dW, dead rows) the policy asks for; made once per name, read-only"""
    key = (name, reduction)
    if key not in _EXPECT:
        B, T, _ = x.shape
        dead = [b for b in range(B) if is_dead(targets[b], T)]
        live = [b for b in range(B) if not is_dead(targets[b], T)]
        assert live, "a case needs a live utterance"
        loss, dxl, dW = OR.asg_loss_grad(x[live], W, [list(targets[b]) for b in live], reduction)
        # the oracle alone, on the live sub-batch: finite, and (but for one class, where the gradient is zero) not lost
        # below the bars' absolute terms
        assert np.isfinite(loss) and np.isfinite(dxl).all() and np.isfinite(dW).all(), name
        assert x.shape[2] == 1 or (np.abs(dxl).max() > 10 * ATOL_DX and np.abs(dW).max() > 10 * ATOL_DW), name
        f = len(live) / B
        dx = np.zeros(x.shape)
        dx[live] = dxl * f
        dW = dW * f
        dx.setflags(write=False), dW.setflags(write=False)
        _EXPECT[key] = (INF if dead else loss, dx, dW, dead)
    return _EXPECT[key]


FORMS = ("leaves", "nonleaf", "late", "only_x", "only_w", "retain", "cpu")


def step(x, W, targets, reduction, form="leaves", monkeypatch=None):
    """One ASG step in a call form -> [(loss, grad_output, dx | None, dW | None), ...] (numpy; `retain` gives two)"""
    E, asg = _mods()
    device = "cpu" if form == "cpu" else "cuda"
    xt = torch.tensor(x, device=device, requires_grad=form != "only_w")
    Wt = torch.tensor(W, device=device, requires_grad=form != "only_x")

    def grads():
        out = tuple(None if t.grad is None else t.grad.detach().cpu().double().numpy() for t in (xt, Wt))
        xt.grad = Wt.grad = None
        return out

    if form == "late":
        monkeypatch.setattr(asg, "_EARLY_GRAD", False)
    if form == "nonleaf":
        loss = asg.ASGLoss(xt * 1.0, Wt * 1.0, targets, reduction)
        (loss * 0.75).backward()
        return [(loss.item(), 0.75) + grads()]
    loss = asg.ASGLoss(xt, Wt, targets, reduction)
    # the forward's gradient buffers are offered exactly where the form says so
    assert (type(loss) is E.EagerLoss) == (form not in ("late", "cpu")), (form, type(loss))
    assert loss.device.type == device
    if form == "retain":
        loss.backward(retain_graph=True)
        first = (loss.item(), 1.0) + grads()
        loss.backward()  # (the buffers are taken: the gradient kernels again, behind fork.join)
        return [first, (loss.item(), 1.0) + grads()]
    loss.backward()
    return [(loss.item(), 1.0) + grads()]


def compare(case, x, W, targets, reduction, form="leaves", monkeypatch=None):
    """a step in `form` against the policy's expectation; returns the step's first (loss, dx, dW)"""
    want_loss, want_dx, want_dW, dead = expectation(case, x, W, targets, reduction)
    results = step(x, W, targets, reduction, form, monkeypatch)
    for k, (loss, g, dx, dW) in enumerate(results):
        tag = f"{case}[{reduction},{form}{',second' if k else ''}]"
        check_loss(tag, loss, want_loss)
        assert (dx is None) == (form == "only_w") and (dW is None) == (form == "only_x"), tag
        if dx is not None:
            for b in dead:
                assert (dx[b] == 0.0).all(), f"{tag}: dead utterance {b} has a gradient, max |dx| {np.abs(dx[b]).max():.3g}"
            check(tag, "dx", dx, g * want_dx, ATOL_DX)
        if dW is not None:
            check(tag, "dW", dW, g * want_dW, ATOL_DW)
    return results[0][0], results[0][2], results[0][3]


def own_losses(case, x, W, targets, reduction):
    """every live utterance's own loss: batches of one against the oracle's batch of one"""
    _, asg = _mods()
    Wd = torch.tensor(W, device="cuda")
    for b, t in enumerate(targets):
        xb = x[b:b + 1]
        got = asg.ASGLoss(torch.tensor(xb, device="cuda"), Wd, [list(t)], reduction).item()
        want = OR.asg_loss_grad(xb, W, [list(t)], reduction)[0]
        check_loss(f"{case}[{reduction},own {b}]", got, want if not is_dead(t, x.shape[1]) else INF)


def dense64(x, W):
    """the denominator of one utterance by the plain recursion in float64: (log Z, state posteriors [T, C])"""
    x, W = np.asarray(x, dtype=np.float64), np.asarray(W, dtype=np.float64)
    T, C = x.shape
    lse = lambda a, axis: np.logaddexp.reduce(a, axis=axis)  # noqa: E731
    alpha, beta = np.empty((T, C)), np.zeros((T, C))
    alpha[0] = x[0] + W[0]
    for t in range(1, T):
        alpha[t] = x[t] + lse(alpha[t - 1][None, :] + W[1:], 1)  # W[1 + cur, prev]
    for t in range(T - 2, -1, -1):
        beta[t] = lse((beta[t + 1] + x[t + 1])[:, None] + W[1:], 0)
    logz = lse(alpha[T - 1], 0)
    return float(logz), np.exp(alpha + beta - logz)


# ---------------------------------------------------------------------------------------------------------------------
# the two references pin each other
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_the_two_oracles_agree(reduction):
    """oracle.recurrences.asg_loss_grad against the graph restatement oracle.criteria.asg: a batch with L = T, a repeated
    label and classes 0 and C - 1 in first and later positions; and the smallest shapes (T = 2, C = 2)"""
    for seed, T, C, targets in ((1, 5, 4, [[3, 0, 0, 3, 1], [2, 2], [0, 3], [3]]), (2, 2, 2, [[1, 1], [0], [1, 0]])):
        _, x, W = draw(seed, len(targets), T, C)
        a, b = OR.asg_loss_grad(x, W, targets, reduction), OC.asg(x, W, targets, reduction)
        assert a[0] == pytest.approx(b[0], rel=1e-12)
        np.testing.assert_allclose(a[1], b[1], rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(a[2], b[2], rtol=1e-9, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# target edges (C = 6, T = 8)
# ---------------------------------------------------------------------------------------------------------------------
def _target_edge_batch():
    C, T = 6, 8
    rs, x, W = draw(601, 8, T, C)
    targets = [[3],                                   # L = 1
               rs.randint(0, C, size=T - 1).tolist(),  # L = T - 1
               rs.randint(0, C, size=T).tolist(),      # L = T: one alignment
               [2, 2],                                 # one label twice: the advance arc shares W[1 + c, c] with the loop
               [4] * T,                                # ... and as long as the input
               [0, 5, 0, 5, 5, 0],                     # classes 0 and C - 1, first and later (W[0, c] | W[1 + c, prev])
               [5, 0, 0, 5],
               [1, 2, 3]]
    return x, W, targets


@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_target_edges(reduction):
    x, W, targets = _target_edge_batch()
    compare("target_edges", x, W, targets, reduction)
    own_losses("target_edges", x, W, targets, reduction)


@pytest.mark.parametrize("b", [2, 4], ids=["random", "one_label"])
def test_target_as_long_as_the_input_has_one_alignment(b):
    """L = T: loss = log Z_dense - sum of the scores along the target, and the numerator's share of dx is one-hot"""
    x, W, targets = _target_edge_batch()
    y, (T, C) = targets[b], x.shape[1:]
    assert len(y) == T
    x64, W64 = x[b].astype(np.float64), W.astype(np.float64)
    along = sum(x64[t, y[t]] + (W64[0, y[0]] if t == 0 else W64[1 + y[t], y[t - 1]]) for t in range(T))
    logz, post = dense64(x[b], W)
    loss, dx, _ = compare(f"single_alignment_{b}", x[b:b + 1], W, [y], "none")
    check_loss(f"single_alignment_{b}[closed form]", loss, logz - along)
    onehot = np.zeros((T, C))
    onehot[np.arange(T), y] = 1.0
    check(f"single_alignment_{b}", "numerator share", post - dx[0], onehot, ATOL_DX)


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_one_and_two_frames(T, reduction):
    C = 6
    targets = [[2], [5], [0]] if T == 1 else [[1], [1, 1], [0, 5], [5, 0], [3]]
    _, x, W = draw(610 + T, len(targets), T, C)
    _, dx, dW = compare(f"frames_{T}", x, W, targets, reduction)
    own_losses(f"frames_{T}", x, W, targets, reduction)
    if T == 1:
        # no frame follows another: only the start row is used, and each utterance adds cf (posteriors) - cf (its label)
        assert (dW[1:] == 0.0).all()
        cf = 1.0 / len(targets)
        labels = np.zeros(C)
        for (c,) in targets:
            labels[c] += cf
        assert abs((dW[0] + labels).sum() - len(targets) * cf) <= ATOL_DW * C
        assert abs(dW[0].sum()) <= ATOL_DW * C


# ---------------------------------------------------------------------------------------------------------------------
# class edges
# ---------------------------------------------------------------------------------------------------------------------
def test_one_class():
    """C = 1: every alignment has the denominator's only path's score, loss = -log (number of alignments) =
    -log C(T - 1, L - 1), gradients zero"""
    T, L = 7, 3
    _, x, W = draw(701, 1, T, 1)
    for reduction in ("none", "mean"):
        loss, dx, dW = compare("one_class", x, W, [[0] * L], reduction)
        want = -math.log(math.comb(T - 1, L - 1)) / (L if reduction == "mean" else 1)
        assert OR.asg_loss_grad(x, W, [[0] * L], reduction)[0] == pytest.approx(want, rel=1e-13)
        check_loss(f"one_class[{reduction},closed form]", loss, want)
        assert np.abs(dx).max() <= ATOL_DX and np.abs(dW).max() <= ATOL_DW


@pytest.mark.parametrize("C", [2, 3, 64, 65, 192, 193, 320, 321])
def test_class_edges(C):
    """2, 3: the smallest matrices; 64 | 65: a class bucket's last and the next one's first; 192 | 193: the on-chip limit;
    320 | 321: the register-resident wide sweep against the per-frame product.  Ragged targets with label C - 1 first and
    last."""
    B, T = 2, 12
    rs, x, W = draw(700 + C, B, T, C)
    targets = [rs.randint(0, C, size=n).tolist() for n in (3, 9)]
    targets[0][0] = targets[1][-1] = C - 1
    targets[1][0] = 0
    for reduction in ("none", "mean"):
        compare(f"classes_{C}", x, W, targets, reduction)


# ---------------------------------------------------------------------------------------------------------------------
# numerator size edges, the streamed numerator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [63, 64, 65, 127, 128, 129])
def test_numerator_sizes_beside_one_label(L):
    """L + 1 states around one and two waves, beside an utterance of two states (ragged max_states)"""
    C, B, T = 10, 3, L + 3
    rs, x, W = draw(800 + L, B, T, C)
    targets = [rs.randint(0, C, size=L).tolist(), [int(rs.randint(C))], rs.randint(0, C, size=L // 2).tolist()]
    compare(f"numerator_{L}", x, W, targets, "mean")


def _streamed_launches():
    from gtn_applications_amd import _native as N
    import ctypes

    out = (ctypes.c_uint64 * 9)()
    N.check(N.lib.wfl_lattice_diagnostics(out, 9))
    return int(out[8])


def _streamed_numerator():
    """runs in a child process under WFL_LATTICE_STREAMED: the force-aligned numerator, whose arcs index W, on the
    L2-streamed sweeps and their gradient"""
    C, B, T = 10, 3, 30
    rs, x, W = draw(850, B, T, C)
    targets = [rs.randint(0, C, size=n).tolist() for n in (27, 1, 12)]
    targets[2][3:6] = [7, 7, 7]
    mode = os.environ["WFL_LATTICE_STREAMED"]
    for form in ("leaves", "only_x"):
        before = _streamed_launches()
        compare(f"streamed_{mode}", x, W, targets, "mean", form)
        torch.cuda.synchronize()
        assert _streamed_launches() - before >= 2, "the numerator's sweeps and gradient were not streamed"


@pytest.mark.parametrize("mode", [1, 2])
def test_numerator_on_the_streamed_sweeps(mode):
    """forced as tests/test_gpu_lattice_streamed.py::test_forced_streamed_path forces them (the variable is read once per
    process): 1 = state vectors in LDS, 2 = in global memory"""
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_asg_edges as m; m._streamed_numerator()"
    env = dict(os.environ, WFL_LATTICE_STREAMED=str(mode))
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail(f"WFL_LATTICE_STREAMED={mode}: no result within 120 s")
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"WFL_LATTICE_STREAMED={mode}: status {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"


# ---------------------------------------------------------------------------------------------------------------------
# batch edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_batch_of_one(reduction):
    rs, x, W = draw(900, 1, 8, 6)
    compare("batch_1", x, W, [rs.randint(0, 6, size=4).tolist()], reduction)


def test_more_utterances_than_compute_units():
    """B = 300 on 256 CUs, L drawn in 0 .. T + 2: about a fifth of the utterances have no alignment, spread through
    the batch"""
    B, T, C = 300, 12, 8
    rs, x, W = draw(901, B, T, C)
    targets = [rs.randint(0, C, size=rs.randint(0, T + 3)).tolist() for _ in range(B)]
    dead = [b for b in range(B) if is_dead(targets[b], T)]
    assert 30 <= len(dead) <= 80 and dead[0] < 20 and dead[-1] >= B - 20
    assert any(len(targets[b]) == 0 for b in dead) and any(len(targets[b]) > T for b in dead)
    assert any(len(t) == T for t in targets)
    compare("batch_300", x, W, targets, "mean")


# ---------------------------------------------------------------------------------------------------------------------
# utterances without an alignment
# ---------------------------------------------------------------------------------------------------------------------
def _dead_batch():
    C, T = 6, 8
    rs, x, W = draw(1001, 5, T, C)
    targets = [[4], rs.randint(0, C, size=T).tolist(), rs.randint(0, C, size=T + 1).tolist(), [1, 1, 3, 0], []]
    return x, W, targets


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_call_forms_with_dead_utterances(reduction, form, monkeypatch):
    """[L = 1, L = T, L = T + 1 (dead), ordinary, L = 0 (dead)]: every form of the call sees the same expectation, scaled
    by its grad_output -- leaves (the forward's buffers become .grad), non-leaf inputs under 0.75 (the node scales those
    buffers), the gradient kernels in backward, one gradient only, a second backward (the recompute route), CPU tensors"""
    x, W, targets = _dead_batch()
    compare("dead", x, W, targets, reduction, form, monkeypatch)


def test_neighbours_do_not_notice_a_dead_utterance():
    """the live rows of a batch with a dead utterance against the same batch with a live one in its place"""
    x, W, targets = _dead_batch()
    _, dx_dead, _ = compare("dead", x, W, targets, "mean")
    alive = list(targets)
    alive[2], alive[4] = targets[2][:5], [2]
    _, dx_live, _ = compare("dead_replaced", x, W, alive, "mean")
    rows = [0, 1, 3]
    check("neighbours", "dx", dx_dead[rows], dx_live[rows], ATOL_DX)


@pytest.mark.parametrize("form", ["leaves", "late", "retain"])
def test_a_frame_without_a_finite_score(form, monkeypatch):
    """One frame of an utterance is all -inf: denominator and numerator are both -inf.  The loss is +inf, not NaN
    (reduce_loss_kernel: -inf - -inf), that row is exactly zero, it has no share in dW, the neighbours meet the bar;
    alone in a batch of one the utterance's loss is +inf as well."""
    _, asg = _mods()
    C, T = 6, 8
    rs, x, W = draw(1002, 3, T, C)
    targets = [rs.randint(0, C, size=n).tolist() for n in (3, 4, 8)]
    x[1, 5, :] = -np.inf
    live = [0, 2]
    want = OR.asg_loss_grad(x[live], W, [targets[b] for b in live], "mean")
    assert np.isfinite(want[0])
    for k, (loss, _, dx, dW) in enumerate(step(x, W, targets, "mean", form, monkeypatch)):
        tag = f"dead_frame[{form}{',second' if k else ''}]"
        check_loss(tag, loss, INF)
        assert (dx[1] == 0.0).all(), f"{tag}: max |dx| of the dead row {np.abs(dx[1]).max():.3g}"
        check(tag, "dx", dx[live], want[1] * (2 / 3), ATOL_DX)
        check(tag, "dW", dW, want[2] * (2 / 3), ATOL_DW)
    alone = asg.ASGLoss(torch.tensor(x[1:2], device="cuda"), torch.tensor(W, device="cuda"), [targets[1]], "none").item()
    assert alone == INF, alone


def test_a_numerator_dead_by_its_scores_only():
    """OPEN: L = T and the first label's emission is -inf, so the only alignment is impossible while
    the denominator lives.  The host cannot see that before the launch; asserted are the loss and the neighbours' rows,
    the utterance's own row is written to the record, not judged."""
    C, T = 6, 8
    rs, x, W = draw(1003, 3, T, C)
    targets = [rs.randint(0, C, size=n).tolist() for n in (3, T, 5)]
    x[1, 0, targets[1][0]] = -np.inf
    live = [0, 2]
    want = OR.asg_loss_grad(x[live], W, [targets[b] for b in live], "mean")
    (loss, _, dx, dW), = step(x, W, targets, "mean")
    check_loss("data_dead", loss, INF)
    check("data_dead", "dx", dx[live], want[1] * (2 / 3), ATOL_DX)
    own = float(np.abs(dx[1]).max())
    print(f"data_dead: max |dx| of the utterance's own row {own:.6g} (not asserted)")
    record("data_dead", own_row_abs_max=own, own_row_abs_sum=float(np.abs(dx[1]).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# the module: replabels and garbage
# ---------------------------------------------------------------------------------------------------------------------
MODULE_TARGETS = [[0, 0, 0, 0, 0, 1],          # a run of five: longer than 1 + num_replabels covers, for all three counts
                  [2, 2, 3, 3, 3],
                  [1, 0, 1],
                  [],                          # with garbage [g]: live; without: no accepting node
                  [0, 1, 2, 3, 0, 1, 2, 3],    # L = 8 <= T; with garbage 2 L + 1 = 17 > T = 14: dead
                  [3]]


@pytest.mark.parametrize("use_garbage", [True, False], ids=["garbage", "plain"])
@pytest.mark.parametrize("num_replabels", [1, 2, 3])
def test_module_packing(num_replabels, use_garbage):
    """ASG.forward: tensor targets (pack_targets_batch, the whole batch as array operations) and the same targets as a tuple
    of arrays (pack_replabels row by row: that route calls t.tolist() on every row as asg.py:202 does, so rows are arrays
    here, not Python lists) against the oracle on oracle.criteria.asg_module_targets"""
    _, asg = _mods()
    nc, T = 4, 14
    m = asg.ASG(nc, num_replabels, use_garbage).cuda()
    rs, x, W = draw(1100 + 2 * num_replabels + use_garbage, len(MODULE_TARGETS), T, m.N)
    with torch.no_grad():
        m.transitions.copy_(torch.from_numpy(W))
    packed = OC.asg_module_targets(MODULE_TARGETS, nc, num_replabels, use_garbage)
    assert packed[3] == ([nc + num_replabels] if use_garbage else [])
    assert [is_dead(p, T) for p in packed] == [False, False, False, not use_garbage, use_garbage, False]
    assert [t.tolist() for t in asg.pack_targets_batch([torch.tensor(t, dtype=torch.int64) for t in MODULE_TARGETS],
                                                       num_replabels, m.garbage_idx)] == packed
    case = f"module_r{num_replabels}_{'garbage' if use_garbage else 'plain'}"
    want_loss, want_dx, want_dW, dead = expectation(case, x, W, packed, "mean")
    got = {}
    routes = {"tensors": [torch.tensor(t, dtype=torch.int64) for t in MODULE_TARGETS],
              "rows": tuple(np.asarray(t, dtype=np.int64) for t in MODULE_TARGETS)}
    for route, targets in routes.items():
        xt = torch.tensor(x, device="cuda", requires_grad=True)
        m.transitions.grad = None
        loss = m(xt, targets)
        loss.backward()
        dx, dW = xt.grad.cpu().double().numpy(), m.transitions.grad.cpu().double().numpy()
        tag = f"{case}[{route}]"
        check_loss(tag, loss.item(), want_loss)
        for b in dead:
            assert (dx[b] == 0.0).all(), (tag, b)
        check(tag, "dx", dx, want_dx, ATOL_DX)
        check(tag, "dW", dW, want_dW, ATOL_DW)
        got[route] = (loss.item(), dx, dW)
    check_loss(f"{case}[tensors against rows]", got["tensors"][0], got["rows"][0])
    check(case, "dx, tensors against rows", got["tensors"][1], got["rows"][1], ATOL_DX)
    check(case, "dW, tensors against rows", got["tensors"][2], got["rows"][2], ATOL_DW)


# ---------------------------------------------------------------------------------------------------------------------
# what ASG.beam_search rests on
# ---------------------------------------------------------------------------------------------------------------------
def test_beam_search_score_is_minus_the_loss_of_the_raw_sequence():
    """C = 5, T = 6, the widest beam (64) over all five classes: the normalised score of the best raw sequence is minus
    ASGLoss of that sequence (a batch of one) at the loss bar -- also where the best sequence has L = T (utterance 2: a
    path of six changing classes lifted by 4).  No beam of 64 keeps every prefix here (5 + 20 + 80 are alive at the
    third frame), so "nothing pruned" is established per utterance by the plain-Python search of
    tests/asg_beam_reference.py under the same beam: the best sequence is the one of highest mass among ALL sequences
    (enumerated), and its score there is its whole mass to 1e-9 -- none of ITS alignments is dropped.  The seed is one
    where that holds for the three utterances (with the first seed tried, one lost 2.4 % of its loss to the beam: a
    lower bound, as ASG.beam_search documents, and no statement about the loss)."""
    import asg_beam_reference as R

    E, asg = _mods()
    C, T = 5, 6
    _, x, W = draw(1228, 3, T, C)
    x[2, np.arange(T), [3, 0, 4, 1, 2, 0]] += 4.0
    xd, Wd = torch.tensor(x, device="cuda"), torch.tensor(W, device="cuda")
    hyps, scores = E.asg_beam_search(xd, Wd, 64, C, 1, normalize=True)
    for b in range(3):
        seq = hyps[b][0].tolist()
        best, mass = R.brute_force(x[b], W)[0]
        ref, margin, _ = R.beam_search(x[b], W, 64, C, 1)
        assert ref[0][0] == best and abs(ref[0][1] - mass) <= 1e-9 and margin >= 1e-9, (b, ref, best, mass, margin)
        assert tuple(seq) == best, (b, seq, best)
        minus_loss = -asg.ASGLoss(xd[b:b + 1], Wd, [seq], "none").item()
        oracle = -OR.asg_loss_grad(x[b:b + 1], W, [seq], "none")[0]
        assert mass - R.denominator(x[b], W) == pytest.approx(oracle, rel=1e-9)
        check_loss(f"beam_tie_in[{b},loss]", -minus_loss, -oracle)
        check_loss(f"beam_tie_in[{b},score]", -float(scores[b, 0]), -oracle)
        check_loss(f"beam_tie_in[{b},score against loss]", -float(scores[b, 0]), -minus_loss)
    assert len(hyps[2][0]) == T
