"""CTC on padded batches (criterions/ctc.py `input_lengths`) on the GPU: the loss and gradient of a batch with lengths
against the float64 oracle run on every utterance's own slice x[b:b+1, :T_b] (oracle.recurrences.ctc_loss_grad; never the
package), for CTCLoss on log-probabilities and the CTC module on raw scores (fused log_softmax), blank at 0 and at C - 1.

The bar is tests/test_gpu_configs.py's: per-utterance loss within 1e-4 relative, every gradient element within
1e-4 |want| + 2e-5 |coef_b| (coef_b = scale_b / B), pad rows == 0.0 exactly.  Per-utterance losses are read through the
engine (the step's nll of the shape), the mean and the gradients through the public calls.  With WFL_WORST_CASES=<file>
the worst measured ratio to the bar of every case is written there (profiles/ctc_lengths_parity_worst_cases.json).

The shapes put T_b on both sides of the 16-frame blocks and of the middle of the sweep, at 1 and at T; take the longest
single-lane target (63 labels), more sweeps than compute units, rows wider than a wave's registers, the log-domain
launch, targets beyond 63 and 255 labels, a call without gradient and emissions that are float64 on the host."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import criteria as OC
from oracle import recurrences as OR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4
ATOL_SCALE = 2e-5
WORST = {}


def _mods():
    from gtn_applications_amd import engine as E
    from gtn_applications_amd.criterions import ctc

    return E, ctc


def record(case, ratio):
    """the worst ratio to the bar per case; the child process under WFL_CTC_PIPELINE=log keeps records of its own"""
    if os.environ.get("WFL_CTC_PIPELINE") == "log":
        case += "_logdomain"
    if ratio > WORST.get(case, -1.0):
        WORST[case] = float(ratio)
        path = os.environ.get("WFL_WORST_CASES")
        if path:
            old = {}
            if os.path.exists(path):
                with open(path) as f:
                    old = json.load(f)
            old[case] = {"max_err_over_tol": max(WORST[case], old.get(case, {}).get("max_err_over_tol", -1.0))}
            with open(path, "w") as f:
                json.dump(old, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------------------------------
# cases: (B, T, C, lengths, target lengths); the data and the oracle's answer are made once per (case, blank, kind)
# ---------------------------------------------------------------------------------------------------------------------
def _targets(rs, C, blank, lens):
    lo, hi = (1, C) if blank == 0 else (0, C - 1)
    return [rs.randint(lo, hi, size=n).tolist() for n in lens]


def case_edges(blank):
    """block and half edges: 16-frame blocks, the middle of the sweep; targets of 0 .. 6 labels"""
    B, T, C = 12, 80, 20
    lengths = [80, 79, 65, 64, 63, 49, 48, 33, 17, 16, 5, 1]
    rs = np.random.RandomState(100 + blank)
    targets = _targets(rs, C, blank, [6, 5, 4, 6, 3, 2, 6, 1, 4, 3, 5, 0])
    a, b = (3, 7) if blank == 0 else (2, 5)
    targets[0][2] = targets[0][3] = a  # adjacent repeats where there is room for them
    targets[3][0] = targets[3][1] = targets[3][2] = b
    targets[8][1] = targets[8][2] = a
    targets[10] = [a, b, b, a, b]  # 5 labels, one repeat: 6 frames needed, T_b = 5 -- but T = 80 would do
    if blank:
        targets[11] = []  # the empty target at T_b = 1
    else:
        targets[11] = [a]  # one label at T_b = 1
    return B, T, C, lengths, targets


def case_edges_b(blank):
    """case_edges with the other choice at T_b = 1 (one label / the empty target) -- both blanks see both"""
    B, T, C, lengths, targets = case_edges(blank)
    targets = [list(t) for t in targets]
    targets[11] = [4] if blank else []
    return B, T, C, lengths, targets


def case_l63(blank):
    B, T, C = 4, 160, 70
    rs = np.random.RandomState(200 + blank)
    return B, T, C, [160, 129, 128, 127], _targets(rs, C, blank, [63, 63, 40, 63])


def case_many(blank):
    B, T, C = 130, 48, 8
    rs = np.random.RandomState(300 + blank)
    lengths = rs.randint(1, 49, size=B).tolist()
    return B, T, C, lengths, _targets(rs, C, blank, rs.randint(0, 7, size=B).tolist())


def case_wide(blank):
    B, T, C = 4, 64, 160
    rs = np.random.RandomState(400 + blank)
    return B, T, C, [64, 50, 32, 9], _targets(rs, C, blank, [9, 6, 0, 3])


def case_l70(blank):
    B, T, C = 3, 200, 30
    rs = np.random.RandomState(500 + blank)
    return B, T, C, [200, 150, 141], _targets(rs, C, blank, [70, 64, 70])


def case_l260(blank):
    B, T, C = 2, 600, 12
    rs = np.random.RandomState(600 + blank)
    return B, T, C, [600, 521], _targets(rs, C, blank, [100, 260])


CASES = {"edges": case_edges, "edges_b": case_edges_b, "l63": case_l63, "many": case_many, "wide": case_wide,
         "l70": case_l70, "l260": case_l260}
_MADE = {}


def expected(case, blank_last, kind):
    """(x float32 [B,T,C], targets, lengths, blank, want losses [B] (scaled), want dx [B,T,C] float64 with zero pad rows,
    coef [B]) -- kind "loss": x holds log-probabilities, CTCLoss(x, ..., "mean"); kind "module": x holds raw scores, the
    CTC module.  The pad frames of x hold ordinary scores: the criterion must not look at them."""
    key = (case, blank_last, kind)
    hit = _MADE.get(key)
    if hit is not None:
        return hit
    B, T, C, lengths, targets = CASES[case](1 if blank_last else 0)
    blank = C - 1 if blank_last else 0
    rs = np.random.RandomState(7 + sum(map(ord, case)) + 2 * blank_last + (kind == "module"))
    x = rs.randn(B, T, C).astype(np.float32)
    if kind == "loss":
        x = OC.log_softmax(x.astype(np.float64)).astype(np.float32)
    x64 = x.astype(np.float64)
    lp = x64 if kind == "loss" else OC.log_softmax(x64)
    losses, dx, coef = np.zeros(B), np.zeros((B, T, C)), np.zeros(B)
    for b, n in enumerate(lengths):
        loss_b, dlp = OR.ctc_loss_grad(lp[b:b + 1, :n], [targets[b]], blank, "mean")
        losses[b] = loss_b
        coef[b] = (1.0 / len(targets[b]) if targets[b] else 1.0) / B
        dlp = dlp[0] / B  # (the slice was a batch of one: ctc_loss_grad divided by 1)
        if kind == "module":  # through the log_softmax: dlp - softmax * sum_c dlp
            dlp = dlp - np.exp(lp[b, :n]) * dlp.sum(axis=1, keepdims=True)
        dx[b, :n] = dlp
    hit = _MADE[key] = (x, targets, lengths, blank, losses, dx, coef)
    return hit


def run_public(kind, xt, targets, blank, lengths):
    _, ctc = _mods()
    if kind == "loss":
        return ctc.CTCLoss(xt, targets, blank, "mean", lengths)
    return ctc.CTC(blank, False)(xt, [torch.tensor(t, dtype=torch.long) for t in targets], lengths)


def check_losses(name, got, want):
    worst = 0.0
    for b, (g, w) in enumerate(zip(got, want)):
        if math.isinf(w):
            assert g == w, (name, b, g, w)
        else:
            err = abs(g - w) / (RTOL * max(abs(w), 1e-300))
            print(f"{name}: utterance {b} loss {g!r} want {w!r} ratio {err:.4f}")
            worst = max(worst, err)
    print(f"{name}: worst loss ratio to the bar {worst:.4f}")
    record(name + "_loss", worst)
    assert worst <= 1.0, (name, worst)


def check_grad(name, grad, want, coef, lengths):
    got = grad.detach().double().cpu().numpy()
    assert got.shape == want.shape
    assert not np.isnan(got).any(), name
    for b, n in enumerate(lengths):
        assert (got[b, n:] == 0.0).all(), (name, "pad rows of utterance", b)
    tol = RTOL * np.abs(want) + ATOL_SCALE * np.abs(coef)[:, None, None]
    ratio = float((np.abs(got - want) / tol).max())
    print(f"{name}: worst gradient ratio to the bar {ratio:.4f}")
    record(name + "_dx", ratio)
    assert ratio <= 1.0, (name, ratio)


def step_nll(x_like, targets, scale=True):
    """the per-utterance nll the last pipelined step of this shape left (the operator's workspace of the stream), as
    mean-reduced losses; and how many utterances its repair launch recomputed"""
    E, _ = _mods()
    B, T, _ = x_like.shape
    max_len = max((len(t) for t in targets), default=0)
    torch.cuda.synchronize()
    ws, nll = E.ctc_workspace(x_like, max_len)
    repaired = E.ctc_pipeline_repaired(ws, B, T, max_len)
    out = nll.double().cpu().numpy()
    if scale:
        out = out / np.array([len(t) if t else 1 for t in targets], dtype=np.float64)
    return out, repaired


def mean_of(losses):
    return float(np.mean(losses))


def lattice_nll(xt, kind, targets, lengths, blank):
    """per-utterance mean-reduced losses of targets beyond the fast path: the route CTCLossFunction takes for them, by
    hand -- pad a copy, the lattice engine's forward sweep (its scores stay inside the operator otherwise)"""
    E, _ = _mods()
    lp = (xt if kind == "loss" else torch.log_softmax(xt, dim=2)).contiguous()
    xlen = E.input_lengths_on_device(lengths, xt.device)
    tg = E.targets_on_device(targets, xt.device)
    pack = E.PackedLattice.ctc(tg.flat, tg.offsets, blank, xt.shape[2], xt.device)
    st = E.lattice_forward(E.ctc_pad_frames(lp, xlen, blank), pack, need_beta=False)
    return -st.logz.double().cpu().numpy() / np.array([len(t) if t else 1 for t in targets], dtype=np.float64)


def run_case(case, blank_last, kind, device_step=True):
    x, targets, lengths, blank, want_losses, want_dx, coef = expected(case, blank_last, kind)
    name = f"{case}_{kind}_blank{'C-1' if blank_last else '0'}"
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    loss = run_public(kind, xt, targets, blank, lengths)
    if device_step:
        got, repaired = step_nll(xt.detach(), targets)
        print(f"{name}: ctc_pipeline_repaired {repaired}")
        check_losses(name, got.tolist(), want_losses.tolist())
    else:
        check_losses(name, lattice_nll(xt.detach(), kind, targets, lengths, blank).tolist(), want_losses.tolist())
    want_mean = mean_of(want_losses)
    if math.isinf(want_mean):
        assert loss.item() == want_mean
    else:
        assert loss.item() == pytest.approx(want_mean, rel=RTOL)
    loss.backward()
    check_grad(name, xt.grad, want_dx, coef, lengths)
    return xt.grad.detach().clone(), loss.detach().clone()


KINDS = ["loss", "module"]
BLANKS = [False, True]


# 1. block and half edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
@pytest.mark.parametrize("case", ["edges", "edges_b"])
def test_block_and_half_edges(case, blank_last, kind):
    """T_b at 80, 79, 65, 64, 63, 49, 48, 33, 17, 16, 5, 1 of T = 80; the utterance with T_b = 5 and five labels with a
    repeat cannot be aligned in its frames (it could in T): loss +inf, zero rows, and the mean is +inf with it"""
    x, targets, lengths, blank, want_losses, want_dx, coef = expected(case, blank_last, kind)
    assert math.isinf(want_losses[10]) and not want_dx[10].any()
    assert np.isfinite(np.delete(want_losses, 10)).all()
    full, _ = OR.ctc_loss_grad((x if kind == "loss" else OC.log_softmax(x.astype(np.float64)))[10:11], [targets[10]], blank)
    assert math.isfinite(full)
    run_case(case, blank_last, kind)


# 2. the longest single-lane target --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
def test_longest_single_lane_target(blank_last, kind):
    run_case("l63", blank_last, kind)


# 3. more sweeps than compute units --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
def test_more_sweeps_than_compute_units(blank_last, kind):
    run_case("many", blank_last, kind)


# 4. wide rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
def test_wide_rows(blank_last, kind):
    run_case("wide", blank_last, kind)


# 5. the log-domain launch, 8. WFL_CTC_FAST_BACKWARD=0: one fresh child process each ---------------------------------
CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_ctc_lengths as M
for kind in M.KINDS:
    for blank_last in M.BLANKS:
        M.run_case("edges", blank_last, kind)
print("CHILD-OK")
"""


def _child(env_name, env_value):
    env = dict(os.environ)
    env[env_name] = env_value
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "CHILD-OK" in r.stdout
    return r.stdout


def test_log_domain_launch():
    """case 1 under WFL_CTC_PIPELINE=log (read once per process): ctc_log_chain_body and ctc_grad_body serve the step and
    substitute the certain-blank frames themselves (CtcArgs.xlen; no padded copy).  (Their REPAIR instantiation only
    runs when a certificate doubts: ctc_pipeline_repaired is printed by every case, not required.)"""
    out = _child("WFL_CTC_PIPELINE", "log")
    repaired = [int(v) for v in re.findall(r"ctc_pipeline_repaired (\d+)", out)]
    print("ctc_pipeline_repaired under the log-domain launch:", repaired)  # (recorded, not required: the step repairs nothing)


def test_engine_backward_in_a_child_process():
    _child("WFL_CTC_FAST_BACKWARD", "0")


@pytest.mark.parametrize("blank_last", BLANKS)
def test_forward_and_grad_entries_with_lengths(blank_last):
    """wfl_ctc_forward_lengths / wfl_ctc_grad_lengths (the log-domain chain and gradient launches, lengths read in the
    launch: no padded copy) on case 1 through the C ABI"""
    import ctypes

    from gtn_applications_amd import _native as N

    E, _ = _mods()
    x, targets, lengths, blank, want_losses, want_dx, coef = expected("edges", blank_last, "loss")
    name = f"edges_abi_blank{'C-1' if blank_last else '0'}"
    xt = torch.tensor(x, device="cuda")
    B, T, C = x.shape
    tg = E.targets_on_device(targets, xt.device)
    xlen = E.input_lengths_on_device(lengths, xt.device)
    n = ctypes.c_int64()
    N.check(N.lib.wfl_ctc_workspace(B, T, C, tg.max_len, ctypes.byref(n)))
    ws = torch.empty(n.value, dtype=torch.float32, device="cuda")
    nll = torch.empty(B, dtype=torch.float32, device="cuda")
    N.check(N.lib.wfl_ctc_forward_lengths(E.ptr(xt), B, T, C, E.ptr(tg.dev_flat), E.ptr(tg.dev_offsets), tg.max_len, blank, 0,
                                          E.ptr(ws), E.ptr(nll), E.ptr(xlen), E.stream_ptr()))
    got = nll.double().cpu().numpy() / np.array([len(t) if t else 1 for t in targets], dtype=np.float64)
    check_losses(name, got.tolist(), want_losses.tolist())
    _, _, cneg = E.loss_factors(tg, "mean")
    dx = torch.zeros_like(xt)
    N.check(N.lib.wfl_ctc_grad_lengths(E.ptr(xt), B, T, C, E.ptr(tg.dev_flat), E.ptr(tg.dev_offsets), tg.max_len, blank,
                                       E.ptr(ws), E.ptr(nll), E.ptr(cneg), None, E.ptr(dx), E.ptr(xlen), E.stream_ptr()))
    E.zero_pad_rows(dx, xlen)
    check_grad(name, dx, want_dx, coef, lengths)
    # without lengths the entries are told so; targets beyond 63 labels are not theirs
    assert N.lib.wfl_ctc_forward_lengths(E.ptr(xt), B, T, C, E.ptr(tg.dev_flat), E.ptr(tg.dev_offsets), tg.max_len, blank, 0,
                                         E.ptr(ws), E.ptr(nll), None, E.stream_ptr()) == N.ERR_INVALID
    assert N.lib.wfl_ctc_forward_lengths(E.ptr(xt), B, T, C, E.ptr(tg.dev_flat), E.ptr(tg.dev_offsets), 64, blank, 0,
                                         E.ptr(ws), E.ptr(nll), E.ptr(xlen), E.stream_ptr()) == N.ERR_UNSUPPORTED


# 6. the copy route: what no kernel with lengths of its own covers ---------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
def test_targets_beyond_one_lane(blank_last, kind):
    run_case("l70", blank_last, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
def test_targets_beyond_the_fast_path(blank_last, kind):
    """260 labels: the lattice engine; the per-utterance losses are read from its forward sweep on the padded copy, the
    mean and the gradient through the public call"""
    run_case("l260", blank_last, kind, device_step=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
def test_loss_only_under_no_grad(blank_last, kind):
    E, ctc = _mods()
    x, targets, lengths, blank, want_losses, _, _ = expected("edges", blank_last, kind)
    xt = torch.tensor(x, device="cuda")
    with torch.no_grad():
        loss = run_public(kind, xt, targets, blank, lengths)
    assert not loss.requires_grad and loss.item() == mean_of(want_losses) == math.inf
    # per utterance: the same route by hand (pad a copy, the forward launch the call without gradient takes)
    lp = xt if kind == "loss" else torch.log_softmax(xt, dim=2)
    xlen = E.input_lengths_on_device(lengths, xt.device)
    tg = E.targets_on_device(targets, xt.device)
    _, nll = E.ctc_forward(E.ctc_pad_frames(lp.contiguous(), xlen, blank), tg, blank)
    got = nll.double().cpu().numpy() / np.array([len(t) if t else 1 for t in targets], dtype=np.float64)
    check_losses(f"edges_nograd_{kind}_blank{'C-1' if blank_last else '0'}", got.tolist(), want_losses.tolist())
    # and a batch without the utterance that cannot be aligned: a finite mean through the public call
    keep = [b for b in range(len(targets)) if b != 10]
    with torch.no_grad():
        loss = run_public(kind, xt[keep].contiguous(), [targets[b] for b in keep], blank, [lengths[b] for b in keep])
    assert loss.item() == pytest.approx(mean_of(want_losses[keep]), rel=RTOL)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
def test_float64_host_emissions(blank_last, kind):
    x, targets, lengths, blank, want_losses, want_dx, coef = expected("edges", blank_last, kind)
    name = f"edges_f64cpu_{kind}_blank{'C-1' if blank_last else '0'}"
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    loss = run_public(kind, xt, targets, blank, lengths)
    assert loss.device.type == "cpu" and loss.item() == math.inf
    # (the module's log_softmax ran on the host in float64; the step behind it is the same shape's, on its output)
    got, _ = step_nll(torch.empty(x.shape, device="cuda"), targets)
    check_losses(name, got.tolist(), want_losses.tolist())
    loss.backward()
    assert xt.grad.dtype == torch.float64 and xt.grad.device.type == "cpu"
    check_grad(name, xt.grad, want_dx, coef, lengths)


@pytest.mark.parametrize("kind,dtype,where", [("loss", torch.float64, "cpu"), ("module", torch.float64, "cpu"),
                                              ("loss", torch.float64, "cuda"), ("module", torch.float64, "cuda"),
                                              ("loss", torch.float16, "cuda")])
@pytest.mark.parametrize("B", [1, 3])
def test_other_dtypes_are_taken_with_lengths_whatever_the_lengths_are(B, dtype, where, kind):
    """Emissions that are not float32 are taken whenever input_lengths is passed -- also for a batch of one and for a
    batch whose lengths all equal T, where nothing is padded; without the argument they are a TypeError as before."""
    _, ctc = _mods()
    T, C, blank = 20, 6, 5
    rs = np.random.RandomState(31 + B)
    x = rs.randn(B, T, C).astype(np.float32)
    if kind == "loss":
        x = OC.log_softmax(x.astype(np.float64)).astype(np.float32)
    x = torch.tensor(x).to(dtype).double().numpy()  # (what the emissions hold once they are of `dtype`)
    targets = [rs.randint(0, C - 1, size=n).tolist() for n in (4, 0, 7)[:B]]
    lp = x if kind == "loss" else OC.log_softmax(x)
    want_loss, want_dx = OR.ctc_loss_grad(lp, targets, blank, "mean")
    if kind == "module":
        want_dx = want_dx - np.exp(lp) * want_dx.sum(axis=2, keepdims=True)
    coef = np.array([(1.0 / len(t) if t else 1.0) / B for t in targets])
    half = dtype == torch.float16  # the gradient comes back rounded to the emissions' dtype: 2^-11 relative
    for lengths in ([T] * B, torch.full((B,), T)):
        xt = torch.tensor(x, dtype=dtype, device=where, requires_grad=True)
        loss = run_public(kind, xt, targets, blank, lengths)
        assert loss.item() == pytest.approx(want_loss, rel=RTOL)
        loss.backward()
        assert xt.grad.dtype == dtype and xt.grad.device.type == where
        if not half:
            check_grad(f"fullT_{kind}_{str(dtype)[6:]}_{where}_B{B}", xt.grad, want_dx, coef, [T] * B)
        else:
            got = xt.grad.double().cpu().numpy()
            assert np.abs(got - want_dx).max() <= 2.0 ** -10 * np.abs(want_dx).max() + ATOL_SCALE * coef.max()
    with pytest.raises(TypeError):
        ctc.CTCLoss(torch.tensor(x, dtype=dtype, device=where), targets, blank, "mean")


# 7. inert when full -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["edges", "bench_like"])
def test_lengths_that_all_equal_T_are_the_call_without_lengths(shape, kind):
    if shape == "edges":
        x, targets, _, blank, _, _, _ = expected("edges", True, kind)
    else:
        rs = np.random.RandomState(9)
        x = rs.randn(128, 64, 100).astype(np.float32)
        if kind == "loss":
            x = OC.log_softmax(x.astype(np.float64)).astype(np.float32)
        targets, blank = [rs.randint(0, 99, size=rs.randint(0, 20)).tolist() for _ in range(128)], 99
    B, T, _ = x.shape
    outs = []
    for lengths in (None, [T] * B, torch.full((B,), T, dtype=torch.int64), torch.full((B,), T, dtype=torch.int32, device="cuda")):
        xt = torch.tensor(x, device="cuda", requires_grad=True)
        loss = run_public(kind, xt, targets, blank, lengths)
        loss.backward()
        outs.append((loss.detach().cpu(), xt.grad.cpu()))
    for loss, grad in outs[1:]:
        assert torch.equal(loss, outs[0][0]) and torch.equal(grad, outs[0][1])


# 8. autograd paths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blank_last", BLANKS)
def test_autograd_paths_give_the_same_gradient(blank_last, kind):
    x, targets, lengths, blank, want_losses, want_dx, coef = expected("edges", blank_last, kind)
    name = f"edges_autograd_{kind}_blank{'C-1' if blank_last else '0'}"
    base, _ = run_case("edges", blank_last, kind)  # loss.backward() on a leaf

    xt = torch.tensor(x, device="cuda", requires_grad=True)  # an upstream gradient
    run_public(kind, xt, targets, blank, lengths).backward(torch.tensor(2.0, device="cuda"))
    check_grad(name + "_x2", xt.grad / 2, want_dx, coef, lengths)

    leaf = torch.tensor(x, device="cuda", requires_grad=True)  # emissions that are a producer's output
    run_public(kind, leaf * 1.0, targets, blank, lengths).backward()
    check_grad(name + "_producer", leaf.grad, want_dx, coef, lengths)

    xt = torch.tensor(x, device="cuda", requires_grad=True)  # a retained graph backwarded twice
    loss = run_public(kind, xt, targets, blank, lengths)
    loss.backward(retain_graph=True)
    first = xt.grad.clone()
    xt.grad = None
    loss.backward()
    check_grad(name + "_retained_1", first, want_dx, coef, lengths)
    check_grad(name + "_retained_2", xt.grad, want_dx, coef, lengths)
    for other in (first, xt.grad, leaf.grad):  # the same gradient every time, to the bar's absolute term
        assert float((other - base).abs().max()) <= 2 * ATOL_SCALE * float(np.abs(coef).max())


# 9. decode and errors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank_last", BLANKS)
def test_viterbi_and_errors_stop_at_the_lengths(blank_last):
    E, ctc = _mods()
    from gtn_applications_amd import metrics as M

    K = E.decode_chunk_frames()
    T, C = 2 * K + 5, 11
    lengths = [K - 1, K, K + 1, 2 * K, 1, T, 2 * K + 1, K + 2]
    B = len(lengths)
    blank = C - 1 if blank_last else 0
    rs = np.random.RandomState(17 + blank_last)
    # peaked emissions: runs of 1 .. 4 frames of one class, blanks among them, so that runs cross the ends and the chunks
    labels = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        t = 0
        while t < T:
            n = rs.randint(1, 5)
            labels[b, t:t + n] = rs.randint(0, C)
            t += n
    for b, n in enumerate(lengths):  # the run at the end of the utterance goes on into the padding, or a new label starts there
        if n < T and b % 2 == 0:
            labels[b, n:n + 3] = labels[b, n - 1]
    x = rs.randn(B, T, C).astype(np.float32)
    x[np.arange(B)[:, None], np.arange(T)[None, :], labels] += 8.0
    for b, n in enumerate(lengths):  # garbage in the pad frames: huge scores for labels, a NaN (torch.argmax's maximum)
        x[b, n:, (blank + 1 + b) % C] += 50.0
        if n + 1 < T:
            x[b, n + 1, (blank + 3) % C] = np.nan
    xt = torch.tensor(x, device="cuda")
    crit = ctc.CTC(blank, False)
    want = [crit.viterbi(xt[b:b + 1, :n].contiguous())[0] for b, n in enumerate(lengths)]
    assert any(len(w) for w in want)
    for form in (lengths, tuple(lengths), torch.tensor(lengths), torch.tensor(lengths, dtype=torch.int32, device="cuda")):
        got = crit.viterbi(xt, form)
        assert len(got) == B
        for b in range(B):
            assert got[b].dtype == want[b].dtype and got[b].tolist() == want[b].tolist(), (b, lengths[b])
    # the C ABI entry itself (what a binding calls; viterbi() reaches it through the operator library)
    import ctypes

    from gtn_applications_amd import _native as N

    cap, nws = ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib.wfl_decode_workspace(B, T, 0, ctypes.byref(cap), ctypes.byref(nws)))
    out = torch.full((cap.value + 8,), -99, dtype=torch.int32, device="cuda")
    offs = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(nws.value, dtype=torch.uint8, device="cuda")
    xlen = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    N.check(N.lib.wfl_decode_emissions_lengths(E.ptr(xt), None, E.ptr(xlen), B, T, C, blank, 0, N.DECODE_NAN_IS_MAX,
                                               E.ptr(scratch), E.ptr(out), cap.value, E.ptr(offs), E.stream_ptr()))
    torch.cuda.synchronize()
    o, f = offs.cpu().numpy(), out.cpu().numpy()
    assert o[0] == 0 and (f[o[B]:] == -99).all()
    assert [f[o[b]:o[b + 1]].tolist() for b in range(B)] == [w.tolist() for w in want]
    whole = crit.viterbi(xt)
    assert any(whole[b].tolist() != want[b].tolist() for b in range(B))  # the padding does decode to something
    host = crit.viterbi(xt.cpu(), lengths)  # the host route takes the lengths too
    assert [h.tolist() for h in host] == [w.tolist() for w in want]
    targets = [rs.randint(1 if blank == 0 else 0, C if blank == 0 else C - 1, size=rs.randint(0, 30)).tolist() for _ in range(B)]
    counter = M.ErrorCounter()
    assert crit.errors(xt, targets, counter, lengths) == counter(want, targets)
    assert crit.errors(xt, targets, counter, [T] * B) == crit.errors(xt, targets, counter)
