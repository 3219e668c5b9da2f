"""The CTC criterion (criterions/ctc.py, csrc/ctc_kernels.hip, csrc/ctc_mitm.h, csrc/torch_ops.cpp) at its label, frame and
layout edges: every launch of the step pinned to the float64 oracle and named; target labels equal to the blank index;
utterances with exactly one alignment, whose loss and gradient are known in closed form; emissions and gradients that
start on an odd float, time-major and expanded emissions; the call forms.

Reference: oracle.recurrences.ctc_loss_grad_batched (float64) on the same float32 inputs, pinned below -- with
ctc_loss_grad -- against the graph restatement oracle.criteria.ctc, once with the blank inside a target.  For the fused
log_softmax the oracle's log_softmax and the chain rule are added by hand; a NaN is read as -inf.

Bars (tests/test_gpu_parity.py): an utterance's loss 1e-4 relative with the golden tests' 1e-5 absolute floor; its gradient
1e-4 |want| + 1e-4 |coef_b grad_output| per element, coef_b = scale_b / B ("1e-4 of the gradient's scale").  An utterance
no alignment fits (T < L + adjacent repeats): loss exactly +inf, rows of dx exactly 0.0.  With WFL_WORST_CASES=<file> the
worst error / tolerance of every case is written there (profiles/ctc_edges_parity_worst_cases.json), and beside it the
gradient's worst ratio to 1e-4 |want| + 1e-5, which is reported, not asserted.

A target label equal to the blank index follows the reference's graph (ctc.py:15-29): the skip arc
into a label exists iff the label differs from the previous LABEL, blank or not.

What this file found: with input lengths, a target that ends in the blank label was scored too well -- the pad frames are
no identity for it (test_blank_labels_under_input_lengths and the layout cases with lengths).

Where this departs from a plain reading of its issue, for reasons of arithmetic: a target of at most 63 labels needs at
most 125 frames, so the repair rows (T = 200) have no infeasible utterance -- one label repeated takes its place; and a
batch whose longest target has L labels holds an infeasible one only while T <= 2 L - 2, so the long-target rows run at
T = 2 L - 3, not 2 L + 5.  The spread of the unstructured scores of the repair rows is REPAIR_SPREAD: 3.0 on all four
-- measured, the certificate rejects 2 of the 5 utterances of the dense row and 3 of 5 on the fused and compact rows at
3.0 already (and as many at 3.5 .. 5.0), so the compact rows needed no wider spread."""
import functools
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import criteria as OC
from oracle import recurrences as OR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
RTOL, ATOL_LOSS, FLAT_FLOOR = 1e-4, 1e-5, 1e-5
INF = float("inf")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _mods():
    from gtn_applications_amd import engine as E
    from gtn_applications_amd.criterions import ctc

    return E, ctc


# ---------------------------------------------------------------------------------------------------------------------
# record, bars
# ---------------------------------------------------------------------------------------------------------------------
def record(case, ratio=None, **notes):
    """the worst ratio to the bar per case (and figures that are reported, not asserted: kept at their maximum)"""
    rec = WORST.setdefault(case, {"max_err_over_tol": -1.0})
    changed = False
    if ratio is not None and ratio > rec["max_err_over_tol"]:
        rec["max_err_over_tol"], changed = float(ratio), True
    for k, v in notes.items():
        if k not in rec or v > rec[k]:
            rec[k], changed = v, True
    path = os.environ.get("WFL_WORST_CASES")
    if changed and path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        new = dict(old.get(case, {}))
        for k, v in rec.items():
            new[k] = max(v, new.get(k, v))
        old[case] = new
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def as64(a):
    return a.detach().cpu().double().numpy() if hasattr(a, "detach") else np.asarray(a, dtype=np.float64)


def check_losses(case, got, want):
    """every utterance's own loss: +inf exactly where the oracle has +inf, |got - want| <= 1e-4 |want| + 1e-5 elsewhere"""
    got, want = np.atleast_1d(as64(got)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (case, got.shape, want.shape)
    worst = 0.0
    for b, (g, w) in enumerate(zip(got, want)):
        if w == INF:
            assert g == INF, f"{case}: loss of utterance {b} is {g!r}, want +inf"
            continue
        assert np.isfinite(g), f"{case}: loss of utterance {b} is {g!r}, want {w!r}"
        ratio = abs(g - w) / (RTOL * abs(w) + ATOL_LOSS)
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{case}: loss of utterance {b} is {g!r}, want {w!r} (err/tol {ratio:.3g})"
    print(f"{case} loss: worst err/tol {worst:.4g}")
    record(case, worst)


def check_dx(case, got, want, coef, gout=1.0, dead=()):
    """|got - gout want| <= 1e-4 |gout want| + 1e-4 |coef_b gout| per element; rows of dead utterances exactly 0.0"""
    got, want = as64(got), np.asarray(want, dtype=np.float64) * gout
    assert got.shape == want.shape, (case, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{case} dx: not finite"
    for b in dead:
        assert (got[b] == 0.0).all(), f"{case}: infeasible utterance {b} has a gradient, max |dx| {np.abs(got[b]).max():.3g}"
    err = np.abs(got - want)
    tol = RTOL * np.abs(want) + RTOL * np.abs(np.asarray(coef, dtype=np.float64) * gout)[:, None, None]
    ratio = err / tol
    k = int(np.argmax(ratio))
    worst = float(ratio.flat[k])
    flat = float((err / (RTOL * np.abs(want) + FLAT_FLOOR)).max())
    print(f"{case} dx: worst err/tol {worst:.4g} (against the flat 1e-5 floor {flat:.4g})")
    record(case, worst, dx_over_flat_floor=flat)
    assert worst <= 1.0, (f"{case} dx: |{got.flat[k]:.9g} - {want.flat[k]:.9g}| = {err.flat[k]:.3g} > {tol.flat[k]:.3g} "
                          f"at {np.unravel_index(k, got.shape)}")


# ---------------------------------------------------------------------------------------------------------------------
# the oracle, the launches
# ---------------------------------------------------------------------------------------------------------------------
def needs(target):
    """frames the shortest alignment takes: L + adjacent repeats"""
    return len(target) + sum(1 for i in range(1, len(target)) if target[i] == target[i - 1])


def factors(targets, reduction):
    B = len(targets)
    return np.array([-(1.0 / len(t) if reduction == "mean" and len(t) else 1.0) / B for t in targets])


_ORACLE = {}


def oracle(key, x, targets, blank, reduction, fused=False, lengths=None):
    """(own losses [B], dx [B,T,C], coef [B], dead utterances) in float64; made once per key, read-only"""
    key = (key, blank, reduction, fused, None if lengths is None else tuple(lengths))
    if key not in _ORACLE:
        B, T, C = x.shape
        x64 = np.where(np.isnan(x), -np.inf, x).astype(np.float64)
        lp = OC.log_softmax(x64) if fused else x64
        if lengths is None:
            losses, dlp = OR.ctc_loss_grad_batched(lp, targets, blank, reduction)
        else:
            losses, dlp = np.zeros(B), np.zeros((B, T, C))
            for b, n in enumerate(lengths):
                own, g = OR.ctc_loss_grad_batched(lp[b:b + 1, :n], [targets[b]], blank, reduction, batch_size=B)
                losses[b], dlp[b, :n] = own[0], g[0]
        dx = dlp - np.exp(lp) * dlp.sum(axis=2, keepdims=True) if fused else dlp
        dead = [b for b, t in enumerate(targets) if needs(t) > (T if lengths is None else lengths[b])]
        assert [b for b in range(B) if losses[b] == INF] == dead, (key, dead, losses)
        assert np.isfinite(dx).all() and all((dx[b] == 0.0).all() for b in dead), key
        dx.setflags(write=False), losses.setflags(write=False)
        _ORACLE[key] = (losses, dx, factors(targets, reduction), dead)
    return _ORACLE[key]


def dev(x, grad=False):
    t = torch.tensor(np.asarray(x), dtype=torch.float32, device="cuda")
    return t.requires_grad_(True) if grad else t


def offset_view(x, grad=False):
    """the same values as a contiguous device tensor that starts on an odd float: what slicing a larger buffer gives"""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(x.shape)
    v.copy_(x)
    v = v.detach()
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v.requires_grad_(True) if grad else v


Served = namedtuple("Served", "own dx loss gave_up repaired ppl")


def step(xt, targets, blank, reduction, fused=False, gout=None, dx=None):
    """the pipelined step at the engine layer (wfl_ctc_forward_backward), from a forgotten launch preference"""
    E, _ = _mods()
    B, T, C = xt.shape
    tg = E.targets_on_device(targets, xt.device)
    scale, _, coef = E.loss_factors(tg, reduction)
    g = None if gout is None else torch.full((1,), gout, device="cuda")
    if dx is None:
        dx = torch.full_like(xt, float("nan"))
    E.ctc_reset_state()
    ws, nll, loss = E.ctc_forward_backward(xt, tg, blank, coef, g, dx, loss_scale=scale, want_loss=True,
                                           lse=E.row_lse(xt) if fused else None)
    torch.cuda.synchronize()
    own = (nll.double() * scale.double()).cpu().numpy()
    mean = float(own.mean())
    assert float(loss) == mean or abs(float(loss) - mean) <= 1e-5 * abs(mean), (float(loss), mean)
    return Served(own, dx, float(loss), E.ctc_pipeline_gave_up(ws, B, T, tg.max_len),
                  E.ctc_pipeline_repaired(ws, B, T, tg.max_len), (tg.max_len + 64) // 64)


def split_step(xt, targets, blank, reduction, gout=None):
    """the forward-only chains (wfl_ctc_forward) and the gradient launch behind them (wfl_ctc_grad)"""
    E, _ = _mods()
    tg = E.targets_on_device(targets, xt.device)
    scale, _, coef = E.loss_factors(tg, reduction)
    g = None if gout is None else torch.full((1,), gout, device="cuda")
    dx = torch.full_like(xt, float("nan"))
    ws, nll = E.ctc_forward(xt, tg, blank)
    E.ctc_grad(xt, tg, blank, ws, nll, coef, g, dx)
    return (nll.double() * scale.double()).cpu().numpy(), dx


def lattice_step(xt, targets, blank, reduction, gout=1.0):
    """the CTC label graphs on the lattice engine (PackedLattice.ctc), as CTCLoss runs them beyond the fast path"""
    E, _ = _mods()
    tg = E.targets_on_device(targets, xt.device)
    pack = E.PackedLattice.ctc(tg.flat, tg.offsets, blank, xt.shape[2], xt.device)
    scale, _, coef = E.loss_factors(tg, reduction)
    st = E.lattice_forward(xt, pack, need_beta=True)
    dx = torch.full_like(xt, float("nan"))
    E.lattice_grad(st, coef, gout=torch.full((1,), gout, device="cuda"), dx=dx)
    return (-st.logz.double() * scale.double()).cpu().numpy(), dx


def compute_units():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------------
# the two oracle functions against the graph restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_the_oracles_agree(reduction):
    """ctc_loss_grad and ctc_loss_grad_batched against oracle.criteria.ctc (minigtn's intersect of the emissions with
    ctc.py:15-29's graph): ordinary targets with a repeat and the empty target, blank last; and blank 4 inside, first,
    last, adjacent and alone in the targets"""
    for seed, T, C, blank, targets in ((1, 6, 5, 4, [[1, 1, 2], [0, 3], [], [2]]),
                                       (2, 6, 5, 4, [[1, 4, 2], [4, 4], [4], [4, 0, 0, 4], [3, 4, 4]])):
        x = np.random.RandomState(seed).randn(len(targets), T, C).astype(np.float32)
        graph = OC.ctc(x, targets, blank, reduction)
        plain = OR.ctc_loss_grad(x, targets, blank, reduction)
        own, dxb = OR.ctc_loss_grad_batched(x, targets, blank, reduction)
        assert plain[0] == pytest.approx(graph[0], rel=1e-12) and float(own.mean()) == pytest.approx(graph[0], rel=1e-12)
        np.testing.assert_allclose(plain[1], graph[1], rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(dxb, graph[1], rtol=1e-9, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# A. every launch, pinned and named
# ---------------------------------------------------------------------------------------------------------------------
REPAIR_SPREAD = {"dense": 3.0, "dense_fused": 3.0, "compact": 3.0, "compact_fused": 3.0}

Row = namedtuple("Row", "name many T C L fused spread kind")
ROWS = [
    # the meet-in-the-middle launch, ctc_mitm_kernel<MitmK<16 | 8>, fused, wide>: 16 waves while 2 B <= compute units
    Row("mitm16_dense", 0, 37, 100, 20, False, 1.0, "mitm"),
    Row("mitm16_dense_fused", 0, 48, 128, 26, True, 1.0, "mitm"),       # C = 128: the widest dense tile
    Row("mitm16_dense_unaligned", 0, 33, 30, 20, False, 1.0, "mitm"),   # C % 4 != 0: the emitter's unaligned stores
    Row("mitm16_dense_at_the_limit", -1, 35, 12, 20, False, 1.0, "mitm"),  # 2 B = compute units: still 16 waves
    Row("mitm16_wide", 0, 33, 132, 20, False, 1.0, "mitm"),
    Row("mitm16_wide_fused_63", 0, 70, 132, 63, True, 1.0, "mitm"),     # 63 labels: one position per lane, every lane
    Row("mitm8_dense", 1, 40, 30, 22, False, 1.0, "mitm"),
    Row("mitm8_dense_fused", 1, 35, 8, 20, True, 1.0, "mitm"),
    Row("mitm8_wide", 1, 34, 132, 19, False, 1.0, "mitm"),
    Row("mitm8_wide_fused", 1, 49, 132, 27, True, 1.0, "mitm"),
    # the repair launch behind it, ctc_repair_kernel<fused, compact>: unstructured scores fail the certificate
    Row("repair_dense", 0, 200, 40, 9, False, REPAIR_SPREAD["dense"], "repair"),
    Row("repair_dense_fused", 0, 200, 40, 9, True, REPAIR_SPREAD["dense_fused"], "repair"),
    Row("repair_compact", 0, 200, 132, 9, False, REPAIR_SPREAD["compact"], "repair"),
    Row("repair_compact_fused", 0, 200, 132, 9, True, REPAIR_SPREAD["compact_fused"], "repair"),
    # ctc_long_pipelined_kernel<2 | 3 | 4, fused>: 64 .. 255 labels, on both sides of every boundary
    Row("long2_64", 0, 125, 9, 64, False, 1.0, "long"),
    Row("long2_127_fused", 0, 251, 11, 127, True, 1.0, "long"),
    Row("long3_128_fused", 0, 253, 15, 128, True, 1.0, "long"),
    Row("long3_191", 0, 379, 13, 191, False, 1.0, "long"),
    Row("long4_192", 0, 381, 10, 192, False, 1.0, "long"),
    Row("long4_255_fused", 0, 507, 12, 255, True, 1.0, "long"),
    Row("long2_600_classes", 0, 125, 600, 64, False, 1.0, "long"),      # the dense tiles [17][C] at their class limit
    Row("long2_602_classes_fused", 0, 125, 602, 64, True, 1.0, "long"),
]
SHORT_ROWS = [r for r in ROWS if r.L <= 63]


def kit(rs, C, blank, T, L, B):
    """B utterances of five kinds in turn: the longest target with the blank label once inside; a ragged short one; the
    empty target; an infeasible one (one label n times, 2 n - 1 > T; where L admits none: one label L times); a short
    one with blank labels first, adjacent in the middle and last"""
    nb = [c for c in range(C) if c != blank]
    pick = lambda n: [nb[i] for i in rs.randint(0, len(nb), size=n)]  # noqa: E731
    n_dead = T // 2 + 2
    out = []
    for i in range(B):
        k = i % 5
        if k == 0:
            t = pick(L)
            t[L // 2] = blank
        elif k == 1:
            t = pick(int(rs.randint(1, min(L, 12) + 1)))
        elif k == 2:
            t = []
        elif k == 3:
            t = pick(1) * (n_dead if n_dead <= L else L)
        else:
            t = pick(min(L, 11))
            t[0] = t[len(t) // 2] = t[len(t) // 2 + 1] = t[-1] = blank
        assert (needs(t) > T) == (k == 3 and n_dead <= L), (k, needs(t), T)
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def row_data(row):
    """(x float32 [B,T,C] with one -inf and one NaN, targets, blank); B from the device's compute units where B selects"""
    cus = compute_units()
    B = {0: 5, 1: cus // 2 + 1, -1: cus // 2}[row.many]
    i = ROWS.index(row)
    rs = np.random.RandomState(4000 + i)
    blank = (0, row.C // 2, row.C - 1)[i % 3]
    x = (row.spread * rs.randn(B, row.T, row.C)).astype(np.float32)
    targets = kit(rs, row.C, blank, row.T, row.L, B)
    assert max(len(t) for t in targets) == row.L
    x[0, 3, (blank + 1) % row.C] = -np.inf
    x[4, 5, (blank + 2) % row.C] = np.nan
    x.setflags(write=False)
    return x, targets, blank


def judge_row(row, served, reduction, gout, tag=""):
    x, targets, blank = row_data(row)
    losses, dx, coef, dead = oracle(row.name, x, targets, blank, reduction, row.fused)
    assert dead or row.kind == "repair"
    case = f"launch_{row.name}{tag}"
    check_losses(f"{case}[{reduction}]", served.own, losses)
    check_dx(f"{case}[{reduction}]", served.dx, dx, coef, 1.0 if gout is None else gout, dead)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_launch_against_the_oracle(row):
    """One row per instantiation ctc_forward_backward_impl can launch (the log-domain pipelined launch: the next test):
      ctc_mitm_kernel<MitmK<16>, fused, wide> and <MitmK<8>, ...>   fused x wide, 2 B <= compute units | beyond
      ctc_repair_kernel<fused, compact>                             the certificate rejects; dense rows C <= 120 | compact
      ctc_long_pipelined_kernel<2 | 3 | 4, fused>                   64 .. 127 | 128 .. 191 | 192 .. 255 labels
    and, on the rows without the fusion, the launches of ctc_forward_impl and ctc_grad_impl behind one another:
      ctc_log_chain_kernel, ctc_long_chain_kernel<2 | 3 | 4>        the forward-only chains
      ctc_grad_kernel<compact>, ctc_long_grad_kernel<2 | 3 | 4>     the gradient launch behind them
    Each row asserts the selectors that ctc_forward_backward_impl reads (positions per lane, 2 B against the compute
    units, C against the dense tile of 128 and the dense log-domain rows of 120, row log-sum-exps or none) and what the
    launch reports: it did not give up; nothing was repaired on the lane-exponent and long rows; something on the
    repair rows.  Every batch has an empty, a ragged, an infeasible and a blank-labelled target, a -inf and a NaN."""
    x, targets, blank = row_data(row)
    B, T, C = x.shape
    xt = dev(x)
    for reduction, gout in (("none", 0.75), ("mean", None)):
        served = step(xt, targets, blank, reduction, row.fused, gout)
        assert not served.gave_up, row.name
        assert served.ppl == (1 if row.L <= 63 else 2 if row.L <= 127 else 3 if row.L <= 191 else 4)
        if row.kind == "mitm":
            assert (2 * B > compute_units()) == (row.many == 1) and ("wide" in row.name) == (C > 128)
            assert served.repaired == 0, f"{row.name}: {served.repaired} utterances went to the repair launch"
        elif row.kind == "repair":
            assert ("compact" in row.name) == (C > 120)
            print(f"{row.name}: spread {row.spread}, {served.repaired} of {B} utterances repaired")
            assert served.repaired >= 1, f"{row.name}: the certificate accepted scores of spread {row.spread}"
        else:
            assert served.repaired == 0
        judge_row(row, served, reduction, gout)
    if not row.fused:
        own, dx = split_step(xt, targets, blank, "mean", 0.75)
        judge_row(row, Served(own, dx, None, False, 0, 0), "mean", 0.75, "_split")


def _log_domain_child(path):
    """runs in a child process under WFL_CTC_PIPELINE=log: ctc_pipelined_kernel<fused, compact> on the short rows"""
    out = {}
    for row in SHORT_ROWS:
        x, targets, blank = row_data(row)
        served = step(dev(x), targets, blank, "mean", row.fused, 0.75)
        assert not served.gave_up and served.repaired == 0, (row.name, served.gave_up, served.repaired)
        out[row.name + ".own"], out[row.name + ".dx"] = served.own, served.dx.cpu().numpy()
    np.savez(path, **out)


def test_log_domain_pipelined_launch_against_the_oracle(tmp_path):
    """ctc_pipelined_kernel<fused, compact>, selected per process (WFL_CTC_PIPELINE=log, read once): the short rows of the
    table -- dense rows at C <= 120, compact beyond, with and without the fusion, B on both sides of the compute units --
    in ONE fresh child process, which reports that nothing gave up and nothing was repaired; its losses and gradients are
    compared with the oracle here"""
    path = str(tmp_path / "log_domain.npz")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_ctc_edges as m; "
            f"m._log_domain_child({path!r})")
    env = dict(os.environ, WFL_CTC_PIPELINE="log")
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=240, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail("WFL_CTC_PIPELINE=log: no result within 240 s")
    assert r.returncode == 0, f"WFL_CTC_PIPELINE=log: status {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    got = np.load(path)
    assert {(r.fused, r.C > 120) for r in SHORT_ROWS} == {(False, False), (False, True), (True, False), (True, True)}
    for row in SHORT_ROWS:
        judge_row(row, Served(got[row.name + ".own"], got[row.name + ".dx"], None, False, 0, 1), "mean", 0.75, "_logdomain")


def test_one_class_beyond_the_dense_tiles_goes_to_the_lattice_engine(monkeypatch):
    """C = 603 with a 64-label target: one class more than ctc_long_pipelined_kernel's tiles hold.  CTCLoss moves to the
    lattice engine (asserted: lattice_forward is called, the fast path refuses the shape) and still meets the bar."""
    E, ctc = _mods()
    C, L, T = 603, 64, 125
    rs = np.random.RandomState(4603)
    blank = C // 2
    x = rs.randn(5, T, C).astype(np.float32)
    targets = kit(rs, C, blank, T, L, 5)
    assert E.ctc_fast_path_ok(L, C - 1) and not E.ctc_fast_path_ok(L, C)
    calls, inner = [], E.lattice_forward
    monkeypatch.setattr(E, "lattice_forward", lambda *a, **k: calls.append(1) or inner(*a, **k))
    losses, dx, coef, dead = oracle("beyond_602", x, targets, blank, "mean")
    live = [b for b in range(5) if b not in dead]
    xt = dev(x, grad=True)
    loss = ctc.CTCLoss(xt, targets, blank, "mean")
    assert calls == [1] and loss.item() == INF
    loss.backward()
    check_dx("beyond_602", xt.grad, dx, coef, 1.0, dead)
    xl = dev(x[live], grad=True)  # the loss itself: the live utterances alone
    loss = ctc.CTCLoss(xl, [targets[b] for b in live], blank, "mean")
    check_losses("beyond_602", loss.item(), losses[live].mean())


# ---------------------------------------------------------------------------------------------------------------------
# B. the label alphabet
# ---------------------------------------------------------------------------------------------------------------------
def _long(n, seed, blanks):
    rs = np.random.RandomState(seed)
    t = rs.randint(0, 1000, size=n).tolist()
    for i in blanks:
        t[i] = "b"
    return t


# name -> (C, T, targets); "b" is the blank label, k the k-th class that is not the blank
ALPHABET = {
    # the blank once, twice apart, twice adjacent, first, last; only blanks; beside ordinary targets
    "blank_inside": (6, 12, [[0, "b", 1], [0, "b", 1, "b", 2], [0, "b", "b", 1], ["b", 0, 1], [0, 1, "b"], ["b"], ["b", "b"],
                             ["b"] * 5, [0, 1, 2], [], [3, 3, "b", 3]]),
    # infeasible only by the frame between adjacent blank labels; [1, 1] likewise; the others fit two frames
    "two_frames": (5, 2, [["b", "b"], ["b"], [0, "b"], [0], [], [1, 1], ["b", 2]]),
    # one label L times at T = 2 L - 1 and at 2 L - 2; a label used adjacent and apart
    "one_label_fits": (5, 13, [[2] * 7, [0, 1, 0, 0, 2, 0], ["b"] * 7, [1]]),
    "one_label_does_not": (5, 12, [[2] * 7, [0, 1, 0, 0, 2, 0], ["b"] * 7, [1]]),
    # 63 distinct labels fill every slot of the compact tile (C = 132) / 63 columns of the dense one; 63 copies of one
    "full_63_compact": (132, 126, [list(range(63)), [5] * 63, ["b"] * 63, [0, "b", 1], [], list(range(62, -1, -1))]),
    "full_63_dense": (100, 126, [list(range(63)), [5] * 63, ["b"] * 63, [0, "b", 1], [], list(range(62, -1, -1))]),
    "one_class": (1, 3, [[], ["b"]]),
    "two_classes": (2, 6, [[0], [0, 0], [0, "b", 0], [], ["b"], ["b", "b", 0]]),
    # two, three and four positions per lane with the blank inside (first, adjacent, last), beside 64 blanks
    "long2": (9, 150, [_long(70, 1, (0, 10, 11, 40, 69)), ["b"] * 64, [0, "b", 1], [], [3] * 76]),
    "long3": (11, 300, [_long(130, 2, (0, 63, 64, 65, 129)), ["b"] * 128, [0, "b", 1], [], [3] * 151]),
    "long4": (11, 440, [_long(200, 3, (0, 127, 128, 191, 192, 199)), ["b"] * 200, [0, "b", 1], [], [3] * 221]),
}
BLANKS = [(name, where) for name in ALPHABET for where in ((0,) if ALPHABET[name][0] == 1 else (0, 1, 2))]


@functools.lru_cache(maxsize=None)
def alphabet_data(name, where):
    C, T, sym = ALPHABET[name]
    blank = (0, C // 2, C - 1)[where]
    nb = [c for c in range(C) if c != blank]
    targets = [[blank if s == "b" else nb[s % len(nb)] for s in t] for t in sym]
    x = np.random.RandomState(5000 + 10 * list(ALPHABET).index(name) + where).randn(len(targets), T, C).astype(np.float32)
    x.setflags(write=False)
    return x, targets, blank


@pytest.mark.parametrize("name,where", BLANKS, ids=[f"{n}-blank_{('first', 'middle', 'last')[w]}" for n, w in BLANKS])
def test_label_alphabet(name, where):
    """Every batch through the pipelined step without and with the fusion (for its shape: the meet-in-the-middle launch
    with dense or wide tiles, or a long-target launch), the forward-only chains with the gradient launch behind them,
    and the lattice engine.  Calm scores: nothing may reach the repair launch -- also not the utterances that miss an
    alignment by exactly one frame, which the launch recognises from the targets alone."""
    x, targets, blank = alphabet_data(name, where)
    xt = dev(x)
    case = f"alphabet_{name}_{('first', 'middle', 'last')[where]}"
    for fused in (False, True):
        losses, dx, coef, dead = oracle(case, x, targets, blank, "mean", fused)
        served = step(xt, targets, blank, "mean", fused)
        assert not served.gave_up and served.repaired == 0, (case, fused, served.gave_up, served.repaired)
        check_losses(f"{case}[step{',fused' if fused else ''}]", served.own, losses)
        check_dx(f"{case}[step{',fused' if fused else ''}]", served.dx, dx, coef, 1.0, dead)
    losses, dx, coef, dead = oracle(case, x, targets, blank, "none")
    own, got = split_step(xt, targets, blank, "none")
    check_losses(f"{case}[split]", own, losses)
    check_dx(f"{case}[split]", got, dx, coef, 1.0, dead)
    own, got = lattice_step(xt, targets, blank, "none", 0.75)
    check_losses(f"{case}[lattice]", own, losses)
    check_dx(f"{case}[lattice]", got, dx, coef, 0.75, dead)


def test_label_alphabet_has_the_edges_it_claims():
    """the cases above, read back: which utterances are infeasible, and by how much"""
    dead = lambda name: [needs(t) - ALPHABET[name][1] for t in alphabet_data(name, 1)[1]]  # noqa: E731
    assert dead("two_frames") == [1, -1, 0, -1, -2, 1, 0]
    assert dead("one_label_fits") == [0, -6, 0, -12] and dead("one_label_does_not") == [1, -5, 1, -11]
    assert dead("full_63_compact")[:3] == [-63, -1, -1] and len(set(alphabet_data("full_63_compact", 1)[1][0])) == 63
    assert [d > 0 for d in dead("long2")] == [d > 0 for d in dead("long3")] == [False, False, False, False, True]


# ---------------------------------------------------------------------------------------------------------------------
# C. one alignment: the answer in closed form
# ---------------------------------------------------------------------------------------------------------------------
def single_alignment(rs, C, blank, L, reps, with_blank):
    """a target of L labels with `reps` adjacent repeats (T = L + reps frames), and its only path"""
    nb = [c for c in range(C) if c != blank]
    rep_at = set((1 + rs.permutation(L - 1)[:reps]).tolist()) if reps else set()
    t = []
    for i in range(L):
        if i in rep_at:
            t.append(t[-1])
        else:
            c = nb[rs.randint(len(nb))]
            while t and c == t[-1]:
                c = nb[rs.randint(len(nb))]
            t.append(c)
    if with_blank:  # the middle run of equal labels becomes blank labels: its neighbours differ from it as before
        starts = [i for i in range(L) if i not in rep_at]
        s = starts[len(starts) // 2]
        e = min([i for i in starts if i > s], default=L)
        t[s:e] = [blank] * (e - s)
    path = []
    for i, c in enumerate(t):
        if i and c == t[i - 1]:
            path.append(blank)
        path.append(c)
    assert needs(t) == len(path) == L + reps
    return t, path


@pytest.mark.parametrize("L,reps", [(1, 0), (2, 0), (2, 1), (17, 0), (17, 14), (17, 15), (17, 16), (63, 0), (63, 1), (63, 2),
                                    (64, 0), (64, 15), (64, 16), (130, 0), (130, 13), (130, 14), (255, 0), (255, 16),
                                    (255, 17)])
def test_single_alignment_closed_form(L, reps):
    """T = L + adjacent repeats: one alignment.  The loss is minus the sum of the scores along it, the gradient coef_b on
    it and zero beside it (less coef_b softmax when the log_softmax is fused) -- computed here from the path alone, no
    oracle.  T = 1 .. 272 lands on both sides of the 16-frame blocks (16 | 17, 32 | 33, 64 | 65, 80, 144, 272) and is odd
    and even, so the sweeps meet on either side of a frame; the second utterance has a blank label.  Plain and fused;
    "none" and "mean" under an upstream 0.6; the pipelined step, and the forward-only chains with the gradient launch."""
    C, T, B = 12, L + reps, 2
    rs = np.random.RandomState(7000 + 300 * L + reps)
    blank = (0, C // 2, C - 1)[(L + reps) % 3]
    pairs = [single_alignment(rs, C, blank, L, reps, with_blank=b == 1) for b in range(B)]
    targets, paths = [p[0] for p in pairs], np.array([p[1] for p in pairs])
    x = (0.5 * rs.randn(B, T, C) - 2.0).astype(np.float32)
    xt = dev(x)
    onehot = np.zeros((B, T, C))
    onehot[np.arange(B)[:, None], np.arange(T)[None, :], paths] = 1.0
    for fused in (False, True):
        lp = OC.log_softmax(x.astype(np.float64)) if fused else x.astype(np.float64)
        nll = -(lp * onehot).sum(axis=(1, 2))
        for reduction, gout in (("none", None), ("mean", 0.6)):
            coef = factors(targets, reduction)
            losses = nll * -coef * B
            assert (np.abs(losses) >= 1.0).all(), losses
            want = coef[:, None, None] * (onehot - np.exp(lp) if fused else onehot)
            case = f"closed_form_L{L}_T{T}[{reduction}{',fused' if fused else ''}]"
            served = step(xt, targets, blank, reduction, fused, gout)
            assert not served.gave_up and served.repaired == 0, (case, served.gave_up, served.repaired)
            check_losses(case, served.own, losses)
            check_dx(case, served.dx, want, coef, 1.0 if gout is None else gout)
            if not fused:
                own, dx = split_step(xt, targets, blank, reduction, gout)
                check_losses(case + "[split]", own, losses)
                check_dx(case + "[split]", dx, want, coef, 1.0 if gout is None else gout)


# ---------------------------------------------------------------------------------------------------------------------
# D. layout at the call boundary
# ---------------------------------------------------------------------------------------------------------------------
def feasible_batch(seed, B, T, C, L, blank):
    """four ragged targets of up to L labels, every one feasible, the blank label inside all but the empty one"""
    assert B == 4
    rs = np.random.RandomState(seed)
    ten = kit(rs, C, blank, T, L, 10)
    targets = [ten[0], ten[4], ten[2], ten[9]]
    assert all(needs(t) <= T for t in targets)
    x = rs.randn(B, T, C).astype(np.float32)
    return x, targets


def through_the_criterion(x, targets, blank, fused, lengths=None, gout=None):
    """CTCLoss(x, ..., "mean") or, fused, the CTC module on raw scores -> (loss, x.grad); x is a leaf on its device"""
    _, ctc = _mods()
    x.grad = None
    if fused:
        loss = ctc.CTC(blank, False)(x, [torch.tensor(t, dtype=torch.long) for t in targets], lengths)
    else:
        loss = ctc.CTCLoss(x, targets, blank, "mean", lengths)
    if gout is None:
        loss.backward()
    else:
        (gout * loss).backward()
    return loss.item(), x.grad


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("C,L,T", [(8, 12, 40), (100, 12, 37), (132, 12, 33), (600, 64, 125)])
def test_emissions_that_start_on_an_odd_float(C, L, T, fused):
    """A contiguous view at data_ptr() % 16 == 4 through CTCLoss and the CTC module (the C++ node takes it: contiguous):
    with C % 4 == 0 only such a view sends the emitters' rows through the unaligned stores, and the fused step reads the
    raw scores there again.  Then the step at the engine layer with dx such a view too, and with dx alone."""
    blank = C // 2
    x, targets = feasible_batch(8000 + C, 4, T, C, L, blank)
    losses, dx, coef, dead = oracle(f"odd_float_{C}", x, targets, blank, "mean", fused)
    assert not dead
    case = f"odd_float_{C}[{'fused' if fused else 'plain'}]"
    loss, grad = through_the_criterion(offset_view(x, grad=True), targets, blank, fused)
    check_losses(case, loss, losses.mean())
    check_dx(case, grad, dx, coef)
    for x_odd in (True, False):
        xt = offset_view(x) if x_odd else dev(x)
        out = offset_view(np.full(x.shape, np.nan, dtype=np.float32))
        served = step(xt, targets, blank, "mean", fused, None, dx=out)
        assert not served.gave_up
        check_losses(f"{case}[engine,{'x and dx' if x_odd else 'dx'}]", served.own, losses)
        check_dx(f"{case}[engine,{'x and dx' if x_odd else 'dx'}]", out, dx, coef)


LAYOUTS = ("odd_float", "time_major", "expanded")


def lay_out(x, layout):
    """a leaf [B,T,C] on the device with x's values in `layout` (expanded: x is [1,T,C], the batch has stride 0)"""
    if layout == "odd_float":
        return offset_view(x, grad=True)
    if layout == "time_major":
        t = dev(np.ascontiguousarray(np.transpose(x, (1, 0, 2)))).permute(1, 0, 2).detach()
        assert not t.is_contiguous() and t.stride(0) == x.shape[2]
    else:
        t = dev(x[:1]).expand(x.shape).detach()
        assert t.stride(0) == 0
    return t.requires_grad_(True)


@pytest.mark.parametrize("kind", ["whole", "lengths", "lengths_blank"])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_emission_layouts_through_the_criterion(layout, fused, kind):
    """An odd-float view, a time-major tensor seen through permute(1, 0, 2) and a batch expanded over stride 0 -- the
    last two leave the C++ node for the Python route: loss and gradient meet the bar, x.grad has x's shape and equals,
    bit for bit, the gradient of the same call on x.contiguous().  Without input lengths (blank labels inside); with
    them and targets free of the blank index, so that the layout itself reaches CTCLossFunction with lengths -- the
    launches that read the lengths on an odd-float x, row_lse on it, the zeroed pad rows; and with them and blank labels,
    which CTCLoss sends through a widened copy first (test_blank_labels_under_input_lengths)."""
    _, ctc = _mods()
    B, T, C, blank = 4, 40, 12, 5
    x, targets = feasible_batch(8100, B, T, C, 9, blank)
    lengths = None
    if kind != "whole":
        lengths = [T, 33, 17, 16]
        targets = [t[:n // 3] for t, n in zip(targets, lengths)]
    if kind == "lengths":
        targets = [[blank + 2 if c == blank else c for c in t] for t in targets]
    if layout == "expanded":
        x = np.broadcast_to(x[:1], x.shape).copy()
    assert all(needs(t) <= (T if lengths is None else lengths[b]) for b, t in enumerate(targets))
    assert any(blank in t for t in targets) == (kind != "lengths")
    if kind == "lengths":  # the node itself takes these targets with lengths: nothing stands between it and the layout
        ctc.CTCLossFunction.apply(lay_out(x, layout), targets, blank, "mean", lengths)
    losses, dx, coef, dead = oracle(f"layout_{layout}_{kind}", x, targets, blank, "mean", fused, lengths)
    case = f"layout_{layout}[{'fused' if fused else 'plain'},{kind}]"
    xt = lay_out(x, layout)
    loss, grad = through_the_criterion(xt, targets, blank, fused, lengths, 0.75)
    assert grad.shape == xt.shape
    check_losses(case, loss, losses.mean())
    check_dx(case, grad, dx, coef, 0.75)
    if lengths is not None:
        for b, n in enumerate(lengths):
            assert (grad[b, n:] == 0.0).all(), (case, b)
    xc = xt.detach().contiguous().requires_grad_(True)
    loss_c, grad_c = through_the_criterion(xc, targets, blank, fused, lengths, 0.75)
    assert loss == loss_c and torch.equal(grad, grad_c), (case, loss, loss_c, float((grad - grad_c).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# E. call forms
# ---------------------------------------------------------------------------------------------------------------------
FORMS = ("node", "apply", "no_grad", "cpu", "nonleaf", "retain_node", "retain_apply")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("size", ["short", "long"])
def test_call_forms_with_the_blank_inside(size, form):
    """One short batch (the meet-in-the-middle launch) and one long (two positions per lane), blank labels inside: the C++
    node behind CTCLoss, CTCLossFunction.apply, torch.no_grad() (the forward-only chains), CPU tensors in and out, an
    input that is not a leaf under an upstream 0.75, and a second backward over a retained graph -- the launch runs
    again, the upstream scalar (0.5) applied in the kernel -- behind the node and behind the Python function."""
    E, ctc = _mods()
    B, C, blank = 4, 12, 5
    T, L = (40, 9) if size == "short" else (150, 70)
    x, targets = feasible_batch(9000 + T, B, T, C, L, blank)
    assert max(len(t) for t in targets) == L and all(blank in t for t in targets if t)
    losses, dx, coef, _ = oracle(f"forms_{size}", x, targets, blank, "mean")
    case = f"forms_{size}[{form}]"
    if form == "no_grad":
        with torch.no_grad():
            loss = ctc.CTCLoss(dev(x, grad=True), targets, blank, "mean")
        assert not loss.requires_grad
        check_losses(case, loss.item(), losses.mean())
        check_losses(case + "[no grad asked]", ctc.CTCLoss(dev(x), targets, blank, "mean").item(), losses.mean())
        return
    xt = torch.tensor(x, requires_grad=True) if form == "cpu" else dev(x, grad=True)
    if form == "nonleaf":
        loss = ctc.CTCLoss(xt * 1.0, targets, blank, "mean")
        (0.75 * loss).backward()
        check_losses(case, loss.item(), losses.mean())
        check_dx(case, xt.grad, dx, coef, 0.75)
        return
    call = ctc.CTCLossFunction.apply if form in ("apply", "retain_apply") else ctc.CTCLoss
    loss = call(xt, targets, blank, "mean")
    assert (type(loss) is ctc._EagerLoss) == (form in ("node", "retain_node")), (form, type(loss))
    assert loss.device.type == ("cpu" if form == "cpu" else "cuda")
    check_losses(case, loss.item(), losses.mean())
    if form.startswith("retain"):
        loss.backward(retain_graph=True)
        check_dx(case + "[first]", xt.grad, dx, coef)
        xt.grad = None
        loss.backward(torch.tensor(0.5, device=loss.device))
        check_dx(case + "[second]", xt.grad, dx, coef, 0.5)
        return
    loss.backward()
    assert xt.grad.device == xt.device
    check_dx(case, xt.grad, dx, coef)


# ---------------------------------------------------------------------------------------------------------------------
# blank labels under input lengths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("size", ["short", "long"])
def test_blank_labels_under_input_lengths(size, fused):
    """A certain-blank pad frame is the identity of the CTC graph only while no label state reads the blank's column
    (DESIGN.md section 16).  A padded batch whose targets hold the blank index goes through a column of its own
    (criterions/ctc.py::_lengths_with_blank_labels): against the oracle on every utterance's slice, for the launches that
    read the lengths themselves (short) and those that run on a padded copy (long), from leaves and from a producer's
    output; pad rows exactly 0.  CTCLossFunction.apply, which cannot add the column, refuses."""
    _, ctc = _mods()
    B, C, blank = 4, 12, 5
    T, L, lengths = (40, 9, [40, 33, 17, 30]) if size == "short" else (150, 70, [150, 97, 1, 96])
    x, targets = feasible_batch(9500 + T, B, T, C, L, blank)
    assert all(needs(t) <= n for t, n in zip(targets, lengths)) and sum(blank in t for t in targets) == 3
    losses, dx, coef, _ = oracle(f"lengths_blank_{size}", x, targets, blank, "mean", fused, lengths)
    case = f"lengths_blank_{size}[{'fused' if fused else 'plain'}]"
    xt = dev(x, grad=True)
    loss, grad = through_the_criterion(xt, targets, blank, fused, lengths)
    check_losses(case, loss, losses.mean())
    check_dx(case, grad, dx, coef)
    for b, n in enumerate(lengths):
        assert (grad[b, n:] == 0.0).all(), (case, b)
    leaf = dev(x, grad=True)
    call = ctc.CTC(blank, False) if fused else (lambda e, t, n: ctc.CTCLoss(e, [v.tolist() for v in t], blank, "mean", n))
    loss = call(leaf * 1.0, [torch.tensor(t, dtype=torch.long) for t in targets], torch.tensor(lengths))
    (0.75 * loss).backward()
    check_losses(case + "[nonleaf]", loss.item(), losses.mean())
    check_dx(case + "[nonleaf]", leaf.grad, dx, coef, 0.75)
    with pytest.raises(ValueError, match="call CTCLoss"):
        ctc.CTCLossFunction.apply(dev(x, grad=True), targets, blank, "mean", lengths)
    if not fused:
        # targets staged by the caller are served as lists are
        E = _mods()[0]
        staged = E.targets_on_device(targets, torch.device("cuda", torch.cuda.current_device()))
        check_losses(case + "[staged]", ctc.CTCLoss(dev(x, grad=True), staged, blank, "mean", lengths).item(), losses.mean())
        # a label outside the caller's C classes is refused as ever, not read as the widened row's last class
        for bad in (C, C + 1, -1):
            with pytest.raises(ValueError, match=rf"target label {bad} is outside \[0, {C}\)"):
                ctc.CTCLoss(dev(x, grad=True), targets[:3] + [[blank, bad]], blank, "mean", lengths)
