"""STC on the device at its graph, length and penalty edges (-m gpu): criterions/stc.py on csrc/lattice_kernels.hip.

An STC acceptor (stc.py:23-64) is not the shape tests/test_gpu_lattice_edges.py draws: 3L+2 states with the L+1 <star>
states numbered BEHIND the 2L+1 CTC states (every token state has an in-arc from about 2L states away), the constant
weight log(prob) on every <star> arc at every frame, three accept states, and the skip arc s-2 -> s kept between equal
labels.

  A  acceptors of 2 .. 1025 states on both sides of every sweep-workgroup size (64, 128, 256, 512, 1024), distinct and
     repeated labels, T = L + 37 and T = L, a ragged batch, targets as tensors, the sweeps' number format
  B  no accepting path: T < L, T = L, a token no frame can emit -- loss +inf, rows exactly zero, neighbours unharmed
  C  the penalty from 1 down to 1e-38, and a batch whose only accepting path collects 280 penalties (log Z = -2581)
  D  the operator: reductions, upstream scalars, retained graphs, forward only, host inputs, refusals before any launch,
     the 1024-distinct-label limit from both sides
  E  the module's penalty schedule beyond step 1, one end-to-end gradient, one pack per recurring batch

Reference of every number: oracle/criteria.py::stc_graph swept by oracle/recurrences.py::lattice_forward_backward in
float64 on the same float32 inputs cast up.  Before the device is asked, every case asserts on the oracle's own output
that log Z is finite where the case is meant to be feasible and that the posteriors of every frame sum to one.  Bar: that
of tests/test_gpu_configs.py through check() -- per-utterance losses at scale 0, gradients at coef_b = scale_b / B; the
one exception (an utterance the range certificate repaired in the log domain) is named in C.  Worst ratios land in the
parity JSON that tests/test_gpu_configs.py writes, under stc_edges_*.  Nothing here reads the reference project."""

import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import criteria as OC  # noqa: E402
from oracle import recurrences as OR  # noqa: E402
# _gpu_and_stats: the module-level fixture of test_gpu_configs, registered for this module too by the import -- skips
# without a GPU, and writes STATS (shared, so with every module's records so far) when this module's tests are over
from test_gpu_configs import ATOL_SCALE, STATS, _gpu_and_stats, check  # noqa: E402,F401

NEG = float("-inf")


# =================================================================================================
# the oracle, and the device's numbers beside it
# =================================================================================================
def _oracle(x, targets, Cp, prob, feasible=None):
    """log Z [B] and posteriors [B, T, 2 Cp] of every utterance (float64), with the worth-comparing conditions asserted:
    finite log Z where `feasible` says so (default: everywhere), a frame's posteriors summing to one."""
    B, T, _ = x.shape
    logz, post = np.zeros(B), np.zeros(x.shape)
    for b in range(B):
        g = OC.stc_graph(targets[b], Cp, prob)
        assert g.num_nodes() == 3 * len(targets[b]) + 2
        logz[b], post[b], _ = OR.lattice_forward_backward(x[b].astype(np.float64), g.src, g.dst, g.ilab, g.w,
                                                          g.start_nodes(), g.accept_nodes(), g.num_nodes())
        if feasible is None or feasible[b]:
            assert np.isfinite(logz[b]), (b, logz[b])
            assert np.abs(post[b].sum(axis=1) - 1.0).max() <= 1e-9, (b, np.abs(post[b].sum(axis=1) - 1.0).max())
        else:
            assert logz[b] == NEG and not post[b].any(), (b, logz[b])
    return logz, post


def _device(x, targets, prob, reduction="none", upstream=None):
    """STCLoss forward + backward: (scalar loss, per-utterance log Z the forward pass left, dx), as numpy."""
    from gtn_applications_amd.criterions import stc

    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    loss = stc.STCLoss(xd, targets, prob, reduction)
    logz = loss.grad_fn.aux[1].logz  # (the LatticeState of the forward pass: ctx.aux = (x, st, cneg))
    (loss if upstream is None else upstream * loss).backward()
    return float(loss.item()), logz.cpu().numpy().astype(np.float64), xd.grad.cpu().numpy()


def _formats(x, targets, prob):
    """How the lattice engine swept each utterance (E.lattice_formats), through the calls STCLossFunction.forward makes."""
    from gtn_applications_amd import engine as E

    xd = torch.from_numpy(x).cuda()
    tg = E.targets_on_device(targets, xd.device)
    Cstar = x.shape[2]
    pack = E.PackedLattice.stc(tg.flat, tg.offsets, Cstar // 2, math.log(prob), Cstar, xd.device)
    assert pack.desc.max_states == 3 * max(len(t) for t in targets) + 2
    st = E.lattice_forward(xd, pack, need_beta=True)
    return E.lattice_formats(st).tolist(), st.logz.cpu().numpy().astype(np.float64), pack.desc


def _compare(name, x, targets, Cp, prob, got, want, feasible=None, norm=1.0, upstream=1.0):
    """Every utterance of one call against the oracle: -log Z at scale 0, dx at coef_b = upstream / (norm * B); an
    utterance without an accepting path has loss +inf and rows that are exactly zero ("No accepting path")."""
    loss, logz, dx = got
    want_logz, post = want
    B = x.shape[0]
    coef = upstream / (norm * B)
    for b in range(B):
        if feasible is not None and not feasible[b]:
            assert logz[b] == NEG, (name, b, logz[b])
            assert not dx[b].any(), (name, b, float(np.abs(dx[b]).max()))
            continue
        check(name + "_nll", np.array([-logz[b]]), np.array([-want_logz[b]]), 0.0)
        check(name + "_dx", dx[b], -post[b] * coef, coef)
    if feasible is None or all(feasible):
        check(name + "_loss", np.array([loss]), np.array([(-want_logz / norm).mean()]), 0.0)
    else:
        assert loss == float("inf"), (name, loss)


def _emissions(rs, B, T, Cp):
    return torch.log_softmax(torch.from_numpy(rs.randn(B, T, 2 * Cp).astype(np.float32)), 2).numpy()


def _distinct_target(rs, L, Cp):
    """As many distinct tokens as the columns allow (labels 1 .. Cp-1; 0 is the blank), the rest drawn at random."""
    first = (1 + rs.permutation(Cp - 1))[:L].tolist()
    return first + rs.randint(1, Cp, size=max(0, L - len(first))).tolist()


def _three_token_target(rs, L):
    """Drawn from 3 tokens: runs of equal labels, which the unconditional skip arc s-2 -> s jumps."""
    return rs.randint(1, 4, size=L).tolist()


# =================================================================================================
# A. acceptor size and shape
# =================================================================================================
SIZES = [(0, 48), (1, 48), (20, 12), (20, 48), (21, 48), (42, 48), (43, 48), (85, 48), (170, 48), (171, 48), (341, 48)]


@functools.lru_cache(maxsize=None)
def _size_case(L, Cp, exact):
    """Two utterances of L labels -- one with as many distinct labels as Cp allows, one drawn from 3 tokens -- at
    T = L + 37 (a partial last 16-frame chunk, but for L = 43) or T = L (only the all-token paths and their blank- / <star>-free
    variants are left), with the oracle's result.  Computed once."""
    rs = np.random.RandomState(1000 * L + Cp + int(exact))
    T = L if exact else L + 37
    targets = [_distinct_target(rs, L, Cp), _three_token_target(rs, L)]
    if L >= 2:
        assert len(set(targets[0])) == min(L, Cp - 1)
    if L >= 8:
        assert any(a == b for a, b in zip(targets[1][:-1], targets[1][1:]))
    x = _emissions(rs, 2, T, Cp)
    return x, targets, _oracle(x, targets, Cp, 0.3)


@pytest.mark.parametrize("L,Cp", SIZES)
def test_acceptors_on_both_sides_of_every_workgroup_size(L, Cp):
    """Q = 3L+2 = 2, 5, 62, 65, 128, 131, 257, 512, 515, 1025 states: up to 64 the banded gradient's gate is open (its
    per-state test then finds that no token state's in-arcs fit the band), 128 / 256 / 512 / 1024 are the sweep workgroup
    sizes, and beyond 1024 the threads loop over the states.  L = 20 runs with 12 and with 48 selected columns (24 and 42
    distinct labels per utterance: an acceptor of at most 64 states cannot name more than 2L+2 = 42, so both stay below
    the banded gate's 64 labels).  Every utterance swept in the probability domain (format 1), loss and gradient of every
    utterance against the oracle."""
    x, targets, want = _size_case(L, Cp, False)
    name = "stc_edges_size"  # (one record per family and quantity; the case is in the test id)
    fmt, logz, desc = _formats(x, targets, 0.3)
    assert desc.max_labels == (2 * len(set(targets[0])) + 2 + 3) // 4 * 4  # (label rows are padded to four)
    assert fmt == [1, 1], (name, fmt)  # ordinary inputs: a silent fall to the log domain would be a finding
    check(name + "_engine_nll", -logz, -want[0], 0.0)
    _compare(name, x, targets, Cp, 0.3, _device(x, targets, 0.3), want)


@pytest.mark.parametrize("L", [1, 21, 171])
def test_exactly_as_many_frames_as_labels(L):
    """T == L: every frame emits a token, through the skip arcs alone (also between equal labels)."""
    x, targets, want = _size_case(L, 48, True)
    name = "stc_edges_T_eq_L"
    fmt, _, _ = _formats(x, targets, 0.3)
    assert fmt == [1, 1], (name, fmt)
    assert not want[1][:, :, 0].any() and not want[1][:, :, 48:].any()  # no path has a frame to spare for blank or <star>
    _compare(name, x, targets, 48, 0.3, _device(x, targets, 0.3), want)


def _device_with_tensor_targets(x, targets, prob):
    """_device() with the targets as 1-D int64 tensors: the stager's second route (engine.py CtcTargets, flatten_any)."""
    from gtn_applications_amd.criterions import stc

    as_tensors = [torch.tensor(t, dtype=torch.int64) for t in targets]
    assert all(t.dim() == 1 and t.numel() == len(y) for t, y in zip(as_tensors, targets))
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    loss = stc.STCLoss(xt, as_tensors, prob, "none")
    logz = loss.grad_fn.aux[1].logz
    loss.backward()
    return float(loss.item()), logz.cpu().numpy().astype(np.float64), xt.grad.cpu().numpy()


# grad_kernel (csrc/lattice_kernels.hip) sums a label slot's arcs in chunks of kChunk = 16 and joins the chunks of one
# slot with float atomics in LDS, whose order is not fixed: a gradient is reproducible bit for bit from run to run only
# while no slot has more than 16 arcs.  The blank slot of an STC acceptor has 3L+2 (L+1 self-loops, L token -> blank,
# L+1 <star> -> blank), so that holds up to L = 4; a token met n times has at most 3n.  (Measured on longer targets: two
# identical calls differ in some 50 elements by one float32 ulp of the sum, 1.5e-8.)  The forward pass has no atomics.
REPRODUCIBLE_MAX_L = 4


def test_ragged_batch_and_targets_as_tensors():
    """L = (0, 1, 21, 171) at one T: short acceptors beside the one that sizes the workgroup (515 states), every utterance
    against the oracle.  The batch goes through the stager as 1-D int tensors first (an empty tensor among them), then
    as lists: both results meet the bar, the loss and log Z are the same bit for bit, and so are the gradient rows of the
    utterances whose gradient is reproducible at all (REPRODUCIBLE_MAX_L).  The batches of L = 0 (only empty tensors) and
    L = 1 of A run both ways too: loss and the whole gradient bit for bit."""
    Cp, lens = 48, (0, 1, 21, 171)
    rs = np.random.RandomState(171)
    T = max(lens) + 37
    targets = [_three_token_target(rs, lens[0]), _distinct_target(rs, lens[1], Cp), _three_token_target(rs, lens[2]),
               _distinct_target(rs, lens[3], Cp)]
    x = _emissions(rs, len(lens), T, Cp)
    want = _oracle(x, targets, Cp, 0.3)
    got_t = _device_with_tensor_targets(x, targets, 0.3)
    got = _device(x, targets, 0.3)
    assert got_t[0] == got[0] and np.array_equal(got_t[1], got[1])
    for b, n in enumerate(lens):
        if n <= REPRODUCIBLE_MAX_L:
            assert np.array_equal(got_t[2][b], got[2][b]), b
    fmt, _, _ = _formats(x, targets, 0.3)
    assert fmt == [1, 1, 1, 1], fmt
    _compare("stc_edges_ragged", x, targets, Cp, 0.3, got, want)
    _compare("stc_edges_ragged_tensor_targets", x, targets, Cp, 0.3, got_t, want)
    for L in (0, 1):
        x, targets, want = _size_case(L, 48, False)
        got_t = _device_with_tensor_targets(x, targets, 0.3)
        got = _device(x, targets, 0.3)
        assert got_t[0] == got[0] and np.array_equal(got_t[1], got[1]) and np.array_equal(got_t[2], got[2]), L
        _compare("stc_edges_tensor_targets", x, targets, 48, 0.3, got_t, want)


# =================================================================================================
# B. feasibility
# =================================================================================================
FEAS_CP = 8


@pytest.mark.parametrize("T,lens", [(5, (6, 6, 6)), (6, (6, 6, 6)), (40, (6, 6, 6)), (5, (6, 2, 0))])
def test_fewer_frames_than_labels(T, lens):
    """Targets of 6 labels at T = 5 (no path), T = 6 (the all-token path only) and T = 40; at T = 5 also beside targets
    of 2 and 0 labels, whose rows must not notice the neighbour without a path."""
    rs = np.random.RandomState(10 * T + len(set(lens)))
    targets = [_three_token_target(rs, lens[0]), _distinct_target(rs, lens[1], FEAS_CP), _distinct_target(rs, lens[2], FEAS_CP)]
    x = _emissions(rs, 3, T, FEAS_CP)
    feasible = [n <= T for n in lens]
    want = _oracle(x, targets, FEAS_CP, 0.3, feasible)
    _compare("stc_edges_feasibility", x, targets, FEAS_CP, 0.3, _device(x, targets, 0.3), want, feasible)


def test_a_token_no_frame_can_emit():
    """-inf in the column of one target token at every frame: no accepting path although T >= L (every path passes
    through every token state: the <star> arcs insert, they do not skip).  The neighbours name other tokens."""
    rs = np.random.RandomState(77)
    T = 30
    targets = [[1, 2, 3, 2, 1, 4], [1, 2, 5, 6], []]
    x = _emissions(rs, 3, T, FEAS_CP)
    x[0, :, 3] = NEG
    x[1, :, 3] = NEG  # (utterance 1 does not name token 3: only its <star> arcs' alternatives lose nothing)
    feasible = [False, True, True]
    want = _oracle(x, targets, FEAS_CP, 0.3, feasible)
    _compare("stc_edges_feasibility", x, targets, FEAS_CP, 0.3, _device(x, targets, 0.3), want, feasible)


# =================================================================================================
# C. penalty range
# =================================================================================================
PEN_L, PEN_T, PEN_CP = 20, 300, 6
PROBS = [1.0, 0.5, 1e-4, 1e-30, 1e-38]


@functools.lru_cache(maxsize=None)
def _penalty_inputs():
    rs = np.random.RandomState(300)
    return _emissions(rs, 1, PEN_T, PEN_CP), [rs.randint(1, PEN_CP, size=PEN_L).tolist()]


@functools.lru_cache(maxsize=None)
def _penalty_oracle(prob):
    x, targets = _penalty_inputs()
    return _oracle(x, targets, PEN_CP, prob)


@pytest.mark.parametrize("prob", PROBS)
def test_penalties_from_one_down_to_1e_38(prob):
    """One target of 20 labels over 300 frames, ordinary emissions.  With prob = 1 the <star> arcs are free and take most
    of the frames; at 1e-30 and 1e-38 (log(prob) = -69, -87.5) they carry nothing: the <star> columns' gradient is then
    below the absolute part of the bar (and no NaN), the rest is CTC without self-loops on the tokens."""
    x, targets = _penalty_inputs()
    want = _penalty_oracle(prob)
    star_mass = [float(_penalty_oracle(p)[1][0, :, PEN_CP:].sum()) for p in PROBS]
    logzs = [float(_penalty_oracle(p)[0][0]) for p in PROBS]
    assert all(a >= b for a, b in zip(logzs[:-1], logzs[1:])) and logzs[0] > logzs[2] + 100, logzs  # less prob, less mass
    assert star_mass[0] > 100.0 and star_mass[-2] < 1e-20 and star_mass[-1] < 1e-25, star_mass
    name = f"stc_edges_penalty_p{prob:g}"
    fmt, _, _ = _formats(x, targets, prob)
    STATS[name + "_formats"] = fmt
    got = _device(x, targets, prob)
    _compare(name, x, targets, PEN_CP, prob, got, want)
    if prob <= 1e-30:
        assert np.abs(got[2][0, :, PEN_CP:]).max() <= ATOL_SCALE * 1.0  # coef_b = 1 / B = 1


def _star_forced_emissions(rs, target):
    """Blank -inf everywhere; position l's token can be emitted at frame f_l alone (0 there, -inf elsewhere; the f_l spread
    evenly over T); the <star> columns random.  The ONE accepting path spends T - L = 280 frames on <star> arcs."""
    x = np.full((PEN_T, 2 * PEN_CP), NEG, np.float32)
    x[:, PEN_CP:] = (0.3 * rs.randn(PEN_T, PEN_CP)).astype(np.float32)
    frames = [(2 * l + 1) * PEN_T // (2 * PEN_L) for l in range(PEN_L)]
    assert len(set(frames)) == PEN_L and frames[0] > 0 and frames[-1] < PEN_T - 1
    for l, f in enumerate(frames):
        x[f, target[l]] = 0.0
    return x


# The bar test_lattice_certificate_sends_what_a_double_cannot_hold_to_the_log_domain (tests/test_gpu_parity.py) grants an
# utterance the certificate repaired in the log domain: 1e-5 relative on log Z, 2e-3 (relative + absolute) on a posterior
REPAIRED_RTOL_LOGZ, REPAIRED_TOL_POST = 1e-5, 2e-3


@pytest.mark.parametrize("prob", [0.5, 1e-4])
def test_a_path_that_collects_280_penalties(prob):
    """Star-forced emissions beside an ordinary utterance: log Z = 280 log(prob) + the <star> emissions along the one
    path -- -196.4 at prob = 0.5, -2581.2 at prob = 1e-4, where e^logZ is not a double.  The sweeps' number
    format of each utterance is part of the record's name.  Format 1 (probability domain, certified): the common bar.
    Format 0 (repaired in the log domain): the bar the certificate test grants a repaired utterance, nothing looser.  A
    finite but wrong Z in format 1 is what this case exists to catch."""
    rs = np.random.RandomState(280)
    x1, targets = _penalty_inputs()
    targets = [targets[0], targets[0]]
    x = np.stack([_star_forced_emissions(rs, targets[0]), x1[0]])
    want_logz, post = _oracle(x, targets, PEN_CP, prob)
    path_frames = int(round(post[0][:, PEN_CP:].sum()))
    assert path_frames == PEN_T - PEN_L  # every accepting path spends 280 frames on <star> arcs
    assert want_logz[0] < (-745.0 if prob == 1e-4 else -150.0)  # (exp(-745) is the smallest double)
    fmt, _, _ = _formats(x, targets, prob)
    loss, logz, dx = _device(x, targets, prob)
    B = 2
    for b in range(B):
        name = f"stc_edges_star_forced_p{prob:g}_utt{b}_format{fmt[b]}"
        assert fmt[b] in (0, 1), (name, fmt)
        print(name, "log Z", logz[b], "oracle", want_logz[b], "max |dx * B + post|", np.abs(dx[b] * B + post[b]).max())
        if fmt[b] == 1:
            check(name + "_nll", np.array([-logz[b]]), np.array([-want_logz[b]]), 0.0)
            check(name + "_dx", dx[b], -post[b] / B, 1.0 / B)
        else:
            assert np.isfinite(logz[b]) and np.isfinite(dx[b]).all(), name
            err_z = abs(logz[b] - want_logz[b]) / abs(want_logz[b])
            err_p = np.abs(-dx[b] * B - post[b])
            tol_p = REPAIRED_TOL_POST * np.abs(post[b]) + REPAIRED_TOL_POST
            STATS[name] = dict(logz_rel_err=float(err_z), logz_rel_tol=REPAIRED_RTOL_LOGZ,
                               post_max_err_over_tol=float((err_p / tol_p).max()), post_max_abs_err=float(err_p.max()))
            assert err_z <= REPAIRED_RTOL_LOGZ, (name, logz[b], want_logz[b])
            assert (err_p <= tol_p).all(), (name, float(err_p.max()))
    assert fmt[1] == 1, fmt  # the ordinary utterance stays in the probability domain


# =================================================================================================
# D. the operator's contract
# =================================================================================================
OP_B, OP_T, OP_CP = 3, 24, 6
OP_TARGETS = [[1, 2, 2, 5], [], [3]]


@functools.lru_cache(maxsize=None)
def _op_case():
    x = _emissions(np.random.RandomState(24), OP_B, OP_T, OP_CP)
    return x, _oracle(x, OP_TARGETS, OP_CP, 0.4)


def test_reductions_and_upstream_scalars():
    """"none" and "mean" give the same per-utterance numbers, except that "mean" divides by T -- not by the target length
    (stc.py:90-91); an upstream factor of 0.75 scales the gradient; a retained graph's second backward doubles it exactly
    (targets of at most REPRODUCIBLE_MAX_L labels: the two passes then give the same bits)."""
    from gtn_applications_amd.criterions import stc

    x, want = _op_case()
    _compare("stc_edges_op_none", x, OP_TARGETS, OP_CP, 0.4, _device(x, OP_TARGETS, 0.4, "none"), want)
    _compare("stc_edges_op_mean", x, OP_TARGETS, OP_CP, 0.4, _device(x, OP_TARGETS, 0.4, "mean"), want, norm=OP_T)
    _compare("stc_edges_op_none_x0.75", x, OP_TARGETS, OP_CP, 0.4, _device(x, OP_TARGETS, 0.4, "none", 0.75), want,
             upstream=0.75)
    _compare("stc_edges_op_mean_x0.75", x, OP_TARGETS, OP_CP, 0.4, _device(x, OP_TARGETS, 0.4, "mean", 0.75), want,
             norm=OP_T, upstream=0.75)
    assert max(len(t) for t in OP_TARGETS) <= REPRODUCIBLE_MAX_L
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    loss = stc.STCLoss(xd, OP_TARGETS, 0.4, "mean")
    loss.backward(retain_graph=True)
    once = xd.grad.clone()
    loss.backward(retain_graph=True)
    assert float(once.abs().max()) > 0 and torch.equal(xd.grad, 2 * once)


def test_forward_only_and_host_inputs():
    """Inputs that do not require a gradient (need_beta=False: the backward sweep is not launched) give the loss of the
    same call with a gradient, bit for bit; CPU float32 inputs get loss and gradient back on the CPU, at the same bar."""
    from gtn_applications_amd.criterions import stc

    x, want = _op_case()
    for reduction in ("none", "mean"):
        with_grad = stc.STCLoss(torch.from_numpy(x).cuda().requires_grad_(True), OP_TARGETS, 0.4, reduction)
        without = stc.STCLoss(torch.from_numpy(x).cuda(), OP_TARGETS, 0.4, reduction)
        assert not without.requires_grad and with_grad.requires_grad
        assert torch.equal(with_grad.detach(), without)
    xh = torch.from_numpy(x.copy()).requires_grad_(True)
    loss = stc.STCLoss(xh, OP_TARGETS, 0.4, "mean")
    logz = loss.grad_fn.aux[1].logz.cpu().numpy().astype(np.float64)
    loss.backward()
    assert loss.device.type == "cpu" and xh.grad.device.type == "cpu" and xh.grad.dtype == torch.float32
    _compare("stc_edges_op_host_inputs", x, OP_TARGETS, OP_CP, 0.4, (float(loss.item()), logz, xh.grad.numpy()), want,
             norm=OP_T)


def test_bad_arguments_are_refused_before_any_launch():
    from gtn_applications_amd.criterions import stc

    x, _ = _op_case()
    xd = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match="reduction"):
        stc.STCLoss(xd, OP_TARGETS, 0.4, "sum")
    with pytest.raises(ValueError, match="2 targets for a batch of 3"):
        stc.STCLoss(xd, OP_TARGETS[:2], 0.4, "none")
    with pytest.raises(ValueError, match="T == 0"):
        stc.STCLoss(xd[:, :0], OP_TARGETS, 0.4, "none")
    with pytest.raises(TypeError, match="float32"):
        stc.STCLoss(xd.double(), OP_TARGETS, 0.4, "none")


def test_the_1024_distinct_label_limit_from_both_sides():
    """512 distinct tokens name 1026 distinct columns (blank, 512 tokens, <star>, 512 <star>\\token; 1028 label slots,
    padded to four): refused by
    wfl_lattice_forward's host-side check, and an ordinary call afterwards is still right.  511 distinct tokens name 1024:
    accepted (1535 states: the sweep threads loop), every number at the bar."""
    from gtn_applications_amd import _native as N
    from gtn_applications_amd.criterions import stc

    T, Cp = 520, 513
    rs = np.random.RandomState(513)
    x = _emissions(rs, 1, T, Cp)
    order = (1 + rs.permutation(Cp - 1)).tolist()
    assert len(set(order)) == 512
    with pytest.raises(N.WflUnsupported, match=r"\d+ distinct labels per utterance \(limit 1024\)"):
        stc.STCLoss(torch.from_numpy(x).cuda().requires_grad_(True), [order], 0.3, "none")
    xo, want = _op_case()
    _compare("stc_edges_after_refusal", xo, OP_TARGETS, OP_CP, 0.4, _device(xo, OP_TARGETS, 0.4), want)
    targets = [order[:511]]
    want = _oracle(x, targets, Cp, 0.3)
    _compare("stc_edges_1024_labels", x, targets, Cp, 0.3, _device(x, targets, 0.3), want)


# =================================================================================================
# E. the module's schedule and its cache
# =================================================================================================
MOD_T, MOD_B, MOD_C = 30, 3, 9
MOD_TARGETS = [[1, 2, 2, 5], [4], [7, 1, 8, 8, 3]]
MOD_P0, MOD_PLAST, MOD_THALF, MOD_STEPS = 0.9, 0.1, 5, 12


@functools.lru_cache(maxsize=None)
def _module_inputs():
    """(T, B, C) log-probabilities, moderate and unpeaked: every exp(token - <star>) stays below 1 - 1e-3, away from the
    1e-7 floor inside logsubexp, where float32 and float64 disagree by construction."""
    rs = np.random.RandomState(30)
    x = torch.log_softmax(torch.from_numpy((0.5 * rs.randn(MOD_T, MOD_B, MOD_C)).astype(np.float32)), 2)
    lse = torch.logsumexp(x[:, :, 1:].double(), 2, keepdim=True)
    assert float(torch.exp(x[:, :, 1:].double() - lse).max()) < 1.0 - 1e-3
    return x


@functools.lru_cache(maxsize=None)
def _module_oracle(step):
    """The oracle's loss and dL/d(augmented emissions) at training step `step` ("mean")."""
    x = _module_inputs()
    aug, tg, select = OC.stc_augment(x.permute(1, 0, 2).numpy().astype(np.float64), MOD_TARGETS)
    loss, daug = OC.stc_function(aug, tg, OC.stc_prob(MOD_P0, MOD_PLAST, MOD_THALF, step), "mean")
    assert np.isfinite(loss)
    assert np.abs(np.abs(daug).sum(axis=2) * (MOD_T * MOD_B) - 1.0).max() <= 1e-9  # a frame's posteriors sum to one
    return loss, daug, select


def _staged_module_targets(dev):
    """The staged-targets object of the batch as STC.forward hands it to STCLoss (labels renumbered by the select list)."""
    from gtn_applications_amd import engine as E

    labels = set(t for target in MOD_TARGETS for t in target)
    target_map = {t: i for i, t in enumerate([0] + list(labels))}
    return E.targets_on_device([[target_map[t] for t in target] for target in MOD_TARGETS], dev)


def _stc_packs(tg):
    return [k for k in tg.cache if isinstance(k, tuple) and k and k[0] == "stc"]


def test_module_penalty_schedule_and_one_pack_per_batch():
    """STC(0, 0.9, 0.1, thalf=5, "mean") on a recurring batch: the loss of training step k is the oracle's at
    stc_prob(0.9, 0.1, 5, k), k = 1 .. 12 (a pack reused from an earlier step would keep that step's penalty); in eval()
    nstep stays and the loss repeats; and the batch holds ONE STC pack afterwards, not one per step."""
    from gtn_applications_amd.criterions import stc

    x = _module_inputs().cuda()
    m = stc.STC(0, MOD_P0, MOD_PLAST, MOD_THALF, "mean")
    m.train()
    for k in range(1, MOD_STEPS + 1):
        loss = m(x, MOD_TARGETS)
        assert m.nstep == k
        check("stc_edges_module_schedule_loss", np.array([loss.item()]), np.array([_module_oracle(k)[0]]), 0.0)
    assert _module_oracle(1)[0] < 0.9 * _module_oracle(MOD_STEPS)[0]  # (the schedule is visible in the oracle's losses)
    m.eval()
    a, b = m(x, MOD_TARGETS).item(), m(x, MOD_TARGETS).item()
    assert m.nstep == MOD_STEPS and a == b
    check("stc_edges_module_schedule_loss", np.array([a]), np.array([_module_oracle(MOD_STEPS)[0]]), 0.0)
    packs = _stc_packs(_staged_module_targets(x.device))
    assert len(packs) == 1, packs


def test_a_pack_replaced_in_the_cache_serves_the_backward_that_still_holds_it():
    """Two forward passes of one batch at different penalties, then the FIRST one's backward: its pack left the cache when
    the second was built, and must still be the one its gradient is formed with."""
    from gtn_applications_amd.criterions import stc

    x, _ = _op_case()
    want = _oracle(x, OP_TARGETS, OP_CP, 0.7)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    first = stc.STCLoss(xd, OP_TARGETS, 0.7, "none")
    logz = first.grad_fn.aux[1].logz.cpu().numpy().astype(np.float64)
    second = stc.STCLoss(torch.from_numpy(x).cuda().requires_grad_(True), OP_TARGETS, 0.05, "none")
    assert first.grad_fn.aux[1].pack is not second.grad_fn.aux[1].pack
    first.backward()
    _compare("stc_edges_replaced_pack", x, OP_TARGETS, OP_CP, 0.7, (float(first.item()), logz, xd.grad.cpu().numpy()), want)


def test_module_gradient_end_to_end():
    """x.grad of the module (augmentation kernels + lattice engine) against the oracle's dL/d(augmented emissions) pulled
    back through a float64 torch autograd of the augmentation's torch spelling (criterions/stc.py, the host-input branch
    of STC.forward), at training step 7 of the schedule."""
    from gtn_applications_amd.criterions import stc

    step = 7
    x = _module_inputs()
    want_loss, daug, select = _module_oracle(step)
    x64 = x.double().requires_grad_(True)
    lp = x64.permute(1, 0, 2)
    lse = torch.logsumexp(lp[:, :, 1:], 2, keepdim=True)
    sel = lp.index_select(2, torch.tensor(select))
    aug = torch.cat([sel, lse, lse + torch.log1p(1e-7 - torch.exp(sel[:, :, 1:] - lse))], dim=2)
    (aug * torch.from_numpy(daug)).sum().backward()
    m = stc.STC(0, MOD_P0, MOD_PLAST, MOD_THALF, "mean")
    m.train()
    m.nstep = step - 1
    xd = x.cuda().requires_grad_(True)
    loss = m(xd, MOD_TARGETS)
    loss.backward()
    assert m.nstep == step
    check("stc_edges_module_loss", np.array([loss.item()]), np.array([want_loss]), 0.0)
    check("stc_edges_module_dx", xd.grad.cpu().numpy(), x64.grad.numpy(), 1.0 / (MOD_T * MOD_B))
