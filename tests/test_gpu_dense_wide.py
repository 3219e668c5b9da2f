"""The dense transition engine beyond the on-chip class limit (csrc/dense_wide.h) at its range, length and batch edges,
against the float64 recurrences of oracle/recurrences.py and the graph oracle of oracle/criteria.py.

Up to wfl_dense_on_chip_classes() (192) the probability-domain sweeps flag what fp32 cannot hold and the log-domain
kernels recompute it; from 193 classes the batched product takes a range verdict on W and a flagged batch is
recomputed in the log domain behind it.  Each range case runs at 192 (the on-chip control), in the register-resident
sweeps (193 .. 320) and in the per-frame launches (321, 1000).  Tolerances as tests/test_gpu_parity.py: 1e-4 relative,
1e-5 absolute on the emission gradient, 5e-5 on the transition gradient."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import criteria as OC  # noqa: E402
from oracle import recurrences as OR  # noqa: E402

RTOL, ATOL = 1e-4, 1e-5
ON_CHIP = 192  # wfl_dense_on_chip_classes(), asserted below
RANGE_C = [192, 193, 200, 257, 320, 321, 1000]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gtn_applications_amd import _native as N

    assert N.lib.wfl_dense_on_chip_classes() == ON_CHIP


def dev(a, grad=False):
    t = torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")
    return t.requires_grad_(True) if grad else t


def close(got, want, rtol=RTOL, atol=ATOL, msg=""):
    got = got.detach().cpu().double().numpy() if hasattr(got, "detach") else np.asarray(got)
    np.testing.assert_allclose(got, np.asarray(want), rtol=rtol, atol=atol, err_msg=msg)


def _dense_check(x, W, expect_flagged, need_dw=True):
    """engine level: E.dense_forward / E.dense_grad (coef = coef_w = 0.5, dx over a NaN-filled buffer) against
    OR.dense_forward_backward per utterance: log Z, dx, dW and the flags.  Returns (logz, dx, dW) of the kernels."""
    from gtn_applications_amd import engine as E

    B, T, C = x.shape
    xt, Wt = dev(x), dev(W)
    st = E.dense_forward(xt, Wt, need_beta=True)
    flagged = E.dense_flagged(st).cpu().tolist()
    coef = torch.full((B,), 0.5, device="cuda")
    dx = torch.full_like(xt, float("nan"))
    dW = torch.zeros_like(Wt) if need_dw else None
    E.dense_grad(xt, Wt, st, coef, coef_w=coef, dx=dx, dW=dW)
    want = [OR.dense_forward_backward(x[b], W) for b in range(B)]
    logz = st.logz.cpu().numpy()
    for b in range(B):
        if np.isfinite(want[b][0]):
            assert logz[b] == pytest.approx(want[b][0], rel=RTOL, abs=1e-4), (b, logz[b], want[b][0])
        else:
            assert logz[b] == want[b][0], b
    close(dx, np.stack([0.5 * np.nan_to_num(w[1]) for w in want]), msg="dx")
    if need_dw:
        close(dW, 0.5 * sum(np.nan_to_num(w[2]) for w in want), atol=5e-5, msg="dW")
    if expect_flagged is not None:
        assert flagged == expect_flagged
    st1 = E.dense_forward(xt, Wt, need_beta=False)  # forward only (no beta sweep): the same log Z
    np.testing.assert_allclose(st1.logz.cpu().numpy(), logz, rtol=1e-6)
    return logz, dx.cpu().numpy(), dW.cpu().numpy() if need_dw else None


# ---------------------------------------------------------------------------------------------------------------------
# range
# ---------------------------------------------------------------------------------------------------------------------
A_, B_, D_ = 0, 1, 2  # the classes of the survivor case


def _range_case(kind, C, seed):
    """(x [2, T, C], W, W[1:] hard?) -- utterance 0 the case, utterance 1 ordinary emissions under the same W"""
    rs = np.random.RandomState(seed)
    T = 6
    x = rs.randn(2, T, C).astype(np.float32)
    W = (0.3 * rs.randn(C + 1, C)).astype(np.float32)
    hard = True
    if kind in ("survivor_inf", "survivor_gap"):
        # frame 0: A scores 0, B -110; D is reachable only from B (and from itself) and the only plausible class after
        x[0] = -200.0
        x[0, 0, A_], x[0, 0, B_] = 0.0, -110.0
        x[0, 1:, D_] = 0.0
        W[1 + D_, :] = -np.inf if kind == "survivor_inf" else -120.0
        W[1 + D_, B_] = W[1 + D_, D_] = 0.0
    elif kind == "dead_row":
        W[1 + 3, :] = -np.inf  # class 3 can never be entered after frame 0
    elif kind == "start_row":
        W[0, :] = -np.inf  # one start class; W[1:] is ordinary
        W[0, 2] = 0.0
        hard = False
    elif kind == "spread_gap":
        x[0, 2:4, :] -= 90.0 * np.arange(C, dtype=np.float32) / C  # 90 nats of spread inside a frame
        W[1 + 5, 7] = W[1 + 5].max() - 50.0  # one transition 50 nats below its row maximum
    else:
        raise ValueError(kind)
    return x, W, hard


@pytest.mark.parametrize("kind", ["survivor_inf", "survivor_gap", "dead_row", "start_row", "spread_gap"])
@pytest.mark.parametrize("C", RANGE_C)
def test_dense_range_cases_on_both_sides_of_the_on_chip_limit(C, kind):
    """A transition matrix whose rows have -inf entries or a gap beyond 2^-60 of their maximum: on chip the sweeps hand
    the batch to the log-domain kernels; beyond, the batched product's range verdict on W does, for every utterance of
    the batch (the well-conditioned second utterance must come out right as well).  The survivor case: the float64
    recurrence gives log Z = -110 where a product that drops values below 2^-126 of a frame's maximum gives -inf."""
    x, W, hard = _range_case(kind, C, seed=C + len(kind))
    if kind == "start_row":
        expect = None if C <= ON_CHIP else [False, False]  # (W[0] has no bearing on the wide verdict: exact zeros)
    else:
        expect = [True, True]
    logz, _, _ = _dense_check(x, W, expect)
    if kind.startswith("survivor"):
        assert logz[0] == pytest.approx(-110.0 + W[0, B_], abs=1e-3)


@pytest.mark.parametrize("kind", ["survivor_inf", "survivor_gap"])
def test_dense_one_more_class_that_nothing_reaches_changes_nothing(kind):
    """The same utterances at 192 classes (on chip) and at 193 (the batched product) -- the extra class has -inf
    emissions and 0 transitions: log Z, and the gradients restricted to the shared classes, agree."""
    x, W, _ = _range_case(kind, ON_CHIP, seed=7)
    B, T, C = x.shape
    x2 = np.concatenate([x, np.full((B, T, 1), -np.inf, np.float32)], axis=2)
    W2 = np.zeros((C + 2, C + 1), np.float32)
    W2[:C + 1, :C] = W
    z1, dx1, dW1 = _dense_check(x, W, [True, True])
    z2, dx2, dW2 = _dense_check(x2, W2, [True, True])
    np.testing.assert_allclose(z2, z1, rtol=RTOL, atol=1e-4)
    close(dx2[:, :, :C], dx1)
    assert not dx2[:, :, C].any()
    close(dW2[:C + 1, :C], dW1, atol=5e-5)
    close(dW2[:, C], 0.0, atol=5e-5)
    close(dW2[C + 1], 0.0, atol=5e-5)


def _hard_W(C, rs, targets):
    """finite, but half of every row 120 nats below its maximum (the oracle's batched path takes finite scores); the
    transitions of the targets' force-aligned paths keep ordinary scores, so that only the denominator is hard"""
    W = (0.3 * rs.randn(C + 1, C)).astype(np.float32)
    mask = rs.rand(C, C) < 0.5
    np.fill_diagonal(mask, False)
    for tg in targets:
        for prev, cur in zip(tg, tg[1:]):
            mask[cur, prev] = False
    W[1:][mask] = -120.0
    return W


@pytest.mark.parametrize("C", [200, 330])
def test_asg_loss_with_hard_transitions_beyond_the_on_chip_limit(C):
    """ASGLoss with half the transitions 120 nats down (none of them on a target's force-aligned path): loss,
    emission gradient and transition gradient against OR.asg_loss_grad_batched; the max-plus decode of the same matrix
    against OR.dense_viterbi (the wide max-plus kernels add log scores: no range to lose)."""
    from gtn_applications_amd import engine as E
    from gtn_applications_amd.criterions import asg

    rs = np.random.RandomState(C)
    B, T = 3, 30
    x = rs.randn(B, T, C).astype(np.float32)
    targets = [rs.randint(0, C, size=n).tolist() for n in (4, 9, 1)]
    W = _hard_W(C, rs, targets)
    want_loss, want_dx, want_dW = OR.asg_loss_grad_batched(x, W, targets)
    xt, Wt = dev(x, grad=True), dev(W, grad=True)
    loss = asg.ASGLoss(xt, Wt, targets)
    loss.backward()
    assert np.isfinite(loss.item())
    assert loss.item() == pytest.approx(want_loss.mean(), rel=RTOL)
    close(xt.grad, want_dx)
    close(Wt.grad, want_dW, atol=5e-5)
    got = E.dense_viterbi(dev(x), dev(W)).cpu().tolist()
    assert got == [OR.dense_viterbi(x[b], W) for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------------
# length
# ---------------------------------------------------------------------------------------------------------------------
def _peaked(rs, B, T, C):
    s = 8.0 * rs.randn(B, T, C)
    s -= s.max(axis=2, keepdims=True)
    return (s - np.log(np.exp(s).sum(axis=2, keepdims=True))).astype(np.float32)


@pytest.mark.parametrize("C", [200, 256, 320, 330])
def test_dense_wide_thousand_frames_of_peaked_emissions(C):
    """T = 1000: the register-resident sweeps (200, 256, 320) and the per-frame launches (330) over log-softmaxed peaked
    emissions (scores x 8): log Z, dx and dW against the float64 recurrences, no flag"""
    rs = np.random.RandomState(1000 + C)
    x = _peaked(rs, 2, 1000, C)
    W = (0.5 * rs.randn(C + 1, C)).astype(np.float32)
    _dense_check(x, W, [False, False])


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("C", [200, 330])
def test_dense_wide_one_and_two_frames(C, T):
    """the shortest utterances: no frame step at all, and one"""
    rs = np.random.RandomState(C + T)
    x = (2.0 * rs.randn(3, T, C)).astype(np.float32)
    W = rs.randn(C + 1, C).astype(np.float32)
    _dense_check(x, W, [False] * 3)


@pytest.mark.parametrize("T", [8192, 8193])
@pytest.mark.parametrize("C", [200, 320])
def test_dense_wide_at_the_resident_length_limit(C, T):
    """8192 frames are the register-resident sweeps' last length (their LDS holds 8 T bytes of the utterance's row
    references: beyond 64 KB there, so the launch asks for the larger allocation); 8193 goes to the per-frame
    launches.  B = 1, log Z and dx against the float64 recurrences."""
    rs = np.random.RandomState(T + C)
    x = _peaked(rs, 1, T, C)
    W = (0.5 * rs.randn(C + 1, C)).astype(np.float32)
    _dense_check(x, W, [False], need_dw=False)


# ---------------------------------------------------------------------------------------------------------------------
# batch / tiling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_dense_wide_batches_around_the_utterance_tiles(B):
    """257 classes, batches around the 64-utterance tiles of the transition-gradient product (and of the per-frame
    launches' 16-utterance tiles); T varies with the batch so that the slabs of K = B (T - 1) rows end mid-chunk"""
    rs = np.random.RandomState(B)
    C, T = 257, 7 + B % 5
    x = (2.0 * rs.randn(B, T, C)).astype(np.float32)
    W = rs.randn(C + 1, C).astype(np.float32)
    _dense_check(x, W, [False] * B)


# ---------------------------------------------------------------------------------------------------------------------
# Transducer: the dense bigram route above the on-chip limit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank,T,hard", [("optional", 12, False), ("none", 16, False), ("optional", 14, True),
                                          ("none", 12, True)])
def test_transducer_dense_bigram_route_beyond_the_on_chip_limit(blank, T, hard):
    """199 single-character tokens, ngram = 2: C = 200 with the optional blank, 199 without -- both on the batched
    product.  Random non-zero transition parameters (hard: most of one bigram row at -150, which puts a 150-nat gap
    into most rows of the engine's W); loss, emission gradient and parameter gradient against TransducerOracle."""
    from gtn_applications_amd.criterions import transducer as tr

    ntok = 199
    tokens = [(i,) for i in range(ntok)]
    g2i = {i: i for i in range(ntok)}
    kw = dict(ngram=2, blank=blank, allow_repeats=(blank == "none"), reduction="mean")
    rs = np.random.RandomState(T + 3 * hard)
    B = 2
    C = ntok + int(blank != "none")
    x = rs.randn(B, T, C).astype(np.float32)
    targets = [rs.randint(0, ntok, size=5).tolist(), rs.randint(0, ntok, size=3).tolist()]
    m = tr.Transducer(tokens, g2i, **kw)
    assert tr._transition_model(m.transitions, C).kind == "bigram"
    params = (0.3 * rs.randn(m.transition_params.numel())).astype(np.float32)
    if hard:
        a = 11  # bigram a -> b at C + a C + b (transducer._bigram_route)
        row = params[C + a * C:C + (a + 1) * C]
        keep = row[[3, 40]].copy()
        row[:] = -150.0
        row[[3, 40]] = keep
    with torch.no_grad():
        m.transition_params.copy_(torch.from_numpy(params))
    m.cuda()
    orc = OC.TransducerOracle(tokens, g2i, **kw)
    orc.transition_params = params.astype(np.float64)
    want_loss, want_dx, want_dp = orc.loss(x, targets)
    xt = dev(x, grad=True)
    loss = m(xt, [torch.tensor(t) for t in targets])
    loss.backward()
    assert np.isfinite(loss.item())
    assert loss.item() == pytest.approx(want_loss, rel=RTOL)
    close(xt.grad, want_dx)
    close(m.transition_params.grad, want_dp, atol=2e-5)
