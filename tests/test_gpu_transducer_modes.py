"""The Transducer loss (criterions/transducer.py, csrc/pack.cpp, csrc/lattice_kernels.hip) in its four token-graph modes
-- blank "none", "optional" with repeats, "optional" without repeats, "forced" -- at sizes where the sweeps' machinery
is at work: workgroups of 128 - 1024 threads, the three degree classes of prob_chain_kernel, acceptors the
probability-domain sweeps must hand to the log domain (more than kLeanDeg arcs at a state, more than 1024 states),
T on both sides of 64 and no multiple of 16, and utterances that cannot be aligned beside ones that can.

Reference: float64, never the package's kernels.  Per utterance the oracle's alignment acceptor
(oracle.criteria.TransducerOracle.alignment_graph), the lattice recurrence on log_softmax(x[b])
(oracle.recurrences.lattice_forward_backward) and the chain rule through log_softmax, as
tests/test_gpu_parity.py::_transducer_oracle; with a transition model TransducerOracle.loss.  The single-alignment cases
have closed forms in numpy that do not need the oracle at all.  Oracle answers are made once per (case, mode).

The bar is tests/test_gpu_configs.py's: per-utterance loss within 1e-4 relative (read from the step's own log Z of
every utterance, under reduction "none" where the case runs it), every gradient element within
1e-4 |want| + 2e-5 |coef_b| (coef_b = scale_b / B), transition-parameter gradients rtol 1e-4 / atol 2e-5.  An utterance
without an alignment: loss +inf, its gradient rows 0.0 exactly.  With WFL_WORST_CASES=<file> the worst ratio to the bar
of every case and the sweep format of each of its utterances (0 log domain, 1 probability domain, 2 met in the middle)
are written there (profiles/transducer_modes_parity_worst_cases.json).

Empty targets are not passed anywhere here (their acceptor has no state: a question for the packer, not for this file)."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

from oracle import criteria as OC
from oracle import recurrences as OR

pytestmark = pytest.mark.gpu

RTOL = 1e-4
ATOL_SCALE = 2e-5
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _tr():
    from gtn_applications_amd.criterions import transducer

    return transducer


def record(case, ratio=None, formats=None):
    """the worst ratio to the bar per case, and the sweep formats of its utterances"""
    rec = WORST.setdefault(case, {"max_err_over_tol": -1.0})
    changed = False
    if ratio is not None and ratio > rec["max_err_over_tol"]:
        rec["max_err_over_tol"], changed = float(ratio), True
    if formats is not None and rec.get("formats") != list(formats):
        rec["formats"], changed = list(formats), True
    path = os.environ.get("WFL_WORST_CASES")
    if changed and path:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        new = dict(rec)
        new["max_err_over_tol"] = max(rec["max_err_over_tol"], old.get(case, {}).get("max_err_over_tol", -1.0))
        old[case] = new
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def check(case, what, got, want, scale):
    """|got - want| <= RTOL |want| + ATOL_SCALE scale, elementwise; the worst ratio goes to the record"""
    got = got.detach().cpu().double().numpy() if hasattr(got, "detach") else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (case, what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{case} {what}: not finite"
    err = np.abs(got - want)
    tol = RTOL * np.abs(want) + ATOL_SCALE * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    k = int(np.argmax(ratio)) if ratio.size else 0
    worst = float(ratio.flat[k]) if ratio.size else 0.0
    print(f"{case} {what}: worst err/tol {worst:.4g}")
    record(case, worst)
    assert worst <= 1.0, (f"{case} {what}: |{got.flat[k]:.9g} - {want.flat[k]:.9g}| = {err.flat[k]:.3g} > {tol.flat[k]:.3g} "
                          f"at flat index {k}")


# ---------------------------------------------------------------------------------------------------------------------
# token sets, modes, cases
# ---------------------------------------------------------------------------------------------------------------------
SETS = {
    "letters": (list("abcde"), "abcde"),
    "pieces12": (["a", "b", "c", "d", "ab", "bc", "abc", "ca", "dd", "cab", "e", "ea"], "abcde"),
    "nested": (["a", "aa", "aaa", "aaaa", "b", "ab", "ba", "aab", "baa", "abab"], "ab"),
    "nested18": (["a", "b", "aa", "ab", "ba", "bb", "aaa", "aab", "aba", "abb", "baa", "bab", "bba", "bbb",
                  "aaaa", "abab", "baba", "bbbb"], "ab"),
    "deep": (["a" * k for k in range(1, 11)] + ["b"], "ab"),
}
SETS.update({f"deep{n}": (["a" * k for k in range(1, n + 1)] + ["b"], "ab") for n in (6, 7, 8)})
MODES = {"none": ("none", True), "optional": ("optional", True), "norepeat": ("optional", False), "forced": ("forced", True)}
MODE_NAMES = list(MODES)
# case: (token set -- or one per mode --, T, targets: a grapheme count of a seeded random target, or the target spelled
# out --, seed).  degree8 / degree9: `deep` with as many pieces as put exactly kLeanDeg = 8 and kLeanDeg + 1 arcs at a
# state of the first utterance -- the last acceptor the lean sweeps take and the first they must decline (`deep` itself
# has 11 - 12).  letters330: T from which the sweeps meet in the middle by default (320), no multiple of 16, with a
# target that the modes without repeats and with forced blanks cannot align.
_PER_MODE = lambda n: {m: f"deep{n - (m == 'optional')}" for m in MODES}  # noqa: E731
CASES = {
    "letters16": ("letters", 16, (1, 7, 8, 16), 2),
    "letters65": ("letters", 65, (1, 2, 32, 33, 64, 65), 1),
    "letters330": ("letters", 330, ("a" * 200, 20, 100), 9),
    "pieces12": ("pieces12", 130, (5, 20, 52), 3),
    "nested": ("nested", 200, (90, 40), 4),
    "deep": ("deep", 80, ("a" * 30, 12), 6),
    "nested18": ("nested18", 300, (250,), 5),
    "degree8": (_PER_MODE(7), 80, ("a" * 30, 12), 7),
    "degree9": (_PER_MODE(8), 80, ("a" * 30, 12), 8),
}


def _criterion(set_name, mode, reduction, **kw):
    pieces, alpha = SETS[set_name]
    blank, rep = MODES[mode]
    return _tr().Transducer(pieces, {ch: i for i, ch in enumerate(alpha)}, blank=blank, allow_repeats=rep,
                            reduction=reduction, **kw)


def _utterance(orc, target, xin):
    """the oracle's acceptor of `target` and the float64 recurrence on the log-probabilities xin [T, C]"""
    ali = orc.alignment_graph(target)
    n = ali.num_nodes()
    src, dst = np.asarray(ali.src, dtype=np.int64), np.asarray(ali.dst, dtype=np.int64)
    assert (np.asarray(ali.ilab) >= 0).all()
    logz, g, _ = OR.lattice_forward_backward(xin, ali.src, ali.dst, ali.ilab, np.zeros(len(src)), ali.start_nodes(),
                                             ali.accept_nodes(), n)
    deg = max(int(np.bincount(dst, minlength=n).max()), int(np.bincount(src, minlength=n).max())) if len(src) else 0
    return dict(states=n, deg=deg, logz=logz, g=g, feasible=bool(np.isfinite(logz)))


class _Case:
    """data and oracle answers of one (case, mode): made once, never written to"""

    def __init__(self, set_name, mode, T, targets, seed):
        pieces, alpha = SETS[set_name]
        blank, rep = MODES[mode]
        self.set_name, self.mode, self.T, self.targets = set_name, mode, T, targets
        self.B, self.C = len(targets), len(pieces) + int(blank != "none")
        self.x = np.random.RandomState(seed).randn(self.B, T, self.C).astype(np.float32)
        self.orc = OC.TransducerOracle(pieces, {ch: i for i, ch in enumerate(alpha)}, blank=blank, allow_repeats=rep)
        self.lp = OC.log_softmax(self.x.astype(np.float64), 2)
        self.utts = [_utterance(self.orc, t, self.lp[b]) for b, t in enumerate(targets)]
        self.feasible = [u["feasible"] for u in self.utts]
        self.x.setflags(write=False)
        self._plain = None

    def tensors(self):
        return [torch.tensor(t) for t in self.targets]

    def scales(self, reduction):
        return np.array([1.0 / len(t) if reduction == "mean" else 1.0 for t in self.targets])

    def want(self, reduction):
        """(per-utterance losses [B] -- +inf without an alignment --, dx [B, T, C] through log_softmax, coef [B])"""
        sc = self.scales(reduction)
        losses, dx = np.full(self.B, np.inf), np.zeros(self.x.shape)
        for b, u in enumerate(self.utts):
            if u["feasible"]:
                din = -u["g"] * sc[b] / self.B
                losses[b] = -u["logz"] * sc[b]
                dx[b] = din - np.exp(self.lp[b]) * din.sum(axis=1, keepdims=True)
        return losses, dx, sc / self.B

    def want_plain(self, reduction):
        """the same for TransducerLoss on the float32 log-probabilities themselves: no chain rule through log_softmax"""
        if self._plain is None:
            lp32 = torch.log_softmax(torch.tensor(self.x), 2).numpy()
            self._plain = (lp32, [_utterance(self.orc, t, lp32[b].astype(np.float64)) for b, t in enumerate(self.targets)])
        lp32, utts = self._plain
        sc = self.scales(reduction)
        losses, dx = np.full(self.B, np.inf), np.zeros(self.x.shape)
        for b, u in enumerate(utts):
            if u["feasible"]:
                losses[b], dx[b] = -u["logz"] * sc[b], -u["g"] * sc[b] / self.B
        return lp32, losses, dx, sc / self.B


def _random_targets(alpha, specs, seed):
    rnd = random.Random(seed)
    g2i = {ch: i for i, ch in enumerate(alpha)}
    return [[g2i[ch] for ch in s] if isinstance(s, str) else [g2i[rnd.choice(alpha)] for _ in range(s)] for s in specs]


@functools.lru_cache(maxsize=None)
def case(name, mode):
    set_name, T, specs, seed = CASES[name]
    set_name = set_name[mode] if isinstance(set_name, dict) else set_name
    return _Case(set_name, mode, T, _random_targets(SETS[set_name][1], specs, seed), seed)


def _rule(mode, target, T):
    """is there an alignment of `target` (single-grapheme tokens) to T frames?"""
    L = len(target)
    r = sum(a == b for a, b in zip(target[:-1], target[1:]))
    return {"none": L <= T, "optional": L <= T, "norepeat": L + r <= T, "forced": 2 * L + 1 <= T}[mode]


def _formats(loss, B, T):
    from test_gpu_parity import _sweep_formats

    return _sweep_formats(loss, B, T)


def step(m, c, x=None, leaf=True, mult=None, call=None):
    """one step of criterion `m` on the case's batch -> (loss, per-utterance log Z [B], gradient, formats, "EagerLoss" if
    the launch of the sweeps wrote the gradient beside them, else "Tensor")"""
    xi = torch.tensor(c.x if x is None else x, device="cuda", requires_grad=True)
    loss = (call or m)(xi if leaf else xi * 1.0, c.tensors())
    fm, kind = _formats(loss, c.B, c.T), type(loss).__name__
    logz = loss.grad_fn.aux.num.logz.detach().cpu().double().numpy().copy()
    (loss if mult is None else loss * mult).backward()
    return loss.detach().clone(), logz, xi.grad.clone(), fm, kind


def check_step(key, c, reduction, loss, logz, dx, mult=1.0, want=None):
    """a step's loss (scalar and per utterance) and gradient against the oracle: the bar on the utterances with an
    alignment, +inf / rows of 0.0 on the others"""
    want_l, want_dx, coef = want or c.want(reduction)
    feas = np.array(c.feasible)
    sc = c.scales(reduction)
    assert loss.dim() == 0
    if feas.all():
        check(key, "loss", np.array(loss.item()), np.array(want_l.mean()), 0.0)
    else:
        assert loss.item() == float("inf"), (key, loss.item())
    got_l = -logz * sc
    assert (got_l[~feas] == np.inf).all(), (key, got_l)
    check(key, "per-utterance loss", got_l[feas], want_l[feas], 0.0)
    dx = dx.detach().cpu().numpy()
    for b in range(c.B):
        if feas[b]:
            check(key, f"dx[{b}]", dx[b], mult * want_dx[b], abs(mult) * coef[b])
        else:
            assert (dx[b] == 0.0).all(), f"{key}: gradient rows of utterance {b} (no alignment) are not exactly zero"


# the class every case is in: states of the utterance named, the most arcs into or out of a state (from the oracle's graph)
def _assert_class(name, mode, c):
    states, degs = [u["states"] for u in c.utts], [u["deg"] for u in c.utts]
    if c.B >= 2:
        assert sum(c.feasible) >= 2, (name, mode, c.feasible)
    if name.startswith("letters"):
        assert c.feasible == [_rule(mode, t, c.T) for t in c.targets]
        assert max(degs) <= 4 and (mode != "none" or max(degs) == 2)
        if name == "letters65":  # what cannot be aligned: 33 and up in forced, 64 and 65 without repeats
            bad = {"forced": [3, 4, 5], "norepeat": [4, 5]}.get(mode, [])
            assert [b for b in range(c.B) if not c.feasible[b]] == bad
    elif name == "pieces12":
        assert 68 <= states[2] <= 121 and max(states) == states[2] and 3 <= max(degs) <= 4, (states, degs)
    elif name == "nested":
        assert 192 <= states[0] <= 283 and 5 <= degs[0] <= 6 and degs[1] <= 8, (states, degs)
    elif name == "deep":
        assert 256 <= states[0] <= 287 and 11 <= degs[0] <= 12 and degs[1] <= 8, (states, degs)
    elif name == "nested18":
        assert states == [814 if mode == "none" else 1065] and max(degs) <= 8, (states, degs)
    elif name in ("degree8", "degree9"):
        assert 129 <= states[0] <= 256 and degs[0] == int(name[-1]) and degs[1] <= degs[0], (states, degs)


def _want_formats(name, mode, c, fm, kind):
    """Format 0 where the lean probability-domain sweeps must decline and their launch hands over to the log domain:
    more than kLeanDeg arcs at a state (the first utterance of deep and degree9), in the launch that writes the gradient
    beside the sweeps (256 - 512 threads; `kind` says that it ran).  Another format at every other utterance with an
    alignment.  nested18 in the blank modes, 1065 states: more than the 1024 threads of its workgroups, so not the lean
    sweep either -- but its launch (no gradient beside the sweeps at 1024 threads) keeps such an acceptor in the
    probability domain, threads looping over the states (run_chain_prob_general, as
    test_gpu_parity.py::test_general_probability_sweep_on_random_acceptors has it at 1100 states): format 1, and the
    log-domain chain_kernel behind it finds nothing to do."""
    declined = [u["deg"] > 8 for u in c.utts]
    assert declined[0] == (name in ("deep", "degree9"))
    if any(declined):
        assert kind == "EagerLoss", (name, mode, kind)
    for b in range(c.B):
        if c.feasible[b]:
            assert (fm[b] == 0) == declined[b], (name, mode, b, fm)
    if name == "nested18":
        assert fm == [1], (name, mode, fm)


# ---------------------------------------------------------------------------------------------------------------------
# 1. loss and gradient in all four modes
# ---------------------------------------------------------------------------------------------------------------------
_TABLE = [(n, r) for n in CASES for r in (("none", "mean") if n.startswith("letters") else ("mean",))]


@pytest.mark.parametrize("name,reduction", _TABLE)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_loss_and_gradient_in_every_mode(mode, name, reduction):
    """the module call (fused log_softmax) on random normal emissions; every case of the table in every mode"""
    c = case(name, mode)
    _assert_class(name, mode, c)
    key = f"{name}/{mode}/{reduction}"
    m = _criterion(c.set_name, mode, reduction)
    loss, logz, dx, fm, kind = step(m, c)
    record(key, formats=fm)
    check_step(key, c, reduction, loss, logz, dx)
    _want_formats(name, mode, c, fm, kind)


@pytest.mark.parametrize("name", ["letters65", "pieces12", "nested"])
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_sweeps_that_meet_in_the_middle_in_every_mode(mode, name, monkeypatch):
    """WFL_LATTICE_MITM=2: the two sweeps of an utterance meet in the middle from 64 frames on (by default from 320), at
    T = 65, 130 and 200 -- one frame past 64, and no multiples of 16.  They do in the launch that writes the gradient
    beside them, workgroups of 256 - 512 threads (format 2); batches of at most 128 states keep the full sweeps
    (format 1): pieces12, and letters65 without a blank."""
    monkeypatch.setenv("WFL_LATTICE_MITM", "2")
    c = case(name, mode)
    key = f"{name}/{mode}/mean/mitm"
    loss, logz, dx, fm, kind = step(_criterion(c.set_name, mode, "mean"), c)
    record(key, formats=fm)
    check_step(key, c, "mean", loss, logz, dx)
    meets = max(u["states"] for u in c.utts) > 128
    assert kind == ("EagerLoss" if meets else "Tensor")
    assert all(f == (2 if meets else 1) for f, ok in zip(fm, c.feasible) if ok), fm


def _single_alignment(mode):
    """(token targets, the one frame path of each) at T = 65, two utterances per mode"""
    rs = np.random.RandomState(11)
    T, blank = 65, 5
    if mode in ("none", "optional"):  # as many labels as frames
        tg = [rs.randint(0, 5, size=T).tolist() for _ in range(2)]
        return tg, [list(t) for t in tg]
    if mode == "forced":  # 2 L + 1 = T: blank, label, blank, ... , blank
        tg = [rs.randint(0, 5, size=32).tolist() for _ in range(2)]
        return tg, [[blank if t % 2 == 0 else g[t // 2] for t in range(T)] for g in tg]
    tg = [[0] * 33, [1] * 33]  # equal neighbours without repeats: label, blank, label, ... , label
    return tg, [[g[t // 2] if t % 2 == 0 else blank for t in range(T)] for g in tg]


@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_single_alignment_closed_form(mode, reduction):
    """exactly one alignment exists: the loss is minus the sum of the log_softmax entries along it (times the scale),
    the gradient -coef_b (onehot(path) - softmax) -- numpy float64, no oracle"""
    tg, paths = _single_alignment(mode)
    B, T = 2, 65
    C = 5 + int(mode != "none")
    x = np.random.RandomState(12).randn(B, T, C).astype(np.float32)
    lp = OC.log_softmax(x.astype(np.float64), 2)
    key = f"single_alignment/{mode}/{reduction}"
    m = _criterion("letters", mode, reduction)
    xi = torch.tensor(x, device="cuda", requires_grad=True)
    loss = m(xi, [torch.tensor(t) for t in tg])
    fm = _formats(loss, B, T)
    record(key, formats=fm)
    logz = loss.grad_fn.aux.num.logz.detach().cpu().double().numpy().copy()
    loss.backward()
    want_l, want_dx = np.zeros(B), np.zeros(x.shape)
    for b in range(B):
        assert len(paths[b]) == T
        sc = 1.0 / len(tg[b]) if reduction == "mean" else 1.0
        onehot = np.zeros((T, C))
        onehot[np.arange(T), paths[b]] = 1.0
        want_l[b] = -lp[b][np.arange(T), paths[b]].sum() * sc
        want_dx[b] = -(sc / B) * (onehot - np.exp(lp[b]))
        check(key, f"per-utterance loss[{b}]", -logz[b:b + 1] * sc, want_l[b:b + 1], 0.0)
        check(key, f"dx[{b}]", xi.grad[b], want_dx[b], sc / B)
    check(key, "loss", np.array(loss.item()), np.array(want_l.mean()), 0.0)
    assert all(f != 0 for f in fm), fm


# ---------------------------------------------------------------------------------------------------------------------
# 2. call forms, per mode, on the pieces12 case -- and on nested
# ---------------------------------------------------------------------------------------------------------------------
# The launch of the sweeps writes the gradient beside them only in workgroups of 256 - 512 threads.  pieces12 has at most
# 121 states: 128 threads, NO gradient from the launch, whatever _IN_LAUNCH_GRAD says -- every call form of it ends in
# the gradient kernels of backward.  nested (192 - 283 states) does get the launch's gradient.  The forms that are about
# that buffer (who takes it, who scales it, what happens when it is gone, what the step gives without it) run on both,
# and each says which of the two it met.
_FORM_CASES = ["pieces12", "nested"]


def _launch_buffer(loss, name, on=True):
    """The gradient buffer the launch of the sweeps left on the loss's node, or None; asserts that there is one exactly
    where there should be: on nested with _IN_LAUNCH_GRAD on.  A device input then gets an EagerLoss."""
    early = loss.grad_fn.early
    buf = early.dx if early is not None else None
    want = on and name == "nested"
    assert (buf is not None) == want, (name, on, early)
    if loss.is_cuda:
        assert type(loss).__name__ == ("EagerLoss" if want else "Tensor"), (name, on, type(loss))
    return buf


@pytest.mark.parametrize("leaf", [True, False])
@pytest.mark.parametrize("name", _FORM_CASES)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_call_forms_leaf_and_non_leaf(mode, name, leaf):
    """nested: a leaf with loss.backward() gets the launch's gradient buffer itself as its .grad (no pass through the
    autograd engine); x * 1.0 with (loss * 0.75).backward() goes through the engine, where the node scales that buffer
    by 0.75 in place.  pieces12: no buffer from the launch, both forms run the gradient kernels in backward."""
    c = case(name, mode)
    key = f"{name}/{mode}/mean/{'leaf' if leaf else 'non_leaf'}"
    xi = torch.tensor(c.x, device="cuda", requires_grad=True)
    loss = _criterion(c.set_name, mode, "mean")(xi if leaf else xi * 1.0, c.tensors())
    buf = _launch_buffer(loss, name)
    logz = loss.grad_fn.aux.num.logz.detach().cpu().double().numpy().copy()
    (loss if leaf else loss * 0.75).backward()
    if leaf and buf is not None:
        assert xi.grad.data_ptr() == buf.data_ptr()
    check_step(key, c, "mean", loss.detach(), logz, xi.grad, mult=1.0 if leaf else 0.75)


@pytest.mark.parametrize("name", _FORM_CASES)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_call_forms_second_backward_over_a_retained_graph(mode, name):
    """nested: the first pass takes the launch's buffer (scaled by grad_output = 1), the second finds it gone and
    recomputes with the gradient kernels.  pieces12: both passes compute in backward.  .grad holds the sum of both."""
    c = case(name, mode)
    key = f"{name}/{mode}/mean/second_backward"
    xi = torch.tensor(c.x, device="cuda", requires_grad=True)
    loss = _criterion(c.set_name, mode, "mean")(xi, c.tensors())
    buf = _launch_buffer(loss, name)
    logz = loss.grad_fn.aux.num.logz.detach().cpu().double().numpy().copy()
    loss.backward(retain_graph=True)
    if buf is not None:
        assert loss.grad_fn.early.dx is None  # taken: the second pass cannot use it
    first = xi.grad.clone()
    check_step(key + "/first", c, "mean", loss.detach(), logz, first)
    loss.backward()
    check_step(key, c, "mean", loss.detach(), logz, xi.grad - first)
    check_step(key + "/sum", c, "mean", loss.detach(), logz, xi.grad, mult=2.0)


@pytest.mark.parametrize("name", _FORM_CASES)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_call_forms_gradient_in_backward(mode, name, monkeypatch):
    """_IN_LAUNCH_GRAD off: no buffer from the launch and a plain tensor as the loss, also on nested, whose step with the
    flag on has both.  The sweeps' arithmetic is the same, so the loss is the same bit for bit; the gradient kernels of
    backward to the bar.  (On pieces12 the flag changes nothing: the same path twice.)"""
    tr = _tr()
    c = case(name, mode)
    key = f"{name}/{mode}/mean/grad_in_backward"
    m = _criterion(c.set_name, mode, "mean")
    xi = torch.tensor(c.x, device="cuda", requires_grad=True)
    ref_loss = m(xi, c.tensors())
    _launch_buffer(ref_loss, name)
    ref_loss.backward()
    monkeypatch.setattr(tr, "_IN_LAUNCH_GRAD", False)
    xi = torch.tensor(c.x, device="cuda", requires_grad=True)
    loss = m(xi, c.tensors())
    assert _launch_buffer(loss, name, on=False) is None and type(loss) is torch.Tensor
    assert loss.item() == ref_loss.item()
    logz = loss.grad_fn.aux.num.logz.detach().cpu().double().numpy().copy()
    loss.backward()
    check_step(key, c, "mean", loss.detach(), logz, xi.grad)


def _direct_and_prepared(c, mode):
    """the case's step through criterion(x, targets) and through criterion(x, criterion.prepare(targets)), each with a
    criterion of its own (so that both pack): (loss, log Z, gradient, packed batch) of either"""
    out = []
    for prepare in (False, True):
        m = _criterion(c.set_name, mode, "mean")
        xi = torch.tensor(c.x, device="cuda", requires_grad=True)
        loss = m(xi, m.prepare(c.tensors()) if prepare else c.tensors())
        num = loss.grad_fn.aux.num
        logz = num.logz.detach().cpu().double().numpy().copy()
        loss.backward()
        out.append((loss.detach().clone(), logz, xi.grad.clone(), num.pack))
    return out


@functools.lru_cache(maxsize=None)
def _one_label_case(mode):
    """two targets of one label each: no emission column collects more than two states' posteriors (the label's one, the
    blank's two), so the float sums of the gradient kernels have one possible value whatever order they are formed in"""
    return _Case("letters", mode, 20, [[1], [3]], 31)


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_call_forms_prepared_targets(mode):
    """criterion(x, criterion.prepare(targets)): built, packed and uploaded on the side thread and its stream.  The
    packed batch is the direct call's byte for byte, the loss bit for bit (the sweeps are deterministic), the gradient
    within the bar -- and bit for bit on a batch whose sums have one possible value in any arithmetic (_one_label_case).
    The gradient of pieces12 bit for bit: test_call_forms_prepared_targets_gradient_bits."""
    c = case("pieces12", mode)
    (ref_loss, _, _, ref_pack), (loss, logz, dx, pack) = _direct_and_prepared(c, mode)
    check_step(f"pieces12/{mode}/mean/prepared", c, "mean", loss, logz, dx)
    assert loss.item() == ref_loss.item()
    assert pack is not ref_pack and bytes(pack.desc) == bytes(ref_pack.desc) and torch.equal(pack._blob, ref_pack._blob)
    small = _one_label_case(mode)
    (ref_loss, _, ref_dx, _), (loss, logz, dx, _) = _direct_and_prepared(small, mode)
    check_step(f"one_label/{mode}/mean/prepared", small, "mean", loss, logz, dx)
    assert loss.item() == ref_loss.item() and torch.equal(dx, ref_dx)


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_call_forms_prepared_targets_gradient_bits(mode):
    """The gradient of pieces12 through prepared targets, bit for bit the direct call's.  This is a statement about the
    gradient kernel as much as about prepare(): the occupancy gradient behind the sweeps (occ_grad_kernel) sums a column's
    states -- dozens for pieces12 -- as fixed-point integers, whose atomics commute.  With float atomics there, two direct
    calls of ONE criterion differed in 22 - 61 of ~5000 elements by up to 3.7e-9 (0.0017 of the bar), and so did this
    comparison.  (The gradient written BESIDE the sweeps, 256 - 512 threads, and grad_kernel's chunks keep float atomics:
    DESIGN 5.)"""
    c = case("pieces12", mode)
    (_, _, ref_dx, _), (_, _, dx, _) = _direct_and_prepared(c, mode)
    diff = (dx - ref_dx).abs()
    print(f"pieces12/{mode} prepared against direct: {int((diff != 0).sum())} of {diff.numel()} gradient elements differ, "
          f"by {diff.max().item():.3g} at most")
    assert torch.equal(dx, ref_dx)


@pytest.mark.parametrize("name", _FORM_CASES)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_call_forms_cpu_in_cpu_out(mode, name):
    """CPU emissions in, CPU loss and gradient out.  On nested the launch's buffer is on the device and nobody may hand
    it to a CPU leaf: the autograd engine runs the node, which copies it back."""
    c = case(name, mode)
    xi = torch.tensor(c.x, requires_grad=True)
    loss = _criterion(c.set_name, mode, "mean")(xi, c.tensors())
    _launch_buffer(loss, name)
    assert type(loss) is torch.Tensor
    logz = loss.grad_fn.aux.num.logz.detach().cpu().double().numpy().copy()
    loss.backward()
    assert loss.device.type == "cpu" and xi.grad.device.type == "cpu"
    check_step(f"{name}/{mode}/mean/cpu", c, "mean", loss.detach(), logz, xi.grad)


# letters / none batches for the route without log_softmax: four distinct emission columns in the first, five in the
# second; at most 63 labels, i.e. 64 states: what the banded sweep and band_grad_kernel take
_BAND = {"letters4": ("abcd", 80, (63, 17, 5), 21), "letters5": ("abcde", 80, (63, 17, 5), 22)}


@functools.lru_cache(maxsize=None)
def _band_case(name):
    alpha, T, specs, seed = _BAND[name]
    targets = _random_targets(alpha, specs, seed)
    assert len({v for t in targets for v in t}) == len(alpha) and max(map(len, targets)) <= 63
    return _Case("letters", "none", T, targets, seed)


@pytest.mark.parametrize("name,mode", [("pieces12", m) for m in MODE_NAMES] + [("letters4", "none"), ("letters5", "none")])
@pytest.mark.parametrize("reduction", ["none", "mean"])
def test_call_forms_unfused_route(name, mode, reduction):
    """TransducerLoss(log_probs, targets, tokens, lexicon) without transitions: the emissions are taken as they are, the
    reference is the oracle's gradient of its input without the softmax chain rule.

    letters4 / letters5 are built so that the first meets the conditions of the banded sweep and band_grad_kernel (at
    most 64 states, a number of distinct emission columns that is a multiple of 4) and the second does not.  Which
    kernels then ran is NOT asserted: both routes report format 1 and the package offers no other read-out, so the two
    batches are held to the oracle whichever route takes them, and a change of the band's eligibility alone would pass
    here.  The banded kernels against the general ones on the same acceptor:
    test_gpu_parity.py::test_banded_gradient_kernel_matches_the_general_kernel, test_banded_sweep_awkward_sizes."""
    tr = _tr()
    c = _band_case(name) if name in _BAND else case(name, mode)
    key = f"{name}/{mode}/{reduction}/unfused"
    lp32, want_l, want_dx, coef = c.want_plain(reduction)
    m = _criterion(c.set_name, mode, reduction)
    # what Transducer.forward does in front of its own call, and TransducerLoss leaves to its caller: the token graph's
    # arcs indexed by output label, the side the lexicon is composed on.  It changes no arc of the criterion's graph.
    m.tokens.arc_sort(True)
    loss, logz, dx, fm, kind = step(m, c, x=lp32, call=lambda xi, tg: tr.TransducerLoss(xi, tg, m.tokens, m.lexicon,
                                                                                    reduction=reduction))
    record(key, formats=fm)
    check_step(key, c, reduction, loss, logz, dx, want=(want_l, want_dx, coef))
    assert all(f != 0 for f in fm), fm


# ---------------------------------------------------------------------------------------------------------------------
# 3. transition models in the modes that lack them
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ngram_case(ngram, mode):
    blank, rep = MODES[mode]
    ntok = 6
    tokens, g2i = [(i,) for i in range(ntok)], {i: i for i in range(ntok)}
    kw = dict(ngram=ngram, blank=blank, allow_repeats=rep, reduction="mean")
    rs = np.random.RandomState(50 + ngram)
    B, T, C = 2, 20, ntok + 1
    x = rs.randn(B, T, C).astype(np.float32)
    targets = [[3, 3, 1, 4, 4, 0], [2, 2]]  # an adjacent equal pair in each: what tells the two optional modes apart
    orc = OC.TransducerOracle(tokens, g2i, **kw)
    params = (0.3 * rs.randn(len(orc.transition_params))).astype(np.float32)
    assert (params != 0).all()
    orc.transition_params = params.astype(np.float64)
    return tokens, g2i, kw, x, targets, params, orc.loss(x, targets)


@pytest.mark.parametrize("ngram,route", [(1, "lattice"), (1, "dense"), (2, "lattice"), (2, "dense")])
@pytest.mark.parametrize("mode", ["forced", "optional"])
def test_ngram_transitions_forced_and_optional_with_repeats(mode, ngram, route, monkeypatch):
    """test_gpu_parity.py::test_transducer_dense_ngram_transitions covers "none" and "optional" without repeats: here
    the other two, by the general lattice sweep and by the dense routes (_DENSE_NGRAM off / on)"""
    tr = _tr()
    monkeypatch.setattr(tr, "_DENSE_NGRAM", route == "dense")
    tokens, g2i, kw, x, targets, params, (want_loss, want_dx, want_dp) = _ngram_case(ngram, mode)
    key = f"ngram{ngram}/{mode}/{route}"
    m = tr.Transducer(tokens, g2i, **kw)
    assert (tr._transition_model(m.transitions, x.shape[2]).kind == "bigram") == (ngram == 2)
    with torch.no_grad():
        m.transition_params.copy_(torch.from_numpy(params))
    m.cuda()
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    loss = m(xt, [torch.tensor(t) for t in targets])
    loss.backward()
    check(key, "loss", np.array(loss.item()), np.array(want_loss), 0.0)
    for b in range(len(targets)):
        check(key, f"dx[{b}]", xt.grad[b], want_dx[b], 1.0 / (len(targets[b]) * len(targets)))
    got_dp = m.transition_params.grad.detach().cpu().double().numpy()
    err, tol = np.abs(got_dp - want_dp), RTOL * np.abs(want_dp) + 2e-5
    print(f"{key} dparams: worst err/tol {float((err / tol).max()):.4g}")
    record(key, float((err / tol).max()))
    np.testing.assert_allclose(got_dp, want_dp, rtol=RTOL, atol=2e-5, err_msg=key)


def test_ngram_cases_tell_the_two_optional_modes_apart():
    """(a property of the inputs, not of the kernels: with an adjacent equal pair the alignments differ)"""
    for ngram in (1, 2):
        tokens, g2i, kw, x, targets, params, (with_rep, _, _) = _ngram_case(ngram, "optional")
        orc = OC.TransducerOracle(tokens, g2i, **dict(kw, allow_repeats=False))
        orc.transition_params = params.astype(np.float64)
        assert abs(orc.loss(x, targets)[0] - with_rep) > 1e-3 * abs(with_rep)


# ---------------------------------------------------------------------------------------------------------------------
# 4. utterances without an alignment beside ones that have one
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_launch", [True, False])
@pytest.mark.parametrize("name", ["letters16", "letters65", "letters65/mitm", "letters330"])
@pytest.mark.parametrize("mode", ["norepeat", "forced"])
def test_infeasible_utterances_beside_feasible_ones(mode, name, in_launch, monkeypatch):
    """the documented policy: +inf loss and gradient rows of exactly 0.0 for the utterance that cannot be aligned; its
    neighbours to the bar, with the gradient written beside the sweeps and in backward.  Under "mean" the loss is +inf
    as well and the neighbours' rows still meet the bar."""
    tr = _tr()
    monkeypatch.setattr(tr, "_IN_LAUNCH_GRAD", in_launch)
    if name.endswith("/mitm"):
        monkeypatch.setenv("WFL_LATTICE_MITM", "2")
    c = case(name.split("/")[0], mode)
    assert not all(c.feasible) and sum(c.feasible) >= 2
    for reduction in ("none", "mean"):
        key = f"{name}/{mode}/{reduction}/infeasible/{'in_launch' if in_launch else 'in_backward'}"
        loss, logz, dx, fm, kind = step(_criterion(c.set_name, mode, reduction), c)
        record(key, formats=fm)
        assert loss.item() == float("inf")
        check_step(key, c, reduction, loss, logz, dx)
        for b in range(c.B):
            if not c.feasible[b]:
                assert logz[b] == -np.inf and (dx[b] == 0.0).all().item()
