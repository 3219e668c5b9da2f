"""ASG prefix beam search on the device (csrc/beam_kernels.hip: wfl_asg_beam_search behind engine.asg_beam_search,
ASG.beam_search and ASG.errors(beam_size=)) against its restatement in plain Python (tests/asg_beam_reference.py, itself
pinned to an enumeration of all frame paths in tests/test_asg_beam_abi.py).

Acceptance of every comparison: the raw class sequences of all returned ranks are equal; unnormalised scores agree to
1e-9 max(1, |s|) -- both sides are float64 and differ in libm rounding only; normalised scores agree at the project's
loss bar (tests/test_gpu_configs.py: 1e-4 |want| + 2e-5), the device's denominator logz being float32.  An utterance
whose smallest selection margin in the reference is below 1e-9 could legitimately come out differently; the seeds are
fixed so that there is none, and every test asserts that."""
import numpy as np
import pytest
import torch

import asg_beam_reference as R
import beam_support as S
from beam_support import emissions, transitions
from beam_support import log_normaliser as log_denominator  # (with transitions: the criterion's denominator, asg.py:114)

pytestmark = pytest.mark.gpu

NEG = R.NEG


def _mods():
    return S.package("engine", "metrics", "criterions.asg")


def reference(x, Wt, W, K, nbest):
    """per utterance (hyps, merges); asserts the margins, so that no utterance is left out of a comparison"""
    return [(hyps, merges) for hyps, _, merges in S.margins_ok(lambda b: R.beam_search(x[b], Wt, W, K, nbest), x.shape[0])]


def device(x, Wt, W, K, nbest, normalize=False, drop=None, num_replabels=0):
    E, _, _ = _mods()
    xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
    hyps, scores = E.asg_beam_search(xd, Wd, W, K, nbest, normalize=normalize, drop=drop, num_replabels=num_replabels)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, Wt, W, K, nbest):
    want = reference(x, Wt, W, K, nbest)
    seqs, raw = device(x, Wt, W, K, nbest)
    nseqs, normed = device(x, Wt, W, K, nbest, normalize=True)
    assert nseqs == seqs  # (the shift never changes the search)
    S.assert_ranks([hyps for hyps, _ in want], seqs, raw, normed, log_denominator(x, Wt), nbest)
    return want


_WIDE = {}


def wide_transitions(C):
    """[(C+1), C] for a wide model (a gigabyte at C = 16384), made once: 257 columns ~ 0.5 N(0,1), repeated along the
    rows -- drawing every entry would take longer than the test, and a search reads a few thousand of them"""
    if C not in _WIDE:
        block = (0.5 * np.random.RandomState(C).randn(C + 1, 257)).astype(np.float32)
        _WIDE[C] = np.ascontiguousarray(np.tile(block, (1, C // 257 + 1))[:, :C])
    return _WIDE[C]


# (T, C, W, K, B): a single frame; K < C, so last labels leave the candidates; K = C; the training shape's classes; a long
# utterance with the default K; more than 512 entries per frame, so the radix select and the 1024-thread
# instantiation run; the widest model; 200 utterances in one call
SHAPES = [(1, 2, 1, 2, 4), (40, 6, 4, 3, 4), (64, 9, 8, 9, 3), (60, 29, 16, 8, 3), (200, 100, 16, 32, 1), (50, 70, 64, 64, 1),
          (3, 16384, 4, 64, 1), (40, 6, 4, 3, 200)]


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("T,C,W,K,B", SHAPES, ids=lambda v: str(v))
def test_random_emissions_against_the_reference(T, C, W, K, B, scale):
    seed = 7919 * T + 31 * C + W + B + int(scale)
    x = emissions(seed, B, T, C, scale)
    Wt = wide_transitions(C) if C > 4096 else transitions(seed + 1, C)
    want = compare(x, Wt, W, K, min(3, W))
    if (T, C) in ((64, 9), (50, 70)):  # (the merge path is taken, many times: K = C keeps every last label a candidate)
        assert all(merges >= 19 for _, merges in want), [m for _, m in want]


def test_log_denominator_helper_is_the_references():
    x, Wt = emissions(1, 2, 5, 4, 1.0), transitions(2, 4)
    got = log_denominator(x, Wt)
    for b in range(2):
        assert abs(got[b] - R.denominator(x[b], Wt)) <= 1e-9


def test_normalised_score_is_minus_the_loss_of_the_raw_hypothesis():
    """The score of a hypothesis is the mass of those of its alignments whose every prefix was in the beam and whose
    every frame class was a candidate.  Where nothing is pruned (W = 64, K = C; C = 3 with T = 4: 45 prefixes, C = 2
    with T <= 8: 16) that is every alignment, and the normalised score is minus the criterion's loss of the raw
    sequence, at the loss bar.  Where the beam prunes (T = 40, C = 6, W = 4, K = 3) it is a lower bound of it."""
    _, _, asg = _mods()

    def minus_loss(xd, Wd, b, seq):
        # (ASGLoss averages over its batch, asg.py:116-121: an utterance's own loss is that of a batch of one)
        return -float(asg.ASGLoss(xd[b:b + 1], Wd, [list(seq)], "none"))

    for (T, C, B), scale in (((4, 3, 4), 1.0), ((4, 3, 4), 3.0), ((8, 2, 4), 1.0), ((6, 2, 4), 3.0)):
        x, Wt = emissions(101 + T + C, B, T, C, scale), transitions(102 + T, C)
        seqs, normed = device(x, Wt, 64, C, 3, normalize=True)
        xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
        for b in range(B):
            for r in range(3):
                if normed[b, r] == NEG:
                    continue
                want = minus_loss(xd, Wd, b, seqs[b][r])
                assert abs(normed[b, r] - want) <= 1e-4 * abs(want) + 2e-5, (T, C, b, r, normed[b, r], want)
    x, Wt = emissions(141, 4, 40, 6, 1.0), transitions(142, 6)
    seqs, normed = device(x, Wt, 4, 3, 1, normalize=True)
    xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
    for b in range(4):
        assert len(seqs[b][0]) > 0
        want = minus_loss(xd, Wd, b, seqs[b][0])
        assert normed[b, 0] <= want + 1e-4 * abs(want) + 2e-5, (b, normed[b, 0], want)


@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_where_nothing_is_pruned_the_probabilities_add_up_to_one(scale):
    """T = 4, C = 3, W = 64, K = 3: at most 45 prefixes, every sequence is in the final beam"""
    x, Wt = emissions(31 + int(scale), 6, 4, 3, scale), transitions(32, 3)
    seqs, normed = device(x, Wt, 64, 3, 64, normalize=True)
    for b in range(6):
        total = float(np.exp(normed[b]).sum())
        assert abs(total - 1.0) <= 1e-4 + 2e-5, (b, total)
        assert len({s for s, v in zip(seqs[b], normed[b]) if v > NEG}) == 3 + 6 + 12 + 24


def test_scattered_nans_count_as_minus_infinity():
    x, Wt = emissions(14, 4, 20, 8, 1.0), transitions(15, 8)
    rs = np.random.RandomState(15)
    x[rs.rand(*x.shape) < 0.2] = np.nan
    assert np.isfinite(x).any(axis=2).all()
    compare(x, Wt, 8, 8, 3)
    y = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    assert device(x, Wt, 8, 8, 3)[0] == device(y, Wt, 8, 8, 3)[0]


def test_half_the_classes_impossible():
    x, Wt = emissions(11, 4, 20, 8, 1.0), transitions(12, 8)
    rs = np.random.RandomState(12)
    for b in range(4):
        for t in range(20):
            x[b, t, rs.permutation(8)[:4]] = -np.inf
    compare(x, Wt, 8, 8, 3)
    compare(x, Wt, 8, 5, 3)


def test_forbidden_transitions_never_appear_in_a_result():
    C = 8
    x, Wt = emissions(41, 4, 30, C, 1.0), transitions(42, C)
    rs = np.random.RandomState(43)
    mask = rs.rand(C + 1, C) < 0.3
    mask[1:][np.eye(C, dtype=bool)] = False  # (the self transitions stay: every class can last)
    mask[0, :2] = False
    Wt[mask] = -np.inf
    Wt[0, 7] = np.nan  # (a NaN counts as -inf)
    want = compare(x, Wt, 16, C, 3)
    seqs, raw = device(x, Wt, 16, C, 16)
    found = 0
    for b in range(4):
        for s, v in zip(seqs[b], raw[b]):
            if v == NEG:
                continue
            found += 1
            assert not mask[0, s[0]] and s[0] != 7, (b, s)
            assert all(not mask[1 + c, l] for l, c in zip(s, s[1:])), (b, s)
    assert found >= 32 and all(h[0][1] > NEG for h, _ in want)


def test_an_utterance_with_an_impossible_frame_decodes_to_nothing():
    x, Wt = emissions(16, 3, 20, 8, 1.0), transitions(17, 8)
    alone = device(x[[0, 2]], Wt, 8, 8, 3)
    x[1, 11, :] = -np.inf
    x[1, 11, 5] = np.nan
    want = compare(x, Wt, 8, 8, 3)
    assert want[1][0] == [((), NEG)] * 3
    seqs, raw = device(x, Wt, 8, 8, 3)
    assert seqs[1] == [(), (), ()] and (raw[1] == NEG).all()
    assert [seqs[0], seqs[2]] == alone[0] and (raw[[0, 2]] == alone[1]).all()  # (its neighbours are unaffected)
    # the same through the mapping of the results, and with normalised scores
    seqs, normed = device(x, Wt, 8, 8, 3, normalize=True, drop=7, num_replabels=1)
    assert seqs[1] == [(), (), ()] and (normed[1] == NEG).all()


def test_exact_ties_follow_the_tie_rule():
    """x and Wt all zero, two frames, C = 70, W = K = 64: frame 0 makes the 64 one-label hypotheses of the classes 0..63,
    all at 0; in frame 1 their 64 stay entries and 64 x 63 extensions all tie at 0 for the 64 places.  So the margin is 0
    and the order is the tie rule's alone: lower class among equal scores, stays before new entries, lower parent rank.
    (More ties than the beam has room for at the cut: the launch's full ranking decides, not its selection by key.)"""
    x, Wt = np.zeros((2, 2, 70), np.float32), np.zeros((71, 70), np.float32)
    hyps, margin, _ = R.beam_search(x[0], Wt, 64, 64, 64)
    assert margin == 0.0
    assert hyps == [((c,), 0.0) for c in range(64)]
    seqs, raw = device(x, Wt, 64, 64, 64)
    for b in range(2):
        assert seqs[b] == [h for h, _ in hyps]
        assert (raw[b] == 0.0).all()
    # one frame, a beam narrower than K: the new entries tie among themselves and the lower candidate position wins
    seqs, raw = device(np.ascontiguousarray(x[:, :1]), Wt, 5, 64, 5)
    assert seqs[0] == seqs[1] == [(c,) for c in range(5)] and (raw == 0.0).all()


def test_the_same_call_twice_is_bit_identical():
    x, Wt = emissions(19, 8, 60, 30, 1.0), transitions(20, 30)
    a = device(x, Wt, 64, 30, 3, normalize=True)
    b = device(x, Wt, 64, 30, 3, normalize=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    c = device(x, Wt, 64, 30, 3, normalize=True, drop=29, num_replabels=2)
    d = device(x, Wt, 64, 30, 3, normalize=True, drop=29, num_replabels=2)
    assert c[0] == d[0] and c[1].tobytes() == a[1].tobytes() == d[1].tobytes()  # (the mapping never touches the scores)


# ------------------------------------------------------------------------------------------------------------------
# the mapping of the results and the module
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,garbage", [(0, True), (1, False), (1, True), (2, True), (3, False)])
def test_results_mapped_on_the_device_are_the_raw_results_unpacked(R_, garbage):
    """few classes and many frames: replabels behind labels, behind replabels and first, garbage between them"""
    C = 3 + R_ + int(garbage)
    drop = C - 1 if garbage else None
    x, Wt = emissions(50 + R_, 5, 70, C, 1.0), transitions(51, C)
    seqs, raw = device(x, Wt, 8, C, 3)
    mapped, scores = device(x, Wt, 8, C, 3, drop=drop, num_replabels=R_)
    assert (scores == raw).all()
    for b in range(5):
        assert [list(m) for m in mapped[b]] == [R.unpack(s, drop, R_) for s in seqs[b]], b
    assert any(m != s for mb, sb in zip(mapped, seqs) for m, s in zip(mb, sb))  # (the mapping is not the identity here)


@pytest.mark.parametrize("num_replabels,use_garbage", [(1, True), (2, True), (1, False), (2, False)])
def test_module_returns_what_viterbi_returns_and_the_scores(num_replabels, use_garbage):
    E, M, asg = _mods()
    crit = asg.ASG(5, num_replabels=num_replabels, use_garbage=use_garbage).cuda()
    C, B, T = crit.N, 4, 50
    x, Wt = emissions(60 + num_replabels, B, T, C, 1.0), transitions(61, C)
    with torch.no_grad():
        crit.transitions.copy_(torch.from_numpy(Wt))
    xd = torch.from_numpy(x).cuda()
    best = crit.beam_search(xd)
    greedy = crit.viterbi(xd)
    assert isinstance(best, list) and len(best) == B == len(greedy)
    assert all(p.dtype == torch.int64 and p.dim() == 1 and not p.is_cuda for p in best)
    raw, _ = device(x, Wt, 16, min(C, 32), 1)
    assert [p.tolist() for p in best] == [R.unpack(s[0], crit.garbage_idx, num_replabels) for s in raw]
    assert [p.tolist() for p in best] == [asg.unpack_replabels([v for v in s[0] if v != crit.garbage_idx], num_replabels)
                                          for s in raw]
    # collapse_and_unpack (what viterbi() applies to its frame paths on the host) applied to the raw results
    paths = np.full((B, T), -1, np.int64)
    for b, s in enumerate(raw):
        paths[b, :len(s[0])] = s[0]
        paths[b, len(s[0]):] = s[0][-1]  # (the last class repeated: collapsed away again)
    assert [p.tolist() for p in best] == [p.tolist() for p in
                                          asg.collapse_and_unpack(paths, crit.garbage_idx, num_replabels)]
    hyps, scores = crit.beam_search(xd, beam_size=8, classes_per_frame=4, nbest=3, return_scores=True)
    assert len(hyps) == B and all(isinstance(h, list) and len(h) == 3 for h in hyps)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (B, 3) and not scores.is_cuda
    raw, normed = device(x, Wt, 8, 4, 3, normalize=True)
    want = reference(x, Wt, 8, 4, 3)
    assert [[h for h, _ in hyps_b] for hyps_b, _ in want] == raw
    assert (scores.numpy() == normed).all()
    for b in range(B):
        assert [p.tolist() for p in hyps[b]] == [R.unpack(s, crit.garbage_idx, num_replabels) for s in raw[b]]
    # other floating dtypes are converted, tensors that are not on a GPU are uploaded: the same search
    for other in (torch.from_numpy(x), xd.double()):
        again = crit.beam_search(other, beam_size=8, classes_per_frame=4, nbest=3)
        assert [[p.tolist() for p in h] for h in again] == [[p.tolist() for p in h] for h in hyps]
    # errors(beam_size=) counts what beam_search predicts; without it the call is what it was
    rs = np.random.RandomState(62)
    targets = [rs.randint(0, 5, size=n).tolist() for n in (7, 0, 12, 3)]
    counter = M.ErrorCounter(wordsep=3)
    for W, K in ((1, C), (16, 4)):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K) == counter(pred, targets)
    assert crit.errors(xd, targets, counter) == counter(crit.viterbi(xd), targets)


def test_on_peaked_emissions_with_zero_transitions_the_search_is_viterbi():
    _, _, asg = _mods()
    crit = asg.ASG(6, num_replabels=2, use_garbage=True).cuda()  # (transitions: zero)
    C, B, T = crit.N, 4, 80
    rs = np.random.RandomState(70)
    x = rs.randn(B, T, C).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            n, c = int(rs.randint(1, 6)), int(rs.randint(0, C))
            x[b, t:t + n, c] += 25.0
            t += n
    xd = torch.from_numpy(x).cuda()
    best, greedy = crit.beam_search(xd), crit.viterbi(xd)
    assert [p.tolist() for p in best] == [g.tolist() for g in greedy]
    assert any(p.numel() > 0 for p in best)
