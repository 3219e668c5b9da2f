"""CTC prefix beam search on the device (csrc/beam_kernels.hip: wfl_ctc_beam_search behind engine.ctc_beam_search,
CTC.beam_search and CTC.errors(beam_size=)) against its restatement in plain Python (tests/beam_reference.py, itself
pinned to a brute-force enumeration in tests/test_beam_abi.py).

Acceptance of every comparison: tests/beam_support.py (assert_ranks, margins_ok), the normalised scores against the
rows' log-sum-exps summed in Python."""
import numpy as np
import pytest
import torch

import beam_reference as R
import beam_support as S
from beam_support import emissions

pytestmark = pytest.mark.gpu


def _mods():
    return S.package("engine", "metrics", "criterions.ctc:CTC")


def reference(x, blank, W, K, nbest, lengths=None):
    """per utterance (hyps, normalised hyps); asserts the margins and returns the merges too"""
    rows = S.utterances(x, lengths)
    out = []
    for b, (hyps, _, merges) in enumerate(S.margins_ok(lambda b: R.beam_search(rows[b], blank, W, K, nbest), len(rows))):
        shift = S.row_shift(rows[b])  # (the same for every hypothesis)
        out.append((hyps, [(h, s - shift if s != R.NEG else s) for h, s in hyps], merges))
    return out


def device(x, blank, W, K, nbest, lengths=None, normalize=False):
    E, _, _ = _mods()
    xd = torch.from_numpy(x).cuda()
    xlen = None if lengths is None else E.input_lengths_on_device(tuple(int(n) for n in lengths), xd.device)
    hyps, scores = E.ctc_beam_search(xd, blank, W, K, nbest, lengths=xlen, normalize=normalize)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, blank, W, K, nbest, lengths=None):
    want = reference(x, blank, W, K, nbest, lengths)
    seqs, raw = device(x, blank, W, K, nbest, lengths)
    nseqs, normed = device(x, blank, W, K, nbest, lengths, normalize=True)
    assert nseqs == seqs  # (the shift never changes the search)
    shifts = [S.row_shift(rows) for rows in S.utterances(x, lengths)]
    S.assert_ranks([hyps for hyps, _, _ in want], seqs, raw, normed, shifts, nbest, blank)
    return want


def merging_emissions(seed, B, T, C, scale, blank, W, K, merges=20):
    """the first B utterances of a seeded stream in which the reference merges at least `merges` extensions"""
    rs, rows = np.random.RandomState(seed), []
    while len(rows) < B:
        x = (rs.randn(T, C) * scale).astype(np.float32)
        if R.beam_search(x, blank, W, K, 1)[2] >= merges:
            rows.append(x)
    return np.stack(rows)


# (T, C, W, K, B)
SHAPES = [(1, 2, 1, 2, 4), (1, 5, 4, 5, 4), (12, 3, 8, 3, 4), (30, 4, 4, 4, 4), (30, 4, 8, 2, 200), (40, 12, 1, 12, 4),
          (40, 12, 16, 6, 4), (37, 65, 64, 64, 2), (64, 70, 64, 64, 1), (25, 1500, 16, 32, 2), (2, 16384, 4, 64, 2),
          (150, 28, 16, 28, 2), (300, 100, 16, 32, 1)]


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("T,C,W,K,B", SHAPES, ids=lambda v: str(v))
def test_random_emissions_against_the_reference(T, C, W, K, B, where, scale):
    blank = {"first": 0, "last": C - 1, "middle": C // 2}[where]
    seed = 7919 * T + 31 * C + W + (17 if where == "last" else 29 if where == "middle" else 0) + int(scale)
    if (T, C, W, K) == (30, 4, 8, 2):  # (the merge path, and prefixes that leave the beam and come back)
        x = merging_emissions(seed, B, T, C, scale, blank, W, K)
    else:
        x = emissions(seed, B, T, C, scale)
    want = compare(x, blank, W, K, min(3, W))
    if (T, C, W, K) == (30, 4, 8, 2):
        assert all(merges >= 20 for _, _, merges in want)


def test_half_the_classes_impossible():
    x = emissions(11, 4, 20, 8, 1.0)
    rs = np.random.RandomState(12)
    for b in range(4):
        for t in range(20):
            x[b, t, rs.permutation(8)[:4]] = -np.inf
    compare(x, 0, 8, 8, 3)
    compare(x, 3, 8, 5, 3)


def test_a_frame_where_only_the_blank_is_finite():
    x = emissions(13, 3, 20, 8, 1.0)
    x[:, 9, :] = -np.inf
    x[:, 9, 2] = 0.25
    x[1, 0, :] = -np.inf
    x[1, 0, 2] = -1.0
    compare(x, 2, 8, 8, 3)
    compare(x, 2, 8, 1, 3)


def test_scattered_nans_count_as_minus_infinity():
    x = emissions(14, 4, 20, 8, 1.0)
    rs = np.random.RandomState(15)
    x[rs.rand(*x.shape) < 0.2] = np.nan
    assert np.isfinite(x).any(axis=2).all()
    compare(x, 7, 8, 8, 3)
    y = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    assert device(x, 7, 8, 8, 3)[0] == device(y, 7, 8, 8, 3)[0]


def test_an_utterance_with_an_impossible_frame_decodes_to_nothing():
    x = emissions(16, 3, 20, 8, 1.0)
    alone = device(x[[0, 2]], 0, 8, 8, 3)
    x[1, 11, :] = -np.inf
    x[1, 11, 5] = np.nan
    want = compare(x, 0, 8, 8, 3)
    assert want[1][0] == [((), R.NEG)] * 3
    seqs, raw = device(x, 0, 8, 8, 3)
    assert seqs[1] == [(), (), ()] and (raw[1] == R.NEG).all()
    assert [seqs[0], seqs[2]] == alone[0] and (raw[[0, 2]] == alone[1]).all()  # (its neighbours are unaffected)


@pytest.mark.parametrize("blank", [0, 69])
def test_exact_ties_follow_the_tie_rule(blank):
    """All scores 0, two frames, C = 70, W = K = 64: after frame 0 every entry has tot = 0 exactly; in frame 1 the 63
    one-label hypotheses all get the same pnb' = lae(0, 0) and tot' = lae(0, pnb'), whatever the libm rounds them to --
    each is the same call on the same operands --, and some 3900 extensions tie at 0 with the empty prefix' stay entry for
    the last place in the beam.  So the margin is 0 and the order is the tie rule's alone: lower class among equal
    scores, stays before new entries, lower parent rank, lower candidate position.  (More ties than the beam has room
    for at the cut: the launch's full ranking decides, not its selection by key.)"""
    x = np.zeros((2, 2, 70), np.float32)
    hyps, margin, _ = R.beam_search(x[0], blank, 64, 64, 64)
    assert margin == 0.0
    labels = [c for c in range(70) if c != blank][:63]
    assert [h for h, _ in hyps] == [(c,) for c in labels] + [()]
    seqs, raw = device(x, blank, 64, 64, 64)
    for b in range(2):
        assert seqs[b] == [h for h, _ in hyps]
        assert all(abs(raw[b, r] - hyps[r][1]) <= 1e-9 for r in range(64))
        assert (raw[b, :63] == raw[b, 0]).all() and raw[b, 63] == 0.0


def test_lengths_decode_each_utterance_as_its_own_slice():
    B, T, C, W, K = 5, 40, 12, 16, 6
    lengths = [1, 7, 39, 40, 23]
    x = emissions(17, B, T, C, 1.0)
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan  # (the frames behind an utterance are not read)
    compare(x, 0, W, K, 3, lengths)
    seqs, raw = device(x, 0, W, K, 3, lengths)
    for b, n in enumerate(lengths):
        s, r = device(np.ascontiguousarray(x[b:b + 1, :n]), 0, W, K, 3)
        assert s[0] == seqs[b] and (r[0] == raw[b]).all(), b
    # no lengths is every utterance at T frames, and lengths beyond [0, T] are clamped by the launch
    y = emissions(18, B, T, C, 1.0)
    full = device(y, 0, W, K, 3)
    same = device(y, 0, W, K, 3, [T] * B)
    assert full[0] == same[0] and (full[1] == same[1]).all()
    E, _, _ = _mods()
    odd = torch.tensor([0, -3, T + 5, T, 2], dtype=torch.int32, device="cuda")
    hyps, scores = E.ctc_beam_search(torch.from_numpy(y).cuda(), 0, W, K, 3, lengths=odd, normalize=False)
    assert [tuple(h.tolist()) for h in hyps[0]] == [(), (), ()] and scores[0].tolist() == [0.0, R.NEG, R.NEG]
    assert scores[1].tolist() == [0.0, R.NEG, R.NEG]
    assert [tuple(h.tolist()) for h in hyps[2]] == full[0][2] and (scores[2].numpy() == full[1][2]).all()


def test_the_same_call_twice_is_bit_identical():
    x = emissions(19, 8, 60, 30, 1.0)
    a = device(x, 29, 64, 30, 3, normalize=True)
    b = device(x, 29, 64, 30, 3, normalize=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
def test_module_returns_what_viterbi_returns_and_the_scores():
    _, _, CTC = _mods()
    crit = CTC(blank=0, use_pt=False)
    B, T, C = 4, 40, 12
    x = emissions(20, B, T, C, 1.0)
    xd = torch.from_numpy(x).cuda()
    best = crit.beam_search(xd)
    greedy = crit.viterbi(xd)
    assert isinstance(best, list) and len(best) == B == len(greedy)
    assert all(type(p) is type(g) and p.dtype == g.dtype == torch.int64 and p.dim() == 1 and not p.is_cuda
               for p, g in zip(best, greedy))
    want = reference(x, 0, 16, 12, 1)
    assert [tuple(p.tolist()) for p in best] == [h[0][0] for h, _, _ in want]
    hyps, scores = crit.beam_search(xd, beam_size=8, classes_per_frame=6, nbest=3, return_scores=True)
    assert len(hyps) == B and all(isinstance(h, list) and len(h) == 3 for h in hyps)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (B, 3) and not scores.is_cuda
    want = reference(x, 0, 8, 6, 3)
    for b in range(B):
        assert [tuple(s.tolist()) for s in hyps[b]] == [h for h, _ in want[b][1]]
        for r in range(3):
            n = want[b][1][r][1]
            assert S.normalised_close(scores[b, r].item(), n)
    one, s1 = crit.beam_search(xd, beam_size=8, classes_per_frame=6, return_scores=True)
    assert tuple(s1.shape) == (B, 1) and [p.tolist() for p in one] == [h[0].tolist() for h in hyps]
    # other floating dtypes are converted, tensors that are not on a GPU are uploaded: the same search
    for other in (torch.from_numpy(x), xd.double()):
        again = crit.beam_search(other, beam_size=8, classes_per_frame=6)
        assert [p.tolist() for p in again] == [p.tolist() for p in one]
    lens = [5, 40, 17, 1]
    cut = crit.beam_search(xd, beam_size=8, classes_per_frame=6, input_lengths=lens)
    for b, n in enumerate(lens):
        assert cut[b].tolist() == crit.beam_search(xd[b:b + 1, :n], beam_size=8, classes_per_frame=6)[0].tolist()


@pytest.mark.parametrize("lens", [None, [9, 40, 23, 40, 1, 31]])
def test_errors_with_a_beam_count_what_beam_search_predicts(lens):
    _, M, CTC = _mods()
    B, T, C = 6, 40, 12
    crit = CTC(blank=C - 1, use_pt=False)
    rs = np.random.RandomState(21)
    xd = torch.from_numpy(emissions(22, B, T, C, 1.0)).cuda()
    targets = [rs.randint(0, C - 1, size=n).tolist() for n in (7, 0, 12, 3, 20, 1)]
    counter = M.ErrorCounter(wordsep=3)
    for W, K in ((1, 12), (16, 6)):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K, input_lengths=lens)
        assert crit.errors(xd, targets, counter, input_lengths=lens, beam_size=W, classes_per_frame=K) == counter(pred, targets)
    # without a beam: today's call, viterbi()'s predictions
    assert crit.errors(xd, targets, counter, input_lengths=lens) == counter(crit.viterbi(xd, lens), targets)
    assert crit.errors(xd, targets, counter, lens) == counter(crit.viterbi(xd, lens), targets)
