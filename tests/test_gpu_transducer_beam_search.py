"""Transducer prefix beam search on the device (csrc/beam_kernels.hip: wfl_transducer_beam_search behind
engine.transducer_beam_search, Transducer.beam_search and Transducer.errors(beam_size=)) against its restatement in
plain Python (tests/transducer_beam_reference.py, itself pinned to an enumeration of all frame paths and to the oracle's
loss in tests/test_transducer_beam_abi.py).

Acceptance of every comparison: the token sequences of all returned ranks are equal; unnormalised scores agree to
1e-9 max(1, |s|) -- both sides are float64 and differ in libm rounding only; normalised scores agree at the project's
loss bar (tests/test_gpu_configs.py: 1e-4 |want| + 2e-5), the device's normaliser being float32.  An utterance whose
smallest selection margin in the reference is below 1e-9 could legitimately come out differently; the seeds are fixed so
that there is none, and every test asserts that."""
import numpy as np
import pytest
import torch

import beam_support as S
import transducer_beam_reference as R
from beam_support import emissions, log_normaliser, transitions  # noqa: F401 (the merged file takes them from here)

pytestmark = pytest.mark.gpu

NEG = R.NEG


def _mods():
    return S.package("engine", "metrics", "criterions.transducer")


def reference(x, Wt, blank, forced, W, K, nbest):
    """per utterance (hyps, merges); asserts the margins, so that no utterance is left out of a comparison"""
    search = lambda b: R.beam_search(x[b], Wt, blank, forced, W, K, nbest)
    return [(hyps, merges) for hyps, _, merges in S.margins_ok(search, x.shape[0])]


def device(x, Wt, blank, forced, W, K, nbest, normalize=False):
    E, _, _ = _mods()
    xd = torch.from_numpy(x).cuda()
    Wd = None if Wt is None else torch.from_numpy(Wt).cuda()
    hyps, scores = E.transducer_beam_search(xd, Wd, blank, forced, W, K, nbest, normalize=normalize)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, Wt, blank, forced, W, K, nbest):
    want = reference(x, Wt, blank, forced, W, K, nbest)
    seqs, raw = device(x, Wt, blank, forced, W, K, nbest)
    nseqs, normed = device(x, Wt, blank, forced, W, K, nbest, normalize=True)
    assert nseqs == seqs  # (the shift never changes the search)
    S.assert_ranks([hyps for hyps, _ in want], seqs, raw, normed, log_normaliser(x, Wt), nbest, blank)
    return want


# (T, C, W, K, B): a single frame; K < C, so the blank is appended in slot K and last labels leave the candidates; K = C,
# the merge path many times; the grapheme models' classes; a long utterance with the default K; more than 512 entries per
# frame, so the radix select and the 1024-thread instantiation run; the 1000-word-piece width; 200 utterances in one call
SHAPES = [(1, 2, 1, 2, 4), (40, 6, 4, 3, 4), (64, 9, 8, 9, 3), (60, 29, 16, 8, 3), (200, 100, 16, 32, 1), (50, 70, 64, 64, 1),
          (3, 1001, 4, 64, 1), (40, 6, 4, 3, 200)]


def _seed(T, C, W, B, scale, forced):
    return 7919 * T + 31 * C + W + B + int(scale) + 1000003 * int(forced)


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("T,C,W,K,B", SHAPES, ids=lambda v: str(v))
def test_random_emissions_against_the_reference(T, C, W, K, B, scale, forced):
    seed = _seed(T, C, W, B, scale, forced)
    x = emissions(seed, B, T, C, scale)
    Wt = transitions(seed + 1, C)
    blank = C - 1 if (T + W) % 2 == 0 else seed % C  # (the module's blank is the last class; the ABI takes any)
    want = compare(x, Wt, blank, forced, W, K, min(3, W))
    if (T, C) == (64, 9):  # (the merge path is taken, many times: K = C keeps every last label a candidate)
        assert all(merges >= 19 for _, merges in want), [m for _, m in want]


@pytest.mark.parametrize("T,C,W,K,B", [(40, 6, 4, 3, 4), (64, 9, 8, 9, 3), (50, 70, 64, 64, 1)], ids=lambda v: str(v))
def test_the_forced_topology_without_transitions(T, C, W, K, B):
    x = emissions(_seed(T, C, W, B, 2.0, True), B, T, C, 1.0)
    compare(x, None, C - 1, True, W, K, min(3, W))


def test_log_normaliser_helper_is_the_references():
    x, Wt = emissions(1, 2, 5, 4, 1.0), transitions(2, 4)
    for W_ in (Wt, None):
        got = log_normaliser(x, W_)
        for b in range(2):
            assert abs(got[b] - R.normaliser(x[b], W_)) <= 1e-9


def test_without_transitions_the_optional_topology_is_the_ctc_search_bit_for_bit():
    E, _, _ = _mods()
    for (T, C, W, K, B), blank in (((60, 29, 16, 8, 3), 28), ((50, 70, 64, 64, 2), 0), ((40, 6, 4, 3, 50), 3)):
        x = emissions(900 + T, B, T, C, 1.0)
        xd = torch.from_numpy(x).cuda()
        for normalize in (False, True):
            a_h, a_s = E.transducer_beam_search(xd, None, blank, False, W, K, min(3, W), normalize=normalize)
            c_h, c_s = E.ctc_beam_search(xd, blank, W, K, min(3, W), normalize=normalize)
            assert [[s.tolist() for s in h] for h in a_h] == [[s.tolist() for s in h] for h in c_h]
            assert a_s.numpy().tobytes() == c_s.numpy().tobytes()


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_half_the_transitions_forbidden(forced):
    C = 8
    x, Wt = emissions(41, 4, 30, C, 1.0), transitions(42, C)
    mask = np.random.RandomState(44).rand(C + 1, C) < 0.5  # (37 of 72; forced: the tokens 1, 4 and 6 can leave and re-enter the blank)
    mask[0, C - 1] = mask[C, C - 1] = False  # (start -> blank and blank -> blank stay: the empty prefix lives)
    Wt[mask] = -np.inf
    want = compare(x, Wt, C - 1, forced, 16, C, 3)
    assert all(h[0][1] > NEG for h, _ in want)
    seqs, raw = device(x, Wt, C - 1, forced, 16, C, 16)
    found = 0
    for b in range(4):
        for s, v in zip(seqs[b], raw[b]):
            if v == NEG or not s:
                continue
            found += 1
            # a first token is entered from the start or the blank, a next one from the token before it or the blank
            assert not (mask[0, s[0]] and mask[1 + s[0], C - 1]), (b, s)
            if forced:
                assert all(not mask[1 + c, C - 1] for c in s[1:]), (b, s)
            else:
                assert all(not (mask[1 + c, l] and mask[1 + c, C - 1]) for l, c in zip(s, s[1:])), (b, s)
    assert found >= 16


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_scattered_nans_count_as_minus_infinity(forced):
    x, Wt = emissions(14, 4, 20, 8, 1.0), transitions(15, 8)
    rs = np.random.RandomState(15)
    x[rs.rand(*x.shape) < 0.2] = np.nan
    Wt[rs.rand(*Wt.shape) < 0.2] = np.nan
    x[:, :, 7] = np.where(np.isnan(x[:, :, 7]), 0.25, x[:, :, 7])  # (the blank stays possible: no utterance dies)
    Wt[0, 7] = 0.125
    Wt[8] = np.where(np.isnan(Wt[8]), 0.125, Wt[8])  # (and can be entered from everywhere: no token is a dead end)
    want = compare(x, Wt, 7, forced, 8, 8, 3)
    # (forced: the last frame of one utterance leaves a beam of fresh extensions, all at pb = -inf -- nothing to return)
    assert sum(h[0][1] > NEG for h, _ in want) >= (3 if forced else 4)
    y = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    Vt = np.where(np.isnan(Wt), -np.inf, Wt).astype(np.float32)
    a, b = device(x, Wt, 7, forced, 8, 8, 3), device(y, Vt, 7, forced, 8, 8, 3)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_a_frame_with_only_the_blank_finite(forced):
    x, Wt = emissions(21, 3, 20, 8, 1.0), transitions(22, 8)
    x[:, 9, :] = -np.inf
    x[:, 9, 2] = 0.5
    x[1, 0, :] = np.nan
    x[1, 0, 2] = -1.0
    compare(x, Wt, 2, forced, 8, 8, 3)
    compare(x, Wt, 2, forced, 8, 3, 3)


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_an_utterance_with_an_impossible_frame_decodes_to_nothing(forced):
    x, Wt = emissions(16, 3, 20, 8, 1.0), transitions(17, 8)
    alone = device(x[[0, 2]], Wt, 7, forced, 8, 8, 3)
    x[1, 11, :] = -np.inf
    x[1, 11, 5] = np.nan
    want = compare(x, Wt, 7, forced, 8, 8, 3)
    assert want[1][0] == [((), NEG)] * 3
    seqs, raw = device(x, Wt, 7, forced, 8, 8, 3)
    assert seqs[1] == [(), (), ()] and (raw[1] == NEG).all()
    assert [seqs[0], seqs[2]] == alone[0] and (raw[[0, 2]] == alone[1]).all()  # (its neighbours are unaffected)
    seqs, normed = device(x, Wt, 7, forced, 8, 8, 3, normalize=True)
    assert seqs[1] == [(), (), ()] and (normed[1] == NEG).all()


def test_forced_ranks_that_end_in_a_token_are_dropped_and_the_ranks_close_up():
    """the blank is forbidden behind token 0 (0 -> blank at -inf): every hypothesis ending in 0 has pb = -inf at the end"""
    C = 4
    x, Wt = emissions(23, 4, 6, C, 1.0), transitions(24, C)
    Wt[1 + 3][0] = -np.inf
    want = compare(x, Wt, 3, True, 64, C, 64)
    seqs, raw = device(x, Wt, 3, True, 64, C, 64)
    for b in range(4):
        live = [s for s, v in zip(seqs[b], raw[b]) if v > NEG]
        assert live and all(not s or s[-1] != 0 for s in live)
        n = len(live)
        assert (raw[b, :n] > NEG).all() and (raw[b, n:] == NEG).all() and all(s == () for s in seqs[b][n:])
        assert (np.diff(raw[b, :n]) <= 0).all()
    assert any(v == NEG for h, _ in want for _, v in h)


def test_the_same_call_twice_is_bit_identical():
    x, Wt = emissions(19, 8, 60, 30, 1.0), transitions(20, 30)
    for forced in (False, True):
        a = device(x, Wt, 29, forced, 64, 30, 3, normalize=True)
        b = device(x, Wt, 29, forced, 64, 30, 3, normalize=True)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
KINDS = [dict(blank="optional", allow_repeats=False), dict(blank="forced")]


def _criterion(tokens, g2i, ngram, kw, seed):
    _, _, TR = _mods()
    crit = TR.Transducer(tokens, g2i, ngram=ngram, **kw).cuda()
    params = None
    if ngram > 0:
        params = (0.5 * np.random.RandomState(seed).randn(crit.transition_params.numel())).astype(np.float32)
        with torch.no_grad():
            crit.transition_params.copy_(torch.from_numpy(params))
    return crit, params


def _operands(x, params, ngram):
    """(emissions, Wt or None) as the criterion's routes form them (_unigram_route, _bigram_dense_operands), float32"""
    C = x.shape[2]
    if ngram == 0:
        return x, None
    if ngram == 1:
        return x + params, None
    n1 = C + C * C
    Wt = np.ascontiguousarray(np.concatenate([params[:C].reshape(1, C), params[C:n1].reshape(C, C).T], axis=0))
    xd = x.copy()
    xd[:, -1] += params[n1 + 1:]
    return xd, Wt


def _minus_loss(crit, xd, b, seq):
    """minus the criterion's loss of `seq` for utterance b, on the device (a batch of one: no batch mean in between)"""
    with torch.no_grad():
        return -float(crit(xd[b:b + 1], [list(seq)]).reshape(-1)[0])


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_module_with_single_grapheme_tokens(ngram, kw):
    forced = kw["blank"] == "forced"
    tokens, g2i = ["a", "b"], {"a": 0, "b": 1}
    crit, params = _criterion(tokens, g2i, ngram, kw, 300 + ngram)
    C, blank = 3, 2
    # nothing is pruned (W = 64, K = C, T <= 5: tests/test_transducer_beam_abi.py): the score is minus the loss
    for T, scale in ((1, 1.0), (3, 1.0), (4, 3.0), (5, 1.0)):
        B = 3
        x = emissions(310 + 10 * T + ngram + int(forced), B, T, C, scale)
        xe, Wt = _operands(x, params, ngram)
        want = reference(xe, Wt, blank, forced, 64, C, 4)
        xd = torch.from_numpy(x).cuda()
        hyps, scores = crit.beam_search(xd, beam_size=64, classes_per_frame=C, nbest=4, return_scores=True)
        assert scores.dtype == torch.float64 and tuple(scores.shape) == (B, 4) and not scores.is_cuda
        logz = log_normaliser(xe, Wt)
        for b in range(B):
            assert all(p.dtype == torch.int32 and not p.is_cuda and p.dim() == 1 for p in hyps[b])
            assert [tuple(p.tolist()) for p in hyps[b]] == [h for h, _ in want[b][0]], (T, b)
            for r, (seq, s) in enumerate(want[b][0]):
                got = float(scores[b, r])
                if s == NEG:
                    assert got == NEG
                    continue
                n = s - logz[b]
                assert S.normalised_close(got, n), (T, b, r, got, n)
                if seq:
                    loss = _minus_loss(crit, xd, b, seq)
                    assert abs(got - loss) <= 1e-4 * abs(loss) + 2e-5, (T, b, r, seq, got, loss)
    # the beam prunes (T = 40, W = 4, K = 3 of 3 classes with W = 4): a lower bound
    B, T = 4, 40
    x = emissions(350 + ngram + int(forced), B, T, C, 1.0)
    xe, Wt = _operands(x, params, ngram)
    want = reference(xe, Wt, blank, forced, 4, 3, 1)
    xd = torch.from_numpy(x).cuda()
    hyps, scores = crit.beam_search(xd, beam_size=4, classes_per_frame=3, return_scores=True)
    assert [tuple(p.tolist()) for p in hyps] == [h[0][0] for h, _ in want]
    for b in range(B):
        assert len(hyps[b]) > 0
        loss = _minus_loss(crit, xd, b, hyps[b].tolist())
        assert float(scores[b, 0]) <= loss + 1e-4 * abs(loss) + 2e-5, (b, float(scores[b, 0]), loss)
    # other floating dtypes are converted, tensors that are not on a GPU are uploaded: the same search
    for other in (torch.from_numpy(x), xd.double()):
        again = crit.beam_search(other, beam_size=4, classes_per_frame=3)
        assert [p.tolist() for p in again] == [p.tolist() for p in hyps]


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 2])
def test_module_with_word_piece_tokens_gives_a_lower_bound_of_minus_the_loss(ngram, kw):
    """the loss sums over every decomposition of the target's graphemes into tokens, the search scores one"""
    forced = kw["blank"] == "forced"
    tokens, g2i = ["a", "b", "ab", "ba", "bab"], {"a": 0, "b": 1}
    crit, params = _criterion(tokens, g2i, ngram, kw, 400 + ngram)
    C, blank, B, T = 6, 5, 4, 12
    x = emissions(410 + ngram + int(forced), B, T, C, 1.0)
    xe, Wt = _operands(x, params, ngram)
    want = reference(xe, Wt, blank, forced, 16, C, 3)
    xd = torch.from_numpy(x).cuda()
    hyps, scores = crit.beam_search(xd, beam_size=16, classes_per_frame=C, nbest=3, return_scores=True)
    strict = 0
    for b in range(B):
        assert [tuple(p.tolist()) for p in hyps[b]] == [h for h, _ in want[b][0]]
        for r in range(3):
            seq = hyps[b][r].tolist()
            got = float(scores[b, r])
            if got == NEG or not seq:
                continue
            graphemes = [g2i[ch] for v in seq for ch in tokens[v]]
            loss = _minus_loss(crit, xd, b, graphemes)
            assert got <= loss + 1e-4 * abs(loss) + 2e-5, (b, r, seq, got, loss)
            strict += got < loss - 1e-3
    assert strict > 0  # (some target here has more than one decomposition)


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_errors_with_a_beam_count_what_beam_search_predicts(ngram, kw):
    _, M, _ = _mods()
    tokens = ["a", "b", "c", "d", "e"]
    crit, _ = _criterion(tokens, {t: i for i, t in enumerate(tokens)}, ngram, kw, 500 + ngram)
    B, T, C = 4, 50, 6
    xd = torch.from_numpy(emissions(510 + ngram, B, T, C, 1.0)).cuda()
    rs = np.random.RandomState(62)
    targets = [rs.randint(0, 5, size=n).tolist() for n in (7, 1, 12, 3)]
    counter = M.ErrorCounter(wordsep=3)
    for W, K in ((1, C), (16, 4)):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K)
        assert any(p.numel() > 0 for p in pred)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K) == counter(pred, targets)
    assert crit.errors(xd, targets, counter) == counter(crit.viterbi(xd), targets)  # (the positional call is what it was)
