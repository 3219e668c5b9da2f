"""ASG prefix beam search with a token-level n-gram LM on the device (csrc/beam_kernels.hip: wfl_asg_beam_search_lm behind
engine.asg_beam_search_lm, ASG.beam_search(token_lm=) and ASG.errors(beam_size=, token_lm=))
against its restatement in plain Python (tests/asg_beam_lm_reference.py, itself pinned to an enumeration of all frame
paths in tests/test_asg_beam_lm_abi.py).

Acceptance of every comparison (beam_support.assert_ranks): the raw class sequences of all returned ranks are equal;
unnormalised scores agree to 1e-9 max(1, |s|); normalised scores agree at the project's loss bar, the device's
denominator logz being float32.  The seeds are fixed so that every utterance's smallest selection margin in the
restatement is at least 1e-9, and every comparison asserts that: no utterance is left out."""
import math

import numpy as np
import pytest
import torch

import asg_beam_lexicon_reference as AX
import asg_beam_lm_reference as AL
import asg_beam_reference as AR
import beam_lm_reference as LR
import beam_support as S
from beam_support import emissions, transitions
from test_asg_beam_lm_abi import BOUND_SEEDS, bound_case

pytestmark = pytest.mark.gpu

NEG = AR.NEG
ALPHA, BETA = 0.8, 0.5
# (R, garbage): no replabel without and with the garbage, one and two replabels with it, three without
ALPHABETS = [(0, False), (0, True), (1, True), (2, True), (3, False)]


def _mods():
    return S.package("engine", "metrics", "criterions.asg", "lm:NGramLM")


def universe(C, R, garbage):
    """(the garbage class or None, the number of tokens) of C raw classes"""
    return (C - 1 if garbage else None), C - R - int(garbage)


def trigram(seed, N):
    """ARPA text of a seeded trigram over N tokens that knows every unigram; the higher grams thin out as N grows"""
    return LR.random_arpa(np.random.RandomState(seed), S.tokens_of(N + 1), 3, min(0.5, 6.0 / N))


def lms(tmp_path, seed, N):
    """(the device's LM through the loader, the restatement's reading of the same text) over N tokens: (N + 1, N)"""
    return S.token_lms(tmp_path, trigram(seed, N), N + 1, N)


def without_token(whole, text, N, gone):
    """(the device's LM, the restatement's) of `whole` / `text` with every arc of token `gone` taken out: the pack is
    constructed directly (the loader would refuse a token without a unigram), the restatement reads the text without
    the lines that name the token (it does not count its sections)"""
    NGramLM = _mods()[3]
    keep = whole.arc_label != gone
    ptr = np.concatenate([[0], np.cumsum([keep[whole.arc_ptr[s]:whole.arc_ptr[s + 1]].sum() for s in range(whole.num_states)])])
    lm = NGramLM(N + 1, N, ptr, whole.arc_label[keep], whole.arc_next[keep], whole.arc_w[keep], whole.bo_next, whole.bo_w,
                 start=whole.start, order=whole.order)
    word = S.tokens_of(N + 1)[gone]
    cut = "\n".join(l for l in text.split("\n") if word not in l.split())
    return lm, LR.ArpaLM(cut, S.tokens_of(N + 1), N)


def reference(x, Wt, W, K, nbest, ref_lm, garbage, R, eos=True, alpha=ALPHA, beta=BETA):
    """per utterance (hyps, merges); asserts the margins, so that no utterance is left out of a comparison"""
    found = S.margins_ok(lambda b: AL.beam_search(x[b], Wt, W, K, nbest, ref_lm, alpha, beta, eos, garbage, R), x.shape[0])
    return [(hyps, merges) for hyps, _, merges in found]


def device(x, Wt, W, K, nbest, lm, garbage, R, eos=True, normalize=False, drop=None, num_replabels=0, alpha=ALPHA, beta=BETA):
    E = _mods()[0]
    xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
    hyps, scores = E.asg_beam_search_lm(xd, Wd, lm, garbage, R, W, K, nbest, normalize=normalize, drop=drop,
                                        num_replabels=num_replabels, lm_weight=alpha, length_bonus=beta, lm_eos=eos)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def plain(x, Wt, W, K, nbest, **kw):
    E = _mods()[0]
    hyps, scores = E.asg_beam_search(torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda(), W, K, nbest, normalize=False, **kw)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, Wt, W, K, nbest, lm, ref_lm, garbage, R, eos=True, alpha=ALPHA, beta=BETA):
    want = reference(x, Wt, W, K, nbest, ref_lm, garbage, R, eos, alpha, beta)
    seqs, raw = device(x, Wt, W, K, nbest, lm, garbage, R, eos, alpha=alpha, beta=beta)
    nseqs, normed = device(x, Wt, W, K, nbest, lm, garbage, R, eos, normalize=True, alpha=alpha, beta=beta)
    assert nseqs == seqs  # (the shift never changes the search)
    S.assert_ranks([hyps for hyps, _ in want], seqs, raw, normed, S.log_normaliser(x, Wt), nbest)
    return want, seqs, raw


# (T, C, W, K, B, the alphabets): a single frame; K < C, so last labels leave the candidates and stand-in extensions bound
# the frame -- every alphabet, and once 200 utterances in one call; a middle shape, every alphabet; the training shape's
# classes = ASG(97 tokens, 2 replabels, garbage) over a long utterance with the default K; more than 512 entries per
# frame, so the radix select and the 1024-thread instantiation run
SHAPES = [(1, 3, 1, 2, 4, [(0, False), (0, True), (1, True)]), (12, 6, 4, 3, 4, ALPHABETS), (30, 12, 16, 8, 2, ALPHABETS),
          (300, 100, 16, 32, 1, [(2, True)]), (50, 70, 64, 64, 1, [(1, True), (3, False)]), (12, 6, 4, 3, 200, [(1, True)])]
CASES = [(T, C, W, K, B, R, g) for T, C, W, K, B, alphabets in SHAPES for R, g in alphabets]


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("T,C,W,K,B,R,garbage", CASES, ids=lambda v: str(v))
def test_random_emissions_against_the_reference(tmp_path, T, C, W, K, B, R, garbage, scale):
    seed = 7919 * T + 31 * C + W + B + 5 * R + int(garbage) + int(scale)
    G, N = universe(C, R, garbage)
    x, Wt = emissions(seed, B, T, C, scale), transitions(seed + 1, C)
    lm, ref_lm = lms(tmp_path, seed + 2, N)
    eos = bool((T + R + int(scale)) % 2)  # (both settings over the cases)
    want, seqs, _ = compare(x, Wt, W, K, min(3, W), lm, ref_lm, G, R, eos=eos)
    if (T, C) == (50, 70):  # (the merge path is taken, many times: K near C keeps last labels candidates)
        assert all(merges >= 19 for _, merges in want), [m for _, m in want]
    if R and (T >= 50 or B == 200):  # (replabels are decoded behind tokens: the LM's steps by a repeated token are exercised)
        repeats = sum(1 for h in seqs for s in h for a, b in zip(s, s[1:]) if b < R and a >= R and a != G)
        assert repeats >= 1


@pytest.mark.parametrize("eos", [True, False])
@pytest.mark.parametrize("R,garbage", ALPHABETS)
def test_an_lm_without_a_token_never_returns_it(tmp_path, R, garbage, eos):
    """token 1 has no arc anywhere: an extension that emits it does not exist -- as the raw class 1 + R, and as a
    replabel behind it, which is why that class is never in a result at all"""
    T, C, W, K, B, gone = 20, 8, 8, 5, 4, 1
    G, N = universe(C, R, garbage)
    seed = 300 + 10 * R + int(garbage)
    x, Wt = emissions(seed, B, T, C, 1.0), transitions(seed + 1, C)
    x[:, :, gone + R] += 1.5  # (the emissions favour it)
    text = trigram(seed + 2, N)
    whole, _ = S.token_lms(tmp_path, text, N + 1, N)
    assert any(gone + R in s for h in device(x, Wt, W, K, 3, whole, G, R, eos)[0] for s in h)  # (with its arcs it is returned)
    lm, ref_lm = without_token(whole, text, N, gone)
    assert lm.num_arcs < whole.num_arcs and lm.score([gone]) == -math.inf
    _, seqs, raw = compare(x, Wt, W, K, 3, lm, ref_lm, G, R, eos=eos)
    assert not any(gone + R in s for h in seqs for s in h)
    assert all(raw[b, 0] > NEG and len(seqs[b][0]) > 0 for b in range(B))


@pytest.mark.parametrize("seed", BOUND_SEEDS)
def test_the_bound_counts_only_entries_that_exist(tmp_path, seed):
    """tests/test_asg_beam_lm_abi.py's cases on the device: a bound that took the absent stand-in extension for an entry
    would cut entries that survive, and the ranks would differ"""
    x, Wt, C, R, garbage, text, hits = bound_case(seed)
    assert hits
    N = C - R - 1
    full = LR.random_arpa(np.random.RandomState(77), S.tokens_of(N + 1), 2, 0.5)  # (the case's LM before token 2 is cut)
    lm, ref_lm = without_token(S.token_lms(tmp_path, full, N + 1, N)[0], full, N, 2)
    assert ref_lm.grams == LR.ArpaLM(text, S.tokens_of(N + 1), N).grams
    _, _, raw = compare(x[None], Wt, 4, 2, 3, lm, ref_lm, garbage, R)
    assert raw[0, 0] > NEG


def test_scattered_nans_count_as_minus_infinity(tmp_path):
    x, Wt = emissions(14, 4, 20, 8, 1.0), transitions(15, 8)
    rs = np.random.RandomState(15)
    x[rs.rand(*x.shape) < 0.2] = np.nan
    assert np.isfinite(x).any(axis=2).all()
    lm, ref_lm = lms(tmp_path, 16, 5)
    compare(x, Wt, 8, 8, 3, lm, ref_lm, 7, 2)
    y = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    assert device(x, Wt, 8, 8, 3, lm, 7, 2)[0] == device(y, Wt, 8, 8, 3, lm, 7, 2)[0]


def test_half_the_classes_impossible(tmp_path):
    x, Wt = emissions(11, 4, 20, 8, 1.0), transitions(12, 8)
    rs = np.random.RandomState(12)
    for b in range(4):
        for t in range(20):
            x[b, t, rs.permutation(8)[:4]] = -np.inf
    lm, ref_lm = lms(tmp_path, 13, 6)
    compare(x, Wt, 8, 8, 3, lm, ref_lm, 7, 1)
    compare(x, Wt, 8, 5, 3, lm, ref_lm, 7, 1, eos=False)


def test_forbidden_transitions_never_appear_in_a_result(tmp_path):
    C = 8
    x, Wt = emissions(41, 4, 30, C, 1.0), transitions(42, C)
    rs = np.random.RandomState(43)
    mask = rs.rand(C + 1, C) < 0.3
    mask[1:][np.eye(C, dtype=bool)] = False  # (the self transitions stay: every class can last)
    mask[0, :2] = False
    Wt[mask] = -np.inf
    Wt[0, 7] = np.nan  # (a NaN counts as -inf)
    lm, ref_lm = lms(tmp_path, 44, 5)
    want, _, _ = compare(x, Wt, 16, C, 3, lm, ref_lm, 7, 2)
    seqs, raw = device(x, Wt, 16, C, 16, lm, 7, 2)
    found = 0
    for b in range(4):
        for s, v in zip(seqs[b], raw[b]):
            if v == NEG:
                continue
            found += 1
            assert not mask[0, s[0]] and s[0] != 7, (b, s)
            assert all(not mask[1 + c, l] for l, c in zip(s, s[1:])), (b, s)
    assert found >= 32 and all(h[0][1] > NEG for h, _ in want)


def test_an_utterance_with_an_impossible_frame_decodes_to_nothing(tmp_path):
    x, Wt = emissions(16, 3, 20, 8, 1.0), transitions(17, 8)
    lm, ref_lm = lms(tmp_path, 18, 6)
    alone = device(x[[0, 2]], Wt, 8, 8, 3, lm, 7, 1)
    x[1, 11, :] = -np.inf
    x[1, 11, 5] = np.nan
    want, seqs, raw = compare(x, Wt, 8, 8, 3, lm, ref_lm, 7, 1)
    assert want[1][0] == [((), NEG)] * 3
    assert seqs[1] == [(), (), ()] and (raw[1] == NEG).all()
    assert [seqs[0], seqs[2]] == alone[0] and (raw[[0, 2]] == alone[1]).all()  # (its neighbours are unaffected)
    # the same through the mapping of the results, and with normalised scores
    seqs, normed = device(x, Wt, 8, 8, 3, lm, 7, 1, normalize=True, drop=7, num_replabels=1)
    assert seqs[1] == [(), (), ()] and (normed[1] == NEG).all()


def test_exact_ties_follow_the_tie_rule(tmp_path):
    """x and Wt all zero, two frames, C = 70 = 68 tokens + a replabel + the garbage, W = K = 64.  With the LM's weight and
    the bonus at 0 every entry of frame 1 ties at 0 for the 64 places, as in the search without an LM: the order is the
    tie rule's alone (the full ranking decides, not the selection by key).  With a bonus alone, an entry is worth the
    number of tokens it spells, and the ties are among entries that spell as many."""
    x, Wt = np.zeros((2, 2, 70), np.float32), np.zeros((71, 70), np.float32)
    lm, ref_lm = lms(tmp_path, 21, 68)
    hyps, margin, _ = AL.beam_search(x[0], Wt, 64, 64, 64, ref_lm, 0.0, 0.0, False, 69, 1)
    assert margin == 0.0 and hyps == [((c,), 0.0) for c in range(64)]
    seqs, raw = device(x, Wt, 64, 64, 64, lm, 69, 1, eos=False, alpha=0.0, beta=0.0)
    for b in range(2):
        assert seqs[b] == [h for h, _ in hyps] and (raw[b] == 0.0).all()
    hyps, margin, _ = AL.beam_search(x[0], Wt, 64, 64, 64, ref_lm, 0.0, 0.25, False, 69, 1)
    assert margin == 0.0 and hyps[0][1] == 0.5 and hyps[-1][1] == 0.5  # (two tokens, or a token and the replabel behind it)
    assert any(s[1] == 0 for s, _ in hyps)
    seqs, raw = device(x, Wt, 64, 64, 64, lm, 69, 1, eos=False, alpha=0.0, beta=0.25)
    for b in range(2):
        assert seqs[b] == [h for h, _ in hyps] and (raw[b] == 0.5).all()
    # one frame, a beam narrower than K: the new entries tie among themselves and the lower candidate position wins
    seqs, raw = device(np.ascontiguousarray(x[:, :1]), Wt, 5, 64, 5, lm, 69, 1, eos=False, alpha=0.0, beta=0.0)
    assert seqs[0] == seqs[1] == [(c,) for c in range(5)] and (raw == 0.0).all()


def test_the_same_call_twice_is_bit_identical(tmp_path):
    x, Wt = emissions(19, 8, 60, 30, 1.0), transitions(20, 30)
    lm, _ = lms(tmp_path, 22, 27)
    a = device(x, Wt, 64, 30, 3, lm, 29, 2, normalize=True)
    b = device(x, Wt, 64, 30, 3, lm, 29, 2, normalize=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    c = device(x, Wt, 64, 30, 3, lm, 29, 2, normalize=True, drop=29, num_replabels=2)
    d = device(x, Wt, 64, 30, 3, lm, 29, 2, normalize=True, drop=29, num_replabels=2)
    assert c[0] == d[0] and c[1].tobytes() == a[1].tobytes() == d[1].tobytes()  # (the mapping never touches the scores)
    assert [[tuple(AR.unpack(s, 29, 2)) for s in h] for h in a[0]] == c[0]


# ------------------------------------------------------------------------------------------------------------------
# what the LM reads, the LM switched off, the module
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eos", [True, False])
def test_the_lm_reads_what_the_write_launch_writes(tmp_path, eos):
    """(T, C, W, K) = (4, 4, 64, 4) with r0 = 0, a = 1, b = 2, G = 3 and enough transitions forbidden that at most 64 raw
    sequences have a finite mass: nothing is pruned, with or without the LM.  Then for every returned rank the LM call's
    score minus the plain search's score of the same raw sequence is a lm.score(mapped) + b len(mapped), `mapped` the
    device's own mapped output of that rank."""
    T, C, R, G, B = 4, 4, 1, 3, 6
    x, Wt = emissions(501, B, T, C, 1.0), transitions(502, C)
    Wt[1 + 2, 1] = Wt[1 + 1, 2] = Wt[1 + 0, 2] = Wt[1 + 3, 0] = Wt[0, 3] = -np.inf  # a -> b, b -> a, b -> r0, r0 -> G, start -> G
    lm, ref_lm = lms(tmp_path, 503, 2)
    finite = [[seq for seq, mass in AR.brute_force(x[b], Wt) if mass > NEG] for b in range(B)]
    assert all(20 <= len(f) <= 64 for f in finite), [len(f) for f in finite]
    seqs, raw = device(x, Wt, 64, 4, 64, lm, G, R, eos)
    mapped, again = device(x, Wt, 64, 4, 64, lm, G, R, eos, drop=G, num_replabels=R)
    assert (again == raw).all()
    pseqs, praw = plain(x, Wt, 64, 4, 64)
    repeated = 0
    for b in range(B):
        ranks = [r for r in range(64) if raw[b, r] > NEG]
        assert len(ranks) == len(finite[b]) and sorted(seqs[b][r] for r in ranks) == sorted(finite[b])
        mass = {s: v for s, v in zip(pseqs[b], praw[b]) if v > NEG}
        assert sorted(mass) == sorted(finite[b])
        for r in ranks:
            m = list(mapped[b][r])
            term = ALPHA * ref_lm.score(m, eos=eos) + BETA * len(m)
            assert abs((raw[b, r] - mass[seqs[b][r]]) - term) <= 1e-9, (b, r, seqs[b][r], m)
            assert abs(ALPHA * lm.score(m, eos=eos) + BETA * len(m) - term) <= 1e-9
            repeated += int(len(m) > sum(1 for c in seqs[b][r] if c != G and c >= R))
    assert repeated >= 20  # (replabels behind tokens among them: the mapped output is longer than the tokens of the raw one)


def test_lm_off_inside_the_lm_path_is_the_plain_asg_search(tmp_path):
    """lm_weight = 0, length_bonus = 0, no </s> and an LM that knows every token: every LM term is 0, so the sequences are
    wfl_asg_beam_search's and the raw scores agree to 1e-9"""
    for (T, C, W, K, B), (R, garbage) in (((40, 6, 4, 3, 4), (1, True)), ((30, 29, 16, 8, 3), (2, True)), ((50, 70, 64, 64, 1), (3, False)),
                                           ((20, 5, 8, 5, 3), (0, True))):
        G, N = universe(C, R, garbage)
        x, Wt = emissions(40 + C, B, T, C, 1.0), transitions(41 + C, C)
        lm, _ = lms(tmp_path, 42 + C, N)
        nbest = min(3, W)
        seqs, raw = device(x, Wt, W, K, nbest, lm, G, R, eos=False, alpha=0.0, beta=0.0)
        pseqs, praw = plain(x, Wt, W, K, nbest)
        assert seqs == pseqs
        assert all(S.raw_close(raw[b, r], praw[b, r]) for b in range(B) for r in range(nbest))
        assert (raw[:, 0] > NEG).all()


def spelling_case(R, garbage, seed=900):
    """(criterion arguments, x, ARPA text): emissions that spell token sequences in raw classes (doubled letters as
    replabels, the garbage between some classes), weakly enough that a second reading is in reach, and a seeded trigram
    over the five tokens with strong preferences"""
    N, B, T = 5, 6, 40
    C = N + R + int(garbage)
    G = C - 1 if garbage else None
    rs = np.random.RandomState(seed)
    words = [[int(t) for t in rs.randint(0, N, size=n)] for n in (2, 3, 3, 4, 2, 3)]
    spellings = {}
    for v, w in enumerate(words):
        spellings.setdefault(next(iter(AX.raw_lexicon([w], R))), v)
    x = S.spelled_asg(seed + 1, B, T, C, spellings, G, hi=2.5)
    return N, C, G, x, LR.random_arpa(np.random.RandomState(seed + 2), S.tokens_of(N + 1), 3, 0.5)


@pytest.mark.parametrize("num_replabels,use_garbage", [(1, True), (2, True), (1, False), (2, False)])
def test_module_returns_the_mapped_results_and_counts_them(tmp_path, num_replabels, use_garbage):
    E, M, asg, _ = _mods()
    N, C, G, x, text = spelling_case(num_replabels, use_garbage)
    crit = asg.ASG(N, num_replabels=num_replabels, use_garbage=use_garbage).cuda()
    assert crit.N == C and crit.garbage_idx == G
    Wt = transitions(61 + num_replabels, C)
    with torch.no_grad():
        crit.transitions.copy_(torch.from_numpy(Wt))
    p = tmp_path / "tokens.arpa"
    p.write_text(text)
    lm = crit.token_lm(str(p), S.tokens_of(N + 1))
    ref_lm = LR.ArpaLM(text, S.tokens_of(N + 1), N)
    xd = torch.from_numpy(x).cuda()
    B = x.shape[0]
    kw = dict(token_lm=lm, lm_weight=2.0, length_bonus=BETA)
    best = crit.beam_search(xd, **kw)
    assert isinstance(best, list) and len(best) == B and all(p.dtype == torch.int64 and p.dim() == 1 and not p.is_cuda for p in best)
    want = reference(x, Wt, 16, min(C, 32), 1, ref_lm, G, num_replabels, alpha=2.0)
    assert [p.tolist() for p in best] == [AR.unpack(h[0][0], G, num_replabels) for h, _ in want]
    raw, _ = device(x, Wt, 16, min(C, 32), 1, lm, G, num_replabels, alpha=2.0)
    assert [[h[0][0]] for h, _ in want] == raw
    # the LM changes what is decoded: it prefers another continuation than the emissions alone
    assert [p.tolist() for p in best] != [p.tolist() for p in crit.beam_search(xd)]
    # n-best lists with scores: the engine's normalised scores, the mapped sequences
    hyps, scores = crit.beam_search(xd, beam_size=8, classes_per_frame=4, nbest=3, return_scores=True, lm_eos=False, **kw)
    assert len(hyps) == B and all(isinstance(h, list) and len(h) == 3 for h in hyps)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (B, 3) and not scores.is_cuda
    raw, normed = device(x, Wt, 8, 4, 3, lm, G, num_replabels, eos=False, normalize=True, alpha=2.0)
    assert (scores.numpy() == normed).all()
    for b in range(B):
        assert [p.tolist() for p in hyps[b]] == [AR.unpack(s, G, num_replabels) for s in raw[b]]
    # other floating dtypes are converted, tensors that are not on a GPU are uploaded: the same search
    for other in (torch.from_numpy(x), xd.double()):
        again = crit.beam_search(other, beam_size=8, classes_per_frame=4, nbest=3, lm_eos=False, **kw)
        assert [[p.tolist() for p in h] for h in again] == [[p.tolist() for p in h] for h in hyps]
    # errors(beam_size=, token_lm=) counts what beam_search predicts; without token_lm the call is what it was
    rs = np.random.RandomState(62)
    targets = [rs.randint(0, N, size=n).tolist() for n in (7, 0, 12, 3, 5, 9)]
    counter = M.ErrorCounter(wordsep=3)
    for W, K in ((1, C), (16, 4)):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K, **kw)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K, **kw) == counter(pred, targets)
    assert crit.errors(xd, targets, counter, beam_size=4) == counter(crit.beam_search(xd, beam_size=4), targets)
