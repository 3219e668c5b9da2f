"""The Transducer beam search that merges hypotheses by spelling, on the device (csrc/beam_kernels.hip:
wfl_transducer_beam_search_merged behind engine.transducer_beam_search(spelling=), Transducer.beam_search(merge_spellings=True)
and Transducer.errors(beam_size=, merge_spellings=True)) against its restatement in plain Python
(tests/transducer_merged_beam_reference.py, itself pinned to an enumeration of all frame paths grouped by spelling and
to the oracle's loss in tests/test_transducer_merged_beam_abi.py).

Acceptance of every comparison, for all returned ranks: the representative token sequences are equal; unnormalised
scores agree to 1e-9 max(1, |s|) -- both sides are float64 and differ in libm rounding only; normalised scores agree at
the project's loss bar (1e-4 |want| + 2e-5, as tests/test_gpu_transducer_beam_search.py), against a float64 normaliser.
An utterance whose smallest selection margin in the reference is below 1e-9 could legitimately come out differently: it
is left out, and at most 2 % of a case's utterances may be (the seeds are fixed, and the reference alone meets this with
them: checked without a device)."""
import os

import numpy as np
import pytest
import torch

import beam_support as BS
import transducer_beam_reference as R
import transducer_merged_beam_reference as MR
from test_gpu_transducer_beam_search import _criterion, _minus_loss, _operands, emissions, log_normaliser, transitions

pytestmark = pytest.mark.gpu

MARGIN = BS.MARGIN
NEG = R.NEG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = [[0], [1], [0, 1]]
AAA = [[0], [0, 0], [0, 0, 0]]
ABBA = [[0], [1], [0, 1], [1, 0]]
ABC = [[0], [1], [2], [0, 1], [1, 2], [0, 1, 2]]


def _mods():
    return BS.package("engine", "metrics", "criterions.transducer")


def with_blank(spell, blank):
    return spell[:blank] + [None] + spell[blank:]


def overlapping_pieces():
    """69 tokens over six graphemes: the six single graphemes, the 15 pairs and the first 48 triples that start in the
    first three graphemes and never repeat a grapheme at once -- many token sequences share a spelling"""
    out = [[g] for g in range(6)]
    out += [[a, b] for a in range(3) for b in range(6) if a != b]
    out += [[a, b, c] for a in range(3) for b in range(6) for c in range(6) if a != b and b != c][:48]
    assert len(out) == 69
    return out


def benchmark_pieces():
    with open(os.path.join(ROOT, "benchmarks", "word_pieces_tokens_1000.txt")) as f:
        tokens = sorted(l.strip() for l in f)
    g2i = {g: i for i, g in enumerate(sorted(set(c for t in tokens for c in t)))}
    return tokens, g2i, [[g2i[c] for c in t] for t in tokens]


def reference(x, Wt, blank, forced, spell, W, K, nbest):
    """per utterance (hyps, new merges, stay merges, pruned), or None for an utterance whose margin is below MARGIN; at
    most 2 % of the utterances may be"""
    out = []
    for b in range(x.shape[0]):
        hyps, margin, new_merges, stay_merges, pruned = MR.merged_beam_search(x[b], Wt, blank, forced, spell, W, K, nbest)
        out.append((hyps, new_merges, stay_merges, pruned) if margin >= MARGIN else None)
    left_out = sum(w is None for w in out)
    assert left_out <= 0.02 * len(out), (left_out, len(out))
    return out


def device(x, Wt, blank, forced, spell, W, K, nbest, normalize=False):
    E, _, _ = _mods()
    table = spell if isinstance(spell, E.Spelling) else E.Spelling.checked(spell, blank)
    xd = torch.from_numpy(x).cuda()
    Wd = None if Wt is None else torch.from_numpy(Wt).cuda()
    hyps, scores = E.transducer_beam_search(xd, Wd, blank, forced, W, K, nbest, normalize=normalize, spelling=table)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, Wt, blank, forced, spell, W, K, nbest):
    want = reference(x, Wt, blank, forced, spell, W, K, nbest)
    seqs, raw = device(x, Wt, blank, forced, spell, W, K, nbest)
    nseqs, normed = device(x, Wt, blank, forced, spell, W, K, nbest, normalize=True)
    assert nseqs == seqs  # (the shift never changes the search)
    table = [tuple(s) if s is not None else () for s in spell]
    for b in range(x.shape[0]):
        live = [MR.spelt(table, s) for s, v in zip(seqs[b], raw[b]) if v > NEG]
        assert len(set(live)) == len(live), (b, seqs[b])  # no two ranks spell the same graphemes
    pairs = [None if w is None else [(rho, s) for rho, _, s in w[0]] for w in want]  # (None: left out, but for the blank)
    BS.assert_ranks(pairs, seqs, raw, normed, log_normaliser(x, Wt), nbest, blank)
    return want


# ------------------------------------------------------------------------------------------------------------------
# the shapes at which nothing is pruned, as a batch
# ------------------------------------------------------------------------------------------------------------------
UNPRUNED = [(AB, 3, (False, True)), (AB, 4, (False, True)), (AB, 5, (True,)), (AAA, 5, (False, True)), (AAA, 6, (False, True)),
            (ABBA, 4, (True,)), (ABC, 3, (True,)), (ABC, 4, (True,))]


@pytest.mark.parametrize("with_Wt", [False, True], ids=["plain", "Wt"])
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("case", range(len(UNPRUNED)))
def test_the_unpruned_shapes_against_the_reference(case, scale, with_Wt):
    spell, T, topologies = UNPRUNED[case]
    C, B = len(spell) + 1, 6
    for forced in topologies:
        for blank in (C - 1, 1):
            seed = 1000 * case + 100 * int(scale) + 10 * int(forced) + 2 * int(with_Wt) + int(blank == 1)
            x = emissions(seed, B, T, C, scale)
            Wt = transitions(seed + 1, C) if with_Wt else None
            want = compare(x, Wt, blank, forced, with_blank(spell, blank), 64, C, 64)
            assert all(w is None or not w[3] for w in want)  # nothing pruned


# (T, tokens, W, K, B): heavy merging under pruning; more than 512 entries per frame, so the radix select and the
# 1024-thread instantiation run, over pieces whose spellings overlap; 200 utterances in one call
def _pruned_case(name):
    if name == "aaa":
        return 30, AAA, 4, 3, 8
    if name == "overlap":
        return 50, overlapping_pieces(), 64, 64, 1
    return 5, AB, 4, 4, 200


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("name", ["aaa", "overlap", "many"])
def test_pruned_searches_against_the_reference(name, scale, forced):
    T, spell, W, K, B = _pruned_case(name)
    C = len(spell) + 1
    seed = {"aaa": 11, "overlap": 22, "many": 33}[name] * 1000 + 10 * int(scale) + int(forced)
    x = emissions(seed, B, T, C, scale)
    Wt = transitions(seed + 1, C)
    blank = C - 1 if name != "many" else 2
    want = compare(x, Wt, blank, forced, with_blank(spell, blank), W, K, min(3, W))
    kept = [w for w in want if w is not None]
    assert all(w[3] for w in kept) or name == "many"
    if name == "aaa":
        assert sum(w[1] for w in kept) >= 20 and sum(w[2] for w in kept) >= 20  # new-entry merges, merges into stays
    if name == "overlap":  # (white noise: hypotheses of one spelling seldom share the optional topology's beam)
        assert kept and kept[0][1] + kept[0][2] >= 30 and (kept[0][1] >= 100 or not forced)


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_the_benchmark_word_pieces(forced):
    _, _, spell = benchmark_pieces()
    C = len(spell) + 1
    assert C == 1001
    x = emissions(77 + int(forced), 1, 3, C, 1.0)
    compare(x, transitions(78, C), C - 1, forced, spell + [None], 4, 64, 3)
    compare(x, None, C - 1, forced, spell + [None], 4, 64, 3)


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_a_token_of_exactly_the_longest_spelling(forced):
    # token 2 spells 64 graphemes, token 3 the first 63 of them, token 0 the last: (3, 0) and (2,) share a spelling
    long = [5 + (i * 7) % 11 for i in range(64)]
    spell = [[long[-1]], [1], long, long[:-1], None]
    x = emissions(91, 4, 8, 5, 1.0)
    want = compare(x, transitions(92, 5), 4, forced, spell, 16, 5, 4)
    assert sum(w[1] + w[2] for w in want if w is not None) > 0


# ------------------------------------------------------------------------------------------------------------------
# edge inputs
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_half_the_transitions_forbidden(forced):
    spell = with_blank(ABBA + [[0, 0], [1, 1], [0, 1, 0]], 7)
    C = 8
    x, Wt = emissions(41, 4, 30, C, 1.0), transitions(42, C)
    mask = np.random.RandomState(44).rand(C + 1, C) < 0.5
    mask[0, C - 1] = mask[C, C - 1] = False  # (start -> blank and blank -> blank stay: the empty spelling lives)
    Wt[mask] = -np.inf
    want = compare(x, Wt, C - 1, forced, spell, 16, C, 3)
    assert all(w is None or w[0][0][2] > NEG for w in want)


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_scattered_nans_count_as_minus_infinity(forced):
    spell = with_blank(ABBA + [[0, 0], [1, 1], [0, 1, 0]], 7)
    x, Wt = emissions(14, 4, 20, 8, 1.0), transitions(15, 8)
    rs = np.random.RandomState(15)
    x[rs.rand(*x.shape) < 0.2] = np.nan
    Wt[rs.rand(*Wt.shape) < 0.2] = np.nan
    x[:, :, 7] = np.where(np.isnan(x[:, :, 7]), 0.25, x[:, :, 7])  # (the blank stays possible: no utterance dies)
    Wt[0, 7] = 0.125
    Wt[8] = np.where(np.isnan(Wt[8]), 0.125, Wt[8])
    compare(x, Wt, 7, forced, spell, 8, 8, 3)
    y = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    Vt = np.where(np.isnan(Wt), -np.inf, Wt).astype(np.float32)
    a, b = device(x, Wt, 7, forced, spell, 8, 8, 3), device(y, Vt, 7, forced, spell, 8, 8, 3)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_an_utterance_with_an_impossible_frame_decodes_to_nothing(forced):
    spell = with_blank(AAA + ABBA, 7)
    x, Wt = emissions(16, 3, 20, 8, 1.0), transitions(17, 8)
    alone = device(x[[0, 2]], Wt, 7, forced, spell, 8, 8, 3)
    x[1, 11, :] = -np.inf
    x[1, 11, 5] = np.nan
    want = compare(x, Wt, 7, forced, spell, 8, 8, 3)
    assert want[1][0] == [((), (), NEG)] * 3
    seqs, raw = device(x, Wt, 7, forced, spell, 8, 8, 3)
    assert seqs[1] == [(), (), ()] and (raw[1] == NEG).all()
    assert [seqs[0], seqs[2]] == alone[0] and (raw[[0, 2]] == alone[1]).all()  # (its neighbours are unaffected)


def test_exact_ties_go_to_the_earlier_place():
    """the tokens a and b have the same scores in every frame, ab and ba as well (and no transitions): every hypothesis
    has a twin with a and b exchanged and exactly its mass -- computed by the same operations, so the tie is exact on both
    sides -- and the order of the twins is the tie rule's.  (No margin to assert: it is 0 by construction.)"""
    spell = with_blank(ABBA, 4)
    x = emissions(5, 6, 6, 5, 1.0)
    x[:, :, 1], x[:, :, 3] = x[:, :, 0], x[:, :, 2]
    for forced in (False, True):
        for W, K in ((4, 5), (8, 3), (64, 5)):
            hyps = [MR.merged_beam_search(x[b], None, 4, forced, spell, W, K, min(4, W))[0] for b in range(x.shape[0])]
            seqs, raw = device(x, None, 4, forced, spell, W, K, min(4, W))
            ties = 0
            for b in range(x.shape[0]):
                assert seqs[b] == [rho for rho, _, _ in hyps[b]], (forced, W, K, b)
                assert all(raw[b, r] == h[2] or abs(raw[b, r] - h[2]) <= 1e-9 for r, h in enumerate(hyps[b]))
                ties += sum(hyps[b][r][2] == hyps[b][r + 1][2] > NEG for r in range(len(hyps[b]) - 1))
            assert ties > 0


def test_the_same_call_twice_is_bit_identical():
    spell = with_blank(overlapping_pieces()[:29], 29)
    x, Wt = emissions(19, 8, 60, 30, 1.0), transitions(20, 30)
    for forced in (False, True):
        a = device(x, Wt, 29, forced, spell, 64, 30, 3, normalize=True)
        b = device(x, Wt, 29, forced, spell, 64, 30, 3, normalize=True)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


def test_with_single_distinct_graphemes_the_results_are_the_unmerged_searchs():
    E, _, _ = _mods()
    for (T, C, W, K, B), blank in (((60, 29, 16, 8, 3), 28), ((50, 70, 64, 64, 2), 0), ((40, 6, 4, 3, 50), 3)):
        x, Wt = emissions(900 + T, B, T, C, 1.0), transitions(901 + T, C)
        spell = with_blank([[3 + 2 * c] for c in range(C - 1)], blank)
        xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
        for forced in (False, True):
            for W_ in (Wd, None):
                m_h, m_s = device(x, None if W_ is None else Wt, blank, forced, spell, W, K, min(3, W), normalize=True)
                p_h, p_s = E.transducer_beam_search(xd, W_, blank, forced, W, K, min(3, W), normalize=True)
                assert m_h == [[tuple(s.tolist()) for s in h] for h in p_h]
                p = p_s.numpy()
                with np.errstate(invalid="ignore"):  # (-inf - -inf for an empty rank: equal already)
                    assert ((m_s == p) | (np.abs(m_s - p) <= 1e-12)).all()


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
KINDS = [dict(blank="optional", allow_repeats=False), dict(blank="forced")]
G2I = {"a": 0, "b": 1}


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
@pytest.mark.parametrize("tokens,T", [(["a", "b", "ab"], 4), (["a", "aa", "aaa"], 5)], ids=["ab4", "aaa5"])
def test_module_score_is_minus_the_loss_of_the_spelling_where_nothing_is_pruned(tokens, T, ngram, kw):
    """W = 64, K = C at a shape where the reference reports nothing pruned: the score of a rank is minus the device loss
    of its spelling as the target.  The unmerged search returns a strictly smaller number for a spelling with more than
    one decomposition."""
    forced = kw["blank"] == "forced"
    crit, params = _criterion(tokens, G2I, ngram, kw, 300 + ngram)
    spell = [[G2I[g] for g in wp] for wp in tokens] + [None]
    C, blank, B = 4, 3, 3
    x = emissions(1310 + 10 * T + ngram + int(forced), B, T, C, 1.0)
    xe, Wt = _operands(x, params, ngram)
    want = reference(xe, Wt, blank, forced, spell, 64, C, 4)
    xd = torch.from_numpy(x).cuda()
    hyps, scores = crit.beam_search(xd, beam_size=64, classes_per_frame=C, nbest=4, return_scores=True, merge_spellings=True)
    plain_h, plain_s = crit.beam_search(xd, beam_size=64, classes_per_frame=C, nbest=64, return_scores=True)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (B, 4) and not scores.is_cuda
    logz = log_normaliser(xe, Wt)
    strict = 0
    for b in range(B):
        assert want[b] is not None and want[b][3] is False
        assert all(p.dtype == torch.int32 and not p.is_cuda and p.dim() == 1 for p in hyps[b])
        assert [tuple(p.tolist()) for p in hyps[b]] == [rho for rho, _, _ in want[b][0]], (T, b)
        spellings = [MR.spelt(spell, p.tolist()) for p, s in zip(hyps[b], scores[b]) if s > NEG]
        assert len(set(spellings)) == len(spellings)
        for r, (rho, S, s) in enumerate(want[b][0]):
            got = float(scores[b, r])
            if s == NEG:
                assert got == NEG
                continue
            n = s - logz[b]
            assert BS.normalised_close(got, n), (T, b, r, got, n)
            if S:
                loss = _minus_loss(crit, xd, b, S)
                assert abs(got - loss) <= 1e-4 * abs(loss) + 2e-5, (T, b, r, S, got, loss)
            # the unmerged search's score of any sequence with this spelling is not above
            for q, v in zip(plain_h[b], plain_s[b]):
                if v > NEG and MR.spelt(spell, q.tolist()) == S:
                    assert float(v) <= got + 1e-9
                    strict += float(v) < got - 1e-3
    # (forced, four frames, {a, b, ab}: a token needs the blank on both sides, so no spelling has two decompositions)
    assert strict > 0 or (forced and T == 4)


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 2])
def test_module_where_the_beam_prunes(ngram, kw):
    """W = 16 over five overlapping pieces, T = 12: the score is a lower bound of minus the loss of the spelling.  That it
    is not below the unmerged search's score of a sequence with that spelling is asserted where nothing is pruned (the
    test above, every rank and every sequence): under pruning the two beams keep different prefixes -- this one ranks per
    (spelling, last token), so hypotheses of one spelling take several slots -- and the rules promise it only for what
    both beams kept.  Measured here, ngram 0, optional topology, utterance 0: merged -14.2269 against -13.9492 for the
    unmerged search's best sequence, with the device equal to the restatement of the rules on both."""
    forced = kw["blank"] == "forced"
    tokens = ["a", "b", "ab", "ba", "bab"]
    crit, params = _criterion(tokens, G2I, ngram, kw, 400 + ngram)
    spell = [[G2I[g] for g in wp] for wp in tokens] + [None]
    C, blank, B, T = 6, 5, 4, 12
    x = emissions(410 + ngram + int(forced), B, T, C, 1.0)
    xe, Wt = _operands(x, params, ngram)
    want = reference(xe, Wt, blank, forced, spell, 16, C, 3)
    xd = torch.from_numpy(x).cuda()
    hyps, scores = crit.beam_search(xd, beam_size=16, classes_per_frame=C, nbest=3, return_scores=True, merge_spellings=True)
    plain_h, plain_s = crit.beam_search(xd, beam_size=16, classes_per_frame=C, nbest=16, return_scores=True)
    again_h, again_s = crit.beam_search(xd, 16, C, 16, True)  # (the positional call is what it was)
    assert [[p.tolist() for p in h] for h in again_h] == [[p.tolist() for p in h] for h in plain_h]
    assert again_s.numpy().tobytes() == plain_s.numpy().tobytes()
    for b in range(B):
        if want[b] is not None:
            assert [tuple(p.tolist()) for p in hyps[b]] == [rho for rho, _, _ in want[b][0]]
        spellings = []
        for r in range(3):
            seq, got = hyps[b][r].tolist(), float(scores[b, r])
            if got == NEG:
                continue
            S = MR.spelt(spell, seq)
            spellings.append(S)
            if S:
                loss = _minus_loss(crit, xd, b, S)
                assert got <= loss + 1e-4 * abs(loss) + 2e-5, (b, r, seq, got, loss)  # a lower bound of minus the loss
        assert len(set(spellings)) == len(spellings)


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_errors_with_merged_spellings_count_what_beam_search_predicts(ngram, kw):
    _, M, _ = _mods()
    tokens = ["a", "b", "ab", "ba", "bab"]
    crit, _ = _criterion(tokens, G2I, ngram, kw, 500 + ngram)
    B, T, C = 4, 50, 6
    xd = torch.from_numpy(emissions(510 + ngram, B, T, C, 1.0)).cuda()
    rs = np.random.RandomState(62)
    targets = [rs.randint(0, 2, size=n).tolist() for n in (7, 1, 12, 3)]
    counter = M.ErrorCounter(hyp_symbols=[[G2I[g] for g in wp] for wp in tokens])
    for W, K in ((1, C), (16, 4)):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K, merge_spellings=True)
        assert any(p.numel() > 0 for p in pred)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K, merge_spellings=True) == counter(pred, targets)
        plain = crit.beam_search(xd, beam_size=W, classes_per_frame=K)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K) == counter(plain, targets)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K, merge_spellings=False) == counter(plain, targets)
    assert crit.errors(xd, targets, counter) == counter(crit.viterbi(xd), targets)  # (the call without a beam is what it was)
