"""CTC prefix beam search with an n-gram LM and a length bonus on the device (csrc/beam_kernels.hip:
wfl_ctc_beam_search_lm behind engine.ctc_beam_search(lm=), CTC.beam_search(lm=) and CTC.errors(beam_size=, lm=)) against
its restatement in plain Python (tests/beam_lm_reference.py, itself pinned to a re-scored brute-force enumeration in
tests/test_beam_lm_abi.py).  The LMs are seeded random ARPA texts: the device side loads them through
NGramLM.from_arpa, the reference reads the same text with its own few lines.

Acceptance of every comparison: tests/beam_support.py (assert_ranks, margins_ok), as in tests/test_gpu_beam_search.py."""
import math

import numpy as np
import pytest
import torch

import beam_lm_reference as LR
import beam_reference as R
import beam_support as S
from beam_support import emissions, tokens_of
from beam_support import token_lms as make_lms

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.8, 0.5


def _mods():
    return S.package("engine", "metrics", "criterions.ctc:CTC", "lm:NGramLM")


def reference(x, blank, W, K, nbest, ref_lm, alpha=ALPHA, beta=BETA, eos=True, lengths=None):
    rows = S.utterances(x, lengths)
    out = []
    for b, (hyps, _, _) in enumerate(S.margins_ok(lambda b: LR.beam_search(rows[b], blank, W, K, nbest, ref_lm, alpha, beta, eos),
                                                  len(rows))):
        shift = S.row_shift(rows[b])
        out.append((hyps, [(h, s - shift if s != R.NEG else s) for h, s in hyps]))
    return out


def device(x, blank, W, K, nbest, lm, alpha=ALPHA, beta=BETA, eos=True, lengths=None, normalize=False):
    E = _mods()[0]
    xd = torch.from_numpy(x).cuda()
    xlen = None if lengths is None else E.input_lengths_on_device(tuple(int(n) for n in lengths), xd.device)
    hyps, scores = E.ctc_beam_search(xd, blank, W, K, nbest, lengths=xlen, normalize=normalize, lm=lm, lm_weight=alpha,
                                     length_bonus=beta, lm_eos=eos)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, blank, W, K, nbest, lm, ref_lm, alpha=ALPHA, beta=BETA, eos=True, lengths=None):
    want = reference(x, blank, W, K, nbest, ref_lm, alpha, beta, eos, lengths)
    seqs, raw = device(x, blank, W, K, nbest, lm, alpha, beta, eos, lengths)
    nseqs, normed = device(x, blank, W, K, nbest, lm, alpha, beta, eos, lengths, normalize=True)
    assert nseqs == seqs
    shifts = [S.row_shift(rows) for rows in S.utterances(x, lengths)]
    S.assert_ranks([hyps for hyps, _ in want], seqs, raw, normed, shifts, nbest, blank)
    return want, seqs, raw


# (T, C, W, K, B)
SHAPES = [(1, 2, 1, 2, 4), (12, 3, 8, 3, 4), (30, 4, 8, 2, 64), (40, 12, 1, 12, 4), (60, 30, 16, 8, 4), (50, 70, 64, 64, 2),
          (120, 100, 16, 32, 2)]


def parity_case(T, C, W, K, B, where, order, scale):
    """(x, blank, ARPA text) of a parity case: everything seeded by the case"""
    blank = {"first": 0, "last": C - 1, "middle": C // 2}[where]
    seed = 7919 * T + 31 * C + W + (17 if where == "last" else 29 if where == "middle" else 0) + 1000 * order
    rs = np.random.RandomState(seed)
    text = LR.random_arpa(rs, tokens_of(C), order, 0.05 if C >= 70 else 0.3)
    return emissions(seed + 1, B, T, C, scale), blank, text


@pytest.mark.parametrize("order,scale", [(2, 1.0), (3, 3.0)])
@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("T,C,W,K,B", SHAPES, ids=lambda v: str(v))
def test_random_emissions_and_lms_against_the_reference(tmp_path, T, C, W, K, B, where, order, scale):
    x, blank, text = parity_case(T, C, W, K, B, where, order, scale)
    lm, ref_lm = make_lms(tmp_path, text, C, blank)
    assert lm.order == order
    compare(x, blank, W, K, min(W, 4), lm, ref_lm)


def test_lm_off_inside_the_lm_path_is_the_search_without_one(tmp_path):
    """alpha = 0, beta = 0, no </s> and an LM that knows every token (all unigrams: no step is -inf): every LM term is
    0, so the sequences are those of wfl_ctc_beam_search and the raw scores agree to 1e-9, absolutely"""
    E = _mods()[0]
    for (T, C, W, K, B), blank in (((60, 30, 16, 8, 4), 0), ((50, 70, 64, 64, 2), 69), ((30, 4, 8, 2, 16), 2)):
        x = emissions(40 + C, B, T, C, 1.0)
        lm, _ = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(C), tokens_of(C), 3, 0.2), C, blank)
        seqs, raw = device(x, blank, W, K, min(W, 4), lm, 0.0, 0.0, False)
        hyps, scores = E.ctc_beam_search(torch.from_numpy(x).cuda(), blank, W, K, min(W, 4), normalize=False)
        assert seqs == [[tuple(s.tolist()) for s in h] for h in hyps]
        plain = scores.numpy()
        assert (np.abs(raw - plain) <= 1e-9).all(), np.abs(raw - plain).max()


def test_a_token_missing_from_the_lm_is_never_emitted(tmp_path):
    """No <unk>, and the arcs of one class are taken out of the pack by constructing it directly (the loader would
    refuse a token without a unigram).  The emissions favour that class, so the same search with the whole LM emits
    it; without its arcs step() is -inf from every state and no hypothesis may contain it."""
    NGramLM = _mods()[3]
    T, C, W, K, B, blank, gone = 40, 12, 16, 6, 4, 0, 5
    x = emissions(51, B, T, C, 1.0)
    x[:, :, gone] += 2.0
    text = LR.random_arpa(np.random.RandomState(52), tokens_of(C), 2, 0.3)
    whole, _ = make_lms(tmp_path, text, C, blank)
    assert any(gone in s for h in device(x, blank, W, K, 4, whole)[0] for s in h)
    keep = whole.arc_label != gone
    ptr = np.concatenate([[0], np.cumsum([keep[whole.arc_ptr[s]:whole.arc_ptr[s + 1]].sum() for s in range(whole.num_states)])])
    lm = NGramLM(C, blank, ptr, whole.arc_label[keep], whole.arc_next[keep], whole.arc_w[keep], whole.bo_next, whole.bo_w,
                 start=whole.start, order=2)
    assert lm.num_arcs < whole.num_arcs and lm.score([gone]) == -math.inf
    word = tokens_of(C)[gone - 1]
    cut = "\n".join(l for l in text.split("\n") if word not in l.split())  # (the reference does not count its sections)
    ref_lm = LR.ArpaLM(cut, tokens_of(C), blank)
    _, seqs, _ = compare(x, blank, W, K, 4, lm, ref_lm)
    assert not any(gone in s for h in seqs for s in h)
    assert any(len(s) > 0 for h in seqs for s in h)


def test_every_end_of_sentence_impossible_gives_empty_ranks(tmp_path):
    T, C, W, K, B = 20, 8, 8, 8, 3
    x = emissions(53, B, T, C, 1.0)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(54), tokens_of(C), 2, 0.3, eos=False), C, 7)
    want = [LR.beam_search(x[b], 7, W, K, 3, ref_lm, ALPHA, BETA, True)[0] for b in range(B)]
    assert want == [[((), R.NEG)] * 3] * B
    for normalize in (False, True):
        seqs, raw = device(x, 7, W, K, 3, lm, normalize=normalize)
        assert seqs == [[(), (), ()]] * B and (raw == R.NEG).all()
    seqs, raw = device(x, 7, W, K, 3, lm, eos=False)  # (the search itself is alive)
    assert np.isfinite(raw).all() and any(len(s) for h in seqs for s in h)


def test_length_bonus_extremes(tmp_path):
    """beta = +50 outweighs every acoustic and LM term of a frame: a label is emitted wherever one can be (a candidate
    other than the last label always exists with K >= 3), so the outputs are about T long and never longer -- the arena
    holds T W records and the output T labels per rank.  beta = -50: nothing is worth a label."""
    T, C, W, K, B = 60, 30, 16, 8, 4
    x = emissions(55, B, T, C, 1.0)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(56), tokens_of(C), 3, 0.3), C, 0)
    _, seqs, _ = compare(x, 0, W, K, 4, lm, ref_lm, beta=50.0)
    assert all(T - 2 <= len(s) <= T for h in seqs for s in h)
    _, seqs, raw = compare(x, 0, W, K, 1, lm, ref_lm, beta=-50.0)
    assert seqs == [[()]] * B and np.isfinite(raw).all()
    _, seqs, _ = compare(emissions(57, 2, 50, 70, 1.0), 69, 64, 64, 4, *make_lms(
        tmp_path, LR.random_arpa(np.random.RandomState(58), tokens_of(70), 2, 0.05), 70, 69), beta=50.0)
    assert all(48 <= len(s) <= 50 for h in seqs for s in h)


def test_a_unigram_lm_of_a_hundred_arcs(tmp_path):
    """order 1: one state with C - 1 token arcs and </s> at C = 100 -- the binary search runs over more than 64 arcs"""
    T, C, W, K, B = 40, 100, 16, 32, 2
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(59), tokens_of(C), 1, 1.0), C, 50)
    assert (lm.order, lm.num_states, lm.num_arcs) == (1, 1, C) and lm.start == 0
    compare(emissions(60, B, T, C, 1.0), 50, W, K, 4, lm, ref_lm)


FOUR = """\\data\\
ngram 1=6
ngram 2=3
ngram 3=2
ngram 4=1

\\1-grams:
-9.0\t<s>\t-0.11
-1.0\t</s>
-0.7\tt0\t-0.13
-0.8\tt1\t-0.17
-0.9\tt2\t-0.19
-1.3\tt3\t-0.23

\\2-grams:
-0.3\t<s> t0\t-0.29
-0.4\tt0 t1\t-0.31
-0.5\tt1 t2\t-0.37

\\3-grams:
-0.2\t<s> t0 t1\t-0.41
-0.25\tt0 t1 t2\t-0.43

\\4-grams:
-0.1\t<s> t0 t1 t2

\\end\\
"""


def test_order_four_with_the_back_off_taken_three_times_in_a_row(tmp_path):
    """After t0 t1 t2 the LM is in the state of the trigram t0 t1 t2; t3 follows none of t0 t1 t2, t1 t2 or t2, so its
    lookup backs off three times in a row and adds the three back-off weights to t3's unigram.  The emissions are peaked
    on blank-separated t0 t1 t2 t3, so that is the best hypothesis."""
    C, blank, T = 5, 4, 8
    lm, ref_lm = make_lms(tmp_path, FOUR, C, blank)
    assert lm.order == 4
    s = lm.start
    for c in (0, 1, 2):
        _, s = lm.step(s, c)
    depth, q = 0, s
    while lm.bo_next[q] >= 0:
        q, depth = int(lm.bo_next[q]), depth + 1
    assert depth == 3
    assert abs(lm.step(s, 3)[0] - (-0.43 - 0.37 - 0.19 - 1.3) * math.log(10.0)) <= 1e-12
    x = emissions(61, 3, T, C, 0.5)
    for t, c in enumerate((0, 4, 1, 4, 2, 4, 3, 4)):
        x[:, t, c] += 6.0
    want, seqs, _ = compare(x, blank, 8, 5, 4, lm, ref_lm)
    assert all(h[0] == (0, 1, 2, 3) for h in seqs)


def test_lengths_decode_each_utterance_as_its_own_slice(tmp_path):
    B, T, C, W, K = 5, 40, 12, 16, 6
    lengths = [0, 1, 39, 40, 23]
    x = emissions(62, B, T, C, 1.0)
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan  # (the frames behind an utterance are not read)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(63), tokens_of(C), 3, 0.3), C, 0)
    _, seqs, raw = compare(x, 0, W, K, 3, lm, ref_lm, lengths=lengths)
    # no frame: the empty sequence with the LM's </s> from the start state
    assert seqs[0] == [(), (), ()] and raw[0, 1] == R.NEG and abs(raw[0, 0] - ALPHA * lm.score([])) <= 1e-12
    assert device(x, 0, W, K, 3, lm, eos=False, lengths=lengths)[1][0].tolist() == [0.0, R.NEG, R.NEG]
    for b, n in enumerate(lengths):
        if n:
            s, r = device(np.ascontiguousarray(x[b:b + 1, :n]), 0, W, K, 3, lm)
            assert s[0] == seqs[b] and (r[0] == raw[b]).all(), b


def test_the_same_call_twice_is_bit_identical(tmp_path):
    x = emissions(64, 8, 60, 30, 1.0)
    lm, _ = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(65), tokens_of(30), 3, 0.3), 30, 29)
    a = device(x, 29, 64, 30, 3, lm, normalize=True)
    b = device(x, 29, 64, 30, 3, lm, normalize=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
def test_module_beam_search_with_an_lm(tmp_path):
    CTC = _mods()[2]
    B, T, C = 4, 40, 12
    crit = CTC(blank=0, use_pt=False)
    x = emissions(66, B, T, C, 1.0)
    xd = torch.from_numpy(x).cuda()
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(67), tokens_of(C), 2, 0.3), C, 0)
    hyps, scores = crit.beam_search(xd, beam_size=8, classes_per_frame=6, nbest=3, return_scores=True, lm=lm, lm_weight=ALPHA,
                                    length_bonus=BETA)
    want = reference(x, 0, 8, 6, 3, ref_lm)
    for b in range(B):
        assert [tuple(s.tolist()) for s in hyps[b]] == [h for h, _ in want[b][1]]
        for r in range(3):
            n = want[b][1][r][1]
            assert S.normalised_close(scores[b, r].item(), n)
    best = crit.beam_search(xd, beam_size=8, classes_per_frame=6, lm=lm, lm_weight=ALPHA, length_bonus=BETA)
    assert [p.tolist() for p in best] == [h[0].tolist() for h in hyps]
    plain = crit.beam_search(xd, beam_size=8, classes_per_frame=6)
    assert [p.tolist() for p in plain] == [list(R.beam_search(x[b], 0, 8, 6, 1)[0][0][0]) for b in range(B)]
    assert [p.tolist() for p in plain] != [p.tolist() for p in best]  # (the LM steers the search)


@pytest.mark.parametrize("lens", [None, [9, 40, 23, 40, 1, 31]])
def test_errors_with_a_beam_and_an_lm_count_what_beam_search_predicts(tmp_path, lens):
    _, M, CTC, _ = _mods()
    B, T, C = 6, 40, 12
    crit = CTC(blank=C - 1, use_pt=False)
    rs = np.random.RandomState(68)
    xd = torch.from_numpy(emissions(69, B, T, C, 1.0)).cuda()
    targets = [rs.randint(0, C - 1, size=n).tolist() for n in (7, 0, 12, 3, 20, 1)]
    counter = M.ErrorCounter(wordsep=3)
    lm, _ = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(70), tokens_of(C), 3, 0.3), C, C - 1)
    for W, K, kw in ((1, 12, dict(lm=lm)), (16, 6, dict(lm=lm, lm_weight=ALPHA, length_bonus=BETA)),
                     (16, 6, dict(lm=lm, lm_weight=2.0, lm_eos=False))):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K, input_lengths=lens, **kw)
        assert crit.errors(xd, targets, counter, input_lengths=lens, beam_size=W, classes_per_frame=K, **kw) == \
            counter(pred, targets)
    # without an lm: the call it was
    pred = crit.beam_search(xd, beam_size=16, classes_per_frame=6, input_lengths=lens)
    assert crit.errors(xd, targets, counter, input_lengths=lens, beam_size=16, classes_per_frame=6) == counter(pred, targets)
