"""CTC prefix beam search with a lexicon and a word-level n-gram LM on the device (csrc/beam_kernels.hip:
wfl_ctc_beam_search_lexicon behind engine.ctc_beam_search(lexicon=), CTC.beam_search(lexicon=) and
CTC.errors(beam_size=, lexicon=)) against its restatement in plain Python (tests/beam_lexicon_reference.py, itself pinned
to a re-scored brute-force enumeration in tests/test_beam_lexicon_abi.py).  Lexicons are seeded random words that end in
a separator class, packed by lexicon.Lexicon on the device side and kept as a dict of spellings on the reference's; word
LMs are seeded random ARPA texts over the word names, loaded through NGramLM.from_arpa(path, words, blank=len(words)) on
the device side and read by the reference's own few lines.

Acceptance of every comparison: tests/beam_support.py (assert_ranks, margins_ok), as in tests/test_gpu_beam_search_lm.py."""
import math

import numpy as np
import pytest
import torch

import beam_lexicon_reference as XR
import beam_lm_reference as LR
import beam_reference as R
import beam_support as S
from beam_support import emissions, names_of
from beam_support import word_lms as make_lms

pytestmark = pytest.mark.gpu

ALPHA, OMEGA, BETA = 0.8, 0.6, 0.3


def _mods():
    return S.package("engine", "metrics", "criterions.ctc:CTC", "lexicon:Lexicon", "lm:NGramLM")


def pack(spellings, C, blank):
    """the device's Lexicon of a reference lexicon {spelling: word id}"""
    Lexicon = _mods()[3]
    by_id = sorted(spellings, key=spellings.get)
    assert [spellings[s] for s in by_id] == list(range(len(by_id)))
    return Lexicon(by_id, C, blank)


def reference(x, blank, W, K, nbest, spellings, ref_lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True, lengths=None):
    rows = S.utterances(x, lengths)
    search = lambda b: XR.beam_search(rows[b], blank, W, K, nbest, spellings, ref_lm, alpha, omega, beta, eos)
    out = []
    for b, (hyps, _, _) in enumerate(S.margins_ok(search, len(rows))):
        shift = S.row_shift(rows[b])
        out.append((hyps, [(h, s - shift if s != R.NEG else s) for h, s in hyps]))
    return out


def device(x, blank, W, K, nbest, lex, lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True, lengths=None, normalize=False):
    E = _mods()[0]
    xd = torch.from_numpy(x).cuda()
    xlen = None if lengths is None else E.input_lengths_on_device(tuple(int(n) for n in lengths), xd.device)
    kw = {} if lm is None else dict(lm=lm, lm_weight=alpha, lm_eos=eos)
    hyps, scores = E.ctc_beam_search(xd, blank, W, K, nbest, lengths=xlen, normalize=normalize, lexicon=lex, word_bonus=omega,
                                     length_bonus=beta, **kw)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, blank, W, K, nbest, spellings, lm, ref_lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True, lengths=None):
    lex = pack(spellings, x.shape[2], blank)
    want = reference(x, blank, W, K, nbest, spellings, ref_lm, alpha, omega, beta, eos, lengths)
    seqs, raw = device(x, blank, W, K, nbest, lex, lm, alpha, omega, beta, eos, lengths)
    nseqs, normed = device(x, blank, W, K, nbest, lex, lm, alpha, omega, beta, eos, lengths, normalize=True)
    assert nseqs == seqs
    shifts = [S.row_shift(rows) for rows in S.utterances(x, lengths)]
    # (every returned sequence is a sequence of whole words: lex.words raises otherwise)
    S.assert_ranks([hyps for hyps, _ in want], seqs, raw, normed, shifts, nbest, blank, check=lambda b, r, seq: lex.words(seq))
    return want, seqs, raw


def peaked(seed, B, T, C, blank, spellings):
    """emissions that spell a sentence of lexicon words: each label of the sentence on a frame of its own, a blank frame
    between equal neighbours, the rest blank, +6 on N(0, 0.5^2) noise -- complete-word hypotheses survive the beam"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, T, C) * 0.5).astype(np.float32)
    words = sorted(spellings, key=spellings.get)
    for b in range(B):
        frames = []
        while True:
            w = words[rs.randint(len(words))]
            more = []
            for c in w:
                if (more or frames) and (more or frames)[-1] == c:
                    more.append(blank)
                more.append(c)
            if len(frames) + len(more) > T:
                break
            frames += more
        for t in range(T):
            x[b, t, frames[t] if t < len(frames) else blank] += 6.0
    return x


def sep_of(C, blank):
    return C - 1 if blank != C - 1 else C - 2


# (T, C, W, K, B, words, longest spelling without its separator)
SHAPES = [(1, 3, 1, 2, 2, 3, 3), (12, 4, 8, 3, 4, 5, 3), (40, 12, 4, 8, 3, 30, 3), (64, 30, 64, 30, 2, 120, 3),
          (120, 100, 16, 32, 2, 300, 2)]
VARIANTS = {"n1-bigram": (1.0, 2), "n3-nolm": (3.0, 0), "peaked-trigram": (None, 3)}


def parity_case(T, C, W, K, B, V, longest, where, variant):
    """(x, blank, {spelling: word id}, ARPA text or None) of a parity case: everything seeded by the case"""
    scale, order = VARIANTS[variant]
    blank = {"first": 0, "last": C - 1, "middle": C // 2}[where]
    seed = 7907 * T + 37 * C + W + {"first": 0, "last": 17, "middle": 29}[where] + 1000 * order
    rs = np.random.RandomState(seed)
    spellings = XR.random_lexicon(rs, C, blank, V, longest, sep_of(C, blank))
    text = LR.random_arpa(rs, names_of(V), order, 0.02 if V >= 100 else 0.3) if order else None
    x = emissions(seed + 1, B, T, C, scale) if scale else peaked(seed + 1, B, T, C, blank, spellings)
    return x, blank, spellings, text


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("T,C,W,K,B,V,longest", SHAPES, ids=lambda v: str(v))
def test_random_lexicons_and_word_lms_against_the_reference(tmp_path, T, C, W, K, B, V, longest, where, variant):
    x, blank, spellings, text = parity_case(T, C, W, K, B, V, longest, where, variant)
    lm, ref_lm = make_lms(tmp_path, text, V)
    _, seqs, _ = compare(x, blank, W, K, min(W, 4), spellings, lm, ref_lm)
    if variant.startswith("peaked") and T >= 12:
        assert all(len(h[0]) > 0 for h in seqs)  # (whole words survive)


# a one-label word; a word with a doubled label; a root with a single arc; a lexicon that uses every class (C = 6,
# blank 2, separator 5)
EDGES = {
    "one-label-word": {(4,): 0, (0, 1, 5): 1, (1, 5): 2, (0, 0, 5): 3},
    "doubled-label": {(1, 1, 5): 0, (1, 5): 1, (3, 3, 3, 5): 2, (3, 1, 1, 5): 3},
    "single-root-arc": {(3, 5): 0, (3, 0, 5): 1, (3, 3, 5): 2, (3, 0, 1, 5): 3},
    "every-class": {(0, 5): 0, (1, 3, 5): 1, (4, 5): 2, (3, 4, 0, 5): 3, (1, 1, 5): 4},
}


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("edge", list(EDGES))
def test_lexicon_edges(tmp_path, edge, order):
    spellings, C, blank, T, B = EDGES[edge], 6, 2, 24, 4
    assert XR.is_prefix_free(spellings)
    if edge == "every-class":
        assert {c for s in spellings for c in s} == set(range(C)) - {blank}
    seed = 300 + 10 * list(EDGES).index(edge) + order
    text = LR.random_arpa(np.random.RandomState(seed), names_of(len(spellings)), order, 0.5) if order else None
    lm, ref_lm = make_lms(tmp_path, text, len(spellings))
    compare(emissions(seed + 1, B, T, C, 1.0), blank, 8, 5, 4, spellings, lm, ref_lm)
    _, seqs, _ = compare(peaked(seed + 2, B, T, C, blank, spellings), blank, 8, 5, 4, spellings, lm, ref_lm)
    assert all(len(h[0]) > 0 for h in seqs)
    if edge == "one-label-word":  # (the word is found)
        x = peaked(seed + 3, 1, 6, C, blank, {(4,): 0})
        assert compare(x, blank, 8, 5, 1, spellings, lm, ref_lm)[1][0][0] == (4,) * 3


def small_case(seed, T=40, C=12, B=4, V=30, blank=0, order=2, keep=0.3, scale=1.0, eos=True):
    rs = np.random.RandomState(seed)
    spellings = XR.random_lexicon(rs, C, blank, V, 3, sep_of(C, blank))
    text = LR.random_arpa(rs, names_of(V), order, keep, eos=eos) if order else None
    return emissions(seed + 1, B, T, C, scale), spellings, text


def test_lexicon_alone_is_the_lexicon_with_a_silent_lm(tmp_path):
    """alpha = 0, omega = 0 and an LM that knows every word (all unigrams: no step is -inf): every LM term is 0, the
    terms are formed by the same operations, so sequences and scores are identical to the search without an LM"""
    for T, C, W, K, B, V, blank in ((40, 12, 16, 8, 4, 30, 0), (64, 30, 64, 30, 2, 120, 29)):
        x, spellings, text = small_case(400 + C, T, C, B, V, blank, order=3)
        x = np.concatenate([x[:B // 2], peaked(401 + C, B - B // 2, T, C, blank, spellings)])
        lex, (lm, _) = pack(spellings, C, blank), make_lms(tmp_path, text, V)
        for eos in (True, False):
            with_lm = device(x, blank, W, K, min(W, 4), lex, lm, alpha=0.0, omega=0.0, eos=eos)
            alone = device(x, blank, W, K, min(W, 4), lex, None, omega=0.0)
            assert with_lm[0] == alone[0] and with_lm[1].tobytes() == alone[1].tobytes()
            assert any(len(s) for h in alone[0] for s in h)


def test_a_frame_where_no_word_can_start():
    """every word's first label is -inf in one frame (and in another the blank as well: only labels inside a word are
    finite there)"""
    T, C, W, K, B, blank = 30, 12, 8, 12, 4, 0
    x, spellings, _ = small_case(410, T, C, B, 20, blank, order=0)
    x = np.concatenate([x[:2], peaked(411, 2, T, C, blank, spellings)])
    first = sorted({s[0] for s in spellings})
    x[:, 7, first] = -np.inf
    x[:, 15, first] = -np.inf
    x[:, 15, blank] = -np.inf
    compare(x, blank, W, K, 4, spellings, None, None)


def test_every_final_hypothesis_inside_a_word_gives_empty_ranks(tmp_path):
    """the blank is impossible and there are fewer frames than the shortest word has labels: every hypothesis of the
    final beam stands inside a word"""
    C, blank, T, B = 8, 3, 2, 3
    spellings = {(0, 1, 7): 0, (1, 2, 7): 1, (4, 4, 7): 2, (5, 0, 6, 7): 3}
    x = emissions(420, B, T, C, 1.0)
    x[:, :, blank] = -np.inf
    lex = pack(spellings, C, blank)
    want = [XR.beam_search(x[b], blank, 8, 8, 3, spellings, None, 1.0, OMEGA, BETA, True)[0] for b in range(B)]
    assert want == [[((), R.NEG)] * 3] * B
    for normalize in (False, True):
        seqs, raw = device(x, blank, 8, 8, 3, lex, None, normalize=normalize)
        assert seqs == [[(), (), ()]] * B and (raw == R.NEG).all()
    x[:, :, blank] = 3.0  # (with a likely blank the empty sequence stays in the beam, and it is a sequence of words)
    _, seqs, raw = compare(x, blank, 8, 8, 3, spellings, None, None)
    assert all(h == [(), (), ()] for h in seqs) and np.isfinite(raw[:, 0]).all() and (raw[:, 1:] == R.NEG).all()


def test_a_word_the_lm_cannot_follow_is_never_emitted(tmp_path):
    """The arcs of one word are taken out of the LM's pack by constructing it directly (the loader would refuse a word
    without a unigram).  The emissions spell that word, so the search with the whole LM emits it; without its arcs
    step() is -inf from every state and no hypothesis may complete it."""
    NGramLM = _mods()[4]
    C, blank, T, B, V, gone = 12, 0, 30, 4, 20, 5
    _, spellings, text = small_case(430, T, C, B, V, blank)
    lex = pack(spellings, C, blank)
    word = sorted(spellings, key=spellings.get)[gone]
    x = peaked(431, B, T, C, blank, {word: 0, sorted(spellings, key=spellings.get)[3]: 1})
    whole, _ = make_lms(tmp_path, text, V)
    assert any(gone in lex.words(s) for h in device(x, blank, 16, 6, 4, lex, whole)[0] for s in h)
    keep = whole.arc_label != gone
    ptr = np.concatenate([[0], np.cumsum([keep[whole.arc_ptr[s]:whole.arc_ptr[s + 1]].sum() for s in range(whole.num_states)])])
    lm = NGramLM(V + 1, V, ptr, whole.arc_label[keep], whole.arc_next[keep], whole.arc_w[keep], whole.bo_next, whole.bo_w,
                 start=whole.start, order=2)
    assert lm.num_arcs < whole.num_arcs and lm.score([gone]) == -math.inf
    cut = "\n".join(l for l in text.split("\n") if f"w{gone}" not in l.split())  # (the reference does not count its sections)
    _, seqs, _ = compare(x, blank, 16, 6, 4, spellings, lm, LR.ArpaLM(cut, names_of(V), V))
    assert not any(gone in lex.words(s) for h in seqs for s in h)
    assert any(len(s) > 0 for h in seqs for s in h)


def test_word_bonus_extremes(tmp_path):
    """omega = +50 outweighs every other term of a word: the best hypotheses complete more words than they did.
    omega = -50: no word is worth completing -- what is left of the beam is the empty sequence, or nothing where the
    prefixes inside a first word (they have paid no bonus yet) have pushed it out."""
    T, C, W, K, B, blank, V = 40, 12, 16, 8, 4, 11, 30
    x, spellings, text = small_case(440, T, C, B, V, blank, order=2)
    x[2:] = peaked(441, 2, T, C, blank, spellings)
    lm, ref_lm = make_lms(tmp_path, text, V)
    lex = pack(spellings, C, blank)
    count = lambda seqs: [len(lex.words(h[0])) for h in seqs]
    _, plain, _ = compare(x, blank, W, K, 4, spellings, lm, ref_lm)
    _, seqs, _ = compare(x, blank, W, K, 4, spellings, lm, ref_lm, omega=50.0)
    assert all(n >= p for n, p in zip(count(seqs), count(plain))) and sum(count(seqs)) >= sum(count(plain)) + B
    for word_lm in ((lm, ref_lm), (None, None)):
        _, seqs, _ = compare(x, blank, W, K, 4, spellings, *word_lm, omega=-50.0)
        assert all(s == () for h in seqs for s in h)


def test_an_order_three_word_lm_backs_off(tmp_path):
    T, C, W, K, B, blank, V = 40, 12, 16, 8, 4, 6, 12
    rs = np.random.RandomState(450)
    spellings = XR.random_lexicon(rs, C, blank, V, 2, sep_of(C, blank))
    text = LR.random_arpa(rs, names_of(V), 3, 0.25)
    lm, ref_lm = make_lms(tmp_path, text, V)
    assert lm.order == 3
    x = peaked(451, B, T, C, blank, spellings)
    _, seqs, _ = compare(x, blank, W, K, 4, spellings, lm, ref_lm)
    lex = pack(spellings, C, blank)
    backed = 0
    for h in seqs:  # the best hypotheses take words whose trigram and bigram are not in the file
        s = lm.start
        for v in lex.words(h[0]):
            direct = v in lm.arc_label[lm.arc_ptr[s]:lm.arc_ptr[s + 1]].tolist()
            backed += (not direct) and lm.bo_next[s] >= 0
            s = lm.step(s, v)[1]
    assert backed >= 4


def test_lengths_decode_each_utterance_as_its_own_slice(tmp_path):
    B, T, C, W, K, V, blank = 5, 40, 12, 16, 6, 30, 0
    lengths = [0, 1, 39, 40, 23]
    x, spellings, text = small_case(460, T, C, B, V, blank, order=3)
    x[2:] = peaked(461, 3, T, C, blank, spellings)
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan  # (the frames behind an utterance are not read)
    lm, ref_lm = make_lms(tmp_path, text, V)
    lex = pack(spellings, C, blank)
    _, seqs, raw = compare(x, blank, W, K, 3, spellings, lm, ref_lm, lengths=lengths)
    # no frame: the empty sequence with the LM's </s> from the start state; 0 without </s> or without an LM
    assert seqs[0] == [(), (), ()] and raw[0, 1] == R.NEG and abs(raw[0, 0] - ALPHA * lm.score([])) <= 1e-12
    assert device(x, blank, W, K, 3, lex, lm, eos=False, lengths=lengths)[1][0].tolist() == [0.0, R.NEG, R.NEG]
    assert device(x, blank, W, K, 3, lex, None, lengths=lengths)[1][0].tolist() == [0.0, R.NEG, R.NEG]
    compare(x, blank, W, K, 3, spellings, None, None, lengths=lengths)
    for b, n in enumerate(lengths):
        if n:
            s, r = device(np.ascontiguousarray(x[b:b + 1, :n]), blank, W, K, 3, lex, lm)
            assert s[0] == seqs[b] and (r[0] == raw[b]).all(), b


def test_the_same_call_twice_is_bit_identical(tmp_path):
    x, spellings, text = small_case(470, 60, 30, 8, 120, 29, order=3, keep=0.05)
    x[4:] = peaked(471, 4, 60, 30, 29, spellings)
    lm, _ = make_lms(tmp_path, text, 120)
    lex = pack(spellings, 30, 29)
    a = device(x, 29, 64, 30, 3, lex, lm, normalize=True)
    b = device(x, 29, 64, 30, 3, lex, lm, normalize=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    assert any(len(s) for h in a[0] for s in h)


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
def test_module_beam_search_with_a_lexicon(tmp_path):
    CTC = _mods()[2]
    B, T, C, V = 4, 40, 12, 30
    crit = CTC(blank=0, use_pt=False)
    x, spellings, text = small_case(480, T, C, B, V, 0)
    x[2:] = peaked(481, 2, T, C, 0, spellings)
    xd = torch.from_numpy(x).cuda()
    lm, ref_lm = make_lms(tmp_path, text, V)
    lex = pack(spellings, C, 0)
    kw = dict(lexicon=lex, word_bonus=OMEGA, lm=lm, lm_weight=ALPHA, length_bonus=BETA)
    hyps, scores = crit.beam_search(xd, beam_size=8, classes_per_frame=6, nbest=3, return_scores=True, **kw)
    want = reference(x, 0, 8, 6, 3, spellings, ref_lm)
    for b in range(B):
        assert [tuple(s.tolist()) for s in hyps[b]] == [h for h, _ in want[b][1]]
        for r in range(3):
            n = want[b][1][r][1]
            assert scores[b, r].item() == n if n == R.NEG else S.normalised_close(scores[b, r].item(), n)
    best = crit.beam_search(xd, beam_size=8, classes_per_frame=6, **kw)
    assert [p.tolist() for p in best] == [h[0].tolist() for h in hyps]
    assert all(lex.words(p) is not None for p in best) and any(len(p) for p in best)
    # the lexicon alone, with a length bonus and no lm
    alone = crit.beam_search(xd, beam_size=8, classes_per_frame=6, lexicon=lex, length_bonus=BETA)
    assert [tuple(p.tolist()) for p in alone] == [h[0][0] for h, _ in reference(x, 0, 8, 6, 1, spellings, None, 1.0, 0.0, BETA)]
    # the emissions may live on the host: the call moves them
    assert [p.tolist() for p in crit.beam_search(torch.from_numpy(x), beam_size=8, classes_per_frame=6, **kw)] == \
        [p.tolist() for p in best]


@pytest.mark.parametrize("lens", [None, [9, 40, 23, 40, 1, 31]])
def test_errors_with_a_beam_and_a_lexicon_count_what_beam_search_predicts(tmp_path, lens):
    _, M, CTC, _, _ = _mods()
    B, T, C, V = 6, 40, 12, 30
    crit = CTC(blank=C - 1, use_pt=False)
    x, spellings, text = small_case(490, T, C, B, V, C - 1, order=3)
    x[3:] = peaked(491, 3, T, C, C - 1, spellings)
    xd = torch.from_numpy(x).cuda()
    rs = np.random.RandomState(492)
    targets = [rs.randint(0, C - 1, size=n).tolist() for n in (7, 0, 12, 3, 20, 1)]
    counter = M.ErrorCounter(wordsep=sep_of(C, C - 1))
    lm, _ = make_lms(tmp_path, text, V)
    lex = pack(spellings, C, C - 1)
    for W, K, kw in ((1, 12, dict(lexicon=lex)), (16, 6, dict(lexicon=lex, lm=lm, lm_weight=ALPHA, word_bonus=OMEGA, length_bonus=BETA)),
                     (16, 6, dict(lexicon=lex, lm=lm, lm_weight=2.0, lm_eos=False)), (16, 6, dict(lexicon=lex, word_bonus=-1.0))):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K, input_lengths=lens, **kw)
        assert crit.errors(xd, targets, counter, input_lengths=lens, beam_size=W, classes_per_frame=K, **kw) == \
            counter(pred, targets)
    assert any(len(p) for p in pred)


def test_without_a_lexicon_the_calls_are_what_they_were(tmp_path):
    """CTC.beam_search and CTC.errors without `lexicon` against direct calls of engine.ctc_beam_search with the
    arguments it had before there was one: bit-identical, plain and with a token LM"""
    E, M, CTC, _, NGramLM = _mods()
    B, T, C, blank = 4, 40, 12, 0
    crit = CTC(blank=blank, use_pt=False)
    xd = torch.from_numpy(emissions(500, B, T, C, 1.0)).cuda()
    p = tmp_path / "tokens.arpa"
    p.write_text(LR.random_arpa(np.random.RandomState(501), [f"t{i}" for i in range(C - 1)], 2, 0.3))
    lm = NGramLM.from_arpa(str(p), [f"t{i}" for i in range(C - 1)], blank)
    for kw in ({}, dict(lm=lm, lm_weight=ALPHA, length_bonus=BETA, lm_eos=True)):
        hyps, scores = crit.beam_search(xd, beam_size=8, classes_per_frame=6, nbest=3, return_scores=True, **kw)
        direct, dscores = E.ctc_beam_search(xd, blank, 8, 6, 3, None, True, *kw.values())
        assert [[s.tolist() for s in h] for h in hyps] == [[s.tolist() for s in h] for h in direct]
        assert scores.numpy().tobytes() == dscores.numpy().tobytes()
        counter = M.ErrorCounter(wordsep=3)
        targets = [[1, 2, 3, 4], [], [5, 3, 6], [7]]
        assert crit.errors(xd, targets, counter, beam_size=8, classes_per_frame=6, **kw) == \
            counter([h[0] for h in direct], targets)
