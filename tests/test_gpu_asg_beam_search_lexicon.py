"""ASG beam search with a lexicon and a word-level LM on the device (csrc/beam_kernels.hip: wfl_asg_beam_search_lexicon
behind engine.asg_beam_search_lexicon, ASG.beam_search(lexicon=) and ASG.errors(beam_size=, lexicon=)) against its
restatement in plain Python (tests/asg_beam_lexicon_reference.py, itself pinned to a brute-force enumeration in
tests/test_asg_beam_lexicon_abi.py).

Acceptance of every comparison: the raw class sequences of all returned ranks are equal; unnormalised scores agree to
1e-9 max(1, |s|) -- both sides are float64 and differ in libm rounding only; normalised scores agree at the project's
loss bar (1e-4 |want| + 2e-5, as in tests/test_gpu_asg_beam_search.py) against a float64 denominator, the device's logz
being float32.  An utterance whose smallest selection margin in the reference is below 1e-9 could legitimately come out
differently; the seeds are fixed so that there is none, and every comparison asserts that.

A universe is (tokens N, replabels R, garbage or not): token i is raw class i + R, replabel k is class k, the garbage
is class N + R, C = N + R + garbage classes in all; the last token is the word separator.  Lexicons are written out or
seeded random token sequences packed by the reference's own raw_lexicon; word LMs are seeded random ARPA texts over
the word names, written into tmp_path and loaded through NGramLM.from_arpa(path, words, blank=len(words)) for the
device and read by beam_lm_reference.ArpaLM for the reference."""
import math

import numpy as np
import pytest
import torch

import asg_beam_lexicon_reference as AX
import asg_beam_reference as AR
import beam_lm_reference as LR
import beam_support as S
from beam_support import emissions, names_of, transitions
from beam_support import log_normaliser as log_denominator  # (with transitions: the criterion's denominator, asg.py:114)
from beam_support import spelled_asg as spelled
from beam_support import word_lms as make_lms

pytestmark = pytest.mark.gpu

NEG = AR.NEG
ALPHA, OMEGA, BETA = 0.8, 0.5, -0.3


def _mods():
    return S.package("engine", "metrics", "criterions.asg", "lexicon:Lexicon", "lm:NGramLM")


def pack(spellings, C, garbage):
    """the device's Lexicon of a reference lexicon {raw spelling: word id}: for (C, garbage), or (C + 1, C) without one"""
    Lexicon = _mods()[3]
    by_id = sorted(spellings, key=spellings.get)
    assert [spellings[s] for s in by_id] == list(range(len(by_id)))
    return Lexicon(by_id, C, garbage) if garbage is not None else Lexicon(by_id, C + 1, C)


def reference(x, Wt, W, K, nbest, spellings, garbage, ref_lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True):
    """per utterance the reference's hyps; asserts the margins, so that no utterance is left out of a comparison"""
    search = lambda b: AX.beam_search(x[b], Wt, W, K, nbest, spellings, garbage, ref_lm, alpha, omega, beta, eos)
    return [res[0] for res in S.margins_ok(search, x.shape[0])]


def device(x, Wt, W, K, nbest, lex, garbage, lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True, normalize=False, drop=None,
           num_replabels=0):
    E = _mods()[0]
    xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
    kw = {} if lm is None else dict(lm=lm, lm_weight=alpha, lm_eos=eos)
    hyps, scores = E.asg_beam_search_lexicon(xd, Wd, lex, garbage, W, K, nbest, normalize=normalize, drop=drop,
                                             num_replabels=num_replabels, word_bonus=omega, length_bonus=beta, **kw)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, Wt, W, K, nbest, spellings, garbage, lm, ref_lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True):
    lex = pack(spellings, x.shape[2], garbage)
    want = reference(x, Wt, W, K, nbest, spellings, garbage, ref_lm, alpha, omega, beta, eos)
    seqs, raw = device(x, Wt, W, K, nbest, lex, garbage, lm, alpha, omega, beta, eos)
    nseqs, normed = device(x, Wt, W, K, nbest, lex, garbage, lm, alpha, omega, beta, eos, normalize=True)
    assert nseqs == seqs  # (the shift never changes the search)

    def whole_words(b, r, seq):
        at = AX.segment(spellings, garbage, seq)
        assert at is not None and at[1] == (), (b, r, seq)

    S.assert_ranks(want, seqs, raw, normed, log_denominator(x, Wt), nbest, check=whole_words)
    return want, seqs, raw


def universe(N, R, use_garbage):
    """(C, garbage class or None, the separator's token index)"""
    return N + R + int(use_garbage), (N + R if use_garbage else None), N - 1


def random_words(rs, N, V, longest):
    """V different seeded random words as token index lists: 1 .. longest tokens that are not the separator N - 1,
    then the separator -- prefix-free by construction, and no word starts with the token a word ends in"""
    found = set()
    for _ in range(200 * V):
        found.add(tuple(int(rs.randint(N - 1)) for _ in range(1 + rs.randint(longest))) + (N - 1,))
        if len(found) == V:
            return [list(w) for w in sorted(found)]
    raise AssertionError("not enough different words at this size")


def favour(frames, C, seed, hi=8.0):
    """[1, T, C]: frame t favours class frames[t] by +hi on N(0, 0.3^2) noise"""
    x = (np.random.RandomState(seed).randn(1, len(frames), C) * 0.3).astype(np.float32)
    for t, c in enumerate(frames):
        x[0, t, c] += hi
    return x


# (T, tokens N, W, K, B, words, longest word without its separator): a single frame; K below C; K = C with merges;
# 1984 entries per frame -- the 1024-thread instantiation and the radix select; the training shape's width
SHAPES = [(1, 3, 1, 2, 2, 3, 2), (12, 5, 4, 3, 3, 6, 3), (40, 9, 8, 9, 3, 20, 3), (64, 30, 64, 30, 2, 100, 3),
          (120, 100, 16, 32, 2, 300, 2)]
VARIANTS = {"n1-bigram": (1.0, 2), "n3-nolm": (3.0, 0), "spelled-trigram": (None, 3)}


def parity_case(T, N, W, K, B, V, longest, R, use_garbage, variant):
    """(x, Wt, C, garbage, {raw spelling: word id}, ARPA text or None) of a parity case: everything seeded by the case"""
    scale, order = VARIANTS[variant]
    C, garbage, _ = universe(N, R, use_garbage)
    seed = 7907 * T + 37 * N + W + 17 * R + 29 * int(use_garbage) + 1000 * order
    rs = np.random.RandomState(seed)
    spellings = AX.raw_lexicon(random_words(rs, N, V, longest), R)
    text = LR.random_arpa(rs, names_of(V), order, 0.02 if V >= 100 else 0.3) if order else None
    x = emissions(seed + 1, B, T, C, scale) if scale else spelled(seed + 1, B, T, C, spellings, garbage)
    return x, transitions(seed + 2, C), C, garbage, spellings, text


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("use_garbage", [True, False])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("T,N,W,K,B,V,longest", SHAPES, ids=lambda v: str(v))
def test_random_lexicons_and_word_lms_against_the_reference(tmp_path, T, N, W, K, B, V, longest, R, use_garbage, variant):
    x, Wt, C, garbage, spellings, text = parity_case(T, N, W, K, B, V, longest, R, use_garbage, variant)
    lm, ref_lm = make_lms(tmp_path, text, V)
    _, seqs, raw = compare(x, Wt, W, K, min(W, 3), spellings, garbage, lm, ref_lm)
    if variant.startswith("spelled") and T >= 12:
        assert all(raw[b, 0] > NEG and AX.segment(spellings, garbage, h[0])[0] for b, h in enumerate(seqs))  # (whole words survive)


# ------------------------------------------------------------------------------------------------------------------
# edges, in the universe of three tokens a, b, | with one replabel and the garbage: r0 = 0, a = 1, b = 2, | = 3, G = 4
# ------------------------------------------------------------------------------------------------------------------
R0, A_, B_, SEP, G_ = 0, 1, 2, 3, 4
C5 = 5
ZERO = np.zeros((C5 + 1, C5), np.float32)


def test_garbage_inside_a_word_keeps_the_node():
    spellings = {(A_, B_, SEP): 0}
    x = favour([A_, A_, G_, B_, G_, G_, SEP], C5, 500)
    _, seqs, _ = compare(x, transitions(501, C5), 8, C5, 3, spellings, G_, None, None)
    assert seqs[0][0] == (A_, G_, B_, G_, SEP)
    mapped, _ = device(x, transitions(501, C5), 8, C5, 3, pack(spellings, C5, G_), G_, None, drop=G_, num_replabels=1)
    assert mapped[0][0] == (0, 1, 2)


def test_a_doubled_letter_is_found_through_its_replabel_arc_only():
    """`aa|` is raw a, r0, |.  Emissions that spell it that way find it; emissions that favour raw a, G, a, | -- which
    unpacks to the same tokens, and which the plain ASG search returns -- do not: that form does not walk the trie"""
    E = _mods()[0]
    spellings = {(A_, R0, SEP): 0, (B_, SEP): 1}
    Wt = transitions(511, C5)
    x = np.concatenate([favour([A_, R0, R0, SEP], C5, 510), favour([A_, G_, A_, SEP], C5, 512)])
    want, seqs, _ = compare(x, Wt, 8, C5, 3, spellings, G_, None, None)
    assert seqs[0][0] == (A_, R0, SEP)
    mapped, _ = device(x, Wt, 8, C5, 3, pack(spellings, C5, G_), G_, None, drop=G_, num_replabels=1)
    assert mapped[0][0] == (0, 0, 2)
    other = (A_, G_, A_, SEP)
    assert AX.segment(spellings, G_, other) is None and AR.unpack(other, G_, 1) == [0, 0, 2]
    plain, _ = E.asg_beam_search(torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda(), 8, C5, 1, normalize=False)
    assert tuple(plain[1][0].tolist()) == other  # (the emissions do favour it)
    assert other not in seqs[1] and seqs[1] == [h for h, _ in want[1]]


def test_a_one_label_word():
    spellings = {(B_,): 0, (A_, SEP): 1}
    x = favour([B_, G_, B_, A_, SEP], C5, 520)
    _, seqs, _ = compare(x, transitions(521, C5), 8, C5, 3, spellings, G_, None, None)
    assert seqs[0][0] == (B_, G_, B_, A_, SEP) and AX.segment(spellings, G_, seqs[0][0]) == ([0, 0, 1], ())


@pytest.mark.parametrize("order", [0, 2])
def test_a_root_with_a_single_arc(tmp_path, order):
    spellings = {(A_, B_, SEP): 0, (A_, SEP): 1, (A_, R0, SEP): 2}
    text = LR.random_arpa(np.random.RandomState(530), names_of(3), order, 0.5) if order else None
    lm, ref_lm = make_lms(tmp_path, text, 3)
    Wt = transitions(531, C5)
    compare(emissions(532, 4, 24, C5, 1.0), Wt, 8, 4, 3, spellings, G_, lm, ref_lm)
    _, seqs, raw = compare(spelled(533, 4, 24, C5, spellings, G_), Wt, 8, 4, 3, spellings, G_, lm, ref_lm)
    assert (raw[:, 0] > NEG).all() and all(AX.segment(spellings, G_, h[0])[0] for h in seqs)


def test_a_lexicon_over_every_class_but_the_garbage_is_the_plain_search():
    """one-label words for r0, a, b and |: every raw sequence is a sequence of words, and without an LM or a bonus
    the search is the ASG search -- the same sequences, scores that differ by added zeros at most"""
    E = _mods()[0]
    spellings = {(c,): c for c in range(C5 - 1)}
    x, Wt = emissions(540, 4, 30, C5, 1.0), transitions(541, C5)
    _, seqs, raw = compare(x, Wt, 8, 4, 3, spellings, G_, None, None, omega=0.0, beta=0.0)
    hyps, scores = E.asg_beam_search(torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda(), 8, 4, 3, normalize=False)
    assert [[tuple(s.tolist()) for s in h] for h in hyps] == seqs
    assert np.abs(scores.numpy() - raw).max() <= 1e-12


def small_case(seed, T=30, N=6, R=1, use_garbage=True, B=4, V=20, order=2, keep=0.3, scale=1.0, eos=True):
    rs = np.random.RandomState(seed)
    C, garbage, _ = universe(N, R, use_garbage)
    spellings = AX.raw_lexicon(random_words(rs, N, V, 3), R)
    text = LR.random_arpa(rs, names_of(V), order, keep, eos=eos) if order else None
    return emissions(seed + 1, B, T, C, scale), transitions(seed + 2, C), C, garbage, spellings, text


def test_lexicon_alone_is_the_lexicon_with_a_silent_lm(tmp_path):
    """alpha = 0, omega = 0 and an LM that knows every word (all unigrams: no step is -inf): every LM term is 0, the
    terms are formed by the same operations, so sequences and scores are identical to the search without an LM"""
    for T, N, W, K, B, V in ((30, 6, 16, 8, 4, 20), (40, 20, 64, 22, 2, 60)):
        x, Wt, C, garbage, spellings, text = small_case(600 + N, T, N, 1, True, B, V, order=3)
        x = np.concatenate([x[:B // 2], spelled(601 + N, B - B // 2, T, C, spellings, garbage)])
        lex, (lm, _) = pack(spellings, C, garbage), make_lms(tmp_path, text, V)
        for eos in (True, False):
            with_lm = device(x, Wt, W, K, 3, lex, garbage, lm, alpha=0.0, omega=0.0, eos=eos)
            alone = device(x, Wt, W, K, 3, lex, garbage, None, omega=0.0)
            assert with_lm[0] == alone[0] and with_lm[1].tobytes() == alone[1].tobytes()
            assert any(len(s) for h in alone[0] for s in h)


def test_a_first_frame_in_which_no_word_can_start():
    """the first class of every word is -inf in frame 0.  Where the garbage is a candidate there the hypotheses live on
    through it; where it is not -- K = 3, the garbage the lowest finite score -- no candidate leaves the root and the
    utterance decodes to nothing"""
    N, R = 7, 1  # six letters and the separator: the words start with the first three letters only
    C, garbage, _ = universe(N, R, True)
    spellings = AX.raw_lexicon([[0, 3, 6], [1, 4, 6], [0, 0, 6], [1, 6], [2, 5, 3, 6], [0, 4, 4, 6], [2, 6]], R)
    x, Wt = emissions(610, 3, 20, C, 1.0), transitions(611, C)
    first = sorted({s[0] for s in spellings})
    assert first == [1, 2, 3] and len(first) + 1 + 3 <= C  # (three candidates that are neither of them nor the garbage)
    x[:, 0, first] = -np.inf
    through = x.copy()
    through[:, 0, garbage] += 5.0
    _, seqs, raw = compare(through, Wt, 8, C, 3, spellings, garbage, None, None)
    assert (raw[:, 0] > NEG).all() and all(h[0][0] == garbage for h in seqs)
    x[:, 0, garbage] = -20.0
    want, seqs, raw = compare(x, Wt, 8, 3, 3, spellings, garbage, None, None)
    assert want == [[((), NEG)] * 3] * 3 and seqs == [[(), (), ()]] * 3 and (raw == NEG).all()


def test_every_final_hypothesis_inside_a_word_gives_empty_ranks():
    """fewer frames than the shortest word has classes, and no garbage to wait in: every hypothesis of the final beam
    stands inside a word.  With a garbage class the all-garbage sequence is left: no word, a finite score"""
    C, garbage, _ = universe(4, 1, False)  # r0, a, b, c, |
    spellings = {(1, 2, 4): 0, (2, 3, 4): 1, (1, 0, 4): 2, (3, 1, 2, 4): 3}
    x, Wt = emissions(620, 3, 2, C, 1.0), transitions(621, C)
    want, seqs, raw = compare(x, Wt, 8, C, 3, spellings, garbage, None, None)
    assert want == [[((), NEG)] * 3] * 3 and seqs == [[(), (), ()]] * 3 and (raw == NEG).all()
    C, garbage, _ = universe(4, 1, True)
    x, Wt = emissions(622, 3, 2, C, 1.0), transitions(623, C)
    _, seqs, raw = compare(x, Wt, 64, C, 3, spellings, garbage, None, None)  # (6 + 30 prefixes: none is pruned)
    assert all(h == [(garbage,), (), ()] for h in seqs) and np.isfinite(raw[:, 0]).all() and (raw[:, 1:] == NEG).all()


def test_a_word_the_lm_cannot_follow_is_never_emitted(tmp_path):
    """The arcs of one word are taken out of the LM's pack by constructing it directly (the loader would refuse a word
    without a unigram).  The emissions spell that word, so the search with the whole LM emits it; without its arcs
    step() is -inf from every state and no hypothesis may complete it."""
    NGramLM = _mods()[4]
    V, gone = 20, 5
    _, Wt, C, garbage, spellings, text = small_case(630, V=V)
    lex = pack(spellings, C, garbage)
    by_id = sorted(spellings, key=spellings.get)
    x = spelled(631, 4, 30, C, {by_id[gone]: 0, by_id[3]: 1}, garbage)
    whole, _ = make_lms(tmp_path, text, V)
    words_of = lambda s: AX.segment(spellings, garbage, s)[0]
    assert any(gone in words_of(s) for h in device(x, Wt, 16, 6, 3, lex, garbage, whole)[0] for s in h)
    keep = whole.arc_label != gone
    ptr = np.concatenate([[0], np.cumsum([keep[whole.arc_ptr[s]:whole.arc_ptr[s + 1]].sum() for s in range(whole.num_states)])])
    lm = NGramLM(V + 1, V, ptr, whole.arc_label[keep], whole.arc_next[keep], whole.arc_w[keep], whole.bo_next, whole.bo_w,
                 start=whole.start, order=2)
    assert lm.num_arcs < whole.num_arcs and lm.score([gone]) == -math.inf
    cut = "\n".join(l for l in text.split("\n") if f"w{gone}" not in l.split())  # (the reference does not count its sections)
    _, seqs, _ = compare(x, Wt, 16, 6, 3, spellings, garbage, lm, LR.ArpaLM(cut, names_of(V), V))
    assert not any(gone in words_of(s) for h in seqs for s in h)
    assert any(len(s) > 0 for h in seqs for s in h)


def test_word_bonus_extremes(tmp_path):
    """omega = +50 outweighs every other term of a word: the best hypotheses complete at least the words they did, and
    more in all.  omega = -50: no word is worth completing -- the all-garbage sequence or nothing is left"""
    x, Wt, C, garbage, spellings, text = small_case(640, T=20, V=20, order=2)
    x[2:] = spelled(641, 2, 20, C, spellings, garbage)
    lm, ref_lm = make_lms(tmp_path, text, 20)
    count = lambda seqs: [len(AX.segment(spellings, garbage, h[0])[0]) for h in seqs]
    _, plain, _ = compare(x, Wt, 16, 8, 3, spellings, garbage, lm, ref_lm)
    _, seqs, _ = compare(x, Wt, 16, 8, 3, spellings, garbage, lm, ref_lm, omega=50.0)
    assert all(n >= p for n, p in zip(count(seqs), count(plain))) and sum(count(seqs)) >= sum(count(plain)) + 4
    for word_lm in ((lm, ref_lm), (None, None)):
        _, seqs, _ = compare(x, Wt, 16, 8, 3, spellings, garbage, *word_lm, omega=-50.0)
        assert all(set(s) <= {garbage} for h in seqs for s in h)


def test_an_order_three_word_lm_backs_off(tmp_path):
    rs = np.random.RandomState(650)
    N, R, V = 7, 2, 12
    C, garbage, _ = universe(N, R, True)
    spellings = AX.raw_lexicon(random_words(rs, N, V, 2), R)
    text = LR.random_arpa(rs, names_of(V), 3, 0.25)
    lm, ref_lm = make_lms(tmp_path, text, V)
    assert lm.order == 3
    x = spelled(651, 4, 40, C, spellings, garbage)
    _, seqs, _ = compare(x, transitions(652, C), 16, 8, 3, spellings, garbage, lm, ref_lm)
    backed = 0
    for h in seqs:  # the best hypotheses take words whose trigram and bigram are not in the file
        s = lm.start
        for v in AX.segment(spellings, garbage, h[0])[0]:
            direct = v in lm.arc_label[lm.arc_ptr[s]:lm.arc_ptr[s + 1]].tolist()
            backed += (not direct) and lm.bo_next[s] >= 0
            s = lm.step(s, v)[1]
    assert backed >= 4


def test_a_forbidden_transition_on_a_trie_arc():
    """a -> b is -inf: the word `ab|` is still found, around the transition -- through the garbage, which the trie does
    not see"""
    spellings = {(A_, B_, SEP): 0, (B_, SEP): 1}
    Wt = transitions(660, C5)
    Wt[1 + B_, A_] = -np.inf
    x = np.concatenate([favour([A_, B_, B_, SEP, SEP], C5, 661), emissions(662, 3, 12, C5, 1.0)[:, :5]])
    x[0, 1, G_] += 6.0  # (the garbage second in the frame behind a)
    _, seqs, raw = compare(x, Wt, 8, C5, 3, spellings, G_, None, None)
    assert all(not (l == A_ and c == B_) for h in seqs for s in h for l, c in zip(s, s[1:]))
    assert seqs[0][0] == (A_, G_, B_, SEP) and raw[0, 0] > NEG


def bound_case(seed):
    """A full beam (W = 4) that holds a hypothesis whose last label has left the candidates (K = 2, the garbage not among
    them) and none of whose extensions is in the trie, while its first own extension -- if it existed -- would rank
    above the W-th best entry of the frame: a bound that took it for an entry would cut entries that survive.
    Returns (x, Wt, C, garbage, spellings, the frames at which that happens); the seeds were searched for on the host."""
    N, R, W, K = 5, 1, 4, 2
    C, garbage, _ = universe(N, R, True)
    rs = np.random.RandomState(5)
    spellings = AX.raw_lexicon(random_words(rs, N, 6, 2), R)
    x, Wt = emissions(seed, 1, 14, C, 2.0), transitions(seed + 1, C)
    hits = []

    def on_frame(t, beam, cand, extension, merged, entries):
        classes = [c for c, _ in cand]
        if len(beam) < W or len(entries) < W or garbage in classes:
            return
        # the bound as section 21 forms it, blind to the trie: the W-th best of one key per hypothesis -- its stay, or
        # its first own extension whether or not that exists
        stays = {idx: s for s, idx, _, _, _ in entries if idx < len(beam)}
        keys, absent = [], False
        for i, (pre, p, part, hist) in enumerate(beam):
            if pre and pre[-1] in classes:
                keys.append(stays.get(i, NEG))
                continue
            own = [c for q, c in enumerate(classes) if not merged[i][q]]
            if not own:
                keys.append(NEG)
                continue
            keys.append((AR.clean(x[0][t])[own[0]] + AR.transition(Wt, pre[-1] if pre else None, own[0])) + p + min(BETA, 0.0))
            absent = absent or all(extension(i, c)[0] == NEG for c in own)
        if absent and min(keys) > entries[W - 1][0]:  # (that bound would cut the true W-th best entry)
            hits.append(t)

    AX.beam_search(x[0], Wt, W, K, 3, spellings, garbage, None, 1.0, OMEGA, BETA, True, on_frame=on_frame)
    return x, Wt, C, garbage, spellings, hits


@pytest.mark.parametrize("seed", [30, 59, 83, 127])
def test_the_bound_counts_only_entries_that_exist(seed):
    x, Wt, C, garbage, spellings, hits = bound_case(seed)
    assert hits, "the case is not what it says"
    _, seqs, raw = compare(x, Wt, 4, 2, 3, spellings, garbage, None, None)
    assert raw[0, 0] > NEG


def test_normalised_scores_against_the_loss_of_the_raw_hypothesis(tmp_path):
    """Where nothing is pruned (W = 64, K = C, a handful of frames: the pin of tests/test_asg_beam_lexicon_abi.py) the
    normalised score is minus the criterion's loss of the raw sequence plus rule 6's terms, at the loss bar; where the
    beam prunes (W = 4, K = 3, 30 frames) it is a lower bound of that."""
    asg = _mods()[2]

    def rule6(xd, Wd, b, seq, spellings, garbage, ref_lm, eos):
        # (ASGLoss averages over its batch, asg.py:116-121: an utterance's own loss is that of a batch of one)
        words = AX.segment(spellings, garbage, seq)[0]
        lm_term = ALPHA * ref_lm.score(words, eos=eos) if ref_lm else 0.0
        return (-float(asg.ASGLoss(xd[b:b + 1], Wd, [list(seq)], "none")) + lm_term + OMEGA * len(words)
                + BETA * sum(1 for c in seq if c != garbage))

    for (C, T, garbage, spellings), order in (((4, 5, 3, {(1, 2): 0, (2,): 1, (1, 0): 2}), 2),
                                              ((4, 6, None, {(1, 3): 0, (2, 0, 3): 1, (2, 3): 2}), 0),
                                              ((3, 7, 2, {(1, 0): 0}), 2)):
        V = len(spellings)
        text = LR.random_arpa(np.random.RandomState(670 + C + T), names_of(V), order, 0.6) if order else None
        lm, ref_lm = make_lms(tmp_path, text, V)
        x, Wt = emissions(671 + T, 4, T, C, 1.0), transitions(672 + T, C)
        lex = pack(spellings, C, garbage)
        xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
        for eos in (True, False):
            seqs, normed = device(x, Wt, 64, C, 3, lex, garbage, lm, eos=eos, normalize=True)
            checked = 0
            for b in range(4):
                for r in range(3):
                    if normed[b, r] == NEG:
                        continue
                    want = rule6(xd, Wd, b, seqs[b][r], spellings, garbage, ref_lm, eos)
                    assert abs(normed[b, r] - want) <= 1e-4 * abs(want) + 2e-5, (C, T, b, r, normed[b, r], want)
                    checked += 1
            assert checked >= 4
    x, Wt, C, garbage, spellings, text = small_case(680, order=2)
    lm, ref_lm = make_lms(tmp_path, text, 20)
    x[2:] = spelled(681, 2, 30, C, spellings, garbage)
    seqs, normed = device(x, Wt, 4, 3, 1, pack(spellings, C, garbage), garbage, lm, normalize=True)
    xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
    assert (normed[:, 0] > NEG).any()
    for b in range(4):
        if normed[b, 0] > NEG:
            want = rule6(xd, Wd, b, seqs[b][0], spellings, garbage, ref_lm, True)
            assert normed[b, 0] <= want + 1e-4 * abs(want) + 2e-5, (b, normed[b, 0], want)


def test_the_same_call_twice_is_bit_identical(tmp_path):
    x, Wt, C, garbage, spellings, text = small_case(690, T=40, N=20, B=4, V=60, order=2)
    x[2:] = spelled(691, 2, 40, C, spellings, garbage)
    lm, _ = make_lms(tmp_path, text, 60)
    lex = pack(spellings, C, garbage)
    a = device(x, Wt, 64, 22, 3, lex, garbage, lm, normalize=True)
    b = device(x, Wt, 64, 22, 3, lex, garbage, lm, normalize=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    c = device(x, Wt, 64, 22, 3, lex, garbage, lm, normalize=True, drop=garbage, num_replabels=1)
    d = device(x, Wt, 64, 22, 3, lex, garbage, lm, normalize=True, drop=garbage, num_replabels=1)
    assert c[0] == d[0] and c[1].tobytes() == a[1].tobytes() == d[1].tobytes()  # (the mapping never touches the scores)


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
TOKENS = list("abcdefg") + ["|"]


def module_case(tmp_path, R, use_garbage, seed):
    """(criterion on the device, its lexicon, the same as a reference dict, word LMs, emissions, transitions)"""
    asg = _mods()[2]
    N = len(TOKENS)
    crit = asg.ASG(N, num_replabels=R, use_garbage=use_garbage).cuda()
    rs = np.random.RandomState(seed)
    token_words = random_words(rs, N, 15, 3) + [[0, 0, N - 1], [1, 2, 2, 2, N - 1]]  # (a doubled and a tripled letter)
    token_words = [list(w) for w in sorted({tuple(w) for w in token_words})]
    words = ["".join(TOKENS[t] for t in w[:-1]) for w in token_words]
    lex = crit.lexicon(words, TOKENS, wordsep="|")
    spellings = AX.raw_lexicon(token_words, R)
    assert lex.spellings == sorted(spellings, key=spellings.get)  # (the module packs as the reference does)
    V = len(words)
    text = LR.random_arpa(rs, names_of(V), 2, 0.3)
    lm, ref_lm = make_lms(tmp_path, text, V)
    C = crit.N
    x = np.concatenate([emissions(seed + 1, 2, 40, C, 1.0), spelled(seed + 2, 2, 40, C, spellings, crit.garbage_idx)])
    Wt = transitions(seed + 3, C)
    with torch.no_grad():
        crit.transitions.copy_(torch.from_numpy(Wt))
    return crit, lex, spellings, lm, ref_lm, x, Wt


@pytest.mark.parametrize("R,use_garbage", [(1, True), (2, True), (1, False), (2, False)])
def test_module_maps_raw_results_and_names_their_words(tmp_path, R, use_garbage):
    M = _mods()[1]
    crit, lex, spellings, lm, ref_lm, x, Wt = module_case(tmp_path, R, use_garbage, 700 + 10 * R + int(use_garbage))
    garbage, B = crit.garbage_idx, x.shape[0]
    xd = torch.from_numpy(x).cuda()
    kw = dict(lexicon=lex, lm=lm, lm_weight=ALPHA, word_bonus=OMEGA, length_bonus=BETA)
    hyps, scores = crit.beam_search(xd, beam_size=8, classes_per_frame=6, nbest=3, return_scores=True, **kw)
    assert len(hyps) == B and all(isinstance(h, list) and len(h) == 3 for h in hyps)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (B, 3) and not scores.is_cuda
    assert all(p.dtype == torch.int64 and p.dim() == 1 and not p.is_cuda for h in hyps for p in h)
    want = reference(x, Wt, 8, 6, 3, spellings, garbage, ref_lm)
    raw, normed = device(x, Wt, 8, 6, 3, lex, garbage, lm, normalize=True)
    assert raw == [[h for h, _ in hyps_b] for hyps_b in want]
    assert (scores.numpy() == normed).all()
    found = 0
    for b in range(B):
        # mapped on the device = the raw results unpacked on the host; the words are the reference's
        assert [p.tolist() for p in hyps[b]] == [AR.unpack(s, garbage, R) for s in raw[b]], b
        for p, s in zip(hyps[b], raw[b]):
            assert crit.words(lex, p) == AX.segment(spellings, garbage, s)[0]
            found += len(crit.words(lex, p))
    assert found >= 6
    best = crit.beam_search(xd, beam_size=8, classes_per_frame=6, **kw)
    assert [p.tolist() for p in best] == [h[0].tolist() for h in hyps]
    # other floating dtypes are converted, tensors that are not on a GPU are uploaded: the same search
    for other in (torch.from_numpy(x), xd.double()):
        again = crit.beam_search(other, beam_size=8, classes_per_frame=6, nbest=3, **kw)
        assert [[p.tolist() for p in h] for h in again] == [[p.tolist() for p in h] for h in hyps]
    # errors(beam_size=, lexicon=) counts what beam_search predicts
    rs = np.random.RandomState(71)
    targets = [rs.randint(0, len(TOKENS), size=n).tolist() for n in (7, 0, 12, 3)]
    counter = M.ErrorCounter(wordsep=len(TOKENS) - 1)
    for W, K, opts in ((8, 6, kw), (1, crit.N, dict(lexicon=lex)), (16, 4, dict(lexicon=lex, lm=lm, lm_eos=False))):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K, **opts)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K, **opts) == counter(pred, targets)


@pytest.mark.parametrize("R,use_garbage", [(1, True), (2, False)])
def test_without_a_lexicon_the_calls_are_what_they_were(tmp_path, R, use_garbage):
    E, M = _mods()[:2]
    crit, _, _, _, _, x, Wt = module_case(tmp_path, R, use_garbage, 720 + R)
    xd, Wd = torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda()
    hyps, scores = crit.beam_search(xd, beam_size=8, classes_per_frame=6, nbest=3, return_scores=True)
    direct, want = E.asg_beam_search(xd, Wd, 8, 6, 3, normalize=True, drop=crit.garbage_idx, num_replabels=R)
    assert [[p.tolist() for p in h] for h in hyps] == [[p.tolist() for p in h] for h in direct]
    assert scores.numpy().tobytes() == want.numpy().tobytes()
    best = crit.beam_search(xd)
    direct, _ = E.asg_beam_search(xd, Wd, 16, min(crit.N, 32), 1, normalize=True, drop=crit.garbage_idx, num_replabels=R)
    assert [p.tolist() for p in best] == [h[0].tolist() for h in direct]
    counter = M.ErrorCounter(wordsep=len(TOKENS) - 1)
    targets = [[0, 1, 7], [], [2, 2, 7, 3], [1]]
    assert crit.errors(xd, targets, counter, beam_size=16) == counter(best, targets)
    assert crit.errors(xd, targets, counter) == counter(crit.viterbi(xd), targets)
