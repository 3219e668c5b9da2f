"""Transducer beam search with a lexicon and a word-level LM on the device (csrc/beam_kernels.hip:
wfl_transducer_beam_search_lexicon behind engine.transducer_beam_search_lexicon, Transducer.beam_search(lexicon=) and
Transducer.errors(beam_size=, lexicon=)) against its restatement in plain Python
(tests/transducer_beam_lexicon_reference.py, itself pinned to a brute-force enumeration in
tests/test_transducer_beam_lexicon_abi.py).

Acceptance of every comparison: the token sequences of all returned ranks are equal; unnormalised scores agree to
1e-9 max(1, |s|) -- both sides are float64 and differ in libm rounding only; normalised scores agree at the project's
loss bar (1e-4 |want| + 2e-5) against a float64 normaliser computed with torch, independently of the library, the
device's logz being float32; every returned sequence segments into whole words.  An utterance whose smallest selection
margin in the reference is below 1e-9 could legitimately come out differently: the seeds are fixed so that there is none,
and every comparison asserts that.  On emissions that spell words the reference returns at least one word at rank 0 for
at least three quarters of the utterances: asserted too, a comparison of empty beams shows nothing.

A universe is (C classes, the blank's class): the tokens are the other classes in ascending order, the last of them the
word separator.  Lexicons are written out or seeded random token sequences; word LMs are seeded random ARPA texts over
the word names, written into tmp_path and loaded through NGramLM.from_arpa(path, words, blank=len(words)) for the
device and read by beam_lm_reference.ArpaLM for the reference."""
import os

import numpy as np
import pytest
import torch

import beam_lexicon_reference as XR
import beam_lm_reference as LR
import beam_support as S
import transducer_beam_lexicon_reference as TX
import transducer_beam_reference as TR
from beam_support import emissions, log_normaliser, names_of, transitions
from beam_support import word_lms as make_lms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = TR.NEG
ALPHA, OMEGA, BETA = 0.8, 0.5, -0.3
TOPOLOGIES = pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])


def _mods():
    return S.package("engine", "metrics", "criterions.transducer", "lexicon:Lexicon", "lm:NGramLM")


def pack(spellings, C, blank):
    """the device's Lexicon of a reference lexicon {token tuple: word id}"""
    Lexicon = _mods()[3]
    by_id = sorted(spellings, key=spellings.get)
    assert [spellings[s] for s in by_id] == list(range(len(by_id)))
    return Lexicon(by_id, C, blank)


def count_words(spellings, seq):
    at = XR.segment(spellings, seq)
    return len(at[0]) if at is not None and at[1] == () else None


def reference(x, Wt, blank, forced, W, K, nbest, spellings, ref_lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True, spells=False,
              on_frame=None):
    """per utterance the reference's hyps; asserts the margins, so that no utterance is left out of a comparison, and --
    `spells`: the emissions spell words -- that a word is found at rank 0 for three quarters of the utterances"""

    def search(b):
        hook = None if on_frame is None else (lambda *a: on_frame(b, *a))
        return TX.beam_search(x[b], Wt, blank, forced, W, K, nbest, spellings, ref_lm, alpha, omega, beta, eos, on_frame=hook)

    found = (lambda hyps: (count_words(spellings, hyps[0][0]) or 0) >= 1) if spells else None
    return [res[0] for res in S.margins_ok(search, x.shape[0], found)]


def device(x, Wt, blank, forced, W, K, nbest, lex, lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True, normalize=False):
    E = _mods()[0]
    xd = torch.from_numpy(x).cuda()
    Wd = None if Wt is None else torch.from_numpy(Wt).cuda()
    kw = {} if lm is None else dict(lm=lm, lm_weight=alpha, lm_eos=eos)
    hyps, scores = E.transducer_beam_search_lexicon(xd, Wd, blank, lex, forced, W, K, nbest, normalize=normalize, word_bonus=omega,
                                                    length_bonus=beta, **kw)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, Wt, blank, forced, W, K, nbest, spellings, lm, ref_lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True, spells=False,
            on_frame=None):
    lex = pack(spellings, x.shape[2], blank)
    want = reference(x, Wt, blank, forced, W, K, nbest, spellings, ref_lm, alpha, omega, beta, eos, spells, on_frame)
    seqs, raw = device(x, Wt, blank, forced, W, K, nbest, lex, lm, alpha, omega, beta, eos)
    nseqs, normed = device(x, Wt, blank, forced, W, K, nbest, lex, lm, alpha, omega, beta, eos, normalize=True)
    assert nseqs == seqs  # (the shift never changes the search)

    def whole_words(b, r, seq):
        assert count_words(spellings, seq) is not None, (b, r, seq)

    S.assert_ranks(want, seqs, raw, normed, log_normaliser(x, Wt), nbest, blank, whole_words)
    return want, seqs, raw


def tokens_of(C, blank):
    """the classes other than the blank, ascending: the last is the separator"""
    return [c for c in range(C) if c != blank]


def random_words(rs, C, blank, V, longest, letters=None):
    """{token tuple: word id} of V different seeded random words: 1 .. longest letters (the first `letters` tokens, all but
    the separator by default), then the separator -- prefix-free by construction"""
    toks = tokens_of(C, blank)
    sep, alphabet = toks[-1], toks[:-1][:letters]
    found = set()
    for _ in range(200 * V):
        found.add(tuple(alphabet[rs.randint(len(alphabet))] for _ in range(1 + rs.randint(longest))) + (sep,))
        if len(found) == V:
            return {w: v for v, w in enumerate(sorted(found))}
    raise AssertionError("not enough different words at this size")


def spelled(seed, B, T, C, blank, spellings, hi=8.0, noise=0.5, run=2):
    """emissions that spell a sentence of lexicon words in a way both topologies accept: a blank frame first, every
    token for one to `run` frames with one blank frame behind it, blanks for what is left of the T frames; +hi on
    N(0, noise^2)"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, T, C) * noise).astype(np.float32)
    words = sorted(spellings, key=spellings.get)
    for b in range(B):
        frames, misses = [blank], 0
        while misses < 8:  # (a word that does not fit any more: another draw, a few times)
            more = []
            for c in words[rs.randint(len(words))]:
                more += [c] * int(rs.randint(1, run + 1)) + [blank]
            if len(frames) + len(more) > T:
                misses += 1
                continue
            frames += more
        for t in range(T):
            x[b, t, frames[t] if t < len(frames) else blank] += hi
    return x


# ------------------------------------------------------------------------------------------------------------------
# the shapes of the issue, (T, C, W, K, B)
# ------------------------------------------------------------------------------------------------------------------
def test_one_frame():
    """(1, 3, 1, 2, 4).  Forced: no extension in frame 0, the empty sequence is all there is.  Optional: a one-token
    word may be returned, a token that only begins a word may not."""
    blank = 2
    spellings = {(0,): 0, (1, 0): 1}
    x = np.array([[[3.0, 0.0, 1.0]], [[0.0, 3.0, 1.0]], [[0.0, 1.0, 3.0]], [[1.0, -np.inf, 0.0]]], np.float32)
    Wt = transitions(100, 3)
    want, seqs, raw = compare(x, Wt, blank, True, 1, 2, 1, spellings, None, None)
    assert seqs == [[()]] * 4 and (raw[:, 0] > NEG).all()  # (the blank alone)
    want, seqs, raw = compare(x, Wt, blank, False, 1, 2, 1, spellings, None, None)
    assert seqs[:3] == [[(0,)], [()], [()]] and seqs[3] in ([(0,)], [()])  # (one-token words only)
    assert raw[1, 0] == NEG  # (the beam of one held (1,): inside a word, nothing is left)
    assert raw[0, 0] > NEG and raw[2, 0] > NEG and raw[3, 0] > NEG
    for forced in (False, True):
        _, seqs, _ = compare(x, None, blank, forced, 1, 2, 1, spellings, None, None)
        assert seqs == ([[()]] * 4 if forced else [[(0,)], [()], [()], [(0,)]])


def case_12(blank_last, order, seed=0):
    """(12, 6, 4, 3, 8) on emissions that spell words: (x, Wt, blank, spellings, ARPA text or None)"""
    T, C, B, V = 12, 6, 8, 6
    blank = C - 1 if blank_last else 0
    rs = np.random.RandomState(1200 + 10 * int(blank_last) + order + 100 * seed)
    spellings = random_words(rs, C, blank, V, 2)
    text = LR.random_arpa(rs, names_of(V), order, 0.5) if order else None
    x = spelled(1201 + 10 * int(blank_last) + order + 100 * seed, B, T, C, blank, spellings, hi=4.0, noise=1.0)
    return x, transitions(1202 + seed, C), blank, spellings, text


@TOPOLOGIES
# (lm_eos belongs to an lm: off only with one)
@pytest.mark.parametrize("order,eos", [(0, True), (2, True), (2, False)], ids=["nolm", "bigram-eos", "bigram-noeos"])
@pytest.mark.parametrize("blank_last", [True, False], ids=["blank-last", "blank-0"])
def test_twelve_frames_with_transitions(tmp_path, blank_last, order, eos, forced):
    x, Wt, blank, spellings, text = case_12(blank_last, order)
    lm, ref_lm = make_lms(tmp_path, text, len(spellings))
    for nbest in (1, 4):
        compare(x, Wt, blank, forced, 4, 3, nbest, spellings, lm, ref_lm, eos=eos, spells=True)


def dense_case(forced):
    """(40, 40, 64, 39, 2): every two-letter word over 12 letters, plus the separator -- 144 words of three tokens"""
    T, C, B = 40, 40, 2
    blank = C - 1
    toks = tokens_of(C, blank)
    sep, letters = toks[-1], toks[:12]
    spellings = {(a, b, sep): 12 * i + j for i, a in enumerate(letters) for j, b in enumerate(letters)}
    x = spelled(4000 + int(forced), B, T, C, blank, spellings, hi=3.0, noise=1.0)
    return x, transitions(4002, C), blank, spellings


@TOPOLOGIES
def test_the_wide_instantiation_and_the_radix_select_on_a_dense_lexicon(forced):
    x, Wt, blank, spellings = dense_case(forced)
    most = [0]

    def on_frame(b, t, beam, cand, extension, merged, entries):
        most[0] = max(most[0], len(entries))

    compare(x, Wt, blank, forced, 64, 39, 3, spellings, None, None, spells=True, on_frame=on_frame)
    assert most[0] > 512, most  # (the select runs only on a list longer than that)


def benchmark_pieces():
    with open(os.path.join(ROOT, "benchmarks", "word_pieces_tokens_1000.txt")) as f:
        tokens = sorted(l.rstrip("\n") for l in f if l.rstrip("\n"))
    g2i = {g: i for i, g in enumerate(sorted(set(c for t in tokens for c in t)))}
    return tokens, g2i


@TOPOLOGIES
def test_the_class_count_of_the_word_piece_recipes(forced):
    """(3, 1001, 4, 64, 1): the lexicon over the recipe's 1000 word pieces, built by word_lexicon(split=)"""
    T = _mods()[2]
    tokens, g2i = benchmark_pieces()
    assert len(tokens) == 1000
    crit = T.Transducer(tokens, g2i, **(dict(blank="forced") if forced else dict(blank="optional", allow_repeats=False)))
    rs = np.random.RandomState(1001)
    table = {}
    # one-piece words over the first half of the pieces and two-piece words that start in the second: prefix-free;
    # written as the pieces' graphemes with a mark between
    for n in (1,) * 40 + (2,) * 40:
        first = int(rs.randint(500)) if n == 1 else 500 + int(rs.randint(500))
        pieces = [tokens[i] for i in [first] + [int(rs.randint(1000)) for _ in range(n - 1)]]
        table["+".join(pieces)] = pieces
    lex = crit.word_lexicon(list(table), split=lambda w: table[w])
    C, blank = 1001, 1000
    assert (lex.num_classes, lex.blank) == (C, blank)
    spellings = {tuple(s): v for v, s in enumerate(lex.spellings)}
    assert XR.is_prefix_free(spellings)
    single = {s: v for s, v in spellings.items() if len(s) == 1}
    x = spelled(1002 + int(forced), 1, 3, C, blank, {s: i for i, s in enumerate(sorted(single))}, hi=6.0, noise=1.0)
    Wt = transitions(1003, C)
    want, seqs, _ = compare(x, Wt, blank, forced, 4, 64, 3, spellings, None, None, spells=True)
    assert crit.words(lex, seqs[0][0]) == [spellings[seqs[0][0]]]


@TOPOLOGIES
def test_two_hundred_utterances_in_one_call(tmp_path, forced):
    """(6, 5, 2, 4, 200)"""
    T, C, B, blank, V = 6, 5, 200, 4, 3
    rs = np.random.RandomState(2000)
    spellings = random_words(rs, C, blank, V, 1)  # (letter, separator: blank l blank | blank fits the six frames)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), 2, 0.5), V)
    x = spelled(2001 + int(forced), B, T, C, blank, spellings, hi=4.0, noise=1.0, run=1)
    compare(x, transitions(2002, C), blank, forced, 2, 4, 2, spellings, lm, ref_lm, spells=True)


def test_without_transitions_the_optional_topology_is_the_ctc_lexicon_search_bit_for_bit(tmp_path):
    E = _mods()[0]
    for (T, C, W, K, B, V), blank, order in (((60, 29, 16, 8, 3, 40), 28, 2), ((40, 40, 64, 39, 2, 60), 0, 0),
                                             ((12, 6, 4, 3, 50, 6), 3, 2)):
        rs = np.random.RandomState(900 + T)
        spellings = random_words(rs, C, blank, V, 2)
        lm, _ = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), order, 0.3) if order else None, V)
        lex = pack(spellings, C, blank)
        x = np.concatenate([emissions(901 + T, B - B // 2, T, C, 1.0), spelled(902 + T, B // 2, T, C, blank, spellings)])
        xd = torch.from_numpy(x).cuda()
        kw = dict(word_bonus=OMEGA, length_bonus=BETA, **({} if lm is None else dict(lm=lm, lm_weight=ALPHA)))
        words = 0
        for normalize in (False, True):
            a_h, a_s = E.transducer_beam_search_lexicon(xd, None, blank, lex, False, W, K, min(3, W), normalize=normalize, **kw)
            c_h, c_s = E.ctc_beam_search(xd, blank, W, K, min(3, W), normalize=normalize, lexicon=lex, **kw)
            assert [[s.tolist() for s in h] for h in a_h] == [[s.tolist() for s in h] for h in c_h]
            assert a_s.numpy().tobytes() == c_s.numpy().tobytes()
            words += sum(len(h[0]) > 0 for h in a_h)
        assert words >= B // 2


# ------------------------------------------------------------------------------------------------------------------
# edge values: finite-arithmetic cases that the rules define
# ------------------------------------------------------------------------------------------------------------------
def edge_case(seed, B=4, T=20, C=8, V=10):
    blank = C - 1
    rs = np.random.RandomState(seed)
    spellings = random_words(rs, C, blank, V, 2)
    x = np.concatenate([emissions(seed + 1, B // 2, T, C, 1.0), spelled(seed + 2, B - B // 2, T, C, blank, spellings, hi=4.0)])
    return x, transitions(seed + 3, C), blank, spellings


@TOPOLOGIES
def test_half_the_transitions_forbidden(forced):
    x, Wt, blank, spellings = edge_case(41)
    C = x.shape[2]
    mask = np.random.RandomState(44).rand(C + 1, C) < 0.5
    mask[0, blank] = mask[1 + blank, blank] = False  # (start -> blank and blank -> blank stay: the empty prefix lives)
    Wt[mask] = -np.inf
    want, seqs, raw = compare(x, Wt, blank, forced, 16, C, 3, spellings, None, None)
    assert all(h[0][1] > NEG for h in want)


@TOPOLOGIES
def test_scattered_nans_count_as_minus_infinity(forced):
    x, Wt, blank, spellings = edge_case(14)
    rs = np.random.RandomState(15)
    x[rs.rand(*x.shape) < 0.2] = np.nan
    Wt[rs.rand(*Wt.shape) < 0.2] = np.nan
    x[:, :, blank] = np.where(np.isnan(x[:, :, blank]), 0.25, x[:, :, blank])  # (the blank stays possible: no utterance dies)
    Wt[0, blank] = 0.125
    Wt[1 + blank] = np.where(np.isnan(Wt[1 + blank]), 0.125, Wt[1 + blank])  # (and can be entered from everywhere)
    want, _, _ = compare(x, Wt, blank, forced, 8, 8, 3, spellings, None, None)
    assert sum(h[0][1] > NEG for h in want) >= 3
    lex = pack(spellings, 8, blank)
    y = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    Vt = np.where(np.isnan(Wt), -np.inf, Wt).astype(np.float32)
    a, b = device(x, Wt, blank, forced, 8, 8, 3, lex, None), device(y, Vt, blank, forced, 8, 8, 3, lex, None)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


@TOPOLOGIES
def test_a_frame_with_only_the_blank_finite(forced):
    x, Wt, blank, spellings = edge_case(21)
    x[:, 9, :] = -np.inf
    x[:, 9, blank] = 0.5
    x[1, 0, :] = np.nan
    x[1, 0, blank] = -1.0
    compare(x, Wt, blank, forced, 8, 8, 3, spellings, None, None)
    compare(x, Wt, blank, forced, 8, 3, 3, spellings, None, None)


@TOPOLOGIES
def test_an_utterance_with_an_impossible_frame_decodes_to_nothing(forced):
    x, Wt, blank, spellings = edge_case(16)
    lex = pack(spellings, 8, blank)
    alone = device(x[[0, 2, 3]], Wt, blank, forced, 8, 8, 3, lex, None)
    x[1, 11, :] = -np.inf
    x[1, 11, 5] = np.nan
    want, seqs, raw = compare(x, Wt, blank, forced, 8, 8, 3, spellings, None, None)
    assert want[1] == [((), NEG)] * 3 and seqs[1] == [(), (), ()] and (raw[1] == NEG).all()
    assert [seqs[0], seqs[2], seqs[3]] == alone[0] and (raw[[0, 2, 3]] == alone[1]).all()  # (its neighbours are unaffected)


def full_beam_case(seed, forced):
    """A full beam (W = 4, K = 2) that holds a hypothesis none of whose extensions by this frame's candidates is in the
    trie.  Returns (x, Wt, blank, spellings, the frames at which that happens)."""
    C, blank, W, K = 7, 6, 4, 2
    rs = np.random.RandomState(5)
    spellings = random_words(rs, C, blank, 6, 2)
    x, Wt = emissions(seed, 1, 14, C, 2.0), transitions(seed + 1, C)
    hits = []

    def on_frame(t, beam, cand, extension, merged, entries):
        if len(beam) < W or (forced and t == 0):
            return
        for i in range(len(beam)):
            own = [c for c, _ in cand if c != blank]
            if own and all(extension(i, c)[0] == NEG for c in own) and any(XR.segment(spellings, beam[i][0] + (c,)) is None for c in own):
                hits.append(t)
                return

    TX.beam_search(x[0], Wt, blank, forced, W, K, 3, spellings, None, 1.0, OMEGA, BETA, True, on_frame=on_frame)
    return x, Wt, blank, spellings, hits


@TOPOLOGIES
@pytest.mark.parametrize("seed", [22, 24])
def test_a_full_beam_with_a_hypothesis_that_no_candidate_extends(seed, forced):
    x, Wt, blank, spellings, hits = full_beam_case(seed, forced)
    assert hits, "the case is not what it says"
    _, seqs, raw = compare(x, Wt, blank, forced, 4, 2, 3, spellings, None, None)
    assert raw[0, 0] > NEG and len(seqs[0][0]) > 0


def test_the_same_call_twice_is_bit_identical(tmp_path):
    T, C, B, V, blank = 40, 30, 4, 60, 29
    rs = np.random.RandomState(690)
    spellings = random_words(rs, C, blank, V, 2)
    lm, _ = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), 2, 0.3), V)
    x = np.concatenate([emissions(691, 2, T, C, 1.0), spelled(692, 2, T, C, blank, spellings)])
    Wt, lex = transitions(693, C), pack(spellings, C, blank)
    for forced in (False, True):
        a = device(x, Wt, blank, forced, 64, 22, 3, lex, lm, normalize=True)
        b = device(x, Wt, blank, forced, 64, 22, 3, lex, lm, normalize=True)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
        assert any(len(s) for h in a[0] for s in h)


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
KINDS = [dict(blank="optional", allow_repeats=False), dict(blank="forced")]


def _criterion(tokens, ngram, kw, seed):
    T = _mods()[2]
    crit = T.Transducer(tokens, {t: i for i, t in enumerate(tokens)}, ngram=ngram, **kw).cuda()
    if ngram > 0:
        params = (0.5 * np.random.RandomState(seed).randn(crit.transition_params.numel())).astype(np.float32)
        with torch.no_grad():
            crit.transition_params.copy_(torch.from_numpy(params))
    return crit


def _route_operands(crit, xd, forced, W, K, nbest, lex):
    """(emissions, Wt or None) on the host, as the module's route forms them for the search (_beam_inputs)"""
    plan, kind = crit._beam_plan(xd, "test", W, K, nbest, lex)
    assert plan.forced == forced
    xe, Wt = crit._beam_inputs(xd, kind)
    return xe.cpu().numpy(), None if Wt is None else Wt.cpu().numpy()


def _minus_loss(crit, xd, b, seq):
    """minus the criterion's loss of `seq` for utterance b, on the device (a batch of one: no batch mean in between)"""
    with torch.no_grad():
        return -float(crit(xd[b:b + 1], [list(seq)]).reshape(-1)[0])


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_module_against_the_reference_and_the_loss(tmp_path, ngram, kw):
    forced = kw["blank"] == "forced"
    tokens = ["a", "b", "|"]
    crit = _criterion(tokens, ngram, kw, 300 + ngram)
    C, blank = 4, 3
    words = ["a", "ab", "b", "ba"]
    lex = crit.word_lexicon(words, wordsep="|")
    spellings = {tuple(s): v for v, s in enumerate(lex.spellings)}
    # nothing is pruned (W = 64, K = C, T = 6: at most 1 + 3 + 9 + 27 + ... prefixes that walk the trie, far fewer live):
    # with alpha = omega = beta = 0 the score of a word sequence is minus the loss of that target
    B, T = 3, 6
    x = spelled(310 + ngram + int(forced), B, T, C, blank, spellings, hi=5.0, noise=1.0, run=1)
    xd = torch.from_numpy(x).cuda()
    xe, Wt = _route_operands(crit, xd, forced, 64, C, 4, lex)
    every = reference(xe, Wt, blank, forced, 10 ** 6, C, 4, spellings, None, 1.0, 0.0, 0.0)
    want = reference(xe, Wt, blank, forced, 64, C, 4, spellings, None, 1.0, 0.0, 0.0, spells=True)
    assert want == every  # (nothing was pruned)
    hyps, scores = crit.beam_search(xd, beam_size=64, classes_per_frame=C, nbest=4, return_scores=True, lexicon=lex)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (B, 4) and not scores.is_cuda
    logz = log_normaliser(xe, Wt)
    checked = 0
    for b in range(B):
        assert all(p.dtype == torch.int32 and not p.is_cuda and p.dim() == 1 for p in hyps[b])
        assert [tuple(p.tolist()) for p in hyps[b]] == [h for h, _ in want[b]], (b,)
        for r, (seq, s) in enumerate(want[b]):
            got = float(scores[b, r])
            if s == NEG:
                assert got == NEG
                continue
            n = s - logz[b]
            assert S.normalised_close(got, n), (b, r, got, n)
            assert crit.words(lex, hyps[b][r]) == XR.segment(spellings, seq)[0]
            if seq:
                loss = _minus_loss(crit, xd, b, seq)
                assert abs(got - loss) <= 1e-4 * abs(loss) + 2e-5, (b, r, seq, got, loss)
                checked += 1
    assert checked >= B
    # the beam prunes (T = 40, W = 4, K = 3), a word LM and bonuses on top: the reference's sequences, and without the
    # terms a lower bound of minus the loss
    B, T = 4, 40
    V = len(words)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(320 + ngram), names_of(V), 2, 0.5), V)
    x = spelled(350 + ngram + int(forced), B, T, C, blank, spellings, hi=5.0, noise=1.0)
    xd = torch.from_numpy(x).cuda()
    xe, Wt = _route_operands(crit, xd, forced, 4, 3, 1, lex)
    opts = dict(lexicon=lex, lm=lm, lm_weight=ALPHA, word_bonus=OMEGA, length_bonus=BETA)
    want = reference(xe, Wt, blank, forced, 4, 3, 2, spellings, ref_lm, spells=True)
    hyps = crit.beam_search(xd, beam_size=4, classes_per_frame=3, nbest=2, **opts)
    assert [[tuple(p.tolist()) for p in h] for h in hyps] == [[s for s, _ in h] for h in want]
    best, scores = crit.beam_search(xd, beam_size=4, classes_per_frame=3, return_scores=True, lexicon=lex)
    assert sum(len(p) > 0 for p in best) >= 3
    for b in range(B):
        if len(best[b]) > 0:
            loss = _minus_loss(crit, xd, b, best[b].tolist())
            assert float(scores[b, 0]) <= loss + 1e-4 * abs(loss) + 2e-5, (b, float(scores[b, 0]), loss)
    # other floating dtypes are converted, tensors that are not on a GPU are uploaded: the same search
    for other in (torch.from_numpy(x), xd.double()):
        again = crit.beam_search(other, beam_size=4, classes_per_frame=3, nbest=2, **opts)
        assert [[p.tolist() for p in h] for h in again] == [[p.tolist() for p in h] for h in hyps]


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_errors_count_what_beam_search_predicts_and_calls_without_a_lexicon_are_what_they_were(tmp_path, ngram, kw):
    E, M = _mods()[:2]
    tokens = ["a", "b", "c", "d", "|"]
    crit = _criterion(tokens, ngram, kw, 500 + ngram)
    B, T, C, blank = 4, 50, 6, 5
    rs = np.random.RandomState(520 + ngram)
    spellings = random_words(rs, C, blank, 8, 2)
    words = ["".join(tokens[t] for t in s[:-1]) for s in sorted(spellings, key=spellings.get)]
    lex = crit.word_lexicon(words, wordsep="|")
    assert [tuple(s) for s in lex.spellings] == sorted(spellings, key=spellings.get)
    lm, _ = make_lms(tmp_path, LR.random_arpa(rs, names_of(8), 2, 0.5), 8)
    x = np.concatenate([emissions(510 + ngram, 2, T, C, 1.0), spelled(511 + ngram, 2, T, C, blank, spellings)])
    xd = torch.from_numpy(x).cuda()
    targets = [rs.randint(0, 5, size=n).tolist() for n in (7, 1, 12, 3)]
    counter = M.ErrorCounter(wordsep=4)
    for W, K, opts in ((1, C, dict(lexicon=lex)), (16, 4, dict(lexicon=lex, lm=lm, lm_weight=ALPHA, word_bonus=OMEGA)),
                       (8, 6, dict(lexicon=lex, lm=lm, lm_eos=False, length_bonus=BETA))):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K, **opts)
        assert W == 1 or any(p.numel() > 0 for p in pred)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K, **opts) == counter(pred, targets)
    # without a lexicon: errors() and errors(beam_size=) count what they counted, beam_search() is plan.search bit for bit
    plain = crit.beam_search(xd, beam_size=16, classes_per_frame=4)
    assert crit.errors(xd, targets, counter, beam_size=16, classes_per_frame=4) == counter(plain, targets)
    assert crit.errors(xd, targets, counter) == counter(crit.viterbi(xd), targets)
    plan, kind = crit._beam_plan(xd, "test", 16, 4, 3)
    assert type(plan) is E.TransducerBeamPlan
    xe, Wt = crit._beam_inputs(xd, kind)
    direct, want = plan.search(xe, Wt, True, torch.int32)
    hyps, scores = crit.beam_search(xd, beam_size=16, classes_per_frame=4, nbest=3, return_scores=True)
    assert [[p.tolist() for p in h] for h in hyps] == [[p.tolist() for p in h] for h in direct]
    assert scores.numpy().tobytes() == want.numpy().tobytes()
