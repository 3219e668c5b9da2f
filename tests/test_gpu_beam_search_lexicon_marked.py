"""The CTC and Transducer beam searches with a START-MARKED lexicon on the device (csrc/beam_kernels.hip:
wfl_ctc_beam_search_lexicon_marked, wfl_transducer_beam_search_lexicon_marked behind engine.ctc_beam_search(lexicon=),
engine.transducer_beam_search_lexicon, CTC.beam_search / errors and Transducer.beam_search / errors; DESIGN.md section
26) against their restatement in plain Python (tests/beam_lexicon_marked_reference.py, itself pinned to a brute-force
enumeration in tests/test_beam_lexicon_marked_abi.py).

Acceptance of every comparison, the bars of the other lexicon searches: the label sequences of all returned ranks are
equal; unnormalised scores agree to 1e-9 max(1, |s|) -- both sides are float64 and differ in libm rounding only;
normalised scores agree at the project's loss bar (1e-4 |want| + 2e-5) against a float64 normaliser computed with torch,
independently of the library; every returned sequence is a sequence of whole words by rule 5.  An utterance whose
smallest selection margin in the reference is below 1e-9 could legitimately come out differently: the seeds are fixed
so that there is none, and every comparison asserts that -- no utterance is left out.

A topology is "ctc" (the CTC entry, with or without input lengths), "optional" or "forced" (the Transducer entry, with
transitions unless said otherwise).  Lexicons are {spelling: word id} dicts, written out or seeded; word LMs are seeded
random ARPA texts over the word names, loaded through NGramLM.from_arpa(path, words, blank=len(words)) for the device
and read by beam_lm_reference.ArpaLM for the reference."""
import os

import numpy as np
import pytest
import torch

import beam_lexicon_marked_reference as MR
import beam_lexicon_reference as XR
import beam_lm_reference as LR
import beam_support as S
from beam_support import emissions, log_normaliser, names_of, random_sentences, transitions
from beam_support import spelled_sentences as spelled
from beam_support import word_lms as make_lms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = MR.NEG
ALPHA, OMEGA, BETA = 0.8, 0.5, -0.3
TOPOLOGIES = pytest.mark.parametrize("topology", ["ctc", "optional", "forced"])


def _mods():
    return S.package("engine", "metrics", "criterions.ctc", "criterions.transducer", "criterions.asg", "lexicon:Lexicon",
                     "lm:NGramLM")


def pack(spellings, C, blank):
    """the device's start-marked Lexicon of a reference lexicon {spelling: word id}"""
    Lexicon = _mods()[5]
    order = sorted(spellings)
    return Lexicon(order, C, blank, boundary="start", word_of=[spellings[s] for s in order])


def reference(topology, x, Wt, blank, W, K, nbest, spellings, ref_lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True,
              lengths=None):
    """per utterance the reference's hyps; asserts the margins, so that no utterance is left out of a comparison"""
    rows = S.utterances(x, lengths)
    search = lambda b: MR.beam_search(rows[b], blank, W, K, nbest, spellings, ref_lm, alpha, omega, beta, eos, Wt=Wt,
                                      forced=topology == "forced")
    return [res[0] for res in S.margins_ok(search, len(rows))]


def device(topology, x, Wt, blank, W, K, nbest, lex, lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True, normalize=False,
           lengths=None):
    E = _mods()[0]
    xd = torch.from_numpy(x).cuda()
    kw = {} if lm is None else dict(lm=lm, lm_weight=alpha, lm_eos=eos)
    if topology == "ctc":
        ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
        hyps, scores = E.ctc_beam_search(xd, blank, W, K, nbest, lengths=ld, normalize=normalize, lexicon=lex, word_bonus=omega,
                                         length_bonus=beta, **kw)
    else:
        Wd = None if Wt is None else torch.from_numpy(Wt).cuda()
        hyps, scores = E.transducer_beam_search_lexicon(xd, Wd, blank, lex, topology == "forced", W, K, nbest,
                                                        normalize=normalize, word_bonus=omega, length_bonus=beta, **kw)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(topology, x, Wt, blank, W, K, nbest, spellings, lm, ref_lm, alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True,
            lengths=None):
    assert MR.is_start_marked(spellings)
    Wt = None if topology == "ctc" else Wt
    lex = pack(spellings, x.shape[2], blank)
    want = reference(topology, x, Wt, blank, W, K, nbest, spellings, ref_lm, alpha, omega, beta, eos, lengths)
    seqs, raw = device(topology, x, Wt, blank, W, K, nbest, lex, lm, alpha, omega, beta, eos, lengths=lengths)
    nseqs, normed = device(topology, x, Wt, blank, W, K, nbest, lex, lm, alpha, omega, beta, eos, normalize=True, lengths=lengths)
    assert nseqs == seqs  # (the shift never changes the search)

    def whole_words(b, r, seq):  # (rule 5, and the device's own segmentation agrees)
        assert MR.words_of(spellings, seq) is not None, (b, r, seq)
        assert lex.words(seq) == MR.words_of(spellings, seq)

    S.assert_ranks(want, seqs, raw, normed, log_normaliser(x, Wt, lengths), nbest, blank, whole_words)
    return want, seqs, raw


# ------------------------------------------------------------------------------------------------------------------
# the shapes of the issue, (T, C, W, K, B)
# ------------------------------------------------------------------------------------------------------------------
@TOPOLOGIES
def test_one_frame(topology):
    """(1, 3, 1, 2, 2).  A one-label word is returned where its class wins the frame (a terminal node after the last
    frame: the pending word's term), a label that only begins a longer word is not; forced: no extension in frame 0."""
    blank = 2
    x = np.array([[[3.0, 0.0, 1.0]], [[0.0, 1.0, 3.0]]], np.float32)
    want, seqs, _ = compare(topology, x, transitions(100, 3), blank, 1, 2, 1, {(0,): 0, (0, 1): 1}, None, None)
    assert seqs == ([[()], [()]] if topology == "forced" else [[(0,)], [()]])
    # the same frame where (0,) is no word: inside a word after the last frame, nothing is left
    want, seqs, raw = compare(topology, x, transitions(100, 3), blank, 1, 2, 1, {(0, 1): 0}, None, None)
    assert seqs[0] == [()] and (topology == "forced" or raw[0, 0] == NEG)


@TOPOLOGIES
@pytest.mark.parametrize("blank", [0, 2, 4], ids=["blank-first", "blank-middle", "blank-last"])
@pytest.mark.parametrize("order", [0, 2])
def test_seven_frames(tmp_path, topology, blank, order):
    """(7, 5, 4, 3, 3)"""
    C, B, T = 5, 3, 7
    rs = np.random.RandomState(200 + blank + order)
    spellings = MR.random_lexicon(rs, C, blank, 5, 2, 2, two_spellings=True)
    V = 5
    text = LR.random_arpa(rs, names_of(V), order, 0.6) if order else None
    lm, ref_lm = make_lms(tmp_path, text, V)
    x = np.concatenate([emissions(210 + blank, 1, T, C, 2.0),
                        spelled(211 + blank, 2, T, C, blank, random_sentences(rs, spellings, 2, 2), hi=4.0, noise=1.0, run=1)])
    compare(topology, x, transitions(220, C), blank, 4, 3, 3, spellings, lm, ref_lm)


@TOPOLOGIES
def test_the_wide_instantiation_on_a_dense_lexicon(tmp_path, topology):
    """(64, 30, 64, 30, 2): W (K + 2) > 1024, the 1024-thread kernel and its radix select"""
    C, blank, B, T, V = 30, 29, 2, 64, 40
    rs = np.random.RandomState(300)
    spellings = MR.random_lexicon(rs, C, blank, V, 3, 6, two_spellings=True)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), 2, 0.2), V)
    x = np.concatenate([emissions(310, 1, T, C, 1.5),
                        spelled(311, 1, T, C, blank, random_sentences(rs, spellings, 1, 12), hi=3.0, noise=1.0)])
    want, _, _ = compare(topology, x, transitions(320, C), blank, 64, 30, 4, spellings, lm, ref_lm)
    assert any(h[0][0] for h in want)


@TOPOLOGIES
def test_a_hundred_classes(tmp_path, topology):
    """(120, 100, 16, 32, 2), an order-3 word LM that backs off"""
    C, blank, B, T, V = 100, 50, 2, 120, 60
    rs = np.random.RandomState(400)
    spellings = MR.random_lexicon(rs, C, blank, V, 3, 20)
    text = LR.random_arpa(rs, names_of(V), 3, 0.05)
    lm, ref_lm = make_lms(tmp_path, text, V)
    assert ref_lm.order == 3 and any(len(g) == 3 for g in ref_lm.grams)
    x = spelled(410, B, T, C, blank, random_sentences(rs, spellings, 2, 20), hi=6.0, noise=1.0)
    want, _, _ = compare(topology, x, transitions(420, C), blank, 16, 32, 2, spellings, lm, ref_lm)
    # the LM backed off on the way: the best sentence has a trigram that is not in the file
    backed = 0
    for hyps in want:
        words = MR.words_of(spellings, hyps[0][0])
        assert len(words) >= 3
        backed += sum(1 for i in range(2, len(words)) if tuple(words[i - 2:i + 1]) not in ref_lm.grams)
    assert backed > 0


def word_piece_lexicon(count=200, seed=0):
    """(tokens, {word: pieces}) over benchmarks/word_pieces_tokens_1000.txt: one start piece joined with 0 - 2 plain
    pieces, every word's shorter forms among the words -- not prefix-free"""
    with open(os.path.join(ROOT, "benchmarks", "word_pieces_tokens_1000.txt"), encoding="utf-8") as f:
        tokens = [line.rstrip("\n") for line in f if line.rstrip("\n")]
    rs = np.random.RandomState(seed)
    first = [t for t in tokens if t.startswith("▁") and len(t) > 1]
    plain = [t for t in tokens if not t.startswith("▁")]
    words = {}
    while len(words) < count:
        pieces = [first[rs.randint(len(first))]] + [plain[rs.randint(len(plain))] for _ in range(rs.randint(3))]
        for k in range(1, len(pieces) + 1):
            words.setdefault("".join(pieces[:k]), pieces[:k])
    return tokens, words


@pytest.mark.parametrize("topology", ["ctc", "forced"])
def test_the_word_piece_file(tmp_path, topology):
    """C = 1001, T = 40, W = 16, K = 32, B = 2: the candidates launch's re-reading path, a lexicon from_words builds"""
    Lexicon = _mods()[5]
    tokens, words = word_piece_lexicon()
    names = sorted(words)
    C, blank, V = 1001, 1000, len(names)
    lex = Lexicon.from_words(names, tokens, blank, split=lambda w: words[w], boundary="start")
    label = {t: i for i, t in enumerate(tokens)}
    spellings = {tuple(label[p] for p in words[w]): v for v, w in enumerate(names)}
    assert sorted(tuple(s) for s in lex.spellings) == sorted(spellings) and not XR.is_prefix_free(spellings)
    rs = np.random.RandomState(500)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), 2, 0.01), V)
    x = spelled(510, 2, 40, C, blank, random_sentences(rs, spellings, 2, 8), hi=9.0, noise=1.0)
    want = reference(topology, x, None, blank, 16, 32, 2, spellings, ref_lm)
    seqs, raw = device(topology, x, None, blank, 16, 32, 2, lex, lm)
    for b, hyps in enumerate(want):
        assert seqs[b] == [h for h, _ in hyps] and len(MR.words_of(spellings, hyps[0][0])) >= 3
        for r, (_, s) in enumerate(hyps):
            assert S.raw_close(raw[b, r], s)


# ------------------------------------------------------------------------------------------------------------------
# the situations of the issue
# ------------------------------------------------------------------------------------------------------------------
# classes: 0 "_a", 1 "_the", 2 "n", 3 "t", 4 "re", 5 the blank
NEST = {(0,): 0, (0, 2): 1, (0, 2, 3): 2, (1,): 3, (1, 4): 4}


@TOPOLOGIES
def test_a_word_that_is_a_proper_prefix_of_two_others(topology):
    """"_a", "_a n", "_a n t": all three decoded from emissions that spell them, and "_a _a", which needs the blank between"""
    sentences = [[(0,)], [(0, 2)], [(0, 2, 3)], [(0,), (0,)], [(0, 2), (0,), (0, 2, 3), (1, 4)]]
    x = spelled(600, 5, 24, 6, 5, sentences, hi=8.0, noise=0.5)
    want, seqs, _ = compare(topology, x, transitions(610, 6), 5, 8, 4, 2, NEST, None, None, omega=0.0, beta=0.0)
    assert [s[0] for s in seqs] == [(0,), (0, 2), (0, 2, 3), (0, 0), (0, 2, 0, 0, 2, 3, 1, 4)]
    assert [MR.words_of(NEST, s[0]) for s in seqs] == [[0], [1], [2], [0, 0], [1, 0, 2, 4]]


@TOPOLOGIES
def test_every_final_hypothesis_inside_a_word(topology):
    """the only word needs three labels and the emissions spell two: every rank is dropped, the empty sequence at -inf"""
    x = spelled(620, 2, 8, 6, 5, [[(0, 2)]], hi=12.0, noise=0.3)
    x[:, :, 3] = -np.inf  # (the third label never comes)
    want, seqs, raw = compare(topology, x, transitions(630, 6), 5, 2, 2, 2, {(0, 2, 3): 0}, None, None)
    assert seqs == [[(), ()]] * 2 and (raw == NEG).all()


@TOPOLOGIES
def test_a_pending_word_the_lm_cannot_follow(tmp_path, topology):
    """word 1 ("_a n") has probability 0 under the LM: it is dropped as a completed word (rule 3) and as the pending one (rule 5)"""
    lines = []
    for line in LR.random_arpa(np.random.RandomState(640), names_of(5), 2, 0.6).split("\n"):
        f = line.split("\t")
        if len(f) >= 2 and f[1].split()[-1] == "w1":
            f[0] = "-inf"  # (every gram that ends in the word: its step is -inf from every history)
        lines.append("\t".join(f))
    lm, ref_lm = make_lms(tmp_path, "\n".join(lines), 5)
    assert ref_lm.step(ref_lm.start, 1)[0] == NEG and lm.step(lm.start, 1)[0] == NEG
    x = spelled(650, 3, 12, 6, 5, [[(0, 2)], [(1,), (0, 2)], [(0, 2), (1,)]], hi=6.0, noise=0.5)
    want, seqs, _ = compare(topology, x, transitions(660, 6), 5, 8, 4, 3, NEST, lm, ref_lm)
    assert all(1 not in MR.words_of(NEST, s) for h in seqs for s in h)
    # without the LM the same emissions decode to it
    _, plain, _ = compare(topology, x, transitions(660, 6), 5, 8, 4, 3, NEST, None, None)
    assert [MR.words_of(NEST, h[0]) for h in plain] == [[1], [3, 1], [1, 3]]


@TOPOLOGIES
def test_a_word_with_two_spellings_takes_both_ranks(topology):
    """"_an" as "_a n" and as the piece "_an" (class 2 here): two label sequences, two hypotheses, one word"""
    # classes: 0 "_a", 1 "n", 2 "_an", 3 the blank
    spellings = {(0, 1): 0, (2,): 0}
    x = np.full((1, 6, 4), -4.0, np.float32)
    for t, (c, d) in enumerate([(3, 3), (0, 2), (3, 3), (1, 3), (3, 3), (3, 3)]):
        x[0, t, c] += 6.0
        x[0, t, d] += 5.5 if d != c else 0.0
    want, seqs, _ = compare(topology, x, transitions(670, 4) * 0.1, 3, 8, 3, 2, spellings, None, None)
    assert sorted(seqs[0]) == [(0, 1), (2,)] and all(MR.words_of(spellings, s) == [0] for s in seqs[0])


@TOPOLOGIES
@pytest.mark.parametrize("omega", [50.0, -50.0])
def test_a_large_word_bonus_either_way(tmp_path, topology, omega):
    rs = np.random.RandomState(680)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    x = np.concatenate([emissions(681, 1, 14, 6, 2.0), spelled(682, 2, 14, 6, 5, random_sentences(rs, NEST, 2, 3), hi=4.0)])
    want, _, _ = compare(topology, x, transitions(690, 6), 5, 8, 5, 3, NEST, lm, ref_lm, omega=omega)
    count = [len(MR.words_of(NEST, h[0][0])) for h in want]
    assert (min(count) >= 3) if omega > 0 and topology != "forced" else (omega > 0 or max(count) <= 1)


@TOPOLOGIES
def test_the_lexicon_alone_against_a_silent_lm_bit_for_bit(tmp_path, topology):
    """a word LM whose every step is 0 (unigrams of probability 1, alpha arbitrary) changes nothing at all"""
    V = 5
    text = "\\data\\\nngram 1=7\n\n\\1-grams:\n" + "".join(f"0\t{w}\n" for w in ["<s>", "</s>"] + names_of(V)) + "\n\\end\\\n"
    lm, ref_lm = make_lms(tmp_path, text, V)
    assert all(ref_lm.step((), v)[0] == 0.0 for v in range(V))
    x = np.concatenate([emissions(700, 2, 20, 6, 2.0), spelled(701, 2, 20, 6, 5, [[(0, 2), (1, 4), (0,)]], hi=4.0)])
    lex = pack(NEST, 6, 5)
    Wt = None if topology == "ctc" else transitions(710, 6)
    a = device(topology, x, Wt, 5, 8, 4, 3, lex, None)
    b = device(topology, x, Wt, 5, 8, 4, 3, lex, lm, alpha=0.7, eos=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and any(s for h in a[0] for s in h)


@pytest.mark.parametrize("topology", ["ctc", "optional"])
def test_a_prefix_free_vocabulary_written_both_ways(tmp_path, topology):
    """End-marked with a separator class "|" behind every word, and start-marked with the separator moved to the front
    of the next word: the same word sequences.  The documented difference: the start-marked sentence has a separator
    ahead of its first word and none behind its last ("| w1 | w2" against "w1 | w2 |"), so each side gets emissions that
    spell its own form of the same sentence, and each returns that form."""
    Lexicon = _mods()[5]
    # classes: 0 "a", 1 "b", 2 "c", 3 "|", 4 the blank
    words = [(0, 1), (1,), (2, 0), (1, 2, 2)]
    end = Lexicon([w + (3,) for w in words], 5, 4)
    start = pack({(3,) + w: v for v, w in enumerate(words)}, 5, 4)
    assert start.boundary == "start" and end.boundary == "end"
    rs = np.random.RandomState(720)
    text = LR.random_arpa(rs, names_of(4), 2, 0.6)
    lm, _ = make_lms(tmp_path, text, 4)
    sentences = [[words[rs.randint(4)] for _ in range(4)] for _ in range(4)]
    xe = spelled(730, 4, 40, 5, 4, [[w + (3,) for w in s] for s in sentences], hi=9.0, noise=0.5, run=1)
    xs = spelled(730, 4, 40, 5, 4, [[(3,) + w for w in s] for s in sentences], hi=9.0, noise=0.5, run=1)
    got_e = device(topology, xe, None, 4, 8, 5, 1, end, lm)
    got_s = device(topology, xs, None, 4, 8, 5, 1, start, lm)
    for b, s in enumerate(sentences):
        want = [words.index(w) for w in s]
        assert end.words(got_e[0][b][0]) == want and start.words(got_s[0][b][0]) == want
        assert got_e[0][b][0] == tuple(c for w in s for c in w + (3,))
        assert got_s[0][b][0] == tuple(c for w in s for c in (3,) + w)
    # and the start-marked side against its restatement
    compare(topology, xs, None, 4, 8, 5, 1, {(3,) + w: v for v, w in enumerate(words)}, lm, LR.ArpaLM(text, names_of(4), 4))


def test_ctc_with_input_lengths(tmp_path):
    """lengths T, in between, 1 and 0: T_b = 0 is the empty sequence scored by </s> alone"""
    rs = np.random.RandomState(740)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    T = 14
    x = np.concatenate([emissions(741, 2, T, 6, 2.0), spelled(742, 3, T, 6, 5, random_sentences(rs, NEST, 3, 3), hi=4.0)])
    lengths = [T, 0, 9, 1, 5]
    want, seqs, raw = compare("ctc", x, None, 5, 8, 4, 3, NEST, lm, ref_lm, lengths=lengths)
    assert seqs[1] == [(), (), ()] and raw[1, 0] == ALPHA * ref_lm.step(ref_lm.start, LR.EOS)[0] and raw[1, 1] == NEG
    # the frames behind an utterance are not looked at
    x[2, 9:] = np.nan
    again = device("ctc", x, None, 5, 8, 4, 3, pack(NEST, 6, 5), lm, lengths=lengths)
    assert again[0] == seqs and again[1].tobytes() == raw.tobytes()


def test_the_transducer_entry_without_transitions_is_the_ctc_entry_bit_for_bit(tmp_path):
    rs = np.random.RandomState(750)
    lm, _ = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    x = np.concatenate([emissions(751, 2, 30, 6, 2.0), spelled(752, 2, 30, 6, 5, random_sentences(rs, NEST, 2, 6), hi=4.0)])
    lex = pack(NEST, 6, 5)
    for normalize in (False, True):
        a = device("ctc", x, None, 5, 8, 4, 3, lex, lm, normalize=normalize)
        b = device("optional", x, None, 5, 8, 4, 3, lex, lm, normalize=normalize)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and any(s for h in a[0] for s in h)


@TOPOLOGIES
def test_the_same_call_twice_is_bit_identical(tmp_path, topology):
    rs = np.random.RandomState(760)
    spellings = MR.random_lexicon(rs, 30, 29, 40, 3, 6, two_spellings=True)
    lm, _ = make_lms(tmp_path, LR.random_arpa(rs, names_of(40), 2, 0.2), 40)
    x = emissions(761, 4, 50, 30, 1.5)
    lex = pack(spellings, 30, 29)
    Wt = None if topology == "ctc" else transitions(770, 30)
    a = device(topology, x, Wt, 29, 64, 30, 4, lex, lm)
    b = device(topology, x, Wt, 29, 64, 30, 4, lex, lm)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------------------------
# the modules
# ------------------------------------------------------------------------------------------------------------------
TOKENS = ["A", "T", "n", "t", "r"]  # "A" and "T" begin words; the blank is class 5
WORDS = ["A", "An", "Ant", "T", "Tr"]


def test_ctc_module_and_errors(tmp_path):
    _, M, ctc, _, _, Lexicon, _ = _mods()
    lex = Lexicon.from_words(WORDS, TOKENS, 5, boundary="start")
    spellings = {tuple(s): v for s, v in zip(lex.spellings, lex.word_of)}
    assert spellings == NEST
    rs = np.random.RandomState(800)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    T = 16
    x = np.concatenate([emissions(801, 1, T, 6, 2.0), spelled(802, 3, T, 6, 5, random_sentences(rs, NEST, 3, 4), hi=4.0)])
    lengths = [T, 11, T, 6]
    crit = ctc.CTC(5, False)
    xd = torch.from_numpy(x).cuda()
    opts = dict(lexicon=lex, lm=lm, lm_weight=ALPHA, word_bonus=OMEGA, length_bonus=BETA)
    hyps, scores = crit.beam_search(xd, 8, 4, 2, input_lengths=lengths, return_scores=True, **opts)
    want = reference("ctc", x, None, 5, 8, 4, 2, NEST, ref_lm, lengths=lengths)
    logz = log_normaliser(x, None, lengths)
    for b in range(4):
        assert [tuple(p.tolist()) for p in hyps[b]] == [h for h, _ in want[b]], b
        for r, (seq, s) in enumerate(want[b]):
            if s > NEG:
                n = s - logz[b]
                assert S.normalised_close(float(scores[b, r]), n)
                assert lex.words(hyps[b][r].tolist()) == MR.words_of(NEST, seq)
    assert sum(len(h[0]) > 0 for h in hyps) >= 3
    counter = M.ErrorCounter()
    targets = [rs.randint(0, 5, size=n).tolist() for n in (7, 1, 12, 3)]
    pred = crit.beam_search(xd, 8, 4, input_lengths=lengths, **opts)
    assert crit.errors(xd, targets, counter, input_lengths=lengths, beam_size=8, classes_per_frame=4, **opts) == \
        counter(pred, targets)


KINDS = [dict(blank="optional", allow_repeats=False), dict(blank="forced")]


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_transducer_module_and_errors(tmp_path, ngram, kw):
    _, M, _, T, _, _, _ = _mods()
    forced = kw["blank"] == "forced"
    crit = T.Transducer(TOKENS, {t: i for i, t in enumerate(TOKENS)}, ngram=ngram, **kw).cuda()
    if ngram > 0:
        params = (0.5 * np.random.RandomState(810 + ngram).randn(crit.transition_params.numel())).astype(np.float32)
        with torch.no_grad():
            crit.transition_params.copy_(torch.from_numpy(params))
    lex = crit.word_lexicon(WORDS, boundary="start")
    assert {tuple(s): v for s, v in zip(lex.spellings, lex.word_of)} == NEST
    rs = np.random.RandomState(820 + ngram)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    B, Tn = 4, 24
    x = np.concatenate([emissions(821 + ngram, 1, Tn, 6, 1.0),
                        spelled(822 + ngram + int(forced), 3, Tn, 6, 5, random_sentences(rs, NEST, 3, 5), hi=5.0, noise=1.0)])
    xd = torch.from_numpy(x).cuda()
    plan, kind = crit._beam_plan(xd, "test", 4, 3, 2, lex)
    assert plan.forced == forced and plan.lexicon.boundary == "start"
    xe, Wt = crit._beam_inputs(xd, kind)
    xe, Wt = xe.cpu().numpy(), None if Wt is None else Wt.cpu().numpy()
    opts = dict(lexicon=lex, lm=lm, lm_weight=ALPHA, word_bonus=OMEGA, length_bonus=BETA)
    topology = "forced" if forced else "optional"
    want = reference(topology, xe, Wt, 5, 4, 3, 2, NEST, ref_lm)
    hyps, scores = crit.beam_search(xd, beam_size=4, classes_per_frame=3, nbest=2, return_scores=True, **opts)
    logz = log_normaliser(xe, Wt)
    assert [[tuple(p.tolist()) for p in h] for h in hyps] == [[s for s, _ in h] for h in want]
    for b in range(B):
        for r, (seq, s) in enumerate(want[b]):
            if s > NEG:
                n = s - logz[b]
                assert S.normalised_close(float(scores[b, r]), n), (b, r)
                assert crit.words(lex, hyps[b][r]) == MR.words_of(NEST, seq)
    assert sum(len(h[0]) > 0 for h in hyps) >= 3
    counter = M.ErrorCounter()
    targets = [rs.randint(0, 5, size=n).tolist() for n in (7, 1, 12, 3)]
    pred = crit.beam_search(xd, beam_size=4, classes_per_frame=3, **opts)
    assert crit.errors(xd, targets, counter, beam_size=4, classes_per_frame=3, **opts) == counter(pred, targets)


def test_asg_refuses():
    _, _, _, _, asg, Lexicon, _ = _mods()
    crit = asg.ASG(2, num_replabels=1, use_garbage=True).cuda()
    marked = Lexicon([(0,), (0, 1)], 4, 3, boundary="start")
    x = torch.zeros(2, 5, 4, device="cuda")
    with pytest.raises(NotImplementedError, match="question of its own"):
        crit.beam_search(x, 4, lexicon=marked)
    assert len(crit.beam_search(x, 4, lexicon=Lexicon([(0, 1), (1, 0)], 4, 3))) == 2
