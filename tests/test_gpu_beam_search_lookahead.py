"""The lexicon searches of CTC and the Transducer with word-LM look-ahead on the device (csrc/beam_kernels.hip: the four
wfl_*_beam_search_lexicon*_lookahead entries behind engine.ctc_beam_search(lookahead=), engine.transducer_beam_search_lexicon
with a prepared LexiconLookahead, CTC.beam_search / errors and Transducer.beam_search / errors)
against their restatement in plain Python (tests/beam_lookahead_reference.py, which never skips a lookup and is itself
pinned to the restatements without look-ahead in tests/test_beam_lookahead_abi.py).

Acceptance of every comparison, the bars of the other lexicon searches: the label sequences of all returned ranks are
equal; unnormalised scores agree to 1e-9 max(1, |s|) -- both sides are float64, form every term by the same operations
and differ in libm rounding only; normalised scores agree at the project's loss bar (1e-4 |want| + 2e-5) against a float64
normaliser computed with torch, independently of the library.  An utterance whose smallest selection margin in the
restatement is below 1e-9 could legitimately come out differently: the seeds are fixed so that there is none, and every
comparison asserts that -- no utterance is left out.

A boundary is "end" (a prefix-free lexicon, a word ends with its last label) or "start" (a start-marked one); a topology
is "ctc" (the CTC entry, with or without input lengths), "optional" or "forced" (the Transducer entry, with transitions
unless said otherwise).  Lexicons are {spelling: word id} dicts; word LMs are seeded random ARPA texts over the word
names, loaded through NGramLM.from_arpa for the device and read by beam_lm_reference.ArpaLM for the restatement; the
look-ahead is "unigram" unless a test passes word scores."""
import numpy as np
import pytest
import torch

import beam_lexicon_marked_reference as MR
import beam_lexicon_reference as XR
import beam_lm_reference as LR
import beam_lookahead_reference as LA
import beam_support as S
from beam_support import emissions, log_normaliser, names_of, random_sentences, transitions
from beam_support import spelled_sentences as spelled
from beam_support import word_lms as make_lms

pytestmark = pytest.mark.gpu

NEG = LA.NEG
ALPHA, OMEGA, BETA = 0.8, 0.5, -0.3
BOUNDARIES = pytest.mark.parametrize("boundary", ["end", "start"])
TOPOLOGIES = pytest.mark.parametrize("topology", ["ctc", "optional", "forced"])


def _mods():
    return S.package("engine", "metrics", "criterions.ctc", "criterions.transducer", "criterions.asg", "lexicon:Lexicon",
                     "lm:NGramLM")


def pack(spellings, C, blank, boundary):
    """the device's Lexicon of a restatement's lexicon {spelling: word id}"""
    Lexicon = _mods()[5]
    if boundary == "start":
        order = sorted(spellings)
        return Lexicon(order, C, blank, boundary="start", word_of=[spellings[s] for s in order])
    return Lexicon([s for s, _ in sorted(spellings.items(), key=lambda kv: kv[1])], C, blank)


def word_scores(ref_lm, V, scores):
    return LA.unigram_scores(ref_lm, V) if isinstance(scores, str) else list(scores)


def reference(topology, boundary, x, Wt, blank, W, K, nbest, spellings, ref_lm, scores="unigram", alpha=ALPHA, omega=OMEGA,
              beta=BETA, eos=True, lengths=None):
    """per utterance the restatement's hyps; asserts the margins, so that no utterance is left out of a comparison.
    scores None: the restatement WITHOUT look-ahead (a look-ahead of zeros is that search, bit for bit)"""
    V = max(spellings.values()) + 1
    marked = boundary == "start"
    look = LA.node_look(spellings, [0.0] * V if scores is None else word_scores(ref_lm, V, scores), marked)
    rows = S.utterances(x, lengths)
    search = lambda b: LA.beam_search(rows[b], blank, W, K, nbest, spellings, ref_lm, look, alpha, omega, beta, eos, marked=marked,
                                      Wt=Wt, forced=topology == "forced")
    return [res[0] for res in S.margins_ok(search, len(rows))]


def device(topology, x, Wt, blank, W, K, nbest, lex, lm, scores="unigram", alpha=ALPHA, omega=OMEGA, beta=BETA, eos=True,
           normalize=False, lengths=None):
    """the engine's call; scores None: the call without the keyword"""
    E = _mods()[0]
    xd = torch.from_numpy(x).cuda()
    kw = dict(lm=lm, lm_weight=alpha, lm_eos=eos, word_bonus=omega, length_bonus=beta, normalize=normalize)
    look = None if scores is None else (scores if isinstance(scores, str) else np.asarray(scores, np.float64))
    if topology == "ctc":
        ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
        more = {} if look is None else dict(lookahead=look)
        hyps, scores_ = E.ctc_beam_search(xd, blank, W, K, nbest, lengths=ld, lexicon=lex, **kw, **more)
    else:
        Wd = None if Wt is None else torch.from_numpy(Wt).cuda()
        if look is not None:  # (this call's signature is pinned: the prepared look-ahead stands in for its lexicon)
            lex = lex.unigram_lookahead(lm) if isinstance(look, str) else lex.lookahead(look)
        hyps, scores_ = E.transducer_beam_search_lexicon(xd, Wd, blank, lex, topology == "forced", W, K, nbest, **kw)
    assert scores_.dtype == torch.float64 and tuple(scores_.shape) == (x.shape[0], nbest) and not scores_.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores_.numpy()


def words_of(spellings, boundary, seq):
    if boundary == "start":
        return MR.words_of(spellings, seq)
    seg = XR.segment(spellings, seq)
    return None if seg is None or seg[1] else seg[0]


def compare(topology, boundary, x, Wt, blank, W, K, nbest, spellings, lm, ref_lm, scores="unigram", alpha=ALPHA, omega=OMEGA,
            beta=BETA, eos=True, lengths=None):
    assert MR.is_start_marked(spellings) if boundary == "start" else XR.is_prefix_free(spellings)
    Wt = None if topology == "ctc" else Wt
    lex = pack(spellings, x.shape[2], blank, boundary)
    want = reference(topology, boundary, x, Wt, blank, W, K, nbest, spellings, ref_lm, scores, alpha, omega, beta, eos, lengths)
    seqs, raw = device(topology, x, Wt, blank, W, K, nbest, lex, lm, scores, alpha, omega, beta, eos, lengths=lengths)
    nseqs, normed = device(topology, x, Wt, blank, W, K, nbest, lex, lm, scores, alpha, omega, beta, eos, normalize=True,
                           lengths=lengths)
    assert nseqs == seqs  # (the shift never changes the search)

    def whole_words(b, r, seq):  # (and the device's own segmentation agrees)
        assert words_of(spellings, boundary, seq) is not None, (b, r, seq)
        assert lex.words(seq) == words_of(spellings, boundary, seq)

    S.assert_ranks(want, seqs, raw, normed, log_normaliser(x, Wt, lengths), nbest, blank, whole_words)
    return want, seqs, raw


def random_lexicon(rs, boundary, C, blank, V, max_len, n_starts):
    if boundary == "start":
        return MR.random_lexicon(rs, C, blank, V, max_len, n_starts, two_spellings=True)
    return XR.random_lexicon(rs, C, blank, V, max_len)


# ------------------------------------------------------------------------------------------------------------------
# the shapes of the issue, (T, C, W, K, B): CTC, end-marked and start-marked, input lengths down to 0
# ------------------------------------------------------------------------------------------------------------------
UNIGRAMS2 = "\\data\\\nngram 1=4\n\n\\1-grams:\n-1.0\t<s>\n-0.5\t</s>\n-0.25\tw0\n-1.5\tw1\n\n\\end\\\n"


@BOUNDARIES
def test_one_frame(tmp_path, boundary):
    """(1, 3, 1, 2, 2), and a length of 0.  End-marked: the one-label word is returned where its class wins the frame
    (rule 2 at the root, whose look-ahead is 0); start-marked: the pending word's settled term after the only frame"""
    blank = 2
    x = np.array([[[3.0, 0.0, 1.0]], [[0.0, 1.0, 3.0]]], np.float32)
    spellings = {(0,): 0, (1, 0): 1} if boundary == "end" else {(0,): 0, (0, 1): 1}
    lm, ref_lm = make_lms(tmp_path, UNIGRAMS2, 2)
    want, seqs, _ = compare("ctc", boundary, x, None, blank, 1, 2, 1, spellings, lm, ref_lm)
    assert seqs == [[(0,)], [()]]
    want, seqs, raw = compare("ctc", boundary, x, None, blank, 1, 2, 1, spellings, lm, ref_lm, lengths=[0, 1])
    assert seqs == [[()], [()]] and raw[0, 0] == ALPHA * ref_lm.step(ref_lm.start, LR.EOS)[0]


@BOUNDARIES
@pytest.mark.parametrize("blank", [0, 2, 4], ids=["blank-first", "blank-middle", "blank-last"])
def test_seven_frames(tmp_path, boundary, blank):
    """(7, 5, 4, 3, 3), input lengths 7, 4 and 0"""
    C, T, V = 5, 7, 5
    rs = np.random.RandomState(1200 + blank)
    spellings = random_lexicon(rs, boundary, C, blank, V, 2, 2)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), 2, 0.6), V)
    x = np.concatenate([emissions(1210 + blank, 1, T, C, 2.0),
                        spelled(1211 + blank, 2, T, C, blank, random_sentences(rs, spellings, 2, 2), hi=4.0, noise=1.0, run=1)])
    compare("ctc", boundary, x, None, blank, 4, 3, 3, spellings, lm, ref_lm)
    compare("ctc", boundary, x, None, blank, 4, 3, 3, spellings, lm, ref_lm, lengths=[4, 7, 0])


@BOUNDARIES
@pytest.mark.parametrize("topology", ["optional", "forced"])
def test_seven_frames_through_the_transducer_entries(tmp_path, boundary, topology):
    """(7, 5, 4, 3, 3) with transitions, the blank in the middle"""
    C, T, V, blank = 5, 7, 5, 2
    rs = np.random.RandomState(1250)
    spellings = random_lexicon(rs, boundary, C, blank, V, 2, 2)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), 2, 0.6), V)
    x = np.concatenate([emissions(1260, 1, T, C, 2.0),
                        spelled(1261, 2, T, C, blank, random_sentences(rs, spellings, 2, 2), hi=4.0, noise=1.0, run=1)])
    compare(topology, boundary, x, transitions(1270, C), blank, 4, 3, 3, spellings, lm, ref_lm)


@BOUNDARIES
def test_the_wide_instantiation_on_a_dense_lexicon(tmp_path, boundary):
    """(64, 30, 64, 30, 2): W (K + 2) > 1024, the 1024-thread kernel and its radix select"""
    C, blank, T, V = 30, 29, 64, 40
    rs = np.random.RandomState(1300)
    spellings = random_lexicon(rs, boundary, C, blank, V, 3, 6)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), 2, 0.2), V)
    x = np.concatenate([emissions(1310, 1, T, C, 1.5),
                        spelled(1311, 1, T, C, blank, random_sentences(rs, spellings, 1, 12), hi=3.0, noise=1.0)])
    want, _, _ = compare("ctc", boundary, x, None, blank, 64, 30, 4, spellings, lm, ref_lm, lengths=[64, 50])
    assert any(h[0][0] for h in want)


@BOUNDARIES
def test_a_hundred_classes(tmp_path, boundary):
    """(120, 100, 16, 32, 2), an order-3 word LM that backs off"""
    C, blank, B, T, V = 100, 50, 2, 120, 60
    rs = np.random.RandomState(1400)
    spellings = random_lexicon(rs, boundary, C, blank, V, 3, 20)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(V), 3, 0.05), V)
    assert ref_lm.order == 3 and any(len(g) == 3 for g in ref_lm.grams)
    x = spelled(1410, B, T, C, blank, random_sentences(rs, spellings, 2, 20), hi=6.0, noise=1.0)
    want, _, _ = compare("ctc", boundary, x, None, blank, 16, 32, 2, spellings, lm, ref_lm)
    backed = 0
    for hyps in want:  # the LM backed off on the way: the best sentence has a trigram that is not in the file
        words = words_of(spellings, boundary, hyps[0][0])
        assert len(words) >= 3
        backed += sum(1 for i in range(2, len(words)) if tuple(words[i - 2:i + 1]) not in ref_lm.grams)
    assert backed > 0


# ------------------------------------------------------------------------------------------------------------------
# bit-for-bit identities
# ------------------------------------------------------------------------------------------------------------------
# classes: 0 "_a", 1 "_the", 2 "n", 3 "t", 4 "re", 5 the blank
NEST = {(0,): 0, (0, 2): 1, (0, 2, 3): 2, (1,): 3, (1, 4): 4}
# the same classes, prefix-free: 3 ends a word
FREE = {(0, 3): 0, (0, 2, 3): 1, (1, 3): 2, (1, 4, 3): 3, (2, 2, 3): 4}
LEXICONS = {"end": FREE, "start": NEST}


def identity_inputs(tmp_path, boundary, seed):
    rs = np.random.RandomState(seed)
    spellings = LEXICONS[boundary]
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    x = np.concatenate([emissions(seed + 1, 2, 24, 6, 2.0),
                        spelled(seed + 2, 2, 24, 6, 5, random_sentences(rs, spellings, 2, 5), hi=4.0)])
    return spellings, pack(spellings, 6, 5, boundary), lm, ref_lm, x


@BOUNDARIES
@TOPOLOGIES
def test_word_scores_of_zero_are_the_call_without_lookahead_bit_for_bit(tmp_path, boundary, topology):
    _, lex, lm, _, x = identity_inputs(tmp_path, boundary, 1500)
    Wt = None if topology == "ctc" else transitions(1510, 6)
    for W in (2, 8):
        a = device(topology, x, Wt, 5, W, 4, min(W, 3), lex, lm, scores=None)
        b = device(topology, x, Wt, 5, W, 4, min(W, 3), lex, lm, scores=[0.0] * 5)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and any(s for h in a[0] for s in h)


@BOUNDARIES
@TOPOLOGIES
def test_a_weight_of_zero_is_the_call_without_lookahead_bit_for_bit(tmp_path, boundary, topology):
    _, lex, lm, _, x = identity_inputs(tmp_path, boundary, 1520)
    Wt = None if topology == "ctc" else transitions(1530, 6)
    a = device(topology, x, Wt, 5, 4, 4, 3, lex, lm, scores=None, alpha=0.0)
    b = device(topology, x, Wt, 5, 4, 4, 3, lex, lm, scores="unigram", alpha=0.0)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and any(s for h in a[0] for s in h)


@BOUNDARIES
def test_the_transducer_entry_without_transitions_is_the_ctc_entry_bit_for_bit(tmp_path, boundary):
    _, lex, lm, _, x = identity_inputs(tmp_path, boundary, 1540)
    for normalize in (False, True):
        a = device("ctc", x, None, 5, 8, 4, 3, lex, lm, normalize=normalize)
        b = device("optional", x, None, 5, 8, 4, 3, lex, lm, normalize=normalize)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and any(s for h in a[0] for s in h)


@BOUNDARIES
@TOPOLOGIES
def test_the_same_call_twice_is_bit_identical(tmp_path, boundary, topology):
    rs = np.random.RandomState(1560)
    spellings = random_lexicon(rs, boundary, 30, 29, 40, 3, 6)
    lm, _ = make_lms(tmp_path, LR.random_arpa(rs, names_of(40), 2, 0.2), 40)
    x = emissions(1561, 4, 50, 30, 1.5)
    lex = pack(spellings, 30, 29, boundary)
    Wt = None if topology == "ctc" else transitions(1570, 30)
    a = device(topology, x, Wt, 29, 64, 30, 4, lex, lm)
    b = device(topology, x, Wt, 29, 64, 30, 4, lex, lm)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------------------------
# the narrow-beam cases (tests/test_beam_lookahead_abi.py checks them on the CPU)
# ------------------------------------------------------------------------------------------------------------------
TWO = {(1, 2, 4): 0, (1, 3, 4): 1}
TWO_TEXT = "\\data\\\nngram 1=4\n\n\\1-grams:\n-1.0\t<s>\n-1.0\t</s>\n-2.0\tw0\n-0.0043648\tw1\n\n\\end\\\n"
BEST = -0.5100503234139004


@BOUNDARIES
@TOPOLOGIES
def test_the_narrow_beam_keeps_the_word_the_lm_wants(tmp_path, boundary, topology):
    """C = 5, the blank 0, the words (1, 2, 4) and (1, 3, 4), log10 p = -2.0 and -0.0043648; alpha = 1, omega = beta = 0,
    no </s>, K = 4 (the forced topology enters a token from the blank only: a blank frame around each of the three)"""
    lm, ref_lm = make_lms(tmp_path, TWO_TEXT, 2)
    x = np.full((1, 3, 5), -4.0, np.float32)
    x[0, 0, 1], x[0, 1, 2], x[0, 1, 3], x[0, 2, 4] = 0.0, 0.0, -0.5, 0.0
    if topology == "forced":
        wide = np.full((1, 7, 5), -4.0, np.float32)
        wide[0, 0::2, 0] = 0.0
        wide[0, 1::2] = x[0]
        x = wide
    lex = pack(TWO, 5, 0, boundary)
    args = dict(alpha=1.0, omega=0.0, beta=0.0, eos=False)
    got = {}
    for W in (1, 64):
        for scores in (None, "unigram"):
            want = reference(topology, boundary, x, None, 0, W, 4, 1, TWO, ref_lm, scores, **args)
            seqs, raw = device(topology, x, None, 0, W, 4, 1, lex, lm, scores, **args)
            assert seqs[0] == [want[0][0][0]] and (raw[0, 0] == NEG if want[0][0][1] == NEG else
                                                   abs(raw[0, 0] - want[0][0][1]) <= 1e-9), (W, scores, seqs, raw, want)
            got[W, scores] = (seqs[0][0], raw[0, 0])
    if topology == "ctc":
        assert abs(got[64, None][1] - BEST) <= 1e-9
    top = got[64, None]
    assert top[0] == (1, 3, 4) and got[64, "unigram"][0] == (1, 3, 4) and abs(got[64, "unigram"][1] - top[1]) <= 1e-9
    # today's search at W = 1 follows the acoustics into (1, 2): nothing (end-marked), or the word the LM rates at 0.01
    assert got[1, None][0] == (() if boundary == "end" else (1, 2, 4)) and got[1, None][1] < top[1] - 2.0
    # with look-ahead W = 1 returns the W = 64 top result
    assert got[1, "unigram"][0] == (1, 3, 4) and abs(got[1, "unigram"][1] - top[1]) <= 1e-9


# ------------------------------------------------------------------------------------------------------------------
# edge cases
# ------------------------------------------------------------------------------------------------------------------
@BOUNDARIES
@TOPOLOGIES
@pytest.mark.parametrize("omega", [50.0, -50.0])
def test_the_skip_bound_under_a_negative_weight_and_a_large_word_bonus(tmp_path, boundary, topology, omega):
    """alpha < 0 turns every range of rule 6 around, omega = +-50 moves the word term far from the inner term: the
    restatement never skips a lookup, so a bound that is no proof shows as a missing hypothesis"""
    spellings = LEXICONS[boundary]
    rs = np.random.RandomState(1680)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    x = np.concatenate([emissions(1681, 1, 14, 6, 2.0), spelled(1682, 2, 14, 6, 5, random_sentences(rs, spellings, 2, 3), hi=4.0)])
    compare(topology, boundary, x, transitions(1690, 6), 5, 8, 5, 3, spellings, lm, ref_lm, alpha=-0.9, omega=omega)
    compare(topology, boundary, x, transitions(1690, 6), 5, 3, 5, 3, spellings, lm, ref_lm, alpha=-0.9, omega=omega,
            scores=[3.0, -2.0, 0.5, -7.0, 1.0])


@BOUNDARIES
@TOPOLOGIES
def test_a_word_the_lm_cannot_follow(tmp_path, boundary, topology):
    """word 1 has probability 0 under the LM: its look-ahead is the substitute, its step -inf -- it is dropped as a
    completed word (rule 2) and, start-marked, as the pending one (rule 4)"""
    spellings = LEXICONS[boundary]
    lines = []
    for line in LR.random_arpa(np.random.RandomState(1640), names_of(5), 2, 0.6).split("\n"):
        f = line.split("\t")
        if len(f) >= 2 and f[1].split()[-1] == "w1":
            f[0] = "-inf"  # (every gram that ends in the word: its step is -inf from every history)
        lines.append("\t".join(f))
    lm, ref_lm = make_lms(tmp_path, "\n".join(lines), 5)
    assert ref_lm.step(ref_lm.start, 1)[0] == NEG and lm.step(lm.start, 1)[0] == NEG and lm.unigram_scores()[1] == NEG
    order = sorted(spellings, key=lambda s: spellings[s])
    sentences = [[order[1]], [order[3], order[1]], [order[1], order[3]]]
    x = spelled(1650, 3, 16, 6, 5, sentences, hi=6.0, noise=0.5)
    want, seqs, _ = compare(topology, boundary, x, transitions(1660, 6), 5, 8, 4, 3, spellings, lm, ref_lm)
    assert all(1 not in words_of(spellings, boundary, s) for h in seqs for s in h)
    assert any(s for h in seqs for s in h)


@TOPOLOGIES
def test_a_word_that_is_a_proper_prefix_of_two_others(tmp_path, topology):
    """"_a", "_a n", "_a n t" with an LM that rates the longest best: all decoded from emissions that spell them -- a
    terminal node's look-ahead counts its own word and those below it"""
    text = "\\data\\\nngram 1=7\n\n\\1-grams:\n-1.0\t<s>\n-1.0\t</s>\n-2.0\tw0\n-1.0\tw1\n-0.1\tw2\n-0.5\tw3\n-1.5\tw4\n\n\\end\\\n"
    lm, ref_lm = make_lms(tmp_path, text, 5)
    sentences = [[(0,)], [(0, 2)], [(0, 2, 3)], [(0,), (0,)], [(0, 2), (0,), (0, 2, 3), (1, 4)]]
    x = spelled(1600, 5, 24, 6, 5, sentences, hi=8.0, noise=0.5)
    want, seqs, _ = compare(topology, "start", x, 0.1 * transitions(1610, 6), 5, 8, 4, 2, NEST, lm, ref_lm, omega=0.0, beta=0.0)
    assert [s[0] for s in seqs] == [(0,), (0, 2), (0, 2, 3), (0, 0), (0, 2, 0, 0, 2, 3, 1, 4)]


@BOUNDARIES
@TOPOLOGIES
def test_an_explicit_score_array(tmp_path, boundary, topology):
    """word scores that are no unigram of the LM, a positive one among them: any finite array telescopes"""
    spellings, _, lm, ref_lm, x = identity_inputs(tmp_path, boundary, 1700)
    compare(topology, boundary, x, transitions(1710, 6), 5, 4, 4, 3, spellings, lm, ref_lm, scores=[-0.5, 2.0, -6.0, 0.0, -1.25])


# ------------------------------------------------------------------------------------------------------------------
# paths and refusals
# ------------------------------------------------------------------------------------------------------------------
@BOUNDARIES
@TOPOLOGIES
def test_a_call_without_the_keyword_is_the_search_it_was(tmp_path, boundary, topology):
    """against the restatement of the search without look-ahead (a look-ahead of zeros: tests/test_beam_lookahead_abi.py
    shows that to be the existing restatements bit for bit)"""
    spellings, _, lm, ref_lm, x = identity_inputs(tmp_path, boundary, 1800)
    compare(topology, boundary, x, transitions(1810, 6), 5, 4, 4, 3, spellings, lm, ref_lm, scores=None)


TOKENS = ["A", "T", "n", "t", "r"]  # the blank is class 5
WORDS = {"start": ["A", "An", "Ant", "T", "Tr"], "end": ["At", "Ant", "Tt", "Trt", "nnt"]}


@BOUNDARIES
def test_ctc_module_and_errors(tmp_path, boundary):
    _, M, ctc, _, _, Lexicon, _ = _mods()
    spellings = LEXICONS[boundary]
    lex = Lexicon.from_words(WORDS[boundary], TOKENS, 5, boundary=boundary)
    assert {tuple(s): v for v, s in enumerate(lex.spellings)} == spellings
    rs = np.random.RandomState(1900)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    T = 16
    x = np.concatenate([emissions(1901, 1, T, 6, 2.0), spelled(1902, 3, T, 6, 5, random_sentences(rs, spellings, 3, 4), hi=4.0)])
    lengths = [T, 11, T, 6]
    crit = ctc.CTC(5, False)
    xd = torch.from_numpy(x).cuda()
    opts = dict(lexicon=lex, lm=lm, lm_weight=ALPHA, word_bonus=OMEGA, length_bonus=BETA, lookahead="unigram")
    want = reference("ctc", boundary, x, None, 5, 8, 4, 2, spellings, ref_lm, lengths=lengths)
    hyps, scores = crit.beam_search(xd, 8, 4, 2, input_lengths=lengths, return_scores=True, **opts)
    logz = log_normaliser(x, None, lengths)
    for b in range(4):
        assert [tuple(p.tolist()) for p in hyps[b]] == [h for h, _ in want[b]], b
        for r, (seq, s) in enumerate(want[b]):
            if s > NEG:
                n = s - logz[b]
                assert S.normalised_close(float(scores[b, r]), n)
    assert sum(len(h[0]) > 0 for h in hyps) >= 3
    counter = M.ErrorCounter()
    targets = [rs.randint(0, 5, size=n).tolist() for n in (7, 1, 12, 3)]
    pred = crit.beam_search(xd, 8, 4, input_lengths=lengths, **opts)
    assert crit.errors(xd, targets, counter, input_lengths=lengths, beam_size=8, classes_per_frame=4, **opts) == \
        counter(pred, targets)


KINDS = [dict(blank="optional", allow_repeats=False), dict(blank="forced")]


@BOUNDARIES
@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_transducer_module_and_errors(tmp_path, boundary, ngram, kw):
    _, M, _, T, _, _, _ = _mods()
    forced = kw["blank"] == "forced"
    spellings = LEXICONS[boundary]
    crit = T.Transducer(TOKENS, {t: i for i, t in enumerate(TOKENS)}, ngram=ngram, **kw).cuda()
    if ngram > 0:
        params = (0.5 * np.random.RandomState(1910 + ngram).randn(crit.transition_params.numel())).astype(np.float32)
        with torch.no_grad():
            crit.transition_params.copy_(torch.from_numpy(params))
    lex = crit.word_lexicon(WORDS[boundary], boundary=boundary)
    assert {tuple(s): v for v, s in enumerate(lex.spellings)} == spellings
    rs = np.random.RandomState(1920 + ngram)
    lm, ref_lm = make_lms(tmp_path, LR.random_arpa(rs, names_of(5), 2, 0.6), 5)
    B, Tn = 4, 24
    x = np.concatenate([emissions(1921 + ngram, 1, Tn, 6, 1.0),
                        spelled(1922 + ngram + int(forced), 3, Tn, 6, 5, random_sentences(rs, spellings, 3, 5), hi=5.0, noise=1.0)])
    xd = torch.from_numpy(x).cuda()
    plan, kind = crit._beam_plan(xd, "test", 4, 3, 2, lex, lm, lookahead="unigram")
    assert plan.forced == forced and plan.lookahead is lex.unigram_lookahead(lm)
    xe, Wt = crit._beam_inputs(xd, kind)
    xe, Wt = xe.cpu().numpy(), None if Wt is None else Wt.cpu().numpy()
    opts = dict(lexicon=lex, lm=lm, lm_weight=ALPHA, word_bonus=OMEGA, length_bonus=BETA, lookahead="unigram")
    topology = "forced" if forced else "optional"
    want = reference(topology, boundary, xe, Wt, 5, 4, 3, 2, spellings, ref_lm)
    hyps, scores = crit.beam_search(xd, beam_size=4, classes_per_frame=3, nbest=2, return_scores=True, **opts)
    logz = log_normaliser(xe, Wt)
    assert [[tuple(p.tolist()) for p in h] for h in hyps] == [[s for s, _ in h] for h in want]
    for b in range(B):
        for r, (seq, s) in enumerate(want[b]):
            if s > NEG:
                n = s - logz[b]
                assert S.normalised_close(float(scores[b, r]), n), (b, r)
                assert crit.words(lex, hyps[b][r]) == words_of(spellings, boundary, seq)
    assert sum(len(h[0]) > 0 for h in hyps) >= 3
    counter = M.ErrorCounter()
    targets = [rs.randint(0, 5, size=n).tolist() for n in (7, 1, 12, 3)]
    pred = crit.beam_search(xd, beam_size=4, classes_per_frame=3, **opts)
    assert crit.errors(xd, targets, counter, beam_size=4, classes_per_frame=3, **opts) == counter(pred, targets)


def test_asg_refuses(tmp_path):
    _, _, _, _, asg, Lexicon, _ = _mods()
    crit = asg.ASG(2, num_replabels=1, use_garbage=True).cuda()
    lex = Lexicon([(0, 1), (1, 0)], 4, 3)
    lm, _ = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(1990), names_of(2), 2, 0.6), 2)
    x = torch.zeros(2, 5, 4, device="cuda")
    with pytest.raises(NotImplementedError, match="question of its own"):
        crit.beam_search(x, 4, lexicon=lex, lm=lm, lookahead="unigram")
    assert len(crit.beam_search(x, 4, lexicon=lex, lm=lm)) == 2
