"""What the eleven tests/test_gpu_*beam_search*.py files share, each stated once: the lazy import of the package, the
seeded inputs and LMs, the float64 normaliser, the loop over a restatement with its margin assertion, and the acceptance
of a comparison.  A plain module, imported as the restatements are; every file keeps its own device() -- the engine call
differs per search --, its cases and its tests.

The acceptance (assert_ranks): the sequences of all returned ranks are equal; unnormalised scores agree to
1e-9 max(1, |s|) -- both sides are float64 and differ in libm rounding only; normalised scores agree at the project's
loss bar (tests/test_gpu_configs.py: 1e-4 |want| + 2e-5), the device's normaliser being float32; a rank that is -inf
stays -inf; the blank never appears.  An utterance whose smallest selection margin in the restatement is below 1e-9
could legitimately come out differently: the seeds are fixed so that there is none, and margins_ok asserts that for
every utterance, so that none is left out of a comparison.  tests/test_beam_support.py shows, without a device, that
each of these bars still bites."""
import importlib
import math

import numpy as np
import torch

import beam_lm_reference as LR
import beam_reference as R

MARGIN = 1e-9
NEG = -math.inf


def package(*names):
    """the named parts of gtn_applications_amd -- "engine", "lm:NGramLM", "criterions.ctc:CTC" --, imported when called:
    collecting a GPU file needs no built library"""
    out = []
    for name in names:
        module, _, attr = name.partition(":")
        mod = importlib.import_module("gtn_applications_amd." + module)
        out.append(getattr(mod, attr) if attr else mod)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------
# inputs and LMs
# ------------------------------------------------------------------------------------------------------------------
def emissions(seed, B, T, C, scale):
    return (np.random.RandomState(seed).randn(B, T, C) * scale).astype(np.float32)


def transitions(seed, C):
    return (0.5 * np.random.RandomState(seed).randn(C + 1, C)).astype(np.float32)


def tokens_of(C):
    """the token names of a token LM over C classes, one of them the blank"""
    return [f"t{i}" for i in range(C - 1)]


def names_of(V):
    """the word names of a word LM over V words"""
    return [f"w{v}" for v in range(V)]


def make_lms(tmp_path, text, names, blank, name="lm.arpa"):
    """(the device's LM through the loader, the restatement's reading of the same text); (None, None) without text"""
    if text is None:
        return None, None
    NGramLM, = package("lm:NGramLM")
    p = tmp_path / name
    p.write_text(text)
    return NGramLM.from_arpa(str(p), names, blank), LR.ArpaLM(text, names, blank)


def token_lms(tmp_path, text, C, blank, tokens=None):
    """make_lms over the tokens of C classes"""
    return make_lms(tmp_path, text, tokens_of(C) if tokens is None else tokens, blank, "tokens.arpa")


def word_lms(tmp_path, text, V, name="words.arpa"):
    """make_lms over V words: word v is label v, the blank is V"""
    return make_lms(tmp_path, text, names_of(V), V, name)


def _favoured(x, b, frames, rest, hi):
    """+hi on frames[t] in frame t of utterance b, on `rest` behind them"""
    for t in range(x.shape[1]):
        x[b, t, frames[t] if t < len(frames) else rest] += hi


def spelled_tokens(seed, B, T, C, blank, hi=8.0, noise=0.5, run=2, letters=None):
    """emissions that spell a token sequence in a way both Transducer topologies accept: a blank frame first, every token
    (one of the first `letters` classes that are not the blank) for one to `run` frames with one blank frame behind it,
    blanks for what is left of the T frames; +hi on N(0, noise^2)"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, T, C) * noise).astype(np.float32)
    toks = [c for c in range(C) if c != blank][:letters]
    for b in range(B):
        frames = [blank]
        while True:
            more = [toks[rs.randint(len(toks))]] * int(rs.randint(1, run + 1)) + [blank]
            if len(frames) + len(more) > T:
                break
            frames += more
        _favoured(x, b, frames, blank, hi)
    return x


def spelled_sentences(seed, B, T, C, blank, sentences, hi=8.0, noise=0.5, run=2):
    """emissions that spell sentences[b] (a list of spellings) in a way every topology accepts: a blank frame first, every
    label for one to `run` frames with one blank frame behind it, blanks for what is left of the T frames; +hi on
    N(0, noise^2).  A sentence that does not fit is cut at a word."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, T, C) * noise).astype(np.float32)
    for b in range(B):
        frames = [blank]
        for word in sentences[b % len(sentences)]:
            more = []
            for c in word:
                more += [c] * int(rs.randint(1, run + 1)) + [blank]
            if len(frames) + len(more) > T:
                break
            frames += more
        _favoured(x, b, frames, blank, hi)
    return x


def random_sentences(rs, spellings, count, words):
    """`count` sentences of `words` spellings each, drawn from a lexicon {spelling: word id}"""
    order = sorted(spellings)
    return [[order[rs.randint(len(order))] for _ in range(words)] for _ in range(count)]


def spelled_asg(seed, B, T, C, spellings, garbage, hi=8.0):
    """emissions that spell a sentence of lexicon words in raw ASG classes, every class for one or two frames, the garbage
    (where there is one) between some of them; what is left of the T frames repeats the last class; +hi on
    N(0, 0.5^2) noise -- complete-word hypotheses survive the beam"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, T, C) * 0.5).astype(np.float32)
    words = sorted(spellings, key=spellings.get)
    for b in range(B):
        frames = []
        while True:
            more = []
            for c in words[rs.randint(len(words))]:
                if garbage is not None and rs.rand() < 0.4:
                    more += [garbage] * int(rs.randint(1, 3))
                more += [c] * int(rs.randint(1, 3))
            if len(frames) + len(more) > T:
                break
            frames += more
        if not frames:
            frames = [garbage if garbage is not None else 0]
        _favoured(x, b, frames, frames[-1], hi)
    return x


# ------------------------------------------------------------------------------------------------------------------
# the normalisers
# ------------------------------------------------------------------------------------------------------------------
def log_normaliser(x, Wt, lengths=None):
    """[B] float64: the normaliser a normalised score is held against, in float64 by torch on the device, independent of
    the library; a NaN counts as -inf, in x and in Wt.  With transitions the log of the summed mass of all frame paths by
    the forward recursion (ASG's denominator, the Transducer's rule 7), without them the rows' log-sum-exps over
    t < lengths[b] (all T frames without lengths; with transitions lengths are not read: no entry with them takes any).

    It stands for four earlier copies, which agree on every input the tests pass.  The ASG files' and the Transducer
    lexicon / token-LM files' cleaned the NaNs of Wt, and need it (their NaN tests: "nans count as minus infinity"); the
    start-marked and look-ahead files' did not, and never pass a Wt with a NaN, so cleaning changes nothing for them;
    only those two pass lengths.  tests/test_gpu_transducer_beam_search.py (and the merged file through it) formed the
    same sums in numpy on the host: float64 either way, apart by rounding, far inside the 1e-9 of its own helper test
    and the 1e-4 |n| + 2e-5 the result is used at."""
    xd = torch.from_numpy(x).cuda().double()
    xd = torch.where(torch.isnan(xd), torch.full_like(xd, NEG), xd)
    if Wt is None:
        lse = torch.logsumexp(xd, dim=2)
        if lengths is not None:
            keep = torch.arange(x.shape[1], device="cuda")[None, :] < torch.tensor(lengths, device="cuda")[:, None]
            lse = torch.where(keep, lse, torch.zeros_like(lse))
        return lse.sum(dim=1).cpu().numpy()
    Wd = torch.from_numpy(Wt).cuda().double()
    Wd = torch.where(torch.isnan(Wd), torch.full_like(Wd, NEG), Wd)
    alpha = xd[:, 0] + Wd[0]
    for t in range(1, x.shape[1]):
        alpha = torch.logsumexp(alpha[:, None, :] + Wd[1:][None], dim=2) + xd[:, t]
    return torch.logsumexp(alpha, dim=1).cpu().numpy()


def row_shift(rows):
    """the sum of the rows' log-sum-exps in plain Python: what CTC's normalisation subtracts from every score"""
    return sum(R.row_lse(R.clean(row)) for row in rows)


# ------------------------------------------------------------------------------------------------------------------
# the restatement per utterance, the acceptance
# ------------------------------------------------------------------------------------------------------------------
def utterances(x, lengths=None):
    """the rows of each utterance: x[b], cut at lengths[b] if given"""
    return [x[b] if lengths is None else x[b][:lengths[b]] for b in range(x.shape[0])]


def margins_ok(search, B, found=None):
    """[search(b) for b < B], a restatement's (hyps, margin, ...) per utterance, with margin >= MARGIN asserted for every
    one of them: no utterance is left out of a comparison.  found(hyps) -> bool, if given: the emissions spell
    something, and rank 0 must show it for at least three quarters of the utterances -- a comparison of empty beams
    shows nothing."""
    out = []
    for b in range(B):
        res = search(b)
        assert res[1] >= MARGIN, (b, res[1])
        out.append(res)
    if found is not None:
        hits = sum(1 for res in out if res[0][0][1] > NEG and found(res[0]))
        assert 4 * hits >= 3 * B, (hits, B)
    return out


def raw_close(got, s):
    """an unnormalised score against the restatement's: float64 on both sides, apart by libm rounding only"""
    return abs(got - s) <= 1e-9 * max(1.0, abs(s))


def normalised_close(got, n):
    """a normalised score at the project's loss bar (tests/test_gpu_configs.py): the device's normaliser is float32"""
    return abs(got - n) <= 1e-4 * abs(n) + 2e-5


def assert_ranks(want, seqs, raw, normed, logz, nbest, blank=None, check=None):
    """The acceptance of a comparison, rank by rank.  want[b]: the restatement's nbest (sequence, score) pairs, or None
    for an utterance that is left out (the merged search alone does that); seqs[b][r], raw[b][r], normed[b][r]: what the
    device returned without and with normalisation; logz[b]: the float64 normaliser of utterance b; check(b, r, seq):
    a file's own demands on every returned sequence.  Works on numpy arrays and on lists."""
    for b, hyps in enumerate(want):
        if blank is not None:
            assert all(blank not in s for s in seqs[b]), (b, seqs[b])
        if hyps is None:
            continue
        assert list(seqs[b]) == [h for h, _ in hyps], (b, seqs[b], hyps)
        for r in range(nbest):
            s = hyps[r][1]
            if check is not None:
                check(b, r, seqs[b][r])
            if s == NEG:
                assert raw[b][r] == NEG and normed[b][r] == NEG, (b, r)
                continue
            n = s - logz[b]
            assert raw_close(raw[b][r], s), (b, r, raw[b][r], s)
            assert normalised_close(normed[b][r], n), (b, r, normed[b][r], n)
