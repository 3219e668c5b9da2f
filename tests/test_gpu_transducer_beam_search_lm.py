"""Transducer beam search with a token-level n-gram LM on the device (csrc/beam_kernels.hip:
wfl_transducer_beam_search_lm behind engine.transducer_beam_search_lm, Transducer.beam_search(token_lm=) and
Transducer.errors(beam_size=, token_lm=)) against its restatement in plain Python
(tests/transducer_beam_lm_reference.py, itself pinned to a brute-force enumeration in
tests/test_transducer_beam_lm_abi.py).

Acceptance of every comparison, as in tests/test_gpu_transducer_beam_search_lexicon.py: the token sequences of all
returned ranks are equal; unnormalised scores agree to 1e-9 max(1, |s|) -- both sides are float64 and differ in libm
rounding only; normalised scores agree at the project's loss bar (1e-4 |want| + 2e-5) against a float64 normaliser
computed with torch, independently of the library, the device's logz being float32; the blank never appears in a
result.  An utterance whose smallest selection margin in the reference is below 1e-9 could legitimately come out
differently: the seeds are fixed so that there is none, and every comparison asserts that.  On emissions that spell
token sequences the reference's rank 0 is non-empty for at least three quarters of the utterances: asserted too, a
comparison of empty beams shows nothing.

A universe is (C classes, the blank's class): the tokens t0, t1, .. are the other classes in ascending order.  LMs are
seeded random ARPA texts over the token names, written into tmp_path and loaded through NGramLM.from_arpa(path, tokens,
blank) for the device and read by beam_lm_reference.ArpaLM for the reference."""
import math
import os

import numpy as np
import pytest
import torch

import beam_lm_reference as LR
import beam_support as S
import transducer_beam_lm_reference as TL
import transducer_beam_reference as TR
from beam_support import emissions, log_normaliser, tokens_of, transitions
from beam_support import spelled_tokens as spelled
from beam_support import token_lms as make_lms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = TR.NEG
ALPHA, BETA = 0.8, 0.5
TOPOLOGIES = pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])


def _mods():
    return S.package("engine", "metrics", "criterions.transducer", "lm:NGramLM")


def reference(x, Wt, blank, forced, W, K, nbest, ref_lm, alpha=ALPHA, beta=BETA, eos=True, spells=False, on_frame=None):
    """per utterance the reference's hyps; asserts the margins, so that no utterance is left out of a comparison, and --
    `spells`: the emissions spell token sequences -- that rank 0 is non-empty for three quarters of the utterances"""

    def search(b):
        hook = None if on_frame is None else (lambda *a: on_frame(b, *a))
        return TL.beam_search(x[b], Wt, blank, forced, W, K, nbest, ref_lm, alpha, beta, eos, on_frame=hook)

    found = (lambda hyps: len(hyps[0][0]) >= 1) if spells else None
    return [res[0] for res in S.margins_ok(search, x.shape[0], found)]


def device(x, Wt, blank, forced, W, K, nbest, lm, alpha=ALPHA, beta=BETA, eos=True, normalize=False):
    E = _mods()[0]
    xd = torch.from_numpy(x).cuda()
    Wd = None if Wt is None else torch.from_numpy(Wt).cuda()
    hyps, scores = E.transducer_beam_search_lm(xd, Wd, blank, lm, forced, W, K, nbest, normalize=normalize, lm_weight=alpha,
                                               length_bonus=beta, lm_eos=eos)
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (x.shape[0], nbest) and not scores.is_cuda
    assert all(len(h) == nbest and all(s.dtype == torch.int64 and not s.is_cuda for s in h) for h in hyps)
    return [[tuple(s.tolist()) for s in h] for h in hyps], scores.numpy()


def compare(x, Wt, blank, forced, W, K, nbest, lm, ref_lm, alpha=ALPHA, beta=BETA, eos=True, spells=False, on_frame=None):
    want = reference(x, Wt, blank, forced, W, K, nbest, ref_lm, alpha, beta, eos, spells, on_frame)
    seqs, raw = device(x, Wt, blank, forced, W, K, nbest, lm, alpha, beta, eos)
    nseqs, normed = device(x, Wt, blank, forced, W, K, nbest, lm, alpha, beta, eos, normalize=True)
    assert nseqs == seqs  # (the shift never changes the search)
    S.assert_ranks(want, seqs, raw, normed, log_normaliser(x, Wt), nbest, blank)
    return want, seqs, raw


# ------------------------------------------------------------------------------------------------------------------
# the shapes of the issue, (T, C, W, K, B)
# ------------------------------------------------------------------------------------------------------------------
ONE_FRAME = "\\data\\\nngram 1=4\n\n\\1-grams:\n-9.0\t<s>\n-1.0\t</s>\n-0.5\tt0\n-2.0\tt1\n\n\\end\\\n"


def one_frame_case():
    blank = 2
    x = np.array([[[3.0, 0.0, 1.0]], [[0.0, 3.0, 1.0]], [[0.0, 1.0, 3.0]], [[1.0, -np.inf, 0.0]]], np.float32)
    return x, transitions(100, 3), blank


def test_one_frame(tmp_path):
    """(1, 3, 1, 2, 4).  Forced: no extension in frame 0, only the empty sequence, scored by the blank's frame and
    a step(start, </s>).  Optional: a one-token result carries its LM term, the length bonus and </s>."""
    x, Wt, blank = one_frame_case()
    lm, ref_lm = make_lms(tmp_path, ONE_FRAME, 3, blank)
    ln10 = math.log(10.0)
    end = ALPHA * (-1.0 * ln10)
    for W in (None, Wt):
        want, seqs, raw = compare(x, W, blank, True, 1, 2, 1, lm, ref_lm)
        assert seqs == [[()]] * 4
        for b in range(4):
            mass = float(x[b, 0, blank]) + (0.0 if W is None else float(W[0, blank]))
            assert abs(raw[b, 0] - (mass + end)) <= 1e-9, (b, raw[b, 0], mass + end)
        want, seqs, raw = compare(x, W, blank, False, 1, 2, 1, lm, ref_lm)
        assert seqs[0] == [(0,)] and seqs[2] == [()] and all(len(h[0]) <= 1 for h in seqs)
        unigram = {0: -0.5 * ln10, 1: -2.0 * ln10}
        for b in range(4):
            c = seqs[b][0][0] if seqs[b][0] else blank
            mass = float(x[b, 0, c]) + (0.0 if W is None else float(W[0, c]))
            term = 0.0 if c == blank else ALPHA * unigram[c] + BETA
            assert abs(raw[b, 0] - ((mass + term) + end)) <= 1e-9, (b, c, raw[b, 0])
    # without </s> the empty sequence scores its mass alone
    _, seqs, raw = compare(x, Wt, blank, True, 1, 2, 1, lm, ref_lm, eos=False)
    assert seqs == [[()]] * 4 and all(abs(raw[b, 0] - (float(x[b, 0, blank]) + float(Wt[0, blank]))) <= 1e-9 for b in range(4))


def case_12(blank_last, order, seed=0):
    """(12, 6, 4, 3, 8) on emissions that spell token sequences: (x, Wt, blank, ARPA text)"""
    T, C, B = 12, 6, 8
    blank = C - 1 if blank_last else 0
    rs = np.random.RandomState(1200 + 10 * int(blank_last) + order + 100 * seed)
    text = LR.random_arpa(rs, tokens_of(C), order, 0.5)
    x = spelled(1201 + 10 * int(blank_last) + order + 100 * seed, B, T, C, blank, hi=4.0, noise=1.0)
    return x, transitions(1202 + seed, C), blank, text


@TOPOLOGIES
@pytest.mark.parametrize("eos", [True, False], ids=["eos", "noeos"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("blank_last", [True, False], ids=["blank-last", "blank-0"])
def test_twelve_frames_with_transitions(tmp_path, blank_last, order, eos, forced):
    x, Wt, blank, text = case_12(blank_last, order)
    lm, ref_lm = make_lms(tmp_path, text, 6, blank)
    assert lm.order == order
    for nbest in (1, 4):
        compare(x, Wt, blank, forced, 4, 3, nbest, lm, ref_lm, eos=eos, spells=True)


def without_token(whole, text, C, blank, gone):
    """(the device's LM, the reference's) of `whole` / `text` with every arc of class `gone` taken out: the pack is
    constructed directly (the loader would refuse a token without a unigram), the reference reads the text without the
    lines that name the token (it does not count its sections)"""
    NGramLM = _mods()[3]
    keep = whole.arc_label != gone
    ptr = np.concatenate([[0], np.cumsum([keep[whole.arc_ptr[s]:whole.arc_ptr[s + 1]].sum() for s in range(whole.num_states)])])
    lm = NGramLM(C, blank, ptr, whole.arc_label[keep], whole.arc_next[keep], whole.arc_w[keep], whole.bo_next, whole.bo_w,
                 start=whole.start, order=whole.order)
    word = tokens_of(C)[gone if gone < blank else gone - 1]
    cut = "\n".join(l for l in text.split("\n") if word not in l.split())
    return lm, LR.ArpaLM(cut, tokens_of(C), blank)


def no_arc_case(blank_last):
    x, Wt, blank, text = case_12(blank_last, 2, seed=1)
    gone = 2
    x[:, :, gone] += 1.5  # (the emissions favour it)
    return x, Wt, blank, text, gone


@TOPOLOGIES
@pytest.mark.parametrize("blank_last", [True, False], ids=["blank-last", "blank-0"])
def test_a_token_without_an_arc_anywhere_is_never_returned(tmp_path, blank_last, forced):
    x, Wt, blank, text, gone = no_arc_case(blank_last)
    whole, _ = make_lms(tmp_path, text, 6, blank)
    assert any(gone in s for h in device(x, Wt, blank, forced, 4, 3, 4, whole)[0] for s in h)  # (with its arcs it is)
    lm, ref_lm = without_token(whole, text, 6, blank, gone)
    assert lm.num_arcs < whole.num_arcs and lm.score([gone]) == -math.inf
    _, seqs, _ = compare(x, Wt, blank, forced, 4, 3, 4, lm, ref_lm)
    assert not any(gone in s for h in seqs for s in h)
    assert any(len(s) > 0 for h in seqs for s in h)


def wide_case(forced):
    """(40, 40, 64, 39, 2): (x, Wt, blank, ARPA text) -- a bigram LM that knows every token, so every extension lives"""
    T, C, B = 40, 40, 2
    blank = C - 1
    text = LR.random_arpa(np.random.RandomState(4003), tokens_of(C), 2, 0.3)
    x = spelled(4000 + int(forced), B, T, C, blank, hi=3.0, noise=1.0, letters=12)
    return x, transitions(4002, C), blank, text


@TOPOLOGIES
def test_the_wide_instantiation_and_the_radix_select(tmp_path, forced):
    x, Wt, blank, text = wide_case(forced)
    lm, ref_lm = make_lms(tmp_path, text, 40, blank)
    most = [0]

    def on_frame(b, t, beam, cand, extension, merged, entries):
        most[0] = max(most[0], len(entries))

    compare(x, Wt, blank, forced, 64, 39, 3, lm, ref_lm, spells=True, on_frame=on_frame)
    assert most[0] > 512, most  # (the select runs only on a list longer than that)


def benchmark_pieces():
    with open(os.path.join(ROOT, "benchmarks", "word_pieces_tokens_1000.txt")) as f:
        tokens = sorted(l.rstrip("\n") for l in f if l.rstrip("\n"))
    g2i = {g: i for i, g in enumerate(sorted(set(c for t in tokens for c in t)))}
    return tokens, g2i


def pieces_text(tokens):
    """a seeded bigram ARPA text with all 1000 unigrams: the arc search of the unigram state runs at its full depth"""
    return LR.random_arpa(np.random.RandomState(1004), tokens, 2, 0.002)


@TOPOLOGIES
def test_the_class_count_of_the_word_piece_recipes(tmp_path, forced):
    """(3, 1001, 4, 64, 1): a module over the recipe's 1000 word pieces with the bigram transition model, the LM read by
    Transducer.token_lm"""
    T = _mods()[2]
    tokens, g2i = benchmark_pieces()
    assert len(tokens) == 1000
    crit = T.Transducer(tokens, g2i, ngram=2, **(dict(blank="forced") if forced else dict(blank="optional", allow_repeats=False)))
    crit = crit.cuda()
    params = (0.5 * np.random.RandomState(1003).randn(crit.transition_params.numel())).astype(np.float32)
    with torch.no_grad():
        crit.transition_params.copy_(torch.from_numpy(params))
    text = pieces_text(tokens)
    p = tmp_path / "pieces.arpa"
    p.write_text(text)
    lm = crit.token_lm(str(p))
    C, blank = 1001, 1000
    assert (lm.num_classes, lm.blank, lm.order) == (C, blank, 2) and lm.num_arcs > 1001
    base = lm.start
    while lm.bo_next[base] >= 0:
        base = int(lm.bo_next[base])
    assert lm.arc_ptr[base + 1] - lm.arc_ptr[base] == 1001  # (every piece and </s>)
    ref_lm = LR.ArpaLM(text, tokens, blank)
    x = spelled(1002 + int(forced), 1, 3, C, blank, hi=6.0, noise=1.0, run=1)
    xd = torch.from_numpy(x).cuda()
    plan, kind = crit._beam_plan(xd, "test", 4, 64, 3, token_lm=lm, lm_weight=ALPHA, length_bonus=BETA)
    assert kind == "bigram" and plan.forced == forced
    xe, Wt = crit._beam_inputs(xd, kind)
    xe, Wt = xe.cpu().numpy(), Wt.cpu().numpy()
    want, seqs, _ = compare(xe, Wt, blank, forced, 4, 64, 3, lm, ref_lm, spells=True)
    hyps, scores = crit.beam_search(xd, beam_size=4, classes_per_frame=64, nbest=3, return_scores=True, token_lm=lm,
                                    lm_weight=ALPHA, length_bonus=BETA)
    assert [[tuple(p.tolist()) for p in h] for h in hyps] == seqs
    logz = log_normaliser(xe, Wt)
    for r, (_, s) in enumerate(want[0]):
        if s > NEG:
            n = s - logz[0]
            assert S.normalised_close(float(scores[0, r]), n), (r, float(scores[0, r]), n)


def two_hundred_case(forced):
    T, C, B, blank = 6, 5, 200, 4
    text = LR.random_arpa(np.random.RandomState(2000), tokens_of(C), 2, 0.5)
    x = spelled(2001 + int(forced), B, T, C, blank, hi=7.0, noise=1.0, run=1)
    return x, transitions(2002, C), blank, text


@TOPOLOGIES
def test_two_hundred_utterances_in_one_call(tmp_path, forced):
    """(6, 5, 2, 4, 200)"""
    x, Wt, blank, text = two_hundred_case(forced)
    lm, ref_lm = make_lms(tmp_path, text, 5, blank)
    compare(x, Wt, blank, forced, 2, 4, 2, lm, ref_lm, spells=True)


def test_without_transitions_the_optional_topology_is_the_ctc_lm_search_bit_for_bit(tmp_path):
    E = _mods()[0]
    for (T, C, W, K, B), blank, order in (((60, 29, 16, 8, 3), 28, 2), ((40, 40, 64, 39, 2), 0, 3), ((12, 6, 4, 3, 50), 3, 1)):
        rs = np.random.RandomState(900 + T)
        lm, _ = make_lms(tmp_path, LR.random_arpa(rs, tokens_of(C), order, 0.3), C, blank)
        x = np.concatenate([emissions(901 + T, B - B // 2, T, C, 1.0), spelled(902 + T, B // 2, T, C, blank)])
        xd = torch.from_numpy(x).cuda()
        kw = dict(lm_weight=ALPHA, length_bonus=BETA)
        found = 0
        for normalize in (False, True):
            for eos in (True, False):
                a_h, a_s = E.transducer_beam_search_lm(xd, None, blank, lm, False, W, K, min(3, W), normalize=normalize, lm_eos=eos,
                                                       **kw)
                c_h, c_s = E.ctc_beam_search(xd, blank, W, K, min(3, W), normalize=normalize, lm=lm, lm_eos=eos, **kw)
                assert [[s.tolist() for s in h] for h in a_h] == [[s.tolist() for s in h] for h in c_h]
                assert a_s.numpy().tobytes() == c_s.numpy().tobytes()
                found += sum(len(h[0]) > 0 for h in a_h)
        assert found >= B // 2


# ------------------------------------------------------------------------------------------------------------------
# edge values: finite-arithmetic cases that the rules define
# ------------------------------------------------------------------------------------------------------------------
def edge_case(seed, B=4, T=20, C=8, order=2):
    blank = C - 1
    text = LR.random_arpa(np.random.RandomState(seed), tokens_of(C), order, 0.4)
    x = np.concatenate([emissions(seed + 1, B // 2, T, C, 1.0), spelled(seed + 2, B - B // 2, T, C, blank, hi=4.0)])
    return x, transitions(seed + 3, C), blank, text


def half_forbidden_case():
    x, Wt, blank, text = edge_case(41)
    C = x.shape[2]
    mask = np.random.RandomState(44).rand(C + 1, C) < 0.5
    mask[0, blank] = mask[1 + blank, blank] = False  # (start -> blank and blank -> blank stay: the empty prefix lives)
    Wt[mask] = -np.inf
    return x, Wt, blank, text


@TOPOLOGIES
def test_half_the_transitions_forbidden(tmp_path, forced):
    x, Wt, blank, text = half_forbidden_case()
    lm, ref_lm = make_lms(tmp_path, text, 8, blank)
    want, _, _ = compare(x, Wt, blank, forced, 16, 8, 3, lm, ref_lm)
    assert all(h[0][1] > NEG for h in want)


def nan_case():
    x, Wt, blank, text = edge_case(14)
    rs = np.random.RandomState(15)
    x[rs.rand(*x.shape) < 0.2] = np.nan
    Wt[rs.rand(*Wt.shape) < 0.2] = np.nan
    x[:, :, blank] = np.where(np.isnan(x[:, :, blank]), 0.25, x[:, :, blank])  # (the blank stays possible: no utterance dies)
    Wt[0, blank] = 0.125
    Wt[1 + blank] = np.where(np.isnan(Wt[1 + blank]), 0.125, Wt[1 + blank])  # (and can be entered from everywhere)
    return x, Wt, blank, text


@TOPOLOGIES
def test_scattered_nans_count_as_minus_infinity(tmp_path, forced):
    x, Wt, blank, text = nan_case()
    lm, ref_lm = make_lms(tmp_path, text, 8, blank)
    want, _, _ = compare(x, Wt, blank, forced, 8, 8, 3, lm, ref_lm)
    assert sum(h[0][1] > NEG for h in want) >= 3
    y = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    Vt = np.where(np.isnan(Wt), -np.inf, Wt).astype(np.float32)
    a, b = device(x, Wt, blank, forced, 8, 8, 3, lm), device(y, Vt, blank, forced, 8, 8, 3, lm)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


def blank_only_case():
    x, Wt, blank, text = edge_case(21)
    x[:, 9, :] = -np.inf
    x[:, 9, blank] = 0.5
    x[1, 0, :] = np.nan
    x[1, 0, blank] = -1.0
    return x, Wt, blank, text


@TOPOLOGIES
def test_a_frame_with_only_the_blank_finite(tmp_path, forced):
    x, Wt, blank, text = blank_only_case()
    lm, ref_lm = make_lms(tmp_path, text, 8, blank)
    compare(x, Wt, blank, forced, 8, 8, 3, lm, ref_lm)
    compare(x, Wt, blank, forced, 8, 3, 3, lm, ref_lm)


def impossible_case():
    x, Wt, blank, text = edge_case(16)
    y = x.copy()
    y[1, 11, :] = -np.inf
    y[1, 11, 5] = np.nan
    return x, y, Wt, blank, text


@TOPOLOGIES
def test_an_utterance_with_an_impossible_frame_decodes_to_nothing(tmp_path, forced):
    x, y, Wt, blank, text = impossible_case()
    lm, ref_lm = make_lms(tmp_path, text, 8, blank)
    alone = device(x[[0, 2, 3]], Wt, blank, forced, 8, 8, 3, lm)
    want, seqs, raw = compare(y, Wt, blank, forced, 8, 8, 3, lm, ref_lm)
    assert want[1] == [((), NEG)] * 3 and seqs[1] == [(), (), ()] and (raw[1] == NEG).all()
    assert [seqs[0], seqs[2], seqs[3]] == alone[0] and (raw[[0, 2, 3]] == alone[1]).all()  # (its neighbours are unaffected)


class ChainLM:
    """A hand-made back-off acceptor over C classes whose chain is as deep as the cap: states 0 .. D, state s < D backs
    off to s + 1 and has one arc of its own, state D (no back-off) has an arc for every token and </s>; all arcs lead
    back into the chain.  step() is the rule of include/wfl.h over dicts -- the reference's side; pack() the arrays of
    the same acceptor for NGramLM -- the device's."""

    def __init__(self, seed, C, blank, depth):
        rs = np.random.RandomState(seed)
        self.C, self.blank, self.depth, self.start = C, blank, depth, 0
        toks = [c for c in range(C) if c != blank]
        self.arcs, self.bo = [], []
        for s in range(depth):
            c = toks[s % len(toks)]
            self.arcs.append({c: (-0.1 - 2.0 * rs.rand(), (s + 1) % depth)})
            self.bo.append((-rs.rand(), s + 1))
        self.arcs.append({c: (-0.1 - 2.0 * rs.rand(), int(rs.randint(depth))) for c in toks + [C]})
        self.bo.append(None)

    def step(self, s, c):
        c = self.C if c == LR.EOS else c
        acc = 0.0
        while True:
            if c in self.arcs[s]:
                w, nxt = self.arcs[s][c]
                return acc + w, nxt
            if self.bo[s] is None:
                return NEG, None
            acc += self.bo[s][0]
            s = self.bo[s][1]

    def pack(self):
        NGramLM = _mods()[3]
        ptr, label, nxt, w = [0], [], [], []
        for arcs in self.arcs:
            for c in sorted(arcs):
                label.append(c), w.append(arcs[c][0]), nxt.append(arcs[c][1])
            ptr.append(len(label))
        return NGramLM(self.C, self.blank, ptr, label, nxt, w, [-1 if b is None else b[1] for b in self.bo],
                       [0.0 if b is None else b[0] for b in self.bo], start=0)


@TOPOLOGIES
def test_a_back_off_chain_as_deep_as_the_cap(forced):
    x, Wt, blank, _ = edge_case(31)
    depth = 8
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        assert f"WFL_NGRAM_LM_MAX_BACKOFF {depth}" in f.read()
    ref_lm = ChainLM(32, 8, blank, depth)
    lm = ref_lm.pack()
    assert lm.order == depth + 1  # (1 + the longest chain: the start state backs off `depth` times)
    assert lm.step(0, 8) == ref_lm.step(0, LR.EOS) and lm.step(0, 8)[0] > NEG
    walked = [0]

    def on_frame(b, t, beam, cand, extension, merged, entries):
        walked[0] += sum(1 for h in beam if h[0] and h[3] == 0)  # (at the deepest state: its lookups walk the whole chain)

    want, seqs, _ = compare(x, Wt, blank, forced, 8, 8, 3, lm, ref_lm, on_frame=on_frame)
    assert walked[0] >= 20 and any(len(s) > 0 for h in seqs for s in h)
    # a chain one deeper is refused where the pack is checked
    with pytest.raises(ValueError, match="deeper"):
        ChainLM(32, 8, blank, depth + 1).pack()


def lm_off_cases():
    return (((20, 8, 8, 8, 4), 7), ((40, 40, 64, 39, 2), 0), ((12, 6, 4, 3, 8), 3))


@TOPOLOGIES
def test_lm_off_inside_the_lm_path_is_the_plain_transducer_search(tmp_path, forced):
    """lm_weight = 0, length_bonus = 0, no </s> and a complete unigram LM (no step is -inf): every LM term is 0, so the
    sequences are those of wfl_transducer_beam_search and the raw scores agree to 1e-9, absolutely"""
    E = _mods()[0]
    for (T, C, W, K, B), blank in lm_off_cases():
        x = np.concatenate([emissions(40 + C, B // 2, T, C, 1.0), spelled(41 + C, B - B // 2, T, C, blank, hi=4.0)])
        Wt = transitions(42 + C, C)
        lm, _ = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(C), tokens_of(C), 1, 1.0), C, blank)
        assert lm.order == 1 and lm.num_arcs == C
        seqs, raw = device(x, Wt, blank, forced, W, K, min(W, 4), lm, 0.0, 0.0, False)
        hyps, scores = E.transducer_beam_search(torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda(), blank, forced, W, K,
                                                min(W, 4), normalize=False)
        assert seqs == [[tuple(s.tolist()) for s in h] for h in hyps]
        plain = scores.numpy()
        both = np.isfinite(plain)
        assert (np.isfinite(raw) == both).all() and (np.abs(raw[both] - plain[both]) <= 1e-9).all()
        assert any(len(s) > 0 for h in seqs for s in h)


def full_beam_case(seed, forced):
    """A full beam (W = 4, K = 2) that holds a hypothesis none of whose extensions by this frame's candidates exists --
    the LM has no arc for one token and half the transitions are forbidden -- while another hypothesis is extended.
    Returns (x, Wt, blank, ARPA text, the token without an arc, the frames at which that happens)."""
    C, blank, W, K, gone = 7, 6, 4, 2, 1
    text = LR.random_arpa(np.random.RandomState(5), tokens_of(C), 2, 0.5)
    x, Wt = emissions(seed, 1, 14, C, 2.0), transitions(seed + 1, C)
    mask = np.random.RandomState(seed + 2).rand(C + 1, C) < 0.5
    mask[:, blank] = False  # (the blank can be entered from everywhere: every hypothesis has its stay)
    Wt[mask] = -np.inf
    word = tokens_of(C)[gone]
    ref_lm = LR.ArpaLM("\n".join(l for l in text.split("\n") if word not in l.split()), tokens_of(C), blank)
    hits = []

    def on_frame(t, beam, cand, extension, merged, entries):
        if len(beam) < W or (forced and t == 0):
            return
        own = [c for c, _ in cand if c != blank]
        dead = [i for i in range(len(beam)) if own and all(extension(i, c)[0] == NEG for c in own)]
        if dead and len(dead) < len(beam):
            hits.append(t)

    TL.beam_search(x[0], Wt, blank, forced, W, K, 3, ref_lm, ALPHA, BETA, True, on_frame=on_frame)
    return x, Wt, blank, text, gone, hits


FULL_BEAM_SEEDS = [22, 24]


@TOPOLOGIES
@pytest.mark.parametrize("seed", FULL_BEAM_SEEDS)
def test_a_full_beam_with_a_hypothesis_that_no_candidate_extends(tmp_path, seed, forced):
    x, Wt, blank, text, gone, hits = full_beam_case(seed, forced)
    assert hits, "the case is not what it says"
    whole, _ = make_lms(tmp_path, text, 7, blank)
    lm, ref_lm = without_token(whole, text, 7, blank, gone)
    _, seqs, raw = compare(x, Wt, blank, forced, 4, 2, 3, lm, ref_lm)
    assert raw[0, 0] > NEG and len(seqs[0][0]) > 0


def test_the_same_call_twice_is_bit_identical(tmp_path):
    T, C, B, blank = 40, 30, 4, 29
    lm, _ = make_lms(tmp_path, LR.random_arpa(np.random.RandomState(690), tokens_of(C), 3, 0.3), C, blank)
    x = np.concatenate([emissions(691, 2, T, C, 1.0), spelled(692, 2, T, C, blank)])
    Wt = transitions(693, C)
    for forced in (False, True):
        a = device(x, Wt, blank, forced, 64, 22, 3, lm, normalize=True)
        b = device(x, Wt, blank, forced, 64, 22, 3, lm, normalize=True)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
        assert any(len(s) for h in a[0] for s in h)


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
KINDS = [dict(blank="optional", allow_repeats=False), dict(blank="forced")]
LETTERS = ["a", "b", "c"]


def _criterion(tokens, ngram, kw, seed):
    T = _mods()[2]
    crit = T.Transducer(tokens, {t: i for i, t in enumerate(tokens)}, ngram=ngram, **kw).cuda()
    if ngram > 0:
        params = (0.5 * np.random.RandomState(seed).randn(crit.transition_params.numel())).astype(np.float32)
        with torch.no_grad():
            crit.transition_params.copy_(torch.from_numpy(params))
    return crit


def _route_operands(crit, xd, forced, W, K, nbest, lm):
    """(emissions, Wt or None) on the host, as the module's route forms them for the search (_beam_inputs)"""
    plan, kind = crit._beam_plan(xd, "test", W, K, nbest, token_lm=lm)
    assert plan.forced == forced
    xe, Wt = crit._beam_inputs(xd, kind)
    return xe.cpu().numpy(), None if Wt is None else Wt.cpu().numpy()


def _minus_loss(crit, xd, b, seq):
    """minus the criterion's loss of `seq` for utterance b, on the device (a batch of one: no batch mean in between)"""
    with torch.no_grad():
        return -float(crit(xd[b:b + 1], [list(seq)]).reshape(-1)[0])


def _lm_terms(ref_lm, seq, alpha, beta, eos):
    """what the LM and the length bonus add to the score of `seq`"""
    return alpha * ref_lm.score(seq, eos=eos) + beta * len(seq)


def module_inputs(ngram, forced, pruned):
    """the emissions of the module tests: (x unpruned [3, 5, 4], x pruned [4, 40, 4])"""
    if not pruned:
        return spelled(310 + ngram + int(forced), 3, 5, 4, 3, hi=8.0, noise=1.0, run=1)
    return spelled(350 + ngram + int(forced), 4, 40, 4, 3, hi=5.0, noise=1.0)


def module_text(ngram):
    return LR.random_arpa(np.random.RandomState(320 + ngram), LETTERS, 2, 0.5)


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_module_against_the_reference_and_the_loss(tmp_path, ngram, kw):
    forced = kw["blank"] == "forced"
    crit = _criterion(LETTERS, ngram, kw, 300 + ngram)
    C, blank = 4, 3
    text = module_text(ngram)
    p = tmp_path / "letters.arpa"
    p.write_text(text)
    lm = crit.token_lm(str(p))
    ref_lm = LR.ArpaLM(text, LETTERS, blank)
    assert (lm.num_classes, lm.blank) == (C, blank)
    # nothing is pruned (W = 64, K = C, T = 5: at most 1 + 3 + 9 + 27 + 81 prefixes, and fewer in either topology than
    # the 64 a frame keeps -- asserted against a search with room for all): single-grapheme tokens, so the score minus
    # its LM terms is minus the loss of that target
    x = module_inputs(ngram, forced, False)
    B = x.shape[0]
    xd = torch.from_numpy(x).cuda()
    xe, Wt = _route_operands(crit, xd, forced, 64, C, 4, lm)
    every = reference(xe, Wt, blank, forced, 10 ** 6, C, 4, ref_lm)
    want = reference(xe, Wt, blank, forced, 64, C, 4, ref_lm, spells=True)
    assert want == every  # (nothing was pruned)
    opts = dict(token_lm=lm, lm_weight=ALPHA, length_bonus=BETA)
    hyps, scores = crit.beam_search(xd, beam_size=64, classes_per_frame=C, nbest=4, return_scores=True, **opts)
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
            if seq:
                loss = _minus_loss(crit, xd, b, seq)
                bare = got - _lm_terms(ref_lm, seq, ALPHA, BETA, True)
                assert abs(bare - loss) <= 1e-4 * abs(loss) + 2e-5, (b, r, seq, bare, loss)
                checked += 1
    assert checked >= B
    # the beam prunes (T = 40, W = 4, K = 3): the reference's sequences, and the score minus its LM terms a lower bound
    # of minus the loss
    x = module_inputs(ngram, forced, True)
    B = x.shape[0]
    xd = torch.from_numpy(x).cuda()
    xe, Wt = _route_operands(crit, xd, forced, 4, 3, 2, lm)
    logz = log_normaliser(xe, Wt)
    for eos in (True, False):
        want = reference(xe, Wt, blank, forced, 4, 3, 2, ref_lm, eos=eos, spells=True)
        hyps, scores = crit.beam_search(xd, beam_size=4, classes_per_frame=3, nbest=2, return_scores=True, lm_eos=eos, **opts)
        assert [[tuple(p.tolist()) for p in h] for h in hyps] == [[s for s, _ in h] for h in want]
        for b in range(B):
            for r, (seq, s) in enumerate(want[b]):
                got = float(scores[b, r])
                if s == NEG:
                    assert got == NEG
                    continue
                n = s - logz[b]
                assert S.normalised_close(got, n), (b, r, got, n)
                if seq:
                    loss = _minus_loss(crit, xd, b, seq)
                    assert got - _lm_terms(ref_lm, seq, ALPHA, BETA, eos) <= loss + 1e-4 * abs(loss) + 2e-5, (b, r, seq, got, loss)
    # other floating dtypes are converted, tensors that are not on a GPU are uploaded: the same search
    hyps = crit.beam_search(xd, beam_size=4, classes_per_frame=3, nbest=2, **opts)
    for other in (torch.from_numpy(x), xd.double()):
        again = crit.beam_search(other, beam_size=4, classes_per_frame=3, nbest=2, **opts)
        assert [[p.tolist() for p in h] for h in again] == [[p.tolist() for p in h] for h in hyps]


@pytest.mark.parametrize("kw", KINDS, ids=["optional", "forced"])
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_errors_count_what_beam_search_predicts_and_calls_without_a_token_lm_are_what_they_were(tmp_path, ngram, kw):
    E, M = _mods()[:2]
    tokens = ["a", "b", "c", "d", "|"]
    crit = _criterion(tokens, ngram, kw, 500 + ngram)
    B, T, C, blank = 4, 50, 6, 5
    rs = np.random.RandomState(520 + ngram)
    p = tmp_path / "tokens.arpa"
    p.write_text(LR.random_arpa(rs, tokens, 3, 0.4))
    lm = crit.token_lm(str(p))
    x = np.concatenate([emissions(510 + ngram, 2, T, C, 1.0), spelled(511 + ngram, 2, T, C, blank)])
    xd = torch.from_numpy(x).cuda()
    targets = [rs.randint(0, 5, size=n).tolist() for n in (7, 1, 12, 3)]
    counter = M.ErrorCounter(wordsep=4)
    for W, K, opts in ((1, C, dict(token_lm=lm)), (16, 4, dict(token_lm=lm, lm_weight=ALPHA, length_bonus=BETA)),
                       (8, 6, dict(token_lm=lm, lm_weight=2.0, lm_eos=False))):
        pred = crit.beam_search(xd, beam_size=W, classes_per_frame=K, **opts)
        assert any(p.numel() > 0 for p in pred)
        assert crit.errors(xd, targets, counter, beam_size=W, classes_per_frame=K, **opts) == counter(pred, targets)
    # no frame: the empty predictions, counted on the host's side of the counter
    none = torch.zeros(4, 0, C)
    assert crit.errors(none, targets, counter, beam_size=4, token_lm=lm) == \
        counter([torch.zeros(0, dtype=torch.int32)] * 4, targets)
    # without a token_lm: errors() and errors(beam_size=) count what they counted, beam_search() is plan.search bit for bit
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
    # and with one, what the plan of the token LM returns
    plan, kind = crit._beam_plan(xd, "test", 16, 4, 3, token_lm=lm, lm_weight=ALPHA, length_bonus=BETA)
    assert type(plan) is E.TransducerLmBeamPlan
    direct, want = plan.search(xe, Wt, True, torch.int32)
    hyps, scores = crit.beam_search(xd, beam_size=16, classes_per_frame=4, nbest=3, return_scores=True, token_lm=lm,
                                    lm_weight=ALPHA, length_bonus=BETA)
    assert [[p.tolist() for p in h] for h in hyps] == [[p.tolist() for p in h] for h in direct]
    assert scores.numpy().tobytes() == want.numpy().tobytes()
