"""CPU tests (-m "not gpu") of the Transducer beam search with a token-level n-gram LM (csrc/beam_kernels.hip:
wfl_transducer_beam_search_lm, include/wfl.h): the header declares the new entry and libwfl.so
exports it, every bad argument is refused before a launch, engine.TransducerLmBeamPlan and the module check their
arguments without a device, Transducer.token_lm reads an ARPA file over the module's own tokens -- and the Python
restatement the GPU tests compare against (tests/transducer_beam_lm_reference.py) is itself pinned to a brute-force
enumeration of all C^T frame paths the token graph accepts, re-scored with the LM, where nothing is pruned, and bounded
by it where something is.  No device compute here."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import beam_lm_reference as LR
import transducer_beam_lm_reference as TL
import transducer_beam_reference as TR
from gtn_applications_amd import _native as N
from gtn_applications_amd import engine as E
from gtn_applications_amd.criterions.transducer import Transducer
from gtn_applications_amd.lm import NGramLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = TR.NEG


def test_header_declares_and_library_exports_the_entry_point():
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(wfl_[a-z0-9_]+)\s*\(", code))
    fresh = ctypes.CDLL(N.LIB_PATH)  # (a handle of its own: what the library exports, not what the table declared)
    name = "wfl_transducer_beam_search_lm"
    assert name in declared and hasattr(fresh, name) and name in N.EXPORTED_SYMBOLS
    from gtn_applications_amd import metrics as M

    assert callable(E.transducer_beam_search_lm) and callable(M.transducer_beam_search_lm_errors)
    assert callable(Transducer.token_lm)
    for fn in ("transducer_beam_search_lm", "transducer_beam_search_lm_errors", "TransducerLmPlan"):
        assert hasattr(N.ops, fn), fn
    assert list(inspect.signature(E.transducer_beam_search_lm).parameters) == [
        "x", "Wt", "blank", "lm", "forced", "beam_size", "classes_per_frame", "nbest", "normalize", "lm_weight", "length_bonus",
        "lm_eos"]
    # (token_lm behind lookahead on beam_search, keyword-only on errors: the calls further down)
    # the plans the other searches are pinned to stay what they were
    assert E.TransducerBeamPlan._fields == ("C", "blank", "forced", "beam", "classes_per_frame", "nbest")
    assert E.TransducerLexiconBeamPlan._fields == ("C", "blank", "forced", "beam", "classes_per_frame", "nbest", "lexicon", "lm",
                                                   "lm_weight", "word_bonus", "length_bonus", "lm_eos")


# (B, T, C, blank, forced, beam, classes_per_frame, nbest, normalize) around a good call
GOOD = dict(B=2, T=5, C=7, blank=6, forced=1, beam=4, K=3, nbest=2, normalize=1)
BAD = [dict(B=0), dict(B=-1), dict(T=0), dict(C=0), dict(beam=0), dict(beam=65), dict(K=0), dict(K=8),
       dict(C=100, K=65), dict(nbest=0), dict(nbest=5), dict(beam=64, nbest=65), dict(blank=-1), dict(blank=7),
       dict(forced=2), dict(forced=-1)]


def _search(a, null=None, lm_change=None, weight=0.8, bonus=0.5, no_lm=False, capacity=None):
    """wfl_transducer_beam_search_lm with host addresses that are never touched: every case here is refused before a
    launch"""
    n = max(1, a["B"] * a["nbest"])
    bufs = dict(x=np.zeros(8, np.float32), Wt=np.zeros(8, np.float32), logz=np.zeros(8, np.float32), ws=np.zeros(8, np.int64),
                out=np.zeros(8, np.int32), offs=np.zeros(n + 1, np.int64), scores=np.zeros(n, np.float64))
    p = {k: (None if k == null or (isinstance(null, tuple) and k in null) else v.ctypes.data) for k, v in bufs.items()}
    arrays = dict(arc_ptr=np.zeros(2, np.int32), arc_label=np.zeros(1, np.int32), arc_next=np.zeros(1, np.int32),
                  arc_w=np.zeros(1, np.float64), bo_next=np.zeros(1, np.int32), bo_w=np.zeros(1, np.float64))
    f = dict(num_states=1, num_arcs=0, start=0, reserved=0, step_min=-1.0, step_max=0.0,
             **{k: v.ctypes.data for k, v in arrays.items()})
    f.update(lm_change or {})
    lm = N.NgramLm(*(f[k] for k in ("num_states", "num_arcs", "start", "reserved", "step_min", "step_max", "arc_ptr",
                                    "arc_label", "arc_next", "arc_w", "bo_next", "bo_w")))
    cap = a["B"] * a["nbest"] * a["T"] if capacity is None else capacity
    return N.lib.wfl_transducer_beam_search_lm(p["x"], p["Wt"], p["logz"], a["B"], a["T"], a["C"], a["blank"], a["forced"],
                                               a["beam"], a["K"], a["nbest"], a["normalize"], None if no_lm else ctypes.byref(lm),
                                               weight, bonus, 1, p["ws"], p["out"], cap, p["offs"], p["scores"], None)


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_search_arguments_are_refused_without_a_device(change):
    a = dict(GOOD, **change)
    if "C" in change and "blank" not in change:
        a["blank"] = 0
    assert _search(a) == N.ERR_INVALID
    assert "transducer_beam_search_lm" in N.last_error()


@pytest.mark.parametrize("null", ["x", "ws", "out", "offs", "scores"])
def test_null_pointers_are_refused(null):
    assert _search(GOOD, null=null) == N.ERR_INVALID
    assert _search(dict(GOOD, forced=0), null=null) == N.ERR_INVALID


def test_the_normaliser_belongs_to_the_transitions():
    assert _search(GOOD, null="logz") == N.ERR_INVALID  # (transitions and normalize, but no logz)
    assert _search(GOOD, null="Wt") == N.ERR_INVALID    # (logz without transitions)


@pytest.mark.parametrize("forced", [0, 1])
@pytest.mark.parametrize("change", [dict(num_states=0), dict(num_arcs=-1), dict(start=-1), dict(start=1), dict(arc_ptr=None),
                                    dict(arc_label=None), dict(arc_next=None), dict(arc_w=None), dict(bo_next=None),
                                    dict(bo_w=None), dict(step_min=math.nan), dict(step_max=math.nan)],
                         ids=lambda c: ",".join(c))
def test_a_bad_lm_struct_is_refused(change, forced):
    assert _search(dict(GOOD, forced=forced), lm_change=change) == N.ERR_INVALID
    assert "language model" in N.last_error()
    # (also where the call would be forwarded to the CTC search with an LM: no transitions, the optional topology)
    assert _search(dict(GOOD, forced=0), lm_change=change, null=("Wt", "logz")) == N.ERR_INVALID


def test_a_null_lm_scalars_that_are_not_finite_small_capacity_and_too_many_classes():
    assert _search(GOOD, no_lm=True) == N.ERR_INVALID
    assert "language model" in N.last_error()
    for w, b in ((math.nan, 0.0), (math.inf, 0.0), (-math.inf, 0.0), (1.0, math.nan), (1.0, math.inf), (1.0, -math.inf)):
        for a, null in ((GOOD, None), (dict(GOOD, forced=0), None), (dict(GOOD, forced=0), ("Wt", "logz"))):
            assert _search(a, weight=w, bonus=b, null=null) == N.ERR_INVALID
            assert "finite" in N.last_error()
    assert _search(GOOD, capacity=2 * 2 * 5 - 1) == N.ERR_INVALID
    assert "out holds" in N.last_error()
    assert _search(dict(GOOD, C=16385)) == N.ERR_UNSUPPORTED
    # the Transducer's own refusals come first, in its order: the sizes, then `forced`, then the LM
    assert _search(dict(GOOD, forced=2), no_lm=True) == N.ERR_INVALID and "forced" in N.last_error()
    assert _search(dict(GOOD, beam=0, forced=2), no_lm=True) == N.ERR_INVALID and "bad arguments" in N.last_error()


# ------------------------------------------------------------------------------------------------------------------
# the host side: Transducer.token_lm, the plan and the module's refusals
# ------------------------------------------------------------------------------------------------------------------
TOKENS = ["a", "b", "c", "|"]
G2I = {g: i for i, g in enumerate(TOKENS)}
OPTIONAL = dict(blank="optional", allow_repeats=False)
FORCED = dict(blank="forced")


def _crit(tokens=TOKENS, g2i=G2I, **kw):
    return Transducer(tokens, g2i, **kw)


def _arpa(tmp_path, tokens, order=2, eos=True, seed=3, name=None):
    p = tmp_path / (name or f"lm{len(tokens)}_{order}_{eos}_{seed}.arpa")
    p.write_text(LR.random_arpa(np.random.RandomState(seed), tokens, order, 0.5, eos=eos))
    return str(p)


def _lm(tmp_path, tokens, blank=None, **kw):
    return NGramLM.from_arpa(_arpa(tmp_path, tokens, **kw), tokens, len(tokens) if blank is None else blank)


def _same_lm(a, b):
    return ((a.num_classes, a.blank, a.start, a.order) == (b.num_classes, b.blank, b.start, b.order) and
            all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("arc_ptr", "arc_label", "arc_next", "arc_w", "bo_next",
                                                                       "bo_w")))


def test_token_lm_is_from_arpa_over_the_modules_tokens(tmp_path):
    path = _arpa(tmp_path, TOKENS, order=3)
    for kw in (OPTIONAL, FORCED, dict(blank="optional", allow_repeats=True)):
        crit = _crit(**kw)
        lm = crit.token_lm(path)
        assert isinstance(lm, NGramLM) and (lm.num_classes, lm.blank, lm.order) == (5, 4, 3)
        assert _same_lm(lm, NGramLM.from_arpa(path, TOKENS, blank=4))
        assert lm.score([0, 1, 3]) == NGramLM.from_arpa(path, TOKENS, blank=4).score([0, 1, 3]) > -math.inf
    # word pieces: the file names a token as the module was given it; the other names of the specials are passed on
    pieces = ["a", "b", "ab", "ba", "_"]
    crit = _crit(pieces, {"a": 0, "b": 1, "_": 2}, **FORCED)
    text = LR.random_arpa(np.random.RandomState(5), pieces, 2, 0.5).replace("<s>", "<bos>").replace("</s>", "<eos>")
    p = tmp_path / "pieces.arpa"
    p.write_text(text)
    lm = crit.token_lm(str(p), bos="<bos>", eos="<eos>")
    assert (lm.num_classes, lm.blank) == (6, 5) and _same_lm(lm, NGramLM.from_arpa(str(p), pieces, 5, bos="<bos>", eos="<eos>"))
    # a token the file does not know takes <unk>'s arcs, or the loader's ValueError names it
    with pytest.raises(ValueError, match="'_'"):
        crit.token_lm(_arpa(tmp_path, pieces[:-1], name="short.arpa"))
    known = crit.token_lm(_arpa(tmp_path, pieces[:-1] + ["<unk>"], name="unk.arpa"))
    assert known.score([4]) > -math.inf
    with pytest.raises(ValueError, match="blank"):
        _crit(blank="none").token_lm(path)
    # plain attributes only: the state_dict is what it was
    for ngram in (0, 2):
        crit = _crit(ngram=ngram, **OPTIONAL)
        crit.token_lm(path)
        assert list(crit.state_dict()) == (["transition_params"] if ngram else []) and list(dict(crit.named_buffers())) == []


def test_plan_fields_and_checks(tmp_path):
    lm = _lm(tmp_path, TOKENS)
    P = E.TransducerLmBeamPlan
    assert P._fields == ("C", "blank", "forced", "beam", "classes_per_frame", "nbest", "lm", "lm_weight", "length_bonus", "lm_eos")
    assert all(callable(getattr(P, f)) for f in ("checked", "no_frames", "search", "on_device"))
    assert P.checked(5, 4, False, 16, None, 1, lm, 1.0, 0.0, True, "t") == (5, 4, False, 16, 5, 1, lm, 1.0, 0.0, True)
    assert P.checked(5, np.int64(4), 1, np.int64(4), 3, 2, lm, 0.5, np.float64(-1), np.bool_(False), "t") == \
        (5, 4, True, 4, 3, 2, lm, 0.5, -1.0, False)
    assert P.checked(5, 4, False, 4, None, 1, lm, torch.tensor(0.25), 2, True, "t")[7:9] == (0.25, 2.0)
    good = dict(C=5, blank=4, forced=False, beam_size=4, classes_per_frame=None, nbest=1, lm=lm, lm_weight=1.0, length_bonus=0.0,
                lm_eos=True)
    bad = (dict(beam_size=0), dict(beam_size=65), dict(beam_size=True), dict(classes_per_frame=6), dict(nbest=5), dict(C=0),
           dict(blank=5), dict(blank=-1), dict(blank=True), dict(forced=2), dict(forced=None),  # what TransducerBeamPlan refuses
           dict(lm=None), dict(lm="lm.arpa"), dict(lm=object()), dict(lm=_lm(tmp_path, TOKENS + ["d"])),
           dict(lm=_lm(tmp_path, TOKENS, blank=1)), dict(C=6, blank=5), dict(blank=3),
           dict(lm_weight=math.nan), dict(lm_weight=math.inf), dict(lm_weight="1"), dict(lm_weight=True), dict(lm_weight=None),
           dict(length_bonus=math.nan), dict(length_bonus=-math.inf), dict(length_bonus="0"), dict(lm_eos=1), dict(lm_eos=None))
    for change in bad:
        with pytest.raises(ValueError, match="^t: "):
            P.checked(**dict(good, **change), what="t")
    # without a frame and without a device
    eos = lm.step(lm.start, 5)[0]
    assert math.isfinite(eos) and eos == lm.score([])
    hyps, scores = P.checked(**dict(good, nbest=2, lm_weight=0.5, length_bonus=3.0), what="t").no_frames(2, torch.int32)
    assert [[h.tolist() for h in u] for u in hyps] == [[[], []]] * 2 and scores.tolist() == [[0.5 * eos, -math.inf]] * 2
    assert all(h.dtype == torch.int32 for u in hyps for h in u)
    hyps, scores = E.transducer_beam_search_lm(torch.zeros(2, 0, 5), torch.zeros(6, 5), 4, lm, nbest=2, lm_weight=0.5)
    assert scores.tolist() == [[0.5 * eos, -math.inf]] * 2 and all(h.dtype == torch.int64 for u in hyps for h in u)
    hyps, scores = E.transducer_beam_search_lm(torch.zeros(0, 7, 5), None, 4, lm, forced=True)
    assert hyps == [] and tuple(scores.shape) == (0, 1)
    assert E.transducer_beam_search_lm(torch.zeros(1, 0, 5), None, 4, lm, lm_eos=False)[1].tolist() == [[0.0]]
    with pytest.raises(ValueError):
        E.transducer_beam_search_lm(torch.zeros(2, 0, 5), torch.zeros(5, 5), 4, lm)  # (transitions of another shape)
    with pytest.raises(ValueError):
        E.transducer_beam_search_lm(torch.zeros(2, 0, 5), None, 3, lm)  # (another blank)


def test_module_refuses_the_ambiguous_graphs_general_models_lexicons_and_merging(tmp_path):
    from gtn_applications_amd import transitions_builder as TB

    x = torch.zeros(2, 5, 5)
    lm = _lm(tmp_path, TOKENS)
    with pytest.raises(NotImplementedError, match="ambiguous"):
        _crit(blank="optional", allow_repeats=True).beam_search(x, token_lm=lm)
    with pytest.raises(NotImplementedError, match="ambiguous"):
        _crit(blank="optional", allow_repeats=True).errors(x, [[0], [1]], None, beam_size=4, token_lm=lm)
    with pytest.raises(NotImplementedError, match="ambiguous"):
        _crit(blank="none").beam_search(torch.zeros(2, 5, 4), token_lm=lm)
    lines = [["a", "b", "a", "c"], ["b", "b", "c"], ["c", "a", "|"]]
    trans = TB.build_transitions(lines, TOKENS, (0, 0), blank="optional", self_loops=True)
    for kw in (OPTIONAL, FORCED):
        with pytest.raises(NotImplementedError, match="transition model"):
            _crit(transitions=trans, **kw).beam_search(x, token_lm=lm)
        crit = _crit(**kw)
        lex = crit.word_lexicon(["ab", "c"], wordsep="|")
        word_lm = _lm(tmp_path, ["ab", "c"], name="words.arpa")
        for more in ({}, dict(lm=word_lm), dict(lookahead="unigram", lm=word_lm)):
            with pytest.raises(NotImplementedError, match="token_lm.*lexicon"):
                crit.beam_search(x, lexicon=lex, token_lm=lm, **more)
            with pytest.raises(NotImplementedError, match="token_lm.*lexicon"):
                crit.errors(x, [[0], [1]], None, beam_size=4, lexicon=lex, token_lm=lm, **more)
        with pytest.raises(NotImplementedError, match="merge_spellings.*token_lm"):
            crit.beam_search(x, token_lm=lm, merge_spellings=True)
        with pytest.raises(NotImplementedError, match="merge_spellings.*token_lm"):
            crit.errors(x, [[0], [1]], None, beam_size=4, token_lm=lm, merge_spellings=True)
        with pytest.raises(NotImplementedError, match="merge_spellings"):
            crit.beam_search(torch.zeros(2, 0, 5), token_lm=lm, merge_spellings=True)  # (before the frames are looked at)
        # both searched graphs, every searched model: nothing raised before the device is asked for (T == 0: never)
        for ngram in (0, 1, 2):
            assert len(_crit(ngram=ngram, **kw).beam_search(torch.zeros(2, 0, 5), token_lm=lm)) == 2


@pytest.mark.parametrize("kw0", [OPTIONAL, FORCED], ids=["optional", "forced"])
def test_module_refuses_bad_token_lm_arguments_before_a_device_is_needed(tmp_path, kw0):
    crit = _crit(**kw0)
    x = torch.zeros(2, 5, 5)
    lm = _lm(tmp_path, TOKENS)
    word_lm = _lm(tmp_path, ["w0", "w1"], name="words.arpa")
    bad = (dict(token_lm="lm.arpa"), dict(token_lm=object()), dict(token_lm=[0, 1]),  # no NGramLM
           dict(token_lm=_lm(tmp_path, TOKENS + ["d"])), dict(token_lm=_lm(tmp_path, TOKENS[:-1])),  # another class count
           dict(token_lm=_lm(tmp_path, TOKENS, blank=0)), dict(token_lm=_lm(tmp_path, TOKENS, blank=2)),  # another blank
           dict(token_lm=lm, lm_weight=math.nan), dict(token_lm=lm, lm_weight=math.inf), dict(token_lm=lm, lm_weight="1"),
           dict(token_lm=lm, length_bonus=math.nan), dict(token_lm=lm, length_bonus=-math.inf), dict(token_lm=lm, lm_eos=1),
           dict(token_lm=lm, lm=word_lm), dict(token_lm=lm, lm=lm),  # `lm` is the word LM of a lexicon
           dict(token_lm=lm, word_bonus=0.5), dict(token_lm=lm, word_bonus=-1), dict(token_lm=lm, word_bonus=math.nan),
           dict(token_lm=lm, word_bonus="0"), dict(token_lm=lm, word_bonus=True),
           dict(token_lm=lm, lookahead="unigram"), dict(token_lm=lm, lookahead=[0.0, 0.0]),
           dict(token_lm=lm, beam_size=65), dict(token_lm=lm, nbest=17), dict(token_lm=lm, classes_per_frame=6),
           # without a token_lm (and a lexicon) the scalars stay refused, as they were
           dict(lm=lm), dict(lm_weight=0.5), dict(length_bonus=0.5), dict(lm_eos=False), dict(word_bonus=0.5))
    for kw in bad:
        with pytest.raises(ValueError):
            crit.beam_search(x, **kw)
        with pytest.raises(ValueError):
            crit.beam_search(torch.zeros(2, 0, 5), **kw)  # (before the frames are looked at)
        if "nbest" not in kw:
            with pytest.raises(ValueError):
                crit.errors(x, [[1], [2]], None, **dict(dict(beam_size=4), **kw))
    with pytest.raises(ValueError):
        crit.beam_search(torch.zeros(2, 5, 6), token_lm=lm)  # (emissions of another width)
    for kw in (dict(token_lm=lm), dict(token_lm=lm, lm_weight=0.5), dict(lm_weight=0.5)):
        with pytest.raises(ValueError):  # (they belong to errors()' beam search)
            crit.errors(x, [[1], [2]], None, **kw)
    with pytest.raises(TypeError):
        crit.errors(x, [[1], [2]], None, 4, None, False, None, None, 1.0, 0.0, True, 0.0, None, lm)  # (keyword-only)


@pytest.mark.parametrize("kw0", [OPTIONAL, FORCED], ids=["optional", "forced"])
def test_no_frames_and_no_utterances_need_no_device(tmp_path, kw0):
    crit = _crit(**kw0)
    lm = _lm(tmp_path, TOKENS)
    eos = lm.step(lm.start, 5)[0]
    assert math.isfinite(eos)
    empty = [[[], []]] * 2
    none = torch.zeros(2, 0, 5)
    hyps, scores = crit.beam_search(none, nbest=2, return_scores=True, token_lm=lm, lm_weight=0.5, length_bonus=1.0)
    assert [[h.tolist() for h in u] for u in hyps] == empty and scores.tolist() == [[0.5 * eos, -math.inf]] * 2
    assert all(h.dtype == torch.int32 for u in hyps for h in u)  # (viterbi()'s dtype)
    # positionally: token_lm behind lookahead
    again = crit.beam_search(none, 16, None, 2, True, False, None, None, 0.5, 1.0, True, 0.0, None, lm)
    assert again[1].tolist() == scores.tolist()
    hyps, scores = crit.beam_search(none, return_scores=True, token_lm=lm, lm_eos=False, lm_weight=2.0)
    assert [h.tolist() for h in hyps] == [[], []] and scores.tolist() == [[0.0]] * 2
    _, scores = crit.beam_search(none, return_scores=True, token_lm=lm, lm_weight=0.0)
    assert scores.tolist() == [[0.0]] * 2
    # an LM without </s>: its step is -inf, the rank is dropped whatever the weight
    mute = _lm(tmp_path, TOKENS, eos=False, seed=4)
    assert mute.score([]) == -math.inf and mute.score([0], eos=False) > -math.inf
    for weight in (0.5, 0.0, -1.0):
        _, scores = crit.beam_search(none, nbest=2, return_scores=True, token_lm=mute, lm_weight=weight)
        assert scores.tolist() == [[-math.inf, -math.inf]] * 2
    assert crit.beam_search(none, return_scores=True, token_lm=mute, lm_eos=False)[1].tolist() == [[0.0]] * 2
    # no utterance at all
    assert crit.beam_search(torch.zeros(0, 5, 5), token_lm=lm) == []
    hyps, scores = crit.beam_search(torch.zeros(0, 5, 5), nbest=3, return_scores=True, token_lm=lm)
    assert hyps == [] and tuple(scores.shape) == (0, 3)
    # without a token_lm the call is what it was
    hyps, scores = crit.beam_search(none, nbest=2, return_scores=True)
    assert [[h.tolist() for h in u] for u in hyps] == empty and scores.tolist() == [[0.0, 0.0]] * 2


# ------------------------------------------------------------------------------------------------------------------
# the reference against all frame paths, re-scored with the LM
# ------------------------------------------------------------------------------------------------------------------
C4 = 4
LMS = ["order1", "order2", "order3", "no-unigram"]


def _ref_lm(rs, kind, blank):
    """an ArpaLM over the three tokens of a C = 4 universe: orders 1 - 3 with about half the higher grams kept (so that
    back-offs occur), or a bigram LM in which the last token has no unigram (its step is -inf from every state)"""
    tokens = [f"t{i}" for i in range(C4 - 1)]
    if kind == "no-unigram":
        return LR.ArpaLM(LR.random_arpa(rs, tokens[:-1], 2, 0.5), tokens, blank)
    return LR.ArpaLM(LR.random_arpa(rs, tokens, int(kind[-1]), 0.5), tokens, blank)


def _instance(T, forced, blank, with_wt, kind, eos):
    seed = 28000 + 997 * T + 131 * LMS.index(kind) + 64 * int(forced) + 16 * blank + 4 * int(with_wt) + int(eos)
    rs = np.random.RandomState(seed)
    x = (rs.randn(T, C4) * (1.0, 2.5)[seed % 2]).astype(np.float32)
    # nothing is pruned where the blank is below every token in every frame (K = C - 1 then keeps all tokens and the
    # blank is appended) and no frame has more than W = 64 live entries (T <= 3: at most 1 + 3 + 9 + 27): every T <= 3
    # instance is made so, and about half of the longer ones have the low blank
    low = T <= 3 or rs.rand() < 0.5
    if low:
        x[:, blank] = x.min(axis=1) - 1.0 - rs.rand(T).astype(np.float32)
    Wt = (0.5 * rs.randn(C4 + 1, C4)).astype(np.float32) if with_wt else None
    lm = _ref_lm(rs, kind, blank)
    alpha, beta = ((0.7, -0.4), (1.3, 0.6), (-0.5, 0.25))[seed % 3]
    return x, Wt, lm, alpha, beta


@pytest.mark.parametrize("eos", [True, False], ids=["eos", "noeos"])
@pytest.mark.parametrize("kind", LMS)
@pytest.mark.parametrize("forced", [False, True], ids=["optional", "forced"])
def test_reference_equals_rescored_brute_force_when_nothing_is_pruned_and_is_bounded_by_it_otherwise(forced, kind, eos):
    W, K, nbest = 64, C4 - 1, 6
    unpruned = live = backoffs = 0
    for T in range(1, 7):
        for blank in (0, C4 - 1):
            for with_wt in (False, True):
                inst = (T, forced, blank, with_wt, kind, eos)
                x, Wt, lm, alpha, beta = _instance(*inst)
                want = TL.brute_force(x, Wt, blank, forced, lm, alpha, beta, eos)
                mass = dict(want)
                if kind == "no-unigram":
                    gone = [c for c in range(C4) if c != blank][-1]
                    assert lm.step(lm.start, gone)[0] == NEG and not any(gone in s for s in mass), inst
                state = dict(full=True)

                def on_frame(t, beam, cand, extension, merged, entries):
                    if len(cand) < C4 or len(entries) > W:
                        state["full"] = False

                hyps, margin, _ = TL.beam_search(x, Wt, blank, forced, W, K, nbest, lm, alpha, beta, eos, on_frame=on_frame)
                got = [(s, v) for s, v in hyps if v > NEG]
                assert all(h == ((), NEG) for h in hyps[len(got):]), inst
                assert all(blank not in s for s, _ in got), inst
                if state["full"]:
                    # unpruned: the n-best are the brute force's top sequences
                    unpruned += 1
                    assert len(got) == min(nbest, len(want)), (inst, got, want[:nbest])
                    assert [s for s, _ in got] == [s for s, _ in want[:len(got)]], (inst, got, want[:nbest])
                    for (s, v), (_, m) in zip(got, want):
                        assert abs(v - m) <= 1e-9, (inst, s, v, m)
                    if len(got) > 1:
                        assert margin > 1e-9, inst
                else:
                    # pruned (this instance: `inst`): every score is a lower bound of its sequence's, best first
                    assert T > 3, inst
                    for s, v in got:
                        assert s in mass and v <= mass[s] + 1e-9, (inst, s, v, mass.get(s))
                    assert all(a[1] >= b[1] for a, b in zip(got, got[1:])), inst
                live += len(got)
                toks = [c for c in range(C4) if c != blank]
                backoffs += int(lm.order > 1 and any((p, c) not in lm.grams for p in toks for c in toks))
                # the normaliser is subtracted and nothing else
                logz = TR.normaliser(x, Wt)
                norm, _, _ = TL.beam_search(x, Wt, blank, forced, W, K, 1, lm, alpha, beta, eos, logz=logz)
                assert norm[0][1] == hyps[0][1] - logz or (norm[0][1] == NEG and hyps[0][1] == NEG), inst
    assert unpruned >= 12  # (every T <= 3 instance: 3 lengths, 2 blanks, with and without transitions)
    assert live >= 24  # (the comparison is not one of empty lists)
    assert kind == "order1" or backoffs >= 12  # (grams are missing: steps back off)


def test_reference_without_transitions_in_the_optional_topology_is_the_ctc_lm_reference():
    rs = np.random.RandomState(12)
    for T, C, W, K in ((30, 6, 4, 3), (20, 8, 8, 8), (12, 4, 2, 4), (1, 3, 1, 2)):
        tokens = [f"t{i}" for i in range(C - 1)]
        for blank in (0, C - 1):
            for order in (1, 2, 3):
                lm = LR.ArpaLM(LR.random_arpa(rs, tokens, order, 0.5), tokens, blank)
                x = (2.0 * rs.randn(T, C)).astype(np.float32)
                n = min(3, W)
                for eos in (True, False):
                    want = LR.beam_search(x, blank, W, K, n, lm, 0.7, -0.2, eos)
                    assert TL.beam_search(x, None, blank, False, W, K, n, lm, 0.7, -0.2, eos) == want
                    zero = np.zeros((C + 1, C), np.float32)
                    assert TL.beam_search(x, zero, blank, False, W, K, n, lm, 0.7, -0.2, eos) == want
    # no frame: the empty sequence, scored by </s> alone
    lm = LR.ArpaLM(LR.random_arpa(rs, ["t0", "t1"], 2, 0.5), ["t0", "t1"], 2)
    end = lm.step(lm.start, LR.EOS)[0]
    assert TL.beam_search(np.zeros((0, 3), np.float32), None, 2, True, 4, 3, 2, lm, 0.5, 9.0, True)[0] == [((), 0.5 * end), ((), NEG)]
    assert TL.beam_search(np.zeros((0, 3), np.float32), None, 2, True, 4, 3, 2, lm, 0.5, 9.0, False)[0] == [((), 0.0), ((), NEG)]


# ------------------------------------------------------------------------------------------------------------------
# named cases of the rules
# ------------------------------------------------------------------------------------------------------------------
UNIGRAMS = "\\data\\\nngram 1=4\n\n\\1-grams:\n-9.0\t<s>\n-1.0\t</s>\n-0.5\tt0\n-2.0\tt1\n\n\\end\\\n"


def test_one_frame_by_hand():
    """(1, 3, ...): forced -- no extension in frame 0, the empty sequence with a step(start, </s>); optional -- a
    one-token result carries its LM term, the length bonus and </s>"""
    lm = LR.ArpaLM(UNIGRAMS, ["t0", "t1"], 2)
    ln10 = math.log(10.0)
    x = np.array([[3.0, 0.0, 1.0]], np.float32)
    a, b = 0.8, 0.5
    one, _, _ = TL.beam_search(x, None, 2, True, 4, 2, 3, lm, a, b, True)
    assert one == [((), 1.0 + a * -1.0 * ln10), ((), NEG), ((), NEG)]
    opt, _, _ = TL.beam_search(x, None, 2, False, 4, 3, 3, lm, a, b, True)
    assert [s for s, _ in opt] == [(0,), (), (1,)]
    assert opt[0][1] == pytest.approx(3.0 + (a * -0.5 * ln10 + b) + a * -1.0 * ln10, abs=1e-12)
    assert opt[1][1] == pytest.approx(1.0 + a * -1.0 * ln10, abs=1e-12)
    assert opt[2][1] == pytest.approx(0.0 + (a * -2.0 * ln10 + b) + a * -1.0 * ln10, abs=1e-12)
    # without </s> the scores are the totals; three frames of the forced topology hold one token between two blanks
    plain, _, _ = TL.beam_search(x, None, 2, False, 4, 2, 1, lm, a, b, False)
    assert plain[0] == ((0,), pytest.approx(3.0 + (a * -0.5 * ln10 + b)))
    x3 = np.concatenate([x, x, x])
    three, _, _ = TL.beam_search(x3, None, 2, True, 8, 3, 8, lm, a, b, False)
    assert {s for s, v in three if v > NEG} == {(), (0,), (1,)}


def test_the_forced_topology_ranks_by_pb_and_drops_ahead_of_the_end_of_sentence():
    # 0 -> blank is forbidden: a hypothesis that ends in token 0 has pb = -inf whatever its total
    x = np.zeros((3, 3), np.float32)
    x[1] = [2.0, 0.5, -1.0]
    Wt = np.zeros((4, 3), np.float32)
    Wt[1 + 2][0] = -np.inf
    lm = LR.ArpaLM(UNIGRAMS, ["t0", "t1"], 2)
    ln10 = math.log(10.0)
    hyps, _, _ = TL.beam_search(x, Wt, 2, True, 64, 3, 4, lm, 1.0, 0.0, True)
    assert [s for s, v in hyps if v > NEG] == [(), (1,)] and hyps[2:] == [((), NEG)] * 2
    assert hyps[0][1] == pytest.approx(-1.0 - ln10) and hyps[1][1] == pytest.approx(0.5 - 2.0 * ln10 - ln10)
    # in the optional topology the same token counts through pnb
    opt, _, _ = TL.beam_search(x, Wt, 2, False, 64, 3, 64, lm, 1.0, 0.0, True)
    assert (0,) in [s for s, v in opt if v > NEG]


def test_an_end_of_sentence_step_of_minus_infinity_drops_every_rank():
    tokens = ["t0", "t1"]
    lm = LR.ArpaLM(LR.random_arpa(np.random.RandomState(8), tokens, 2, 0.5, eos=False), tokens, 2)
    assert lm.step(lm.start, LR.EOS)[0] == NEG
    x = np.zeros((3, 3), np.float32)
    for forced in (False, True):
        assert TL.beam_search(x, None, 2, forced, 64, 3, 2, lm, 1.0, 0.0, True)[0] == [((), NEG)] * 2
        without = TL.beam_search(x, None, 2, forced, 64, 3, 2, lm, 1.0, 0.0, False)[0]
        assert without[0][1] > NEG
        assert [s for s, _ in without] == [s for s, _ in TL.brute_force(x, None, 2, forced, lm, 1.0, 0.0, False)[:2]]
