"""CPU tests (-m "not gpu") of the beam searches with a start-marked lexicon (csrc/beam_kernels.hip:
wfl_ctc_beam_search_lexicon_marked, wfl_transducer_beam_search_lexicon_marked; include/wfl.h): the
header declares the new entries and libwfl.so exports them, every bad argument is refused before a launch, the plans and
the modules check their arguments and answer T = 0 without a device, ASG refuses such a lexicon -- and the Python
restatement the GPU tests compare against (tests/beam_lexicon_marked_reference.py) is itself pinned to a brute-force
enumeration of all C^T frame paths scored by rule 6.  No device compute here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import beam_lexicon_marked_reference as MR
import beam_lm_reference as LR
from gtn_applications_amd import _native as N
from gtn_applications_amd import engine as E
from gtn_applications_amd.criterions.asg import ASG
from gtn_applications_amd.criterions.ctc import CTC
from gtn_applications_amd.criterions.transducer import Transducer
from gtn_applications_amd.lexicon import Lexicon
from gtn_applications_amd.lm import NGramLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = MR.NEG
ENTRIES = ("wfl_ctc_beam_search_lexicon_marked", "wfl_transducer_beam_search_lexicon_marked")


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(wfl_[a-z0-9_]+)\s*\(", code))
    fresh = ctypes.CDLL(N.LIB_PATH)  # (a handle of its own: what the library exports, not what the table declared)
    for name in ENTRIES + ("wfl_lexicon_marked_check",):
        assert name in declared and hasattr(fresh, name) and name in N.EXPORTED_SYMBOLS, name
    assert re.search(r"typedef struct wfl_lexicon_marked \{\s*wfl_lexicon trie;[^}]*const int32_t\* node_word;[^}]*"
                     r"const int32_t\* start_node;[^}]*\} wfl_lexicon_marked;", code)
    # wfl_lexicon keeps its layout, and the mirror of the new struct follows the header's
    assert [f[0] for f in N.Lexicon._fields_] == ["num_nodes", "num_arcs", "num_words", "reserved", "arc_ptr", "arc_label",
                                                  "arc_next"]
    assert [f[0] for f in N.LexiconMarked._fields_] == ["trie", "node_word", "start_node"]
    assert ctypes.sizeof(N.LexiconMarked) == ctypes.sizeof(N.Lexicon) + 2 * ctypes.sizeof(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------------------------
# refusals before a launch
# ------------------------------------------------------------------------------------------------------------------
GOOD = dict(B=2, T=5, C=7, blank=6, forced=1, beam=4, K=3, nbest=2, normalize=1)
BAD = [dict(B=0), dict(T=0), dict(C=0), dict(beam=0), dict(beam=65), dict(K=0), dict(K=8), dict(nbest=0), dict(nbest=5),
       dict(blank=-1), dict(blank=7)]


def _search(entry, a, null=None, lex_change=None, weight=0.8, word=0.3, bonus=0.5, no_lex=False, with_lm=True, capacity=None,
            lm_change=None):
    """a marked entry with host addresses that are never touched: every case here is refused before a launch"""
    n = max(1, a["B"] * a["nbest"])
    bufs = dict(x=np.zeros(8, np.float32), Wt=np.zeros(8, np.float32), logz=np.zeros(8, np.float32), ws=np.zeros(8, np.int64),
                out=np.zeros(8, np.int32), offs=np.zeros(n + 1, np.int64), scores=np.zeros(n, np.float64),
                lengths=np.zeros(8, np.int32))
    p = {k: (None if k == null or (isinstance(null, tuple) and k in null) else v.ctypes.data) for k, v in bufs.items()}
    larrays = dict(arc_ptr=np.array([0, 1, 1], np.int32), arc_label=np.array([1], np.int32), arc_next=np.array([1], np.int32),
                   node_word=np.array([-1, 0], np.int32), start_node=np.array([-1, 1, -1, -1, -1, -1, -1], np.int32))
    lf = dict(num_nodes=2, num_arcs=1, num_words=1, reserved=0, **{k: v.ctypes.data for k, v in larrays.items()})
    lf.update(lex_change or {})
    trie = N.Lexicon(*(lf[k] for k in ("num_nodes", "num_arcs", "num_words", "reserved", "arc_ptr", "arc_label", "arc_next")))
    lex = N.LexiconMarked(trie, lf["node_word"], lf["start_node"])
    arrays = dict(arc_ptr=np.zeros(2, np.int32), arc_label=np.zeros(1, np.int32), arc_next=np.zeros(1, np.int32),
                  arc_w=np.zeros(1, np.float64), bo_next=np.zeros(1, np.int32), bo_w=np.zeros(1, np.float64))
    f = dict(num_states=1, num_arcs=0, start=0, reserved=0, step_min=-1.0, step_max=0.0,
             **{k: v.ctypes.data for k, v in arrays.items()})
    f.update(lm_change or {})
    lm = N.NgramLm(*(f[k] for k in ("num_states", "num_arcs", "start", "reserved", "step_min", "step_max", "arc_ptr",
                                    "arc_label", "arc_next", "arc_w", "bo_next", "bo_w")))
    cap = a["B"] * a["nbest"] * a["T"] if capacity is None else capacity
    lexp, lmp = None if no_lex else ctypes.byref(lex), ctypes.byref(lm) if with_lm else None
    if entry == ENTRIES[0]:
        return N.lib.wfl_ctc_beam_search_lexicon_marked(p["x"], p["lengths"], a["B"], a["T"], a["C"], a["blank"], a["beam"],
                                                        a["K"], a["nbest"], a["normalize"], lexp, lmp, weight, word, bonus, 1,
                                                        p["ws"], p["out"], cap, p["offs"], p["scores"], None)
    return N.lib.wfl_transducer_beam_search_lexicon_marked(p["x"], p["Wt"], p["logz"], a["B"], a["T"], a["C"], a["blank"],
                                                           a["forced"], a["beam"], a["K"], a["nbest"], a["normalize"], lexp, lmp,
                                                           weight, word, bonus, 1, p["ws"], p["out"], cap, p["offs"],
                                                           p["scores"], None)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_bad_search_arguments_are_refused_without_a_device(entry, change):
    a = dict(GOOD, **change)
    if "C" in change and "blank" not in change:
        a["blank"] = 0
    for with_lm in (True, False):
        assert _search(entry, a, with_lm=with_lm) == N.ERR_INVALID
        assert entry[4:] in N.last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers_bad_structs_and_constants_are_refused(entry):
    for null in ("x", "ws", "out", "offs", "scores"):
        assert _search(entry, GOOD, null=null) == N.ERR_INVALID
    assert _search(entry, GOOD, no_lex=True) == N.ERR_INVALID
    for change in (dict(num_nodes=0), dict(num_arcs=0), dict(num_words=0), dict(num_words=2 ** 31 - 1), dict(arc_ptr=None),
                   dict(arc_label=None), dict(arc_next=None), dict(node_word=None), dict(start_node=None)):
        for with_lm in (True, False):
            assert _search(entry, GOOD, lex_change=change, with_lm=with_lm) == N.ERR_INVALID, change
            assert "lexicon" in N.last_error()
    for change in (dict(num_states=0), dict(start=1), dict(arc_w=None), dict(step_min=math.nan)):
        assert _search(entry, GOOD, lm_change=change) == N.ERR_INVALID
    for w, o, b in ((math.nan, 0.0, 0.0), (math.inf, 0.0, 0.0), (1.0, math.nan, 0.0), (1.0, -math.inf, 0.0),
                    (1.0, 0.0, math.nan), (1.0, 0.0, math.inf)):
        for with_lm in (True, False):
            assert _search(entry, GOOD, weight=w, word=o, bonus=b, with_lm=with_lm) == N.ERR_INVALID
            assert "finite" in N.last_error()
    assert _search(entry, GOOD, capacity=2 * 2 * 5 - 1) == N.ERR_INVALID
    assert "out holds" in N.last_error()
    assert _search(entry, dict(GOOD, C=16385)) == N.ERR_UNSUPPORTED


def test_the_transducer_entry_keeps_its_own_refusals_and_forwards_like_its_sibling():
    entry = ENTRIES[1]
    for forced in (2, -1):
        assert _search(entry, dict(GOOD, forced=forced)) == N.ERR_INVALID
        assert "forced" in N.last_error()
    assert _search(entry, GOOD, null="logz") == N.ERR_INVALID  # (transitions and normalize, but no logz)
    assert _search(entry, GOOD, null="Wt") == N.ERR_INVALID    # (logz without transitions)
    # no transitions, the optional topology: the CTC entry's search runs, behind the same checks
    assert _search(entry, dict(GOOD, forced=0), null=("Wt", "logz"), weight=math.nan) == N.ERR_INVALID
    assert _search(entry, dict(GOOD, forced=0), null=("Wt", "logz"), capacity=1) == N.ERR_INVALID
    assert "out holds" in N.last_error()


# ------------------------------------------------------------------------------------------------------------------
# the plans and the modules, without a device
# ------------------------------------------------------------------------------------------------------------------
TOKENS = ["_a", "_the", "n", "t", "re"]  # classes 0 .. 4, the blank 5
WORDS = ["_a", "_an", "_ant", "_the", "_there"]
TABLE = {"_a": ["_a"], "_an": ["_a", "n"], "_ant": ["_a", "n", "t"], "_the": ["_the"], "_there": ["_the", "re"]}


def _word_lm(words, tmp_path, order=2, seed=3, eos=True, listed=None):
    p = tmp_path / f"words{len(words)}_{order}_{seed}_{eos}.arpa"
    text = LR.random_arpa(np.random.RandomState(seed), words if listed is None else listed, order, 0.5, eos=eos)
    p.write_text(text)
    return NGramLM.from_arpa(str(p), words, len(words)), LR.ArpaLM(text, words, len(words))


def test_plans_and_modules_take_a_start_marked_lexicon_without_a_new_keyword(tmp_path):
    lex = Lexicon.from_words(WORDS, TOKENS, 5, split=lambda w: TABLE[w], boundary="start")
    lm, _ = _word_lm(WORDS, tmp_path)
    plan = E.BeamPlan.checked(6, 5, 4, None, 2, lm, 0.5, 0.25, True, lex, 1.5, "t")
    assert plan.lexicon is lex and plan.lexicon.boundary == "start" and plan.word_bonus == 1.5
    tplan = E.TransducerLexiconBeamPlan.checked(6, 5, True, 4, None, 2, lex, lm, 0.5, 1.5, 0.25, True, "t")
    assert tplan.lexicon is lex
    other = Lexicon([(0,), (0, 1)], 7, 6, boundary="start")
    for bad in (dict(lexicon=other), dict(lm=_word_lm(WORDS + ["_w"], tmp_path)[0])):
        kw = dict(dict(lexicon=lex, lm=lm), **bad)
        with pytest.raises(ValueError, match="^t: "):
            E.BeamPlan.checked(6, 5, 4, None, 2, kw["lm"], 0.5, 0.25, True, kw["lexicon"], 1.5, "t")
        with pytest.raises(ValueError, match="^t: "):
            E.TransducerLexiconBeamPlan.checked(6, 5, True, 4, None, 2, kw["lexicon"], kw["lm"], 0.5, 1.5, 0.25, True, "t")
    # T = 0: the empty sequence, scored by </s> alone -- rule 5 for a rank at the root
    end = 0.5 * lm.step(lm.start, len(WORDS) + 1)[0]
    hyps, scores = plan.no_frames(2)
    assert [[h.tolist() for h in u] for u in hyps] == [[[], []]] * 2 and scores.tolist() == [[end, -math.inf]] * 2
    hyps, scores = E.transducer_beam_search_lexicon(torch.zeros(2, 0, 6), None, 5, lex, nbest=2, lm=lm, lm_weight=0.5)
    assert scores.tolist() == [[end, -math.inf]] * 2
    ctc = CTC(5, False)
    out = ctc.beam_search(torch.zeros(2, 0, 6), 4, lexicon=lex, word_bonus=1.0, return_scores=True)
    assert [h.tolist() for h in out[0]] == [[], []]
    with pytest.raises(ValueError):
        ctc.beam_search(torch.zeros(2, 3, 7), 4, lexicon=lex)  # (built for other classes)
    with pytest.raises(ValueError):
        ctc.errors(torch.zeros(2, 3, 6), [[0], [1]], None, lexicon=lex)  # (a lexicon needs a beam_size)


def test_transducer_word_lexicon_forwards_the_convention():
    for kw in (dict(blank="optional", allow_repeats=False), dict(blank="forced")):
        crit = Transducer(TOKENS, {"_": 0, "a": 1, "t": 2, "h": 3, "e": 4, "n": 5, "r": 6}, **kw)
        with pytest.raises(ValueError, match="not prefix-free"):
            crit.word_lexicon(WORDS, split=lambda w: TABLE[w])
        lex = crit.word_lexicon(WORDS, split=lambda w: TABLE[w], boundary="start")
        assert lex.boundary == "start" and (lex.num_classes, lex.blank) == (6, 5) and lex.word_names == WORDS
        assert [tuple(s) for s in lex.spellings] == [(0,), (0, 2), (0, 2, 3), (1,), (1, 4)]
        assert crit.words(lex, [0, 2, 1, 4, 0]) == [1, 4, 0]
        with pytest.raises(ValueError, match="no wordsep"):
            crit.word_lexicon(WORDS, wordsep="n", boundary="start")
        with pytest.raises(ValueError, match="needs boundary='start'"):
            crit.word_lexicon(WORDS, splits=lambda w: [TABLE[w]])
        two = crit.word_lexicon(["_a", "_the"], boundary="start", splits=lambda w: [[w], ["_a", "t"]] if w == "_the" else [[w]])
        assert two.num_words == 2 and two.words([0, 3, 1]) == [1, 1]
        # no frame: no device; the same keywords as with an end-marked lexicon
        res = crit.beam_search(torch.zeros(2, 0, 6), 4, lexicon=lex, word_bonus=0.5, length_bonus=0.5)
        assert len(res) == 2
        with pytest.raises(NotImplementedError):
            crit.beam_search(torch.zeros(2, 0, 6), 4, lexicon=lex, merge_spellings=True)


def test_asg_refuses_a_start_marked_lexicon():
    crit = ASG(2, num_replabels=1, use_garbage=True)  # classes 0 and 1, the replabel 2 and the garbage 3
    good = Lexicon([(0, 1), (1, 0)], 4, 3)
    marked = Lexicon([(0,), (0, 1)], 4, 3, boundary="start")
    assert len(crit.beam_search(torch.zeros(2, 0, 4), 4, lexicon=good)) == 2
    with pytest.raises(NotImplementedError, match="replabels.*across a word boundary.*question of its own"):
        crit.beam_search(torch.zeros(2, 0, 4), 4, lexicon=marked)
    with pytest.raises(NotImplementedError, match="start-marked"):
        crit.errors(torch.zeros(2, 0, 4), [[0], [1]], None, beam_size=4, lexicon=marked)
    with pytest.raises(NotImplementedError):
        E.AsgLexiconBeamPlan.checked(4, 4, None, 1, 3, marked, None, 1.0, 0.0, 0.0, True, "t")


# ------------------------------------------------------------------------------------------------------------------
# the restatement against brute force (rule 6): all C^T frame paths, W = 64 prunes nothing
# ------------------------------------------------------------------------------------------------------------------
# C = 4, the blank 3: class 0 begins words, 1 and 2 continue them; word 0 has two spellings; (0,) is a proper prefix of
# (0, 1) and (0, 2), (0, 1) of (0, 1, 2)
LEX_A = {(0,): 0, (0, 1): 1, (0, 1, 2): 2, (0, 2): 0}
# two start classes, one-piece words, a word that is never complete before its third label
LEX_B = {(0,): 0, (1,): 1, (1, 2, 2): 2, (0, 2): 1}
WORDS3 = ["w0", "w1", "w2"]


def _arpa(seed, order, eos=True, listed=None):
    text = LR.random_arpa(np.random.RandomState(seed), WORDS3 if listed is None else listed, order, 0.6, eos=eos)
    return LR.ArpaLM(text, WORDS3, 3)


PIN = [
    # (name, lexicon, T, blank, lm, alpha, omega, beta, score_eos)
    ("no-lm", LEX_A, 5, 3, None, 1.0, 0.0, 0.0, False),
    ("no-lm-bonuses", LEX_A, 5, 3, None, 1.0, 0.7, -0.4, False),
    ("lm-eos", LEX_A, 5, 3, ("lm", 5, 2, True), 0.8, 0.3, 0.5, True),
    ("lm-no-eos", LEX_B, 4, 3, ("lm", 6, 3, True), 1.3, -0.6, 0.2, False),
    ("lm-eos-blank-first", LEX_A, 5, 0, ("lm", 7, 2, True), 0.5, 1.0, -0.3, True),
    ("lm-eos-blank-middle", LEX_B, 4, 1, ("lm", 8, 3, True), 0.9, 0.2, 0.1, True),
    ("lm-missing-word", LEX_A, 5, 3, ("lm", 9, 2, True, ["w0", "w2"]), 0.8, 0.3, 0.5, True),
    ("two-spellings-T6", {(0,): 0, (0, 1): 0}, 6, 3, ("lm", 10, 2, True, ["w0"]), 0.7, 0.4, 0.3, True),
]


def _shift(lexicon, blank):
    """the lexicon over classes renumbered so that `blank` (not 3) is the blank: class c >= blank moves up by one"""
    move = lambda c: c if c < blank else c + 1
    return lexicon if blank == 3 else {tuple(move(c) for c in s): v for s, v in lexicon.items()}


@pytest.mark.parametrize("topology", ["ctc", "optional", "forced"])
@pytest.mark.parametrize("case", PIN, ids=[c[0] for c in PIN])
def test_the_restatement_is_rule_6_on_all_frame_paths(case, topology):
    name, lexicon, T, blank, lm_spec, alpha, omega, beta, eos = case
    lexicon = _shift(lexicon, blank)
    assert MR.is_start_marked(lexicon)
    lm = None if lm_spec is None else _arpa(*lm_spec[1:])
    forced = topology == "forced"
    T += 1 if forced and T == 4 else 0  # (the forced topology spells less: a frame more where the others have four)
    rs = np.random.RandomState(len(name) + 17 * T)
    C = 4
    x = (1.5 * rs.randn(T, C)).tolist()
    Wt = None if topology == "ctc" else rs.randn(C + 1, C).tolist()
    want = MR.brute_force(x, blank, lexicon, lm, alpha, omega, beta, eos, Wt=Wt, forced=forced, ctc=topology == "ctc")
    hyps, _, merges = MR.beam_search(x, blank, 64, C, 64, lexicon, lm, alpha, omega, beta, eos, Wt=Wt, forced=forced)
    got = [(pre, s) for pre, s in hyps if s > NEG]
    assert len(want) >= 4, "the case decodes too little to pin anything"
    assert any(pre and MR.segment(lexicon, pre)[1] for pre, _ in want)
    assert sorted(p for p, _ in got) == sorted(p for p, _ in want)
    have = dict(got)
    for pre, s in want:
        assert abs(have[pre] - s) <= 1e-9 * max(1.0, abs(s)), (pre, have[pre], s)
    assert [p for p, _ in got] == [p for p, _ in want]  # (the ranks too: no two scores within the tolerance)
    for (_, a), (_, b) in zip(want, want[1:]):
        assert a - b > 1e-8
    if topology != "forced":
        assert merges > 0
    if "two-spellings" in name:
        assert {(0,), (0, 1)} <= set(have) and MR.words_of(lexicon, (0, 0, 1)) == [0, 0]
    if "missing" in name:  # word 1 = (0, 1) has no unigram: no sequence with it survives, pending or completed
        assert all(1 not in MR.words_of(lexicon, pre) for pre in have)
        assert any(MR.words_of(lexicon, pre) is not None and 1 in MR.words_of(lexicon, pre)
                   for pre, _ in MR.brute_force(x, blank, lexicon, None, alpha, omega, beta, eos, Wt=Wt, forced=forced,
                                                ctc=topology == "ctc"))
