"""CPU tests (-m "not gpu") of gtn_applications_amd/lm.py: the ARPA loader on the golden file and on malformed files,
NGramLM.score against the dict-based restatement of tests/beam_lm_reference.py on random LMs, and the pack check of
libwfl (wfl_ngram_lm_check) on every kind of bad pack.  No device compute here."""
import ctypes
import math
import os

import numpy as np
import pytest

import beam_lm_reference as LR
from gtn_applications_amd import _native as N
from gtn_applications_amd.lm import NGramLM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_small.arpa")
TOKENS = ["wood", "cindy", "pittsburgh", "jean"]
LN10 = math.log(10.0)


def test_golden_sentence_score():
    """The sentence the reference's ARPA script compares with kenlm.  kenlm is not at hand, so the expectation is
    derived by hand from the file: <s> has no bigram with wood, so its back-off (-0.3064) and wood's unigram
    (-0.6990); then the bigrams wood pittsburgh, pittsburgh cindy, cindy jean (-0.2550 each) and jean </s>
    (-0.5560), all taken without a back-off."""
    want = (-0.3064 - 0.6990 - 3 * 0.2550 - 0.5560) * LN10
    for blank in (0, 2, 4):
        lm = NGramLM.from_arpa(GOLDEN, TOKENS, blank)
        assert (lm.order, lm.num_classes, lm.blank) == (2, 5, blank)
        # states: the empty history, <s>, and the four words (<unk> is no token and nothing maps to it: dropped)
        assert lm.num_states == 6 and lm.num_arcs == 5 + 5 and lm.start != 0
        assert abs(lm.score("wood pittsburgh cindy jean", eos=True) - want) <= 1e-12
        labels = [lm.class_of(w) for w in "wood pittsburgh cindy jean".split()]
        assert blank not in labels and abs(lm.score(labels) - want) <= 1e-12
        assert abs(lm.score(labels, eos=False) - (want + 0.5560 * LN10)) <= 1e-12


def test_a_present_bigram_is_taken_without_back_off():
    lm = NGramLM.from_arpa(GOLDEN, TOKENS, 4)
    wood, cindy, pitt, jean = range(4)
    w, s_wood = lm.step(lm.start, wood)
    assert abs(w - (-0.3064 - 0.6990) * LN10) <= 1e-12  # (backed off from <s>)
    w, s_pitt = lm.step(s_wood, pitt)
    assert w == -0.2550 * LN10  # (the bigram's own weight, nothing added)
    w, _ = lm.step(s_wood, cindy)  # (absent: wood's back-off and cindy's unigram)
    assert abs(w - (-0.2553 - 0.6990) * LN10) <= 1e-12
    w, _ = lm.step(s_pitt, lm.num_classes)  # </s> after pittsburgh: back-off and the unigram
    assert abs(w - (-0.2553 - 1.0) * LN10) <= 1e-12
    assert lm.step(lm.step(lm.step(s_pitt, cindy)[1], jean)[1], lm.num_classes)[0] == -0.5560 * LN10


def test_tokens_without_a_unigram_take_the_arcs_of_unk():
    lm = NGramLM.from_arpa(GOLDEN, TOKENS + ["zed", "yew"], 0)
    zed, yew, wood = lm.class_of("zed"), lm.class_of("yew"), lm.class_of("wood")
    assert (zed, yew, wood) == (5, 6, 1)
    # "<s> <unk>" and "<unk> wood" are bigrams of the file
    for c in (zed, yew):
        assert lm.score([c], eos=False) == -0.2550 * LN10
        assert abs(lm.score([c, wood], eos=False) - 2 * -0.2550 * LN10) <= 1e-12
        assert abs(lm.score([wood, c], eos=False) - (-0.3064 - 0.6990 - 0.2553 - 1.0) * LN10) <= 1e-12
    assert lm.step(lm.start, zed) == lm.step(lm.start, yew)  # (the same arc, once per class)
    with_unk = NGramLM.from_arpa(GOLDEN, TOKENS + ["<unk>"], 5)
    assert with_unk.score([4], eos=False) == -0.2550 * LN10
    with pytest.raises(ValueError, match="zed"):
        NGramLM.from_arpa(GOLDEN, TOKENS + ["zed"], 0, unk="<none>")
    # a word of the file that is no token is dropped with its grams
    fewer = NGramLM.from_arpa(GOLDEN, ["wood", "jean"], 2)
    assert fewer.num_states == 4 and fewer.num_arcs == 3 + 2  # unigrams wood jean </s>; jean </s>, jean wood


def _write(tmp_path, text):
    p = tmp_path / "lm.arpa"
    p.write_text(text)
    return str(p)


GOOD = open(GOLDEN).read()
TRIGRAM = """\\data\\
ngram 1=4
ngram 2=2
ngram 3=1

\\1-grams:
-1.0\t<s>\t-0.5
-1.0\t</s>
-1.0\twood\t-0.5
-1.0\tjean\t-0.5

\\2-grams:
-0.5\twood jean\t-0.1
-0.5\tjean wood\t-0.1

\\3-grams:
-0.2\t%s

\\end\\
"""
MALFORMED = {
    "no data": (GOOD.replace("\\data\\", "\\date\\"), None),
    "no counts": (GOOD.replace("ngram 1=7\nngram 2=7\n", ""), 2),
    "count mismatch": (GOOD.replace("ngram 2=7", "ngram 2=8"), 14),
    "count line": (GOOD.replace("ngram 2=7", "ngram 2=seven"), 3),
    "orders out of sequence": (GOOD.replace("ngram 2=7", "ngram 3=7"), 3),
    "missing section": (GOOD.replace("\\2-grams:", "\\3-grams:"), 14),
    "too few fields": (GOOD.replace("-0.2550\tcindy jean", "-0.2550\tcindy"), 18),
    "too many fields": (GOOD.replace("-0.2550\tcindy jean", "-0.2550\tcindy jean 0.1 0.2"), 18),
    "not a number": (GOOD.replace("-0.2550\tcindy jean", "x.2550\tcindy jean"), 18),
    "suffix absent": (TRIGRAM % "jean wood wood", 17),  # (jean wood is there, wood wood is not)
    "history absent": (TRIGRAM % "wood wood jean", 17),  # (wood jean is there, wood wood is not)
    "twice": (GOOD.replace("-0.5560\tjean wood", "-0.5560\tjean </s>"), 21),
    "no end": (GOOD.replace("\\end\\", ""), None),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_files_raise_with_the_line(tmp_path, case):
    text, line = MALFORMED[case]
    path = _write(tmp_path, text)
    tokens = ["wood", "jean"] if text.startswith(TRIGRAM[:20]) and "3-grams" in text else TOKENS
    with pytest.raises(ValueError) as err:
        NGramLM.from_arpa(path, tokens, 0)
    assert path in str(err.value)
    if line is not None:
        assert f"{path}:{line}:" in str(err.value), str(err.value)


def test_the_trigram_of_the_malformed_cases_loads_when_its_parts_are_there(tmp_path):
    lm = NGramLM.from_arpa(_write(tmp_path, TRIGRAM % "jean wood jean"), ["wood", "jean"], 0)
    assert (lm.order, lm.num_states) == (3, 1 + 3 + 2)
    assert lm.score([2, 1, 2], eos=False) == (-0.5 - 1.0) * LN10 + -0.5 * LN10 + -0.2 * LN10


def test_loader_argument_checks(tmp_path):
    for tokens, blank in ((TOKENS, -1), (TOKENS, 5), (TOKENS + ["wood"], 0), (TOKENS + ["<s>"], 0), (TOKENS + ["</s>"], 0)):
        with pytest.raises(ValueError):
            NGramLM.from_arpa(GOLDEN, tokens, blank)
    nine = "\\data\\\n" + "".join(f"ngram {n}=0\n" for n in range(1, 10)) + "\n\\end\\\n"
    with pytest.raises(ValueError, match="order"):
        NGramLM.from_arpa(_write(tmp_path, nine), TOKENS, 0)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_score_equals_the_reference_restatement_on_random_lms(tmp_path, order, seed):
    rs = np.random.RandomState(100 * order + seed)
    C = 6
    blank = (0, 3, 5)[seed]
    tokens = [f"t{i}" for i in range(C - 1)]
    text = LR.random_arpa(rs, tokens, order, 0.5, eos=seed != 2)
    lm = NGramLM.from_arpa(_write(tmp_path, text), tokens, blank)
    ref = LR.ArpaLM(text, tokens, blank)
    assert lm.order == order == ref.order
    labels = [c for c in range(C) if c != blank]
    seen_inf = seen_finite = 0
    for _ in range(200):
        seq = [labels[i] for i in rs.randint(0, C - 1, size=rs.randint(0, 8))]
        for eos in (False, True):
            got, want = lm.score(seq, eos=eos), ref.score(seq, eos=eos)
            if want == LR.NEG:
                assert got == LR.NEG
                seen_inf += 1
            else:
                assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (seq, eos, got, want)
                seen_finite += 1
    assert seen_finite > 20
    if seed == 2:
        assert seen_inf >= 200  # (no </s> in the file)
    with pytest.raises(ValueError):
        lm.score([blank])
    with pytest.raises(ValueError):
        lm.score([C + 1])


# ------------------------------------------------------------------------------------------------------------------
# wfl_ngram_lm_check
# ------------------------------------------------------------------------------------------------------------------
def _pack():
    """C = 4, blank 1; state 0: the empty history with arcs 0, 2, 3, </s>; state 1 (start) and 2 back off to 0"""
    return dict(num_classes=4, blank=1, arc_ptr=[0, 4, 5, 6], arc_label=[0, 2, 3, 4, 2, 0], arc_next=[2, 0, 0, 0, 2, 0],
                arc_w=[-1.0, -2.0, -0.5, -1.5, -0.25, -math.inf], bo_next=[-1, 0, 0], bo_w=[0.0, -0.1, -0.2], start=1)


def _desc(p):
    """(the struct, the arrays it points into -- to be kept alive)"""
    arrays = [np.ascontiguousarray(p[k], dtype=t) for k, t in (("arc_ptr", np.int32), ("arc_label", np.int32),
                                                                ("arc_next", np.int32), ("arc_w", np.float64),
                                                                ("bo_next", np.int32), ("bo_w", np.float64))]
    return N.NgramLm(len(p["bo_next"]), len(p["arc_label"]), p["start"], 0, p.get("step_min", 0.0), p.get("step_max", 0.0),
                     *(a.ctypes.data for a in arrays)), arrays


def _check(p):
    desc, _arrays = _desc(p)
    return N.lib.wfl_ngram_lm_check(ctypes.byref(desc), p["num_classes"], p["blank"])


def _chain(n):
    """n + 1 states, state s backs off to s - 1: the chain of the last state has n links"""
    return dict(num_classes=4, blank=1, arc_ptr=[0] + [1] * (n + 1), arc_label=[0], arc_next=[0], arc_w=[-1.0],
                bo_next=[-1] + list(range(n)), bo_w=[0.0] * (n + 1), start=n)


BAD_PACKS = {
    "start below": dict(start=-1),
    "start beyond": dict(start=3),
    "arc_ptr does not start at 0": dict(arc_ptr=[1, 4, 5, 6]),
    "arc_ptr does not end at A": dict(arc_ptr=[0, 4, 5, 5]),
    "arc_ptr descends": dict(arc_ptr=[0, 5, 4, 6]),
    "arc_ptr leaves the arcs": dict(arc_ptr=[0, 7, 5, 6]),
    "label negative": dict(arc_label=[-1, 2, 3, 4, 2, 0]),
    "label above </s>": dict(arc_label=[0, 2, 3, 5, 2, 0]),
    "label is the blank": dict(arc_label=[0, 1, 3, 4, 2, 0]),
    "labels equal": dict(arc_label=[0, 2, 2, 4, 2, 0]),
    "labels descend": dict(arc_label=[0, 3, 2, 4, 2, 0]),
    "next beyond": dict(arc_next=[2, 0, 3, 0, 2, 0]),
    "next negative": dict(arc_next=[2, 0, -1, 0, 2, 0]),
    "weight NaN": dict(arc_w=[-1.0, math.nan, -0.5, -1.5, -0.25, -1.0]),
    "weight +inf": dict(arc_w=[-1.0, math.inf, -0.5, -1.5, -0.25, -1.0]),
    "back-off beyond": dict(bo_next=[-1, 3, 0]),
    "back-off below -1": dict(bo_next=[-2, 0, 0]),
    "back-off weight NaN": dict(bo_w=[0.0, math.nan, -0.2]),
    "back-off to itself": dict(bo_next=[-1, 1, 0]),
    "back-off cycle": dict(bo_next=[2, 0, 1]),
    "blank beyond": dict(blank=4),
    "no classes": dict(num_classes=0, blank=0),
}


def test_the_pack_check_accepts_a_good_pack_and_the_loaders():
    assert _check(_pack()) == N.WFL_OK
    lm = NGramLM(**_pack())
    assert (lm.order, lm.num_states, lm.num_arcs) == (2, 3, 6)
    assert lm.score([2, 0]) == -math.inf and lm.score([2, 2], eos=False) == -0.25 + (-0.2 - 2.0)
    assert _check(_chain(8)) == N.WFL_OK and NGramLM(**_chain(8)).order == 9
    NGramLM.from_arpa(GOLDEN, TOKENS, 0)  # (the constructor runs the check)
    assert N.lib.wfl_ngram_lm_check(None, 4, 1) == N.ERR_INVALID
    desc = N.NgramLm(1, 0, 0, 0, 0.0, 0.0, None, None, None, None, None, None)
    assert N.lib.wfl_ngram_lm_check(ctypes.byref(desc), 4, 1) == N.ERR_INVALID


@pytest.mark.parametrize("case", sorted(BAD_PACKS))
def test_the_pack_check_refuses_every_kind_of_bad_pack(case):
    p = dict(_pack(), **BAD_PACKS[case])
    assert _check(p) == N.ERR_INVALID
    assert "ngram_lm_check" in N.last_error()
    with pytest.raises(ValueError):
        NGramLM(**p)


def test_the_pack_check_writes_the_step_bounds():
    """the pack's arc weights lie in [-inf, -0.25] and its back-off weights in [-0.2, 0]; what the fields held is not read"""
    lm = NGramLM(**_pack())
    assert (lm.step_min, lm.step_max) == (-math.inf, -0.25)
    finite = dict(_pack(), arc_w=[-1.0, -2.0, -0.5, -1.5, -0.25, -3.0])
    assert (NGramLM(**finite).step_min, NGramLM(**finite).step_max) == (-3.0 + 8 * -0.2, -0.25)
    positive = dict(finite, bo_w=[0.0, 0.3, -0.2])
    assert NGramLM(**positive).step_max == -0.25 + 8 * 0.3
    for held in ((0.0, 0.0), (math.nan, math.nan), (5.0, -5.0)):
        desc, _ = _desc(dict(finite, step_min=held[0], step_max=held[1]))
        assert N.lib.wfl_ngram_lm_check(ctypes.byref(desc), 4, 1) == N.WFL_OK
        assert (desc.step_min, desc.step_max) == (-3.0 + 8 * -0.2, -0.25)
    desc, _ = _desc(dict(num_classes=4, blank=1, arc_ptr=[0, 0], arc_label=[], arc_next=[], arc_w=[], bo_next=[-1],
                         bo_w=[0.0], start=0, step_min=7.0, step_max=7.0))
    assert N.lib.wfl_ngram_lm_check(ctypes.byref(desc), 4, 1) == N.WFL_OK and (desc.step_min, desc.step_max) == (0.0, 0.0)
    desc, _ = _desc(dict(_pack(), start=3, step_min=7.0, step_max=7.0))  # (refused: the fields are left alone)
    assert N.lib.wfl_ngram_lm_check(ctypes.byref(desc), 4, 1) == N.ERR_INVALID and (desc.step_min, desc.step_max) == (7.0, 7.0)


def test_the_pack_check_refuses_a_chain_deeper_than_eight():
    assert _check(_chain(9)) == N.ERR_INVALID
    with pytest.raises(ValueError, match="deeper"):
        NGramLM(**_chain(9))
    with pytest.raises(ValueError):  # arrays that do not fit each other never reach the check
        NGramLM(**dict(_pack(), arc_w=[0.0]))
