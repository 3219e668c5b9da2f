"""tests/beam_support.py's acceptance still bites: assert_ranks passes a hand-made two-utterance, two-rank result and
raises on each single departure from it, margins_ok raises on a margin below its bar.  No device, no library."""
import copy
import math

import numpy as np
import pytest

import beam_support as S

NEG = -math.inf
BLANK = 3
WANT = [[((0, 1), -12.5), ((2,), -14.25)], [((1,), -0.5), ((), NEG)]]
LOGZ = [-3.0, 2.0]


def result():
    """(seqs, raw, normed) of a device that agrees with WANT"""
    seqs = [[h for h, _ in hyps] for hyps in WANT]
    raw = np.array([[s for _, s in hyps] for hyps in WANT])
    normed = np.array([[s - LOGZ[b] for _, s in hyps] for b, hyps in enumerate(WANT)])
    return seqs, raw, normed


def accept(seqs, raw, normed):
    S.assert_ranks(WANT, seqs, raw, normed, LOGZ, 2, blank=BLANK)


def test_an_agreeing_result_passes_as_arrays_and_as_lists():
    seqs, raw, normed = result()
    accept(seqs, raw, normed)
    accept(seqs, raw.tolist(), normed.tolist())
    calls = []
    S.assert_ranks(WANT, seqs, raw, normed, LOGZ, 2, check=lambda b, r, seq: calls.append((b, r, seq)))
    assert calls == [(0, 0, (0, 1)), (0, 1, (2,)), (1, 0, (1,)), (1, 1, ())]  # (every rank, the -inf one too)
    S.assert_ranks([None, WANT[1]], [[(9,), (9,)], seqs[1]], raw, normed, LOGZ, 2)  # (None: the utterance is left out)


@pytest.mark.parametrize("b,r", [(0, 0), (0, 1), (1, 0)])
def test_a_raw_score_off_by_twice_its_bar_fails(b, r):
    seqs, raw, normed = result()
    for sign in (1.0, -1.0):
        off = raw.copy()
        off[b, r] += sign * 2e-9 * max(1.0, abs(raw[b, r]))
        with pytest.raises(AssertionError):
            accept(seqs, off, normed)
        near = raw.copy()
        near[b, r] += sign * 0.5e-9 * max(1.0, abs(raw[b, r]))
        accept(seqs, near, normed)


@pytest.mark.parametrize("b,r", [(0, 0), (0, 1), (1, 0)])
def test_a_normalised_score_off_by_twice_its_bar_fails(b, r):
    seqs, raw, normed = result()
    for sign in (1.0, -1.0):
        off = normed.copy()
        off[b, r] += sign * 2.0 * (1e-4 * abs(normed[b, r]) + 2e-5)
        with pytest.raises(AssertionError):
            accept(seqs, raw, off)
        near = normed.copy()
        near[b, r] += sign * 0.5 * (1e-4 * abs(normed[b, r]) + 2e-5)
        accept(seqs, raw, near)


def test_two_ranks_swapped_fail():
    seqs, raw, normed = result()
    seqs[0] = seqs[0][::-1]
    with pytest.raises(AssertionError):
        accept(seqs, raw, normed)


def test_a_minus_infinity_rank_that_comes_back_finite_fails():
    seqs, raw, normed = result()
    for which in (0, 1):
        got = [raw.copy(), normed.copy()]
        got[which][1, 1] = -1e300
        with pytest.raises(AssertionError):
            accept(seqs, *got)


def test_the_blank_in_a_sequence_fails():
    seqs, raw, normed = result()
    want = copy.deepcopy(WANT)
    want[0][1] = ((2, BLANK), -14.25)  # (even where the restatement said so too)
    seqs[0][1] = (2, BLANK)
    S.assert_ranks(want, seqs, raw, normed, LOGZ, 2)
    with pytest.raises(AssertionError):
        S.assert_ranks(want, seqs, raw, normed, LOGZ, 2, blank=BLANK)
    with pytest.raises(AssertionError):  # (and in an utterance that is left out)
        S.assert_ranks([None, want[1]], seqs, raw, normed, LOGZ, 2, blank=BLANK)


def test_a_failing_check_fails():
    seqs, raw, normed = result()

    def check(b, r, seq):
        assert seq != ()

    with pytest.raises(AssertionError):
        S.assert_ranks(WANT, seqs, raw, normed, LOGZ, 2, check=check)


def test_margins_ok_raises_below_its_bar_and_counts_what_was_found():
    hyps = [((1,), -2.0)]
    assert S.margins_ok(lambda b: (hyps, 1e-9, b), 3) == [(hyps, 1e-9, 0), (hyps, 1e-9, 1), (hyps, 1e-9, 2)]
    with pytest.raises(AssertionError):
        S.margins_ok(lambda b: (hyps, 5e-10 if b == 2 else 1.0, 0), 3)
    empty = [((), -1.0)]
    found = lambda h: len(h[0][0]) >= 1
    S.margins_ok(lambda b: (empty if b == 0 else hyps, 1.0, 0), 4, found)  # (three of four)
    with pytest.raises(AssertionError):
        S.margins_ok(lambda b: (empty if b < 2 else hyps, 1.0, 0), 4, found)
    with pytest.raises(AssertionError):  # (a rank 0 of -inf shows nothing)
        S.margins_ok(lambda b: ([((1,), NEG)] if b < 2 else hyps, 1.0, 0), 4, found)
