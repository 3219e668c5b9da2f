"""The device error counts (csrc/error_kernels.hip: wfl_errors_count) past the sizes tests/test_gpu_errors.py runs: a
strip of the distance launch that needs more than one LDS fill of K = wfl_errors_chunk_steps() wavefront steps (cell
values and the diagonal carried in registers, the 62 rows before the fill loaded again, the boundary column read at a
fill behind the first while the strip's last lane overwrites it for the next strip), more than one fill in first, middle
and last strips, and more utterances than a wave has lanes (the second trip of the loops that find an utterance's labels
and its block's base).  The expectation is test_gpu_errors.py's: a plain row-by-row Levenshtein on Python lists; every
count is compared with ==, every buffer lies between guard words.  Each case asserts from this side that it reaches the
branch it is about: steps against K from the stripped lengths, reference symbols against 64, B against 64."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_errors import FLIPS, Guarded, alignment, check, emissions, expected  # noqa: E402

LANES = 64  # reference columns per strip, utterances per trip
SEP = 4     # the separator where one is on: a symbol of the five-symbol alphabet


def _mods():
    from gtn_applications_amd import _native as N
    from gtn_applications_amd import engine as E

    return N, E


def K():
    return _mods()[1].errors_chunk_steps()


def stripped(row, sep):
    lo, hi = 0, len(row)
    while sep >= 0 and lo < hi and row[lo] == sep:
        lo += 1
    while sep >= 0 and hi > lo and row[hi - 1] == sep:
        hi -= 1
    return row[lo:hi]


def fills(n, m):
    """LDS fills of each strip of an n-row, m-column distance: a strip of W columns runs n + W - 1 steps"""
    return [-(-(n + min(LANES, m - j0) - 1) // K()) for j0 in range(0, m, LANES)]


def symbol_fills(hyp, ref, sep):
    return fills(len(stripped(hyp, sep)), len(stripped(ref, sep)))


def words(row, sep):
    out, cur = [], []
    for v in row:
        if v == sep:
            if cur:
                out.append(cur)
            cur = []
        else:
            cur.append(v)
    return out + ([cur] if cur else [])


def keep_ends(row, sep, rs):
    """no separator first or last: stripping leaves the length alone"""
    if sep >= 0 and row:
        for i in (0, -1):
            if row[i] == sep:
                row[i] = int(rs.randint(0, sep))
    return row


def families(rs, n, m, sep):
    """[(hypothesis of n symbols, reference of m symbols, the distance where a closed form gives it)], n >= m >= 1"""
    assert n >= m >= 1
    draw = lambda k: keep_ends(rs.randint(0, 5, size=k).tolist(), sep, rs)  # noqa: E731
    ref = draw(m)
    out = [(draw(n), ref, None)]                                              # random over five symbols: ties
    edited = ref + rs.randint(0, 5, size=n - m).tolist()                      # the reference, three single edits, a tail
    for i in rs.randint(0, m, size=3):
        edited[i] = (edited[i] + 1) % 5
    out.append((keep_ends(edited, sep, rs), ref, None))
    c = m // 2                                                                # the reference with a block of n - m inside:
    out.append((keep_ends(ref[:c] + rs.randint(0, 5, size=n - m).tolist() + ref[c:], sep, rs), ref, n - m))  # |n - m| at least, and at most
    out.append(([2] * n, ref, n - ref.count(2)))                              # one symbol repeated: what matches is the 2s
    out.append(([5 + v for v in draw(n)], ref, n))                            # disjoint alphabets: the longer one's length
    return out


def run_sizes(rs, sizes):
    """every family at every (n, m) of `sizes`, with and without the separator, one launch per setting"""
    for sep in (-1, SEP):
        rows = [(h, r, d, n, m) for n, m in sizes for h, r, d in families(rs, n, m, sep)]
        for h, r, _, n, m in rows:
            assert (len(stripped(h, sep)), len(stripped(r, sep))) == (n, m)
        want = check([r[0] for r in rows], [r[1] for r in rows], sep=sep)
        for w, (_, _, d, n, m) in zip(want, rows):
            assert w[1] == m and (d is None or w[0] == d), (n, m, sep, w, d)


# ------------------------------------------------------------------------------------------------------------------
# one strip across the fill
# ------------------------------------------------------------------------------------------------------------------
def one_strip_cases():
    k = K()
    # (reference m, hypothesis n, steps n + m - 1)
    return [(64, k - 64, k - 1), (64, k - 63, k), (64, k - 62, k + 1), (1, k - 1, k - 1), (1, k, k), (1, k + 1, k + 1), (1, 2 * k, 2 * k),
            (1, 2 * k + 1, 2 * k + 1), (7, k + 5, k + 11)]


@pytest.mark.parametrize("case", range(9))
def test_one_strip_across_the_fill(case):
    m, n, steps = one_strip_cases()[case]
    k = K()
    assert m <= LANES and n + m - 1 == steps and fills(n, m) == [-(-steps // k)]
    assert fills(n, m)[0] == (1 if steps <= k else 2 if steps <= 2 * k else 3)
    if case == 8:
        assert (steps - k) % 2 == 1  # the steps of the second fill: no multiple of an even unroll
    run_sizes(np.random.RandomState(1000 + case), [(n, m)])


# ------------------------------------------------------------------------------------------------------------------
# fills x strips: the boundary column is read at fills behind the first, in first, middle and last strips
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,last_width", [(65, 1), (128, 64), (129, 1), (200, 8)])
def test_fills_times_strips(m, last_width):
    k = K()
    assert m > LANES and m - LANES * ((m - 1) // LANES) == last_width
    sizes = [(n, m) for n in (k - 63, k + 1, 2 * k + 1, 2 * k + 76)]
    assert all(f == 1 for f in fills(k - 63, m))          # the longest hypothesis no strip refills for
    assert min(fills(k + 1, m)) == 2 and min(fills(2 * k + 1, m)) == 3 and min(fills(2 * k + 76, m)) == 3  # every strip, the last included
    assert len(fills(k + 1, m)) == -(-m // LANES) >= (3 if m > 128 else 2)  # (129, 200: a strip neither first nor last)
    run_sizes(np.random.RandomState(m), sizes)


def test_a_removed_block_with_the_best_path_through_row_k():
    """the hypothesis is the reference without 70 symbols that sat around column K: the best path runs down the diagonal
    across row K (and the fill that starts there), takes 70 steps to the right, and goes on down the diagonal"""
    k = K()
    rs = np.random.RandomState(70)
    for sep in (-1, SEP):
        hyp, ref = [], []
        for cut in (k - 35, k - 70, k):
            r = keep_ends(rs.randint(0, 5, size=k + 100).tolist(), sep, rs)
            h = r[:cut] + r[cut + 70:]
            assert len(stripped(h, sep)) == k + 30 and min(symbol_fills(h, r, sep)) == 2 and len(symbol_fills(h, r, sep)) > 2
            hyp.append(h), ref.append(r)
        want = check(hyp, ref, sep=sep)
        assert all(w[:2] == [70, k + 100] for w in want), want  # (|n - m| at least; the removal gives it)


# ------------------------------------------------------------------------------------------------------------------
# separators and words
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [5, 70])
def test_leading_separators_under_a_refill(lead):
    """the stripped range starts at hlo = lead > 0: the fills behind the first read the symbols from there too"""
    k = K()
    rs = np.random.RandomState(lead)
    hyp, ref = [], []
    for n, m in ((k + 1, 64), (k + 1, 129), (2 * k + 3, 65)):
        for h, r, _ in families(rs, n, m, SEP)[:3]:
            h = [SEP] * lead + h + [SEP] * 3
            assert h[lead] != SEP and len(stripped(h, SEP)) == n and min(symbol_fills(h, r, SEP)) >= 2
            hyp.append(h), ref.append([SEP] * 2 + r)
    want = check(hyp, ref, sep=SEP)
    assert [w[1] for w in want] == [64] * 3 + [129] * 3 + [65] * 3
    check(hyp, ref, sep=-1)  # (nothing stripped: the same labels, longer strings)


def test_the_word_distance_across_the_fill():
    """2K + 40 words of one and two symbols against 1, 64, 65 and 130 reference words taken from the hypothesis's last
    words -- the rows behind the second fill -- every third one longer by a symbol, every third one with another last
    symbol"""
    k = K()
    rs = np.random.RandomState(8)
    hwords = [rs.randint(0, 4, size=1 + rs.randint(2)).tolist() for _ in range(2 * k + 40)]
    hyp_row = [v for w in hwords for v in w + [SEP]]
    hyp, ref, counts = [], [], (1, 64, 65, 130)
    for nw in counts:
        rwords = [list(w) for w in hwords[-nw:]]
        for i, w in enumerate(rwords):
            if i % 3 == 1:
                w.append(int(rs.randint(0, 4)))         # differs only in its length
            elif i % 3 == 2:
                w[-1] = (w[-1] + 1) % 4                 # ... only in its last symbol
        hyp.append(hyp_row), ref.append([v for w in rwords for v in [SEP] + w])
        assert len(words(hyp_row, SEP)) == 2 * k + 40 and len(words(ref[-1], SEP)) == nw
        assert min(fills(2 * k + 40, nw)) == 3 and len(fills(2 * k + 40, nw)) == -(-nw // LANES)
    want = check(hyp, ref, sep=SEP)
    assert [w[3] for w in want] == list(counts)
    assert all(2 * k + 40 - nw <= w[2] <= 2 * k + 40 for nw, w in zip(counts, want))
    # the hypothesis's last 65 words as they are: every word before them is a deletion, nothing else
    tail = [v for w in hwords[-65:] for v in w + [SEP]]
    assert check([hyp_row], [tail], sep=SEP)[0][2:] == [2 * k + 40 - 65, 65]


def test_a_word_longer_than_the_fill():
    k = K()
    rs = np.random.RandomState(9)
    long_word = rs.randint(0, 4, size=k + 10).tolist()
    the = [1, 2, 3]
    other = long_word[:-1] + [(long_word[-1] + 1) % 4]
    hyp = [long_word + [SEP] + the, long_word + [SEP] + the, the + [SEP] + long_word, long_word, long_word + [0]]
    ref = [long_word + [SEP] + the, other + [SEP] + the, the + [SEP] + other + [SEP], other, long_word]
    for h, r in zip(hyp, ref):
        assert max(len(w) for w in words(h, SEP)) > k and min(symbol_fills(h, r, SEP)) >= 2
    want = check(hyp, ref, sep=SEP)
    assert want[0] == [0, k + 14, 0, 2] and want[1] == [1, k + 14, 1, 2] and want[2] == [1, k + 14, 1, 2]
    assert want[3] == [1, k + 10, 1, 1] and want[4] == [1, k + 10, 1, 1]


# ------------------------------------------------------------------------------------------------------------------
# expansion tables: about 300 labels, more than 2K symbols
# ------------------------------------------------------------------------------------------------------------------
def test_expansion_tables_across_the_fill():
    k = K()
    twelve = [1, 2, 3, 1, 2, 3, 1, 1, 2, 2, 3, 3]
    table = [[], [1], twelve, [SEP, SEP], [2, SEP, 3], [3, 1], [2], twelve[::-1]]
    rs = np.random.RandomState(12)
    labels = rs.randint(0, len(table), size=300).tolist()
    labels[0], labels[-1] = 1, 6  # (no separator at either end)
    L = sum(len(table[v]) for v in labels)
    assert L > 2 * k, L
    short, longer = keep_ends(rs.randint(1, 5, size=200).tolist(), SEP, rs), keep_ends(rs.randint(1, 5, size=k + 5).tolist(), SEP, rs)
    for sep in (SEP, -1):
        assert min(fills(L, 200)) >= 3 and len(fills(L, 200)) == 4
        want = check([labels, labels], [short, longer], hyp_table=table, sep=sep)
        assert [w[1] for w in want] == [200, k + 5]
        # the sides swapped: 2K symbols and more of reference, strip after strip, without a refill and with one
        assert max(fills(200, L)) == 1 and min(fills(k + 5, L)) == 2 and len(fills(k + 5, L)) > 16
        want = check([short, longer], [labels, labels], ref_table=table, sep=sep)
        assert [w[1] for w in want] == [L, L]


# ------------------------------------------------------------------------------------------------------------------
# more utterances than lanes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [33, 64, 65, 130])
def test_more_utterances_than_lanes(B):
    """b >= 64: the second trip over the offsets that finds an utterance's labels; 2 B > 64: the second trip over the
    blocks before a reference's (the hypotheses' blocks come first).  Two batches: ragged rows with empty ones around
    the 64th utterance and at both ends, and the same with the last utterances filled and, where B > 64, a long pair -- a
    refill, three strips -- behind the first 64."""
    k = K()
    assert 2 * B > LANES and (B > LANES) == (B in (65, 130))
    rs = np.random.RandomState(B)
    table = [[], [1], [1, 2, 3, 1, 2, 3, 1, 1, 2, 2, 3, 3], [SEP, SEP], [2, SEP, 3], [3, 1], [2], [3]]
    single = {1: 1, 2: 6, 3: 7}  # symbol -> a label that stands for it alone
    for tabled in (False, True):
        top = len(table) if tabled else 5
        kw = dict(hyp_table=table, ref_table=table) if tabled else {}
        hyp = [rs.randint(0, top, size=rs.randint(0, 41)).tolist() for _ in range(B)]
        ref = [rs.randint(0, top, size=rs.randint(0, 41)).tolist() for _ in range(B)]
        for b in (0, 63, 64, 65, B - 1):
            if b < B:
                hyp[b], ref[b] = [], []
        if B > 66:
            hyp[B - 2], ref[66] = [], []  # (one side empty)
        for sep in (-1, SEP):
            want = check(hyp, ref, sep=sep, **kw)
            assert len(want) == B and all(want[b] == [0, 0, 0, 0] for b in (0, 63, 64, 65, B - 1) if b < B)
        # the same batch with its last utterances filled: the last reference's block is the one with most blocks before it
        for b in (B - 2, B - 1):
            hyp[b], ref[b] = rs.randint(0, top, size=20 + b % 7).tolist(), rs.randint(0, top, size=30 + b % 5).tolist()
        if B > LANES:
            hyp[63], ref[63] = [1, 2, 1], [2, 1]  # (the utterance before the long pair is not empty)
        for b in (64, 129):
            if b < B:
                n, m = k + 90, 130
                h, r = families(rs, n, m, -1)[b % 2][:2]
                if tabled:
                    h, r = [single[1 + v % 3] for v in h], [single[1 + v % 3] for v in r]
                assert (len(h), len(r)) == (n, m) and min(fills(n, m)) == 2 and len(fills(n, m)) == 3
                hyp[b], ref[b] = h, r
        for sep in (-1, SEP):
            want = check(hyp, ref, sep=sep, **kw)
            assert want[B - 1][1] > 0 and (B <= LANES or want[64][1] > LANES) and (B < 130 or want[129][1] > LANES)


def test_offsets_that_do_not_ascend_with_more_utterances_than_lanes():
    """whatever the offsets say the kernels stay inside the buffers (the count itself is then unspecified)"""
    N, E = _mods()
    B, n = 130, 300
    assert B > 2 * LANES
    rs = np.random.RandomState(130)
    lab = Guarded(n).set(rs.randint(0, 5, size=n).astype(np.int32))
    wild = rs.randint(-50, n + 50, size=B + 1).astype(np.int64)
    wild[[3, 64, 65, 129]] = [1 << 40, -(1 << 40), 0x7fffffff, -1]
    down = np.arange(n, n - B - 1, -1).astype(np.int64)
    good = np.sort(rs.randint(0, n + 1, size=B + 1)).astype(np.int64)
    good[0], good[B] = 0, n
    bad, worse, fine = (Guarded(2 * (B + 1)).set(o) for o in (wild, down, good))
    nws = ctypes.c_int64()
    N.check(N.lib.wfl_errors_workspace(B, n, n, 1, 1, ctypes.byref(nws)))
    ws, counts = Guarded(nws.value // 4), Guarded(4 * B)
    for ho, ro in ((bad, fine), (fine, bad), (bad, bad), (worse, fine), (fine, worse), (bad, worse)):
        for sep in (2, -1):
            N.check(N.lib.wfl_errors_count(lab.ptr, ho.ptr, lab.ptr, ro.ptr, B, None, None, 0, None, None, 0, sep, n, n, ws.ptr, counts.ptr,
                                           E.stream_ptr()))
            torch.cuda.synchronize()
            assert all(g.intact() for g in (lab, bad, worse, fine, ws, counts))
            assert np.all(counts.data() >= 0) and np.all(counts.data() <= n)
    # (ascending on both sides: the same buffers count what the lists say)
    rows = [lab.data()[good[b]:good[b + 1]].tolist() for b in range(B)]
    N.check(N.lib.wfl_errors_count(lab.ptr, fine.ptr, lab.ptr, fine.ptr, B, None, None, 0, None, None, 0, 2, n, n, ws.ptr, counts.ptr, E.stream_ptr()))
    torch.cuda.synchronize()
    assert counts.data().reshape(B, 4).tolist() == expected(rows, rows, sep=2) and all(c[0] == 0 for c in counts.data().reshape(B, 4))


# ------------------------------------------------------------------------------------------------------------------
# the modules: errors() == counter(viterbi()) == the expectation
# ------------------------------------------------------------------------------------------------------------------
def module_counts(crit, x, targets, counter, table, sep):
    xd = x.cuda()
    hyp = [t.tolist() for t in crit.viterbi(xd)]
    rows = [t.tolist() for t in targets]
    want_rows = expected(hyp, rows, table, table, sep)
    want = (sum(r[0] for r in want_rows), sum(r[2] for r in want_rows), sum(r[1] for r in want_rows), sum(r[3] for r in want_rows))
    assert crit.errors(xd, targets, counter) == counter(crit.viterbi(xd), targets) == want
    return hyp, want


def ctc_setup():
    from gtn_applications_amd import ErrorCounter
    from gtn_applications_amd.criterions import ctc

    tokens = ["a", "b", "c", "d", "_"]
    return ctc.CTC(blank=len(tokens), use_pt=False), ErrorCounter(tokens, tokens, "_"), tokens, len(tokens) + 1, len(tokens), 0


def asg_setup():
    from gtn_applications_amd import ErrorCounter
    from gtn_applications_amd.criterions import asg

    tokens = ["a", "b", "c", "_", "d", "e"]
    R = 2
    crit = asg.ASG(len(tokens), num_replabels=R, use_garbage=False).cuda()
    with torch.no_grad():
        crit.transitions.copy_(torch.from_numpy(0.1 * np.random.RandomState(32).randn(crit.N + 1, crit.N).astype(np.float32)))
    return crit, ErrorCounter(tokens, tokens, "_"), tokens, crit.N, None, R


@pytest.mark.parametrize("shape", ["across the fill", "more than 64 utterances"])
@pytest.mark.parametrize("setup", [ctc_setup, asg_setup])
def test_module_errors_across_the_fill_and_the_lanes(setup, shape):
    """peaked emissions (test_gpu_errors.py's helpers): B = 3, T = 2K + 200 with targets of about K labels -- the decoded
    hypotheses need a second fill --, and B = 70, T = 130 with short targets"""
    crit, counter, tokens, C, blank, R = setup()
    k, ntok = K(), len(tokens)
    rs = np.random.RandomState(77 + len(shape))
    if shape == "across the fill":
        B, T, lens = 3, 2 * k + 200, [k, k - 20, k + 10]
    else:
        B, T, lens = 70, 130, [0] + [int(v) for v in rs.randint(0, 30, size=68)] + [0]
    # (no label twice in a row: the alignment spells a target with its own labels, without blanks between or replabels)
    rows = [[int(v) for v in (rs.permutation(ntok).tolist() * (n // ntok + 1))[:n]] for n in lens]
    targets = [torch.tensor(r, dtype=torch.int64) for r in rows]
    frames = alignment(rs, [[v + R for v in r] for r in rows], T, -1 if blank is None else blank)
    if blank is None:  # ASG without garbage: the frames between the labels repeat the label before them
        for b in range(B):
            for t in range(T):
                if frames[b, t] < 0:
                    frames[b, t] = frames[b, t - 1] if t else (rows[b][0] if rows[b] else 0) + R
    x = emissions(rs, "peaked", frames, C)
    table = [[counter.symbol_ids[c] for c in t] for t in tokens]
    sep = counter.symbol_ids["_"]
    hyp, want = module_counts(crit, x, targets, counter, table, sep)
    if shape == "across the fill":
        for h, r in zip(hyp, rows):
            hs, rr = stripped([table[v][0] for v in h], sep), stripped([table[v][0] for v in r], sep)
            assert len(hs) > k - 63 and len(rr) > LANES and min(fills(len(hs), len(rr))) >= 2, (len(hs), len(rr))
        assert 0 < want[0] <= 4 * FLIPS * B, want  # small and not zero
    else:
        assert B > LANES and len(hyp) == B and any(hyp[LANES:])
