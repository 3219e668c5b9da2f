"""Token and word error counts on the device (csrc/error_kernels.hip: wfl_errors_count) against the reference's
compute_edit_distance (train.py:74-87) restated here: a plain row-by-row Levenshtein on Python lists, the join, strip and
split by Python's own str methods on strings built from the tables.  Everything is integers and compared with ==.
Through the C ABI every buffer has poisoned words around it; through the modules, errors() must give what
counter(viterbi()) gives, on the device route and the host route, at frame counts that straddle the decode's chunk."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B
GUARD = 16  # int32 words on either side of every buffer


def _mods():
    from gtn_applications_amd import _native as N
    from gtn_applications_amd import engine as E

    return N, E


# ------------------------------------------------------------------------------------------------------------------
# the expectation
# ------------------------------------------------------------------------------------------------------------------
def levenshtein(a, b):
    """row by row, unit costs; a and b are lists (of symbols, or of words)"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[len(b)]


_CHARS = {}


def char(symbol):
    """a character of its own per symbol (symbols are any int32: labels under an identity table)"""
    return _CHARS.setdefault(symbol, chr(0x100 + len(_CHARS)))


def text(labels, table):
    """the labels' symbols as a str, one character per symbol (a label outside the table expands to nothing)"""
    if table is None:
        return "".join(char(v) for v in labels)
    return "".join(char(s) for v in labels if 0 <= v < len(table) for s in table[v])


def expected(hyp, ref, hyp_table=None, ref_table=None, sep=-1):
    """compute_edit_distance's four numbers per utterance (train.py:79-86)"""
    rows = []
    for h, r in zip(hyp, ref):
        p, t = text(h, hyp_table), text(r, ref_table)
        if sep < 0:
            rows.append([levenshtein(list(p), list(t)), len(t), 0, 0])
            continue
        c = char(sep)
        p, t = p.strip(c), t.strip(c)
        pw, tw = list(filter(None, p.split(c))), list(filter(None, t.split(c)))
        rows.append([levenshtein(list(p), list(t)), len(t), levenshtein(pw, tw), len(tw)])
    return rows


# ------------------------------------------------------------------------------------------------------------------
# the C ABI, every buffer between guard words
# ------------------------------------------------------------------------------------------------------------------
class Guarded:
    """an int32 device (or pinned host) buffer of n words with GUARD poisoned words on either side"""

    def __init__(self, n, fill=POISON, pinned=False):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device="cpu" if pinned else "cuda")
        if pinned:
            self.buf = self.buf.pin_memory()
        self.buf[GUARD:GUARD + n] = fill

    def set(self, values):
        v = torch.from_numpy(np.ascontiguousarray(values)).view(torch.int32)
        assert v.numel() == self.n
        self.buf[GUARD:GUARD + self.n] = v.to(self.buf.device)
        return self

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def data(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy()

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:GUARD] == POISON) and np.all(b[GUARD + self.n:] == POISON))


def flatten(rows):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return np.asarray([v for r in rows for v in r], np.int32), off


def device_table(table):
    """(Guarded [exp_ptr | exp_sym], V, longest) of a list of symbol lists"""
    ptr = np.zeros(len(table) + 1, np.int32)
    np.cumsum([len(s) for s in table], out=ptr[1:])
    sym = np.asarray([s for e in table for s in e], np.int32)
    both = np.concatenate([ptr, sym]).astype(np.int32)
    return Guarded(len(both)).set(both), len(table), max(len(s) for s in table)


def abi_counts(hyp, ref, hyp_table=None, ref_table=None, sep=-1, pinned=False, slack=5):
    """wfl_errors_count on lists of label lists; `slack`: capacity of the hypothesis buffer beyond its labels (the decode's
    out holds B T labels, few of them used).  Checks the guard words of every buffer."""
    N, E = _mods()
    B = len(hyp)
    hflat, hoff = flatten(hyp)
    rflat, roff = flatten(ref)
    hcap, rn = len(hflat) + slack, len(rflat)
    gh = Guarded(max(hcap, 1), fill=0x7FFFFFF0)  # (behind the labels: never read as labels)
    gh.buf[GUARD:GUARD + len(hflat)] = torch.from_numpy(hflat).cuda()
    gr = Guarded(max(rn, 1)).set(rflat if rn else np.array([POISON], np.int32))
    gho, gro = Guarded(2 * (B + 1)).set(hoff), Guarded(2 * (B + 1)).set(roff)
    ht = device_table(hyp_table) if hyp_table is not None else (None, 0, 1)
    rt = device_table(ref_table) if ref_table is not None else (None, 0, 1)
    nws = ctypes.c_int64()
    N.check(N.lib.wfl_errors_workspace(B, hcap, rn, ht[2], rt[2], ctypes.byref(nws)))
    assert nws.value % 4 == 0
    ws = Guarded(nws.value // 4)
    counts = Guarded(4 * B, pinned=pinned)

    def tp(t, part):
        return None if t[0] is None else t[0].ptr + (4 * (t[1] + 1) if part else 0)

    N.check(N.lib.wfl_errors_count(gh.ptr, gho.ptr, gr.ptr, gro.ptr, B, tp(ht, 0), tp(ht, 1), ht[1], tp(rt, 0), tp(rt, 1), rt[1],
                                   sep, hcap, rn, ws.ptr, counts.ptr, E.stream_ptr()))
    torch.cuda.synchronize()
    for name, g in (("hyp", gh), ("ref", gr), ("hyp_off", gho), ("ref_off", gro), ("ws", ws), ("counts", counts), ("hyp table", ht[0]),
                    ("ref table", rt[0])):
        assert g is None or g.intact(), f"stores outside {name}"
    assert np.array_equal(gh.data()[:len(hflat)], hflat) and np.array_equal(gho.data().view(np.int64), hoff)  # (inputs untouched)
    return counts.data().reshape(B, 4).tolist()


def check(hyp, ref, **kw):
    want = expected(hyp, ref, kw.get("hyp_table"), kw.get("ref_table"), kw.get("sep", -1))
    got = abi_counts(hyp, ref, **kw)
    assert got == want, (kw, [(h, r) for h, r, g, w in zip(hyp, ref, got, want) if g != w][:2])
    return want


REF_LENS = (0, 1, 63, 64, 65, 128, 129)
HYP_LENS = (0, 1, 63, 64, 65, 130, 257)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_lengths_around_the_strip_width(B):
    """every pair of lengths over a 5-symbol alphabet (many ties among the three moves), ragged rows"""
    rs = np.random.RandomState(B)
    pairs = [(r, h) for r in REF_LENS for h in HYP_LENS]
    for k in range(0, len(pairs), B):
        rows = pairs[k:k + B]
        rows += [(REF_LENS[rs.randint(7)], HYP_LENS[rs.randint(7)]) for _ in range(B - len(rows))]
        ref = [rs.randint(0, 5, size=r).tolist() for r, _ in rows]
        hyp = [rs.randint(0, 5, size=h).tolist() for _, h in rows]
        # mostly equal strings with a few edits exercise the diagonal move; random ones the ties
        for b, (r, h) in enumerate(rows):
            if (k + b) % 2 and r and h:
                n = min(r, h)
                hyp[b][:n] = ref[b][:n]
                for i in rs.randint(0, n, size=3):
                    hyp[b][i] = (hyp[b][i] + 1) % 5
        want = check(hyp, ref)
        check(hyp, ref, sep=4)  # the same strings with one of the five symbols as the separator
        assert [w[1] for w in want] == [r for r, _ in rows]


@pytest.mark.parametrize("n", [64, 65])
def test_structured_pairs(n):
    rs = np.random.RandomState(n)
    a = rs.randint(0, 5, size=n).tolist()
    ref = [a, a, a, a[:n - 7], a, a[7:], a, [2] * n, a]
    hyp = [a, [v + 5 for v in a], a[:n - 7], a, a[7:], a, [2] * n, a, []]
    want = check(hyp, ref)
    assert want[0][0] == 0 and want[1][0] == n and want[2][0] == 7 and want[3][0] == 7 and want[4][0] == 7 and want[5][0] == 7
    assert want[6][0] == n - a.count(2) == want[7][0] and want[8][0] == n
    # disjoint alphabets of different lengths: the longer one's length
    assert check([[9] * (n + 3), [9] * 5], [a, a])[0][0] == n + 3


def test_separator_handling():
    s = 0
    the, then = [3, 4, 5], [3, 4, 5, 6]
    long_word = list(range(1, 71))
    cases = [
        ([s, s] + the + [s] + then + [s], the + [s] + then),                # leading, trailing
        (the + [s, s, s] + then, the + [s] + then),                          # doubled inside: the strings differ, the words do not
        ([s, s, s], the),                                                     # only separators
        (the, [s]),
        ([s], [s, s]),
        ([], [s]),
        (the + [s] + then, then + [s] + the),                                 # words that differ only in length
        ([3, 4, 5] + [s] + [3, 4, 7], [3, 4, 6] + [s] + [3, 4, 7]),           # ... only in the last symbol
        (long_word + [s] + the, long_word[:-1] + [99] + [s] + the),           # a word of 70 symbols, the last one differs
        (long_word + [s] + the, long_word + [s] + then),
        ([v for k in range(130) for v in (1 + k % 3, s)], [v for k in range(130) for v in (1 + (k // 2) % 3, s)]),  # 130 one-symbol words
        ([s] + [v for k in range(130) for v in (1 + k % 3, s)], [1]),
    ]
    hyp, ref = [c[0] for c in cases], [c[1] for c in cases]
    want = check(hyp, ref, sep=s)
    assert want[0] == [0, 8, 0, 2] and want[1] == [2, 8, 0, 2] and want[2] == [3, 3, 1, 1] and want[3] == [3, 0, 1, 0]
    assert want[4] == [0, 0, 0, 0] and want[6][2:] == [2, 2] and want[7][2:] == [1, 2] and want[8][2:] == [1, 2] and want[9] == [1, 75, 1, 2]
    assert want[10][3] == 130 and want[11][2:] == [129, 1]
    # sep = -1: nothing is stripped, no words
    want = check(hyp, ref, sep=-1)
    assert want[0][:2] == [3, 8] and all(w[2:] == [0, 0] for w in want)
    # a separator that no string contains
    assert all(w[3] == (1 if w[1] else 0) for w in check(hyp, ref, sep=1000))


def test_expansion_tables():
    s = 0
    twelve = list(range(1, 13))
    # label: 0 nothing, 1 one symbol, 2 twelve symbols, 3 only separators, 4 a separator inside, 5 / 6 words
    table_a = [[], [5], twelve, [s, s], [7, s, 8], [3, 4], [9]]
    table_b = [[s], [3, 4, s], [5], [], twelve + [s], [7], [8, s, 9]]
    rs = np.random.RandomState(5)
    hyp = [rs.randint(0, 7, size=n).tolist() for n in (0, 1, 9, 40, 64, 65, 3)] + [[3, 3], [0, 0, 0], [2] * 11]
    ref = [rs.randint(0, 7, size=n).tolist() for n in (2, 0, 11, 33, 65, 64, 3)] + [[1], [3], [2] * 11]
    for kw in (dict(hyp_table=table_a, ref_table=table_b), dict(hyp_table=table_b, ref_table=table_a), dict(hyp_table=table_a),
               dict(ref_table=table_b), dict(hyp_table=table_a, ref_table=table_a)):
        for sep in (s, -1):
            check(hyp, ref, sep=sep, **kw)
    want = check(hyp, ref, hyp_table=table_a, ref_table=table_a, sep=s)
    assert want[7] == [1, 1, 1, 1] and want[8] == [0, 0, 0, 0] and want[9] == [0, 132, 0, 1]


def test_out_of_table_labels_expand_to_nothing():
    table = [[1], [2, 0], [3]]
    hyp = [[0, 7, 1, -1, 2], [1000000, -5], [2, 2, 0x7FFFFFFF]]
    ref = [[0, 1, 2], [1, 3], [2, -2147483648, 2]]
    want = check(hyp, ref, hyp_table=table, ref_table=table, sep=0)
    assert want == [[0, 4, 0, 2], [1, 1, 1, 1], [0, 2, 0, 1]]
    check(hyp, ref, hyp_table=table, sep=0)  # (identity on the reference side: any label is a symbol)


def test_counts_in_pinned_host_memory():
    rs = np.random.RandomState(3)
    hyp = [rs.randint(0, 4, size=n).tolist() for n in (70, 0, 5, 131)]
    ref = [rs.randint(0, 4, size=n).tolist() for n in (66, 3, 0, 20)]
    assert abi_counts(hyp, ref, sep=0, pinned=True) == abi_counts(hyp, ref, sep=0) == expected(hyp, ref, sep=0)


def test_offsets_that_do_not_ascend_stay_inside_the_buffers():
    """whatever the offsets say the kernels stay inside the buffers (the count itself is then unspecified)"""
    N, E = _mods()
    B = 3
    lab = Guarded(10).set(np.arange(10, dtype=np.int32))
    bad = Guarded(2 * (B + 1)).set(np.array([5, 99, -3, 7], np.int64))
    good = Guarded(2 * (B + 1)).set(np.array([0, 3, 3, 10], np.int64))
    nws = ctypes.c_int64()
    N.check(N.lib.wfl_errors_workspace(B, 10, 10, 1, 1, ctypes.byref(nws)))
    ws, counts = Guarded(nws.value // 4), Guarded(4 * B)
    for ho, ro in ((bad, good), (good, bad), (bad, bad)):
        N.check(N.lib.wfl_errors_count(lab.ptr, ho.ptr, lab.ptr, ro.ptr, B, None, None, 0, None, None, 0, 2, 10, 10, ws.ptr, counts.ptr,
                                       E.stream_ptr()))
        torch.cuda.synchronize()
        assert all(g.intact() for g in (lab, bad, good, ws, counts))
        assert np.all(counts.data() >= 0) and np.all(counts.data() <= 10)


# ------------------------------------------------------------------------------------------------------------------
# the modules: errors() == counter(viterbi()) == the same on the host route == the expectation
# ------------------------------------------------------------------------------------------------------------------
def frame_counts():
    K = _mods()[0].lib.wfl_decode_chunk_frames()
    return [K - 1, K, K + 1, 2 * K + 1]


FLIPS = 2


def emissions(rs, kind, aligned, C):
    """white noise, or scores peaked on the frame labels `aligned` [B, T] with FLIPS frames per utterance moved to
    another class"""
    B, T = aligned.shape
    if kind == "noise":
        return torch.from_numpy(rs.randn(B, T, C).astype(np.float32))
    lab = aligned.copy()
    for b in range(B):
        for t in rs.choice(T, size=FLIPS, replace=False):
            lab[b, t] = (lab[b, t] + 1 + rs.randint(C - 1)) % C
    x = 0.1 * rs.randn(B, T, C).astype(np.float32)
    x[np.arange(B)[:, None], np.arange(T)[None, :], lab] += 8.0
    return torch.from_numpy(x)


def alignment(rs, rows, T, filler):
    """frame labels [B, T]: the labels of each row in order, each over a run of frames, `filler` (blank / garbage) frames
    between and around them where there is room"""
    out = np.full((len(rows), T), filler, np.int64)
    for b, row in enumerate(rows):
        assert 2 * len(row) + 1 <= T
        cuts = np.sort(rs.choice(np.arange(1, T), size=2 * len(row), replace=False))
        for k, v in enumerate(row):
            out[b, cuts[2 * k]:cuts[2 * k + 1]] = v
    return out


def module_routes(crit, x, targets, counter, want_rows):
    """the four ways to the same tuple"""
    want = (sum(r[0] for r in want_rows), sum(r[2] for r in want_rows), sum(r[1] for r in want_rows), sum(r[3] for r in want_rows))
    xd = x.cuda()
    fused = crit.errors(xd, targets, counter)
    assert all(type(v) is int for v in fused) and len(fused) == 4
    assert fused == counter(crit.viterbi(xd), targets) == counter(crit.viterbi(x), targets) == crit.errors(x, targets, counter) == want
    return want


def test_ctc_module_errors(monkeypatch):
    from gtn_applications_amd import ErrorCounter
    from gtn_applications_amd import metrics as M
    from gtn_applications_amd.criterions import ctc

    tokens = ["a", "b", "c", "d", "_"]
    C, blank, sep = len(tokens) + 1, len(tokens), 4
    counter = ErrorCounter(tokens, tokens, "_")
    table = [[counter.symbol_ids[c] for c in t] for t in tokens]
    crit = ctc.CTC(blank=blank, use_pt=False)
    used = []
    real = M.decode_emissions_errors
    monkeypatch.setattr(M, "decode_emissions_errors", lambda *a, **k: used.append(1) or real(*a, **k))
    rs = np.random.RandomState(21)
    for T in frame_counts():
        B = 4
        targets = [torch.from_numpy(rs.randint(0, len(tokens), size=n)) for n in (T // 3, 1, T // 4, 0)]
        rows = [t.tolist() for t in targets]
        for kind in ("noise", "peaked"):
            x = emissions(rs, kind, alignment(rs, rows, T, blank), C)
            hyp = [t.tolist() for t in crit.viterbi(x)]
            want = module_routes(crit, x, targets, counter, expected(hyp, rows, table, table, counter.symbol_ids["_"]))
            if kind == "peaked":
                assert 0 < want[0] <= 4 * FLIPS * B, want  # small and not zero
    assert len(used) == 2 * len(frame_counts())  # (the device inputs took the fused route, the host inputs did not)
    # lists as targets, an identity counter without a separator
    ident = ErrorCounter()
    x = emissions(rs, "noise", np.zeros((2, 70), np.int64), C)
    hyp = [t.tolist() for t in crit.viterbi(x)]
    module_routes(crit, x, [[1, 2, 3], [0]], ident, expected(hyp, [[1, 2, 3], [0]]))


@pytest.mark.parametrize("R,garbage", [(1, True), (2, False)])
def test_asg_module_errors(R, garbage):
    from gtn_applications_amd import ErrorCounter
    from gtn_applications_amd.criterions import asg

    tokens = ["a", "b", "c", "_", "d", "e"]
    crit = asg.ASG(len(tokens), num_replabels=R, use_garbage=garbage).cuda()
    rs = np.random.RandomState(30 + R)
    with torch.no_grad():
        crit.transitions.copy_(torch.from_numpy(0.1 * rs.randn(crit.N + 1, crit.N).astype(np.float32)))
    counter = ErrorCounter(tokens, tokens, "_")
    table = [[counter.symbol_ids[c] for c in t] for t in tokens]
    for T in frame_counts():
        B = 3
        # (no label twice in a row: the alignment below spells a target with its own labels, without replabels)
        rows = [[int(v) for v in (rs.permutation(len(tokens)).tolist() * T)[:n]] for n in (T // 4, 2, T // 5)]
        targets = [torch.tensor(r) for r in rows]
        filler = crit.garbage_idx if garbage else None
        frames = alignment(rs, [[v + R for v in r] for r in rows], T, -1)
        for b in range(B):  # frames between the labels: garbage, or the label before them
            for t in range(T):
                if frames[b, t] < 0:
                    frames[b, t] = filler if filler is not None else (frames[b, t - 1] if t else rows[b][0] + R)
        for kind in ("noise", "peaked"):
            x = emissions(rs, kind, frames, crit.N)
            hyp = [t.tolist() for t in crit.viterbi(x.cuda())]
            want = module_routes(crit, x, targets, counter, expected(hyp, rows, table, table, counter.symbol_ids["_"]))
            if kind == "peaked":
                assert 0 < want[0] <= 4 * FLIPS * B, want


@pytest.mark.parametrize("blank,ngram", [("optional", 0), ("none", 1), ("forced", 0), ("optional", 2)])
def test_transducer_module_errors(blank, ngram):
    """single graphemes as tokens: the tables of both sides are the same"""
    from gtn_applications_amd import ErrorCounter
    from gtn_applications_amd.criterions import transducer as TR

    toks = ["a", "b", "_", "c"]
    crit = TR.Transducer(toks, {t: i for i, t in enumerate(toks)}, ngram=ngram, blank=blank, allow_repeats=True).cuda()
    rs = np.random.RandomState(40 + ngram)
    if ngram:
        with torch.no_grad():
            crit.transition_params.copy_(torch.from_numpy(0.1 * rs.randn(crit.transition_params.numel()).astype(np.float32)))
    C = len(toks) + int(blank != "none")
    counter = ErrorCounter(toks, toks, "_")
    table = [[counter.symbol_ids[c] for c in t] for t in toks]
    for T in frame_counts():
        rows = [[int(v) for v in (rs.permutation(len(toks)).tolist() * T)[:n]] for n in (T // 4, 3, T // 6)]
        targets = [torch.tensor(r) for r in rows]
        frames = alignment(rs, rows, T, C - 1 if blank != "none" else -1)
        for b in range(len(rows)):
            for t in range(T):
                if frames[b, t] < 0:
                    frames[b, t] = frames[b, t - 1] if t else rows[b][0]
        for kind in ("noise", "peaked"):
            x = emissions(rs, kind, frames, C)
            hyp = [t.tolist() for t in crit.viterbi(x.cuda())]
            want = module_routes(crit, x, targets, counter, expected(hyp, rows, table, table, counter.symbol_ids["_"]))
            if kind == "peaked" and blank != "forced":  # (a flipped frame can make the forced graph reject the row)
                assert 0 < want[0] < want[2], want


def test_transducer_with_word_pieces():
    """predictions are word pieces that begin with the separator, targets are graphemes (train.py:80: tokens_to_text
    for the predictions, to_text for the targets): a table for the hypotheses, identity for the references"""
    from gtn_applications_amd import ErrorCounter
    from gtn_applications_amd.criterions import transducer as TR

    graphemes = ["_", "a", "b", "c", "d"]
    g2i = {g: i for i, g in enumerate(graphemes)}
    pieces = ["_", "a", "b", "c", "d", "_a", "_b", "_ab", "_cab", "ab", "_dab", "ba"]
    crit = TR.Transducer(pieces, g2i, ngram=0, blank="optional", allow_repeats=True).cuda()
    hyp_table = [[g2i[c] for c in p] for p in pieces]
    counter = ErrorCounter(hyp_symbols=hyp_table, wordsep=g2i["_"])
    same = ErrorCounter.for_preprocessor(type("Pre", (), dict(tokens=pieces, graphemes=graphemes, lexicon=None, wordsep="_")))
    C = len(pieces) + 1
    rs = np.random.RandomState(50)
    K = _mods()[0].lib.wfl_decode_chunk_frames()
    for T in (K + 1, 2 * K + 1):
        piece_rows = [rs.randint(5, len(pieces), size=n).tolist() for n in (T // 4, 2, T // 8)]
        rows = [[g for p in r for g in hyp_table[p]] for r in piece_rows]  # the targets: the pieces' graphemes
        targets = [torch.tensor(r) for r in rows]
        for kind in ("noise", "peaked"):
            x = emissions(rs, kind, alignment(rs, piece_rows, T, C - 1), C)
            hyp = [t.tolist() for t in crit.viterbi(x.cuda())]
            want = module_routes(crit, x, targets, counter, expected(hyp, rows, hyp_table, None, g2i["_"]))
            assert same(crit.viterbi(x), targets) == want == crit.errors(x.cuda(), targets, same)
            if kind == "peaked":
                assert 0 < want[0] < want[2] and 0 < want[1] <= want[3], want


def test_errors_and_viterbi_alternate():
    """both go through the decode's launch and its per-device buffers: either order, the same results"""
    from gtn_applications_amd import ErrorCounter
    from gtn_applications_amd.criterions import ctc

    rs = np.random.RandomState(60)
    C = 6
    crit = ctc.CTC(blank=C - 1, use_pt=False)
    counter = ErrorCounter(wordsep=0)
    xa = torch.from_numpy(rs.randn(5, 150, C).astype(np.float32)).cuda()
    xb = torch.from_numpy(rs.randn(2, 70, C).astype(np.float32)).cuda()
    ta = [rs.randint(0, C - 1, size=n).tolist() for n in (40, 0, 7, 66, 20)]
    tb = [rs.randint(0, C - 1, size=n).tolist() for n in (9, 30)]
    va, vb = [t.tolist() for t in crit.viterbi(xa)], [t.tolist() for t in crit.viterbi(xb)]
    ea, eb = crit.errors(xa, ta, counter), crit.errors(xb, tb, counter)
    assert ea == counter(va, ta) and eb == counter(vb, tb)
    kept = crit.viterbi(xa)
    for _ in range(2):
        assert crit.errors(xa, ta, counter) == ea
        assert [t.tolist() for t in crit.viterbi(xb)] == vb
        assert crit.errors(xb, tb, counter) == eb
        assert [t.tolist() for t in crit.viterbi(xa)] == va
    assert [t.tolist() for t in kept] == va  # (what viterbi() returned is not the operators' buffer)
