"""The ASG prefix beam search of include/wfl.h (wfl_asg_beam_search) restated in plain Python:
float64, lists and tuples only (prefixes are compared as tuples, nothing is hashed), one utterance at a time.  It is the
expectation of the ASG beam search tests and nothing else; the rules are the header's, in the header's order.

beam_search() also reports what a comparison needs to know about the utterance: the smallest selection margin it met --
kept against first dropped entry in every frame, and between consecutive ranks of the final beam up to the first one not
returned -- and the number of merged extensions."""
import math

from beam_reference import NEG, clean, lae


def candidates(row, K):
    """[(class, score)]: the K classes of highest emission score of a frame (already clean), ties to the lower class, in
    that order; transitions do not enter, nothing is appended"""
    return [(c, row[c]) for c in sorted(range(len(row)), key=lambda c: (-row[c], c))[:K]]


def transition(Wt, last, c):
    """the weight into class c behind `last` (None: from the start): Wt[0][c] / Wt[1 + c][last], as a Python float, a NaN
    counts as -inf (cleaned where it is read: the matrix of a wide model is never walked as a whole)"""
    w = float(Wt[0][c] if last is None else Wt[1 + c][last])
    return NEG if w != w else w


def beam_search(x, Wt, W, K, nbest, logz=None):
    """x: the [T, C] scores of one utterance, Wt: the [(C+1), C] transitions (rows of floats; a NaN counts as -inf in
    both).  Returns (hyps, margin, merges): hyps = nbest pairs (class tuple, score), the score minus logz if given;
    ranks beyond the final beam are ((), -inf)."""
    beam = [((), 0.0)]  # (prefix, p), ranked
    margin, merges = math.inf, 0
    for raw in x:
        row = clean(raw)
        cand = candidates(row, K)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        n = len(beam)
        # the stay entries: only where the last label is a candidate; the empty prefix has none
        stay = [NEG] * n
        last_pos = [None] * n
        for i, (pre, p) in enumerate(beam):
            if pre and pre[-1] in pos:
                last_pos[i] = pos[pre[-1]]
                stay[i] = (row[pre[-1]] + transition(Wt, pre[-1], pre[-1])) + p

        def extension(i, c):
            pre, p = beam[i]
            return (row[c] + transition(Wt, pre[-1] if pre else None, c)) + p

        # an extension whose prefix is in the beam merges into that hypothesis' stay entry (its parent is determined)
        merged = [[False] * len(cand) for _ in range(n)]
        for j, (pj, _) in enumerate(beam):
            if last_pos[j] is None:
                continue
            for i, (pi, _) in enumerate(beam):
                if len(pi) + 1 == len(pj) and pi == pj[:-1]:
                    stay[j] = lae(stay[j], extension(i, pj[-1]))
                    merged[i][last_pos[j]] = True
                    merges += 1
                    break
        # (p', entry index, prefix): the entry index is the tie order -- stays by rank, then new entries by (parent
        # rank, candidate position)
        entries = [(stay[i], i, beam[i][0]) for i in range(n)]
        for i in range(n):
            pre = beam[i][0]
            for p, (c, _) in enumerate(cand):
                if not (pre and pre[-1] == c) and not merged[i][p]:
                    entries.append((extension(i, c), n + i * len(cand) + p, pre + (c,)))
        entries = [e for e in entries if e[0] > NEG]  # (-inf dropped: an extension over a -inf transition among them)
        entries.sort(key=lambda e: (-e[0], e[1]))
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [(pre, p) for p, _, pre in entries[:W]]
        if not beam:
            break
    for r in range(min(nbest, len(beam) - 1)):
        margin = min(margin, beam[r][1] - beam[r + 1][1])
    hyps = [(pre, p - logz if logz is not None else p) for pre, p in beam[:nbest]]
    hyps += [((), NEG)] * (nbest - len(hyps))
    return hyps, margin, merges


def brute_force(x, Wt):
    """[(class tuple, log mass)] of every class sequence without equal neighbours, by enumerating all C^T frame paths
    (emissions plus transitions) and grouping them by their collapsed sequence, best first (ties: the sequence that
    sorts first)"""
    rows = [clean(r) for r in x]
    C = len(rows[0]) if rows else 0
    paths = [((), None, 0.0)]  # (collapsed classes, last frame class, score)
    for row in rows:
        paths = [(pre if c == last else pre + (c,), c, s + (row[c] + transition(Wt, last, c)))
                 for pre, last, s in paths for c in range(C)]
    mass = {}
    for pre, _, s in paths:
        mass[pre] = lae(mass.get(pre, NEG), s)
    return sorted(mass.items(), key=lambda e: (-e[1], e[0]))


def denominator(x, Wt):
    """log of the summed mass of all C^T frame paths, by the forward recursion in float64 (asg.py:114)"""
    rows = [clean(r) for r in x]
    C = len(rows[0])
    alpha = [rows[0][c] + transition(Wt, None, c) for c in range(C)]
    for row in rows[1:]:
        nxt = []
        for c in range(C):
            acc = NEG
            for j in range(C):
                acc = lae(acc, alpha[j] + transition(Wt, j, c))
            nxt.append(acc + row[c])
        alpha = nxt
    total = NEG
    for a in alpha:
        total = lae(total, a)
    return total


def unpack(seq, drop, num_replabels):
    """what ASG.viterbi does to a collapsed path (asg.py:35-49, 228-234): `drop` removed, a label v >= R becomes v - R, a
    replabel right behind a label repeats it r + 1 times, any other replabel is dropped"""
    out, prev = [], -1
    for v in seq:
        if drop is not None and v == drop:
            continue
        if v >= num_replabels:
            out.append(v - num_replabels)
            prev = v
        elif prev != -1:
            out.extend([prev - num_replabels] * (v + 1))
            prev = -1
    return out
