"""The Transducer prefix beam search of include/wfl.h (wfl_transducer_beam_search) restated in
plain Python: float64, lists and tuples only (prefixes are compared as tuples, nothing is hashed), one utterance at a
time.  It is the expectation of the Transducer beam search tests and nothing else; the rules are the header's, in the
header's order.

beam_search() also reports what a comparison needs to know about the utterance: the smallest selection margin it met --
kept against first dropped entry in every frame, and between consecutive ranks of the result up to the first one not
returned -- and the number of merged extensions."""
import itertools
import math

from beam_reference import NEG, candidates, clean, lae, row_lse


def weight(Wt, p, c):
    """w(p, c): the weight into class c behind frame label p (None: from the start): Wt[0][c] / Wt[1 + c][p] as a Python
    float, a NaN counts as -inf; 0 without a matrix"""
    if Wt is None:
        return 0.0
    w = float(Wt[0][c] if p is None else Wt[1 + c][p])
    return NEG if w != w else w


def beam_search(x, Wt, blank, forced, W, K, nbest, norm=None):
    """x: the [T, C] scores of one utterance, Wt: the [(C+1), C] transitions or None (rows of floats; a NaN counts as
    -inf in both).  Returns (hyps, margin, merges): hyps = nbest pairs (token tuple, score), the score minus `norm` if
    given; ranks beyond the result are ((), -inf)."""
    beam = [((), 0.0, NEG)]  # (prefix, pb, pnb), ranked
    margin, merges = math.inf, 0
    for t, raw in enumerate(x):
        row = clean(raw)
        cand = candidates(row, blank, K)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        beta = None if t == 0 else blank  # the state behind pb: the start in frame 0, the blank from frame 1 on
        n = len(beam)

        def extension(i, c):  # rule 4
            pre, pb, pnb = beam[i]
            m = pb + weight(Wt, beta, c)
            if not forced and pre and pre[-1] != c:
                m = lae(m, pnb + weight(Wt, pre[-1], c))
            return row[c] + m

        # rule 3: the stay entries
        spb, spnb = [NEG] * n, [NEG] * n
        for i, (pre, pb, pnb) in enumerate(beam):
            m = pb + weight(Wt, beta, blank)
            if pre:
                m = lae(m, pnb + weight(Wt, pre[-1], blank))
            spb[i] = row[blank] + m
            if pre and pre[-1] in pos:
                spnb[i] = (row[pre[-1]] + pnb) + weight(Wt, pre[-1], pre[-1])
        no_extension = forced and t == 0
        # an extension whose prefix is in the beam merges into that hypothesis' stay entry (its parent is determined)
        merged = [[False] * len(cand) for _ in range(n)]
        if not no_extension:
            for j, (pj, _, _) in enumerate(beam):
                if not pj or pj[-1] not in pos:
                    continue
                for i, (pi, _, _) in enumerate(beam):
                    if len(pi) + 1 == len(pj) and pi == pj[:-1]:
                        spnb[j] = lae(spnb[j], extension(i, pj[-1]))
                        merged[i][pos[pj[-1]]] = True
                        merges += 1
                        break
        # (tot', entry index, prefix, pb', pnb'): the entry index is the tie order -- stays by rank, then new entries by
        # (parent rank, candidate position)
        entries = [(lae(spb[i], spnb[i]), i, beam[i][0], spb[i], spnb[i]) for i in range(n)]
        if not no_extension:
            for i in range(n):
                pre = beam[i][0]
                for p, (c, _) in enumerate(cand):
                    if c != blank and not merged[i][p]:
                        e = extension(i, c)
                        entries.append((e, n + i * len(cand) + p, pre + (c,), NEG, e))
        entries = [e for e in entries if e[0] > NEG]
        entries.sort(key=lambda e: (-e[0], e[1]))
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [(pre, pb, pnb) for _, _, pre, pb, pnb in entries[:W]]
        if not beam:
            break
    if forced:  # rule 6: a path ends in the blank
        final = sorted(((pre, pb, r) for r, (pre, pb, _) in enumerate(beam) if pb > NEG), key=lambda e: (-e[1], e[2]))
        final = [(pre, s) for pre, s, _ in final]
    else:  # rule 5
        final = [(pre, lae(pb, pnb)) for pre, pb, pnb in beam]
    for r in range(min(nbest, len(final) - 1)):
        margin = min(margin, final[r][1] - final[r + 1][1])
    hyps = [(pre, s - norm if norm is not None else s) for pre, s in final[:nbest]]
    hyps += [((), NEG)] * (nbest - len(hyps))
    return hyps, margin, merges


def brute_force(x, Wt, blank, forced):
    """[(token tuple, log mass)] of every token sequence with an alignment, by enumerating all C^T frame paths (emissions
    plus transitions), keeping those the token graph accepts and grouping them by the sequence they spell, best first
    (ties: the sequence that sorts first).  Optional blank without repeats: every path, a token begins where the frame
    label changes to it.  Forced blank: a path starts and ends in the blank and a token follows the blank only."""
    rows = [clean(r) for r in x]
    C = len(rows[0]) if rows else 0
    mass = {}
    for path in itertools.product(range(C), repeat=len(rows)):
        if forced:
            if path and (path[0] != blank or path[-1] != blank):
                continue
            if any(c != blank and p != blank and p != c for p, c in zip(path, path[1:])):
                continue
        s, last, seq = 0.0, None, ()
        for t, c in enumerate(path):
            s += rows[t][c] + weight(Wt, last, c)
            if c != blank and c != last:
                seq += (c,)
            last = c
        if s > NEG:
            mass[seq] = lae(mass.get(seq, NEG), s)
    return sorted(mass.items(), key=lambda e: (-e[1], e[0]))


def normaliser(x, Wt):
    """the float64 normaliser of rule 7: with transitions the log of the summed mass of all C^T frame paths, by the forward
    recursion; without them the sum of the rows' log-sum-exps"""
    rows = [clean(r) for r in x]
    if Wt is None:
        return math.fsum(row_lse(r) for r in rows)
    C = len(rows[0])
    alpha = [rows[0][c] + weight(Wt, None, c) for c in range(C)]
    for row in rows[1:]:
        nxt = []
        for c in range(C):
            acc = NEG
            for j in range(C):
                acc = lae(acc, alpha[j] + weight(Wt, j, c))
            nxt.append(acc + row[c])
        alpha = nxt
    total = NEG
    for a in alpha:
        total = lae(total, a)
    return total
