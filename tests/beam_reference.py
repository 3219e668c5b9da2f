"""The CTC prefix beam search of include/wfl.h (wfl_ctc_beam_search) restated in plain Python: float64, lists and tuples
only (prefixes are compared as tuples, nothing is hashed), one utterance at a time.  It is the expectation of the beam
search tests and nothing else; the rules are the header's, in the header's order.

beam_search() also reports what a comparison needs to know about the utterance: the smallest selection margin it met --
kept against first dropped entry in every frame, and between consecutive ranks of the final beam up to the first one not
returned -- and the number of merged extensions."""
import math

NEG = -math.inf


def lae(a, b):
    """log(exp(a) + exp(b)), -inf the identity"""
    if a == NEG:
        return b
    if b == NEG:
        return a
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def clean(row):
    """the scores of a frame as Python floats, a NaN counts as -inf"""
    return [NEG if v != v else float(v) for v in row]


def candidates(row, blank, K):
    """[(class, score)]: the K best classes of a frame (already clean), ties to the lower class, in that order; the
    blank appended if it is not among them"""
    order = sorted(range(len(row)), key=lambda c: (-row[c], c))[:K]
    if blank not in order:
        order.append(blank)
    return [(c, row[c]) for c in order]


def row_lse(row):
    """log-sum-exp over all classes of a clean frame"""
    m = max(row)
    if m == NEG:
        return NEG
    return m + math.log(math.fsum(math.exp(v - m) for v in row))


def beam_search(x, blank, W, K, nbest, normalize=False):
    """x: the [T_b, C] scores of one utterance (rows of floats).  Returns (hyps, margin, merges): hyps = nbest pairs
    (label tuple, score), ranks beyond the final beam are ((), -inf)."""
    beam = [((), 0.0, NEG)]  # (prefix, pb, pnb), ranked
    margin, merges, norm = math.inf, 0, 0.0
    for raw in x:
        row = clean(raw)
        norm += row_lse(row)
        cand = candidates(row, blank, K)
        pos = lambda c: next((p for p, (cc, _) in enumerate(cand) if cc == c), None)
        s_blank = row[blank]
        n = len(beam)
        tot = [lae(pb, pnb) for _, pb, pnb in beam]
        stay_pb = [s_blank + tot[i] for i in range(n)]
        stay_pnb = [NEG] * n
        last_pos = [None] * n
        for i, (pre, pb, pnb) in enumerate(beam):
            if pre:
                last_pos[i] = pos(pre[-1])
                if last_pos[i] is not None:
                    stay_pnb[i] = row[pre[-1]] + pnb

        def extension(i, c):
            pre, pb, _ = beam[i]
            return row[c] + (pb if pre and pre[-1] == c else tot[i])

        # an extension whose prefix is in the beam merges into that hypothesis' stay entry (its parent is determined)
        merged = [[False] * len(cand) for _ in range(n)]
        for j, (pj, _, _) in enumerate(beam):
            if last_pos[j] is None:
                continue
            for i, (pi, _, _) in enumerate(beam):
                if len(pi) + 1 == len(pj) and pi == pj[:-1]:
                    stay_pnb[j] = lae(stay_pnb[j], extension(i, pj[-1]))
                    merged[i][last_pos[j]] = True
                    merges += 1
                    break
        # (tot', entry index, prefix, pb', pnb'): the entry index is the tie order -- stays by rank, then new entries by
        # (parent rank, candidate position)
        entries = [(lae(stay_pb[i], stay_pnb[i]), i, beam[i][0], stay_pb[i], stay_pnb[i]) for i in range(n)]
        for i in range(n):
            for p, (c, _) in enumerate(cand):
                if c != blank and not merged[i][p]:
                    e = extension(i, c)
                    entries.append((e, n + i * len(cand) + p, beam[i][0] + (c,), NEG, e))
        entries = [e for e in entries if e[0] != NEG]
        entries.sort(key=lambda e: (-e[0], e[1]))
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [(pre, pb, pnb) for _, _, pre, pb, pnb in entries[:W]]
        if not beam:
            break
    final = [(pre, lae(pb, pnb)) for pre, pb, pnb in beam]
    for r in range(min(nbest, len(final) - 1)):
        margin = min(margin, final[r][1] - final[r + 1][1])
    hyps = [(pre, s - norm if normalize else s) for pre, s in final[:nbest]]
    hyps += [((), NEG)] * (nbest - len(hyps))
    return hyps, margin, merges


def brute_force(x, blank):
    """[(label tuple, log mass)] of every label sequence, by enumerating all C^T alignments, best first (ties: the
    sequence that sorts first)"""
    rows = [clean(r) for r in x]
    C = len(rows[0]) if rows else 0
    seqs, mass = [], []
    paths = [((), -1, 0.0)]  # (collapsed labels, last frame label, score)
    for row in rows:
        paths = [(pre + (c,) if c != blank and c != last else pre, c, s + row[c]) for pre, last, s in paths for c in range(C)]
    for pre, _, s in paths:
        if pre in seqs:
            k = seqs.index(pre)
            mass[k] = lae(mass[k], s)
        else:
            seqs.append(pre)
            mass.append(s)
    return sorted(zip(seqs, mass), key=lambda e: (-e[1], e[0]))
