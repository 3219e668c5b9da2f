"""The CTC prefix beam search of include/wfl.h (wfl_ctc_beam_search) restated in plain Python: float64, lists and tuples
only (prefixes are compared as tuples, nothing is hashed), one utterance at a time.  It is the expectation of the beam
search tests and nothing else; the rules are the header's, in the header's order.  search() is the frame loop itself, which
the restatements of the other two-mass searches (LM, lexicons, look-ahead, the Transducer's) hand their rules to.

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


def weight(Wt, p, c):
    """w(p, c): the weight into class c behind frame label p (None: from the start): Wt[0][c] / Wt[1 + c][p] as a Python
    float, a NaN counts as -inf; 0 without a matrix"""
    if Wt is None:
        return 0.0
    w = float(Wt[0][c] if p is None else Wt[1 + c][p])
    return NEG if w != w else w


def search(x, blank, W, K, nbest, start=(), extend=None, finish=None, Wt=None, forced=False, normalize=False, logz=None,
           on_frame=None):
    """The two-mass frame loop of every prefix search here but the ASG ones (asg_beam_reference.search) and the one that
    merges by spelling (transducer_merged_beam_reference): CTC is Wt None and forced False -- every transition weight 0,
    both masses into an extension unless it repeats the last label.  A search hands in its rules:

    start: the state of the empty prefix, a tuple (LM history, labels of the current word, ...);
    extend(state, prefix, c) -> (term, next state) or None: what label c behind `prefix` adds to the extension's mass,
        as ONE float -- the loop forms `mass + term` once, the rule keeps its own parenthesisation --, None: the extension
        does not exist; it is asked only where the mass is finite; without one there is no state and no term;
    finish(state, s) -> s' or None: what a rank's score gets after the last frame, None: the rank is dropped.

    The beam holds flat tuples (prefix, pb, pnb, *state), ranked -- one container per hypothesis beside its prefix: a
    state kept as a tuple of its own costs the collector more than the loop.  on_frame(t, beam, cand, extension, merged,
    entries), if given, is called in every frame with the beam, the candidates, extension(i, c) -> (e, *next state)
    (e = -inf: it does not exist), the merged flags and the sorted live entries (tot', entry index, prefix, pb', pnb',
    *state).
    Returns (hyps, margin, merges): hyps = nbest pairs (label tuple, score) -- minus logz if given, else minus the rows'
    log-sum-exps if `normalize` --, ((), -inf) beyond what is left after the last frame.

    Every restatement but those three runs THIS loop: a test that compares two of them with each other (the search
    without transitions is the CTC search, a look-ahead of zeros is the search without one) shows that their rules
    agree, not that the loop is right.  The loop's independent check is the brute-force enumerations of the
    tests/test_*_abi.py files (brute_force* here and in the sibling modules, which never come through here): none of
    those pins is redundant."""
    dead = (NEG,) + (None,) * len(start)
    beam = [((), 0.0, NEG) + tuple(start)]
    margin, merges, norm = math.inf, 0, 0.0
    for t, raw in enumerate(x):
        row = clean(raw)
        if normalize:
            norm += row_lse(row)
        cand = candidates(row, blank, K)  # (by emission score alone)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        brow = None if t == 0 else blank  # the state behind pb: the start in frame 0, the blank from frame 1 on
        n = len(beam)
        no_extension = forced and t == 0
        # without transitions every weight is 0 and both masses go into a stay or a new label together (the empty
        # prefix has pnb = -inf): their sum is formed once per hypothesis, as CTC's rules state it
        tot = [lae(h[1], h[2]) for h in beam] if Wt is None else None

        def extension(i, c):
            """(e, *next state) of i + c: pb from behind the blank, pnb too unless forced or c repeats the last label"""
            h = beam[i]
            pre = h[0]
            if no_extension:
                return dead
            if Wt is None:
                m = h[1] if forced or (pre and pre[-1] == c) else tot[i]
            else:
                m = h[1] + weight(Wt, brow, c)
                if not forced and pre and pre[-1] != c:
                    m = lae(m, h[2] + weight(Wt, pre[-1], c))
            ac = row[c] + m
            if extend is None:
                return (ac,)
            if ac == NEG:
                return dead  # (the rule is not asked)
            to = extend(h[3:], pre, c)
            return dead if to is None else (ac + to[0],) + to[1]

        # the stays add no term and keep their state
        spb, spnb = [NEG] * n, [NEG] * n
        for i, h in enumerate(beam):
            pre, pb, pnb = h[0], h[1], h[2]
            if Wt is None:
                spb[i] = row[blank] + tot[i]
                if pre and pre[-1] in pos:
                    spnb[i] = row[pre[-1]] + pnb
                continue
            m = pb + weight(Wt, brow, blank)
            if pre:
                m = lae(m, pnb + weight(Wt, pre[-1], blank))
            spb[i] = row[blank] + m
            if pre and pre[-1] in pos:
                spnb[i] = (row[pre[-1]] + pnb) + weight(Wt, pre[-1], pre[-1])
        # an extension whose prefix is in the beam merges into that hypothesis' stay entry (its parent is determined)
        merged = [[False] * len(cand) for _ in range(n)]
        if not no_extension:
            pres = [h[0] for h in beam]
            for j, pj in enumerate(pres):
                if not pj or pj[-1] not in pos:
                    continue
                head = pj[:-1]
                for i, pi in enumerate(pres):
                    if len(pi) == len(head) and pi == head:
                        spnb[j] = lae(spnb[j], extension(i, pj[-1])[0])
                        merged[i][pos[pj[-1]]] = True
                        merges += 1
                        break
        # (tot', entry index, prefix, pb', pnb', *state), -inf dropped: the entry index is the tie order -- stays by rank,
        # then new entries by (parent rank, candidate position)
        entries = [(lae(spb[i], spnb[i]), i, beam[i][0], spb[i], spnb[i]) + beam[i][3:] for i in range(n)]
        entries = [e for e in entries if e[0] > NEG]
        if not no_extension:
            for i in range(n):
                pre, flags, at = beam[i][0], merged[i], n + i * len(cand)
                for p, (c, _) in enumerate(cand):
                    if c != blank and not flags[p]:
                        e = extension(i, c)
                        if e[0] > NEG:
                            entries.append((e[0], at + p, pre + (c,), NEG) + e)
        entries.sort(key=lambda e: -e[0])  # (they were made in index order, and the sort is stable: ties by index)
        if on_frame is not None:
            on_frame(t, beam, cand, extension, merged, entries)
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [e[2:] for e in entries[:W]]
        if not beam:
            break
    # after the last frame: the topology's score (forced: a path ends in the blank; -inf dropped), the search's terms,
    # the ranks again
    final = []
    for r, h in enumerate(beam):
        s = h[1] if forced else lae(h[1], h[2])
        if s == NEG:
            continue
        if finish is not None:
            s = finish(h[3:], s)
            if s is None:
                continue
        final.append((s, r, h[0]))
    final.sort(key=lambda e: (-e[0], e[1]))
    for r in range(min(nbest, len(final) - 1)):
        margin = min(margin, final[r][0] - final[r + 1][0])
    sub = logz if logz is not None else norm if normalize else None
    hyps = [(pre, s if sub is None else s - sub) for s, _, pre in final[:nbest]]
    hyps += [((), NEG)] * (nbest - len(hyps))
    return hyps, margin, merges


def beam_search(x, blank, W, K, nbest, normalize=False):
    """x: the [T_b, C] scores of one utterance (rows of floats).  Returns (hyps, margin, merges): hyps = nbest pairs
    (label tuple, score), ranks beyond the final beam are ((), -inf)."""
    return search(x, blank, W, K, nbest, normalize=normalize)


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
