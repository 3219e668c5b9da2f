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


def search(x, Wt, W, K, nbest, start=(), extend=None, finish=None, logz=None, on_frame=None):
    """The single-mass frame loop of the ASG searches (this module's and asg_beam_lexicon_reference's), as
    beam_reference.search is the two-mass loop of the others, with the same three rules handed in:

    start: the state of the empty prefix, a tuple;
    extend(state, prefix, c) -> (term, next state) or None: what class c behind `prefix` adds, as ONE float the loop
        adds once, None: the extension does not exist; asked only where the mass is finite; without one no state, no term;
    finish(state, s) -> s' or None: what a rank's score gets after the last frame, None: the rank is dropped.

    The beam holds flat tuples (prefix, p, *state), ranked.  on_frame(t, beam, cand, extension, merged, entries), if
    given, sees in every frame the beam, the candidates, extension(i, c) -> (e, *next state) (e = -inf: it does not
    exist), the merged flags and the sorted live entries (p', entry index, prefix, *state).  Returns (hyps, margin,
    merges): hyps = nbest pairs (class tuple, score), the score minus logz if given; ((), -inf) beyond what is left.

    Both ASG restatements run THIS loop, so comparing them with each other shows that their rules agree, not that the
    loop is right: its independent check is brute_force below and asg_beam_lexicon_reference.brute_force (pinned in
    tests/test_asg_beam_abi.py and tests/test_asg_beam_lexicon_abi.py), which never come through here."""
    dead = (NEG,) + (None,) * len(start)
    beam = [((), 0.0) + tuple(start)]
    margin, merges = math.inf, 0
    for t, raw in enumerate(x):
        row = clean(raw)
        cand = candidates(row, K)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        n = len(beam)
        # the stay entries: only where the last label is a candidate; the empty prefix has none; they add no term and
        # keep their state
        stay = [NEG] * n
        last_pos = [None] * n
        for i, h in enumerate(beam):
            pre = h[0]
            if pre and pre[-1] in pos:
                last_pos[i] = pos[pre[-1]]
                stay[i] = (row[pre[-1]] + transition(Wt, pre[-1], pre[-1])) + h[1]

        def extension(i, c):
            """(e, *next state) of i + c"""
            h = beam[i]
            pre = h[0]
            ac = (row[c] + transition(Wt, pre[-1] if pre else None, c)) + h[1]
            if extend is None:
                return (ac,)
            if ac == NEG:
                return dead  # (the rule is not asked)
            to = extend(h[2:], pre, c)
            return dead if to is None else (ac + to[0],) + to[1]

        # an extension whose prefix is in the beam merges into that hypothesis' stay entry (its parent is determined)
        merged = [[False] * len(cand) for _ in range(n)]
        pres = [h[0] for h in beam]
        for j, pj in enumerate(pres):
            if last_pos[j] is None:
                continue
            head = pj[:-1]
            for i, pi in enumerate(pres):
                if len(pi) == len(head) and pi == head:
                    stay[j] = lae(stay[j], extension(i, pj[-1])[0])
                    merged[i][last_pos[j]] = True
                    merges += 1
                    break
        # (p', entry index, prefix, *state), -inf dropped: the entry index is the tie order -- stays by rank, then new
        # entries by (parent rank, candidate position)
        entries = [(stay[i], i, beam[i][0]) + beam[i][2:] for i in range(n) if stay[i] > NEG]
        for i in range(n):
            pre, flags, at = beam[i][0], merged[i], n + i * len(cand)
            last = pre[-1] if pre else None
            for p, (c, _) in enumerate(cand):
                if c != last and not flags[p]:
                    e = extension(i, c)
                    if e[0] > NEG:  # (-inf dropped: an extension over a -inf transition among them)
                        entries.append((e[0], at + p, pre + (c,)) + e[1:])
        entries.sort(key=lambda e: -e[0])  # (they were made in index order, and the sort is stable: ties by index)
        if on_frame is not None:
            on_frame(t, beam, cand, extension, merged, entries)
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [(e[2], e[0]) + e[3:] for e in entries[:W]]
        if not beam:
            break
    final = []
    for r, h in enumerate(beam):
        s = h[1] if finish is None else finish(h[2:], h[1])
        if s is not None:
            final.append((s, r, h[0]))
    final.sort(key=lambda e: (-e[0], e[1]))
    for r in range(min(nbest, len(final) - 1)):
        margin = min(margin, final[r][0] - final[r + 1][0])
    hyps = [(pre, s - logz if logz is not None else s) for s, _, pre in final[:nbest]]
    hyps += [((), NEG)] * (nbest - len(hyps))
    return hyps, margin, merges


def beam_search(x, Wt, W, K, nbest, logz=None):
    """x: the [T, C] scores of one utterance, Wt: the [(C+1), C] transitions (rows of floats; a NaN counts as -inf in
    both).  Returns (hyps, margin, merges): hyps = nbest pairs (class tuple, score), the score minus logz if given;
    ranks beyond the final beam are ((), -inf)."""
    return search(x, Wt, W, K, nbest, logz=logz)


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
