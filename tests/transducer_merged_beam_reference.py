"""The Transducer prefix beam search that merges hypotheses by spelling (wfl_transducer_beam_search_merged of
include/wfl.h) restated in plain Python: float64, lists and tuples only (spellings and token
sequences are compared as tuples, nothing is hashed), one utterance at a time.  It is the expectation of the merged beam
search tests and nothing else; the rules are the header's, in the header's order.

merged_beam_search() also reports what a comparison needs to know about the utterance: the smallest selection margin it
met -- kept against first dropped entry in every frame, and between consecutive ranks of the merged result up to the
first one not returned --, the number of extensions that merged into a new entry, the number that merged into a stay,
and whether any frame had more entries than the beam holds (`pruned`)."""
import math

from beam_reference import NEG, candidates, clean, lae
from transducer_beam_reference import brute_force, weight


def spelt(spell, seq):
    """the graphemes a token sequence spells"""
    return tuple(g for c in seq for g in spell[c])


def merged_beam_search(x, Wt, blank, forced, spell, W, K, nbest, norm=None):
    """x: the [T, C] scores of one utterance, Wt: the [(C+1), C] transitions or None, spell: per class the sequence of
    its graphemes (the blank's: empty or None).  Returns (hyps, margin, new_merges, stay_merges, pruned): hyps = nbest
    triples (representative token tuple, spelling tuple, score), the score minus `norm` if given; ranks beyond the result
    are ((), (), -inf)."""
    spell = [tuple(s) if s is not None else () for s in spell]
    beam = [(((), None), 0.0, NEG, ())]  # ((S, l), pb, pnb, rho), ranked
    margin, new_merges, stay_merges, pruned = math.inf, 0, 0, False
    for t, raw in enumerate(x):
        row = clean(raw)
        cand = candidates(row, blank, K)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        beta = None if t == 0 else blank
        n = len(beam)

        def extension(i, c):  # section 22 rule 4, per hypothesis
            (_, l), pb, pnb, _ = beam[i]
            m = pb + weight(Wt, beta, c)
            if not forced and l is not None and l != c:
                m = lae(m, pnb + weight(Wt, l, c))
            return row[c] + m

        # section 22 rule 3: the stay entries
        spb, spnb = [NEG] * n, [NEG] * n
        for i, ((_, l), pb, pnb, _) in enumerate(beam):
            m = pb + weight(Wt, beta, blank)
            if l is not None:
                m = lae(m, pnb + weight(Wt, l, blank))
            spb[i] = row[blank] + m
            if l is not None and l in pos:
                spnb[i] = (row[l] + pnb) + weight(Wt, l, l)
        # rule 3: the extensions by key, parents in rank order
        identity = {beam[i][0]: i for i in range(n)}
        new = {}  # key -> [mass, entry index, rho]
        if not (forced and t == 0):
            for i in range(n):
                (S, _), _, _, rho = beam[i]
                for p, (c, _) in enumerate(cand):
                    if c == blank:
                        continue
                    e = extension(i, c)
                    key = (S + spell[c], c)
                    if key in identity:  # behind j's own stay term; j keeps its rho
                        j = identity[key]
                        spnb[j] = lae(spnb[j], e)
                        stay_merges += 1
                    elif key in new:
                        ent = new[key]
                        if e > NEG:
                            if ent[0] == NEG:  # every parent so far contributed -inf: rho comes from this one
                                ent[2] = rho + (c,)
                            ent[0] = lae(ent[0], e)
                        new_merges += 1
                    else:  # the place of its lowest-ranked parent, finite or not
                        new[key] = [e, n + i * len(cand) + p, rho + (c,)]
        entries = [(lae(spb[i], spnb[i]), i, beam[i][0], spb[i], spnb[i], beam[i][3]) for i in range(n)]
        entries += [(m, idx, key, NEG, m, rho) for key, (m, idx, rho) in new.items()]
        entries = [e for e in entries if e[0] > NEG]
        entries.sort(key=lambda e: (-e[0], e[1]))
        if len(entries) > W:
            pruned = True
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [(key, pb, pnb, rho) for _, _, key, pb, pnb, rho in entries[:W]]
        if not beam:
            break
    # rule 4: the score per hypothesis, merged by spelling in rank order, ranked again
    merged = {}
    for r, ((S, _), pb, pnb, rho) in enumerate(beam):
        s = pb if forced else lae(pb, pnb)
        if s == NEG:
            continue
        if S in merged:
            merged[S][0] = lae(merged[S][0], s)
        else:
            merged[S] = [s, r, rho]
    final = sorted(((rho, S, s, r) for S, (s, r, rho) in merged.items()), key=lambda e: (-e[2], e[3]))
    for r in range(min(nbest, len(final) - 1)):
        margin = min(margin, final[r][2] - final[r + 1][2])
    hyps = [(rho, S, s - norm if norm is not None else s) for rho, S, s, _ in final[:nbest]]
    hyps += [((), (), NEG)] * (nbest - len(hyps))
    return hyps, margin, new_merges, stay_merges, pruned


def brute_force_spellings(x, Wt, blank, forced, spell):
    """[(spelling tuple, log mass)]: transducer_beam_reference.brute_force grouped by spelling, best first (ties: the
    spelling that sorts first)"""
    spell = [tuple(s) if s is not None else () for s in spell]
    mass = {}
    for seq, m in brute_force(x, Wt, blank, forced):
        S = spelt(spell, seq)
        mass[S] = lae(mass.get(S, NEG), m)
    return sorted(mass.items(), key=lambda e: (-e[1], e[0]))
