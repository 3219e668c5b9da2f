"""The Transducer prefix beam search of include/wfl.h (wfl_transducer_beam_search) restated in
plain Python: float64, lists and tuples only (prefixes are compared as tuples, nothing is hashed), one utterance at a
time.  It is the expectation of the Transducer beam search tests and nothing else; the rules are the header's, in the
header's order.

beam_search() also reports what a comparison needs to know about the utterance: the smallest selection margin it met --
kept against first dropped entry in every frame, and between consecutive ranks of the result up to the first one not
returned -- and the number of merged extensions."""
import itertools
import math

from beam_reference import NEG, clean, lae, row_lse, search, weight  # noqa: F401 (weight: its users import it from here)


def beam_search(x, Wt, blank, forced, W, K, nbest, norm=None):
    """x: the [T, C] scores of one utterance, Wt: the [(C+1), C] transitions or None (rows of floats; a NaN counts as
    -inf in both).  Returns (hyps, margin, merges): hyps = nbest pairs (token tuple, score), the score minus `norm` if
    given; ranks beyond the result are ((), -inf).  The rules are beam_reference.search's own -- rule 3 its stays,
    rule 4 its extensions, rules 5 and 6 its scores after the last frame --, nothing is added."""
    return search(x, blank, W, K, nbest, Wt=Wt, forced=forced, logz=norm)


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
