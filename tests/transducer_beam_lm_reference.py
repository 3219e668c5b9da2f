"""The Transducer prefix beam search with a token-level n-gram LM and a length bonus (include/wfl.h:
wfl_transducer_beam_search_lm) restated in plain Python, as tests/transducer_beam_reference.py
restates the Transducer search and tests/beam_lm_reference.py the CTC search with an LM: float64, tuples for prefixes,
one utterance at a time.  Nothing here uses gtn_applications_amd.lm or its packed acceptor: the LM is
beam_lm_reference.ArpaLM over class labels, walked by the textbook back-off rule.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after the topology's drop and </s> up to
the first one not returned -- and the number of merged extensions."""
import math

from beam_lm_reference import EOS
from beam_reference import NEG, candidates, clean, lae
from transducer_beam_reference import weight


def beam_search(x, Wt, blank, forced, W, K, nbest, lm, alpha, beta, score_eos, logz=None, on_frame=None):
    """transducer_beam_reference.beam_search with the additions of section 28.  lm: an ArpaLM over the classes.  Returns
    (hyps, margin, merges): hyps = nbest pairs (token tuple, score), the score minus logz if given; ranks beyond what is
    left after the last frame are ((), -inf).  on_frame(t, beam, cand, extension, merged, entries): called in every
    frame with the ranked beam [(prefix, pb, pnb, history)], the candidates, the extension function, the merged flags
    and the sorted live entries -- for a test that has to know a situation occurred."""
    beam = [((), 0.0, NEG, lm.start)]  # (prefix, pb, pnb, LM history), ranked
    margin, merges = math.inf, 0
    for t, raw in enumerate(x):
        row = clean(raw)
        cand = candidates(row, blank, K)  # (by emission score alone)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        brow = None if t == 0 else blank  # the state behind pb: the start in frame 0, the blank from frame 1 on
        n = len(beam)
        no_extension = forced and t == 0

        def extension(i, c):
            """(e, next history) of i + c: rule 4's mass with the LM's term; e = -inf: it does not exist"""
            pre, pb, pnb, hist = beam[i]
            if no_extension:
                return NEG, None
            m = pb + weight(Wt, brow, c)
            if not forced and pre and pre[-1] != c:
                m = lae(m, pnb + weight(Wt, pre[-1], c))
            ac = row[c] + m
            if ac == NEG:
                return NEG, None  # (not looked up)
            l, nxt = lm.step(hist, c)
            if l == NEG:
                return NEG, None
            return ac + (alpha * l + beta), nxt

        # rule 3: the stays add no term and keep their state
        spb, spnb = [NEG] * n, [NEG] * n
        for i, (pre, pb, pnb, _) in enumerate(beam):
            m = pb + weight(Wt, brow, blank)
            if pre:
                m = lae(m, pnb + weight(Wt, pre[-1], blank))
            spb[i] = row[blank] + m
            if pre and pre[-1] in pos:
                spnb[i] = (row[pre[-1]] + pnb) + weight(Wt, pre[-1], pre[-1])
        # an extension whose prefix is in the beam merges into that hypothesis' stay entry, with the same term
        merged = [[False] * len(cand) for _ in range(n)]
        if not no_extension:
            for j, pj in enumerate(h[0] for h in beam):
                if not pj or pj[-1] not in pos:
                    continue
                for i, pi in enumerate(h[0] for h in beam):
                    if len(pi) + 1 == len(pj) and pi == pj[:-1]:
                        spnb[j] = lae(spnb[j], extension(i, pj[-1])[0])
                        merged[i][pos[pj[-1]]] = True
                        merges += 1
                        break
        entries = [(lae(spb[i], spnb[i]), i, beam[i][0], spb[i], spnb[i], beam[i][3]) for i in range(n)]
        if not no_extension:
            for i in range(n):
                for p, (c, _) in enumerate(cand):
                    if c != blank and not merged[i][p]:
                        e, nxt = extension(i, c)
                        entries.append((e, n + i * len(cand) + p, beam[i][0] + (c,), NEG, e, nxt))
        entries = [e for e in entries if e[0] > NEG]
        entries.sort(key=lambda e: (-e[0], e[1]))
        if on_frame is not None:
            on_frame(t, beam, cand, extension, merged, entries)
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [e[2:] for e in entries[:W]]
        if not beam:
            break
    # after the last frame: the topology's score (forced: pb, -inf dropped), </s> on top, the ranks again
    final = []
    for r, (pre, pb, pnb, hist) in enumerate(beam):
        s = pb if forced else lae(pb, pnb)
        if s == NEG:
            continue
        if score_eos:
            l, _ = lm.step(hist, EOS)
            if l == NEG:
                continue
            s += alpha * l
        final.append((s, r, pre))
    final.sort(key=lambda e: (-e[0], e[1]))
    for r in range(min(nbest, len(final) - 1)):
        margin = min(margin, final[r][0] - final[r + 1][0])
    hyps = [(pre, s - logz if logz is not None else s) for s, _, pre in final[:nbest]]
    hyps += [((), NEG)] * (nbest - len(hyps))
    return hyps, margin, merges


def brute_force(x, Wt, blank, forced, lm, alpha, beta, score_eos):
    """[(token tuple, score)]: transducer_beam_reference.brute_force's mass of every token sequence over all C^T frame
    paths the token graph accepts, re-scored with alpha LM(tokens) + beta #tokens and the </s> term; a sequence the LM
    cannot follow is left out; best first (ties: the sequence that sorts first)"""
    from transducer_beam_reference import brute_force as masses

    out = []
    for pre, mass in masses(x, Wt, blank, forced):
        if mass == NEG:
            continue
        hist, total, dead = lm.start, 0.0, False
        for c in list(pre) + ([EOS] if score_eos else []):
            l, hist = lm.step(hist, c)
            if l == NEG:
                dead = True
                break
            total += l
        if dead:
            continue
        out.append((pre, mass + alpha * total + beta * len(pre)))
    return sorted(out, key=lambda e: (-e[1], e[0]))
