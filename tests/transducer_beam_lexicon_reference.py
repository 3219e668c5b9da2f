"""The Transducer prefix beam search with a lexicon and a word-level n-gram LM (include/wfl.h:
wfl_transducer_beam_search_lexicon) restated in plain Python, as tests/transducer_beam_reference.py
restates the Transducer search and tests/beam_lexicon_reference.py the CTC search with a lexicon: float64, tuples for
prefixes, one utterance at a time.  Nothing here uses gtn_applications_amd.lexicon or its packed trie: the lexicon is a
dict from token tuple to word id, the position inside a word is the tuple of tokens since the last word end, checked
against the set of the spellings' proper prefixes, and the LM is beam_lm_reference.ArpaLM over word ids (word v is label
v, the blank is V) or None.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after the final drop and </s> up to the
first one not returned -- and the number of merged extensions."""
import math

from beam_lexicon_reference import proper_prefixes, segment
from beam_lm_reference import EOS
from beam_reference import NEG, candidates, clean, lae
from transducer_beam_reference import weight


def beam_search(x, Wt, blank, forced, W, K, nbest, lexicon, lm, alpha, omega, beta, score_eos, logz=None, on_frame=None):
    """transducer_beam_reference.beam_search with the additions of section 25.  lexicon: {token tuple: word id},
    prefix-free; lm: an ArpaLM over word ids or None.  Returns (hyps, margin, merges): hyps = nbest pairs (token tuple,
    score), the score minus logz if given; ranks beyond what is left after the last frame are ((), -inf).
    on_frame(t, beam, cand, extension, merged, entries): called in every frame with the ranked beam [(prefix, pb, pnb,
    part, history)], the candidates, the extension function, the merged flags and the sorted live entries -- for a test
    that has to know a situation occurred."""
    inside = proper_prefixes(lexicon)
    beam = [((), 0.0, NEG, (), lm.start if lm else None)]  # (prefix, pb, pnb, tokens since the last word, LM history)
    margin, merges = math.inf, 0
    for t, raw in enumerate(x):
        row = clean(raw)
        cand = candidates(row, blank, K)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        brow = None if t == 0 else blank  # the state behind pb: the start in frame 0, the blank from frame 1 on
        n = len(beam)
        no_extension = forced and t == 0

        def extension(i, c):
            """rule 2: (e, tokens since the last word, next history) of i + c; e = -inf: it does not exist"""
            pre, pb, pnb, part, hist = beam[i]
            if no_extension:
                return NEG, None, None
            m = pb + weight(Wt, brow, c)
            if not forced and pre and pre[-1] != c:
                m = lae(m, pnb + weight(Wt, pre[-1], c))
            ac = row[c] + m
            if ac == NEG:
                return NEG, None, None
            part = part + (c,)
            if part in lexicon:  # the token completes a word
                l, nxt = lm.step(hist, lexicon[part]) if lm else (0.0, None)
                if l == NEG:
                    return NEG, None, None
                return ac + ((alpha * l + omega) + beta), (), nxt
            if part in inside:
                return ac + beta, part, hist
            return NEG, None, None

        # rule 3: the stays add no term and keep node and state
        spb, spnb = [NEG] * n, [NEG] * n
        for i, (pre, pb, pnb, _, _) in enumerate(beam):
            m = pb + weight(Wt, brow, blank)
            if pre:
                m = lae(m, pnb + weight(Wt, pre[-1], blank))
            spb[i] = row[blank] + m
            if pre and pre[-1] in pos:
                spnb[i] = (row[pre[-1]] + pnb) + weight(Wt, pre[-1], pre[-1])
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
        entries = [(lae(spb[i], spnb[i]), i, beam[i][0], spb[i], spnb[i], beam[i][3], beam[i][4]) for i in range(n)]
        if not no_extension:
            for i in range(n):
                for p, (c, _) in enumerate(cand):
                    if c != blank and not merged[i][p]:
                        e, part, nxt = extension(i, c)
                        entries.append((e, n + i * len(cand) + p, beam[i][0] + (c,), NEG, e, part, nxt))
        entries = [e for e in entries if e[0] > NEG]
        entries.sort(key=lambda e: (-e[0], e[1]))
        if on_frame is not None:
            on_frame(t, beam, cand, extension, merged, entries)
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [e[2:] for e in entries[:W]]
        if not beam:
            break
    # rule 5: a rank inside a word is dropped, the topology's score, </s>, the ranks again
    final = []
    for r, (pre, pb, pnb, part, hist) in enumerate(beam):
        if part:
            continue
        s = pb if forced else lae(pb, pnb)
        if s == NEG:
            continue
        if score_eos and lm:
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


def brute_force(x, Wt, blank, forced, lexicon, lm, alpha, omega, beta, score_eos):
    """[(token tuple, score)] by rule 6: transducer_beam_reference.brute_force's mass of every token sequence over all
    C^T frame paths the token graph accepts, those kept that segment into lexicon words, re-scored with alpha LM(words) +
    omega #words + beta #tokens and the </s> term; best first"""
    from transducer_beam_reference import brute_force as masses

    out = []
    for pre, mass in masses(x, Wt, blank, forced):
        at = segment(lexicon, pre)
        if at is None or at[1] or mass == NEG:
            continue
        words = at[0]
        s = mass + omega * len(words) + beta * len(pre)
        if lm:
            hist, total, dead = lm.start, 0.0, False
            for v in words + ([EOS] if score_eos else []):
                l, hist = lm.step(hist, v)
                if l == NEG:
                    dead = True
                    break
                total += l
            if dead:
                continue
            s += alpha * total
        out.append((pre, s))
    return sorted(out, key=lambda e: (-e[1], e[0]))
