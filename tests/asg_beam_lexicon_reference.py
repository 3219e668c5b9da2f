"""The ASG prefix beam search with a lexicon and a word-level n-gram LM (include/wfl.h: wfl_asg_beam_search_lexicon;
DESIGN.md section 24) restated in plain Python, as tests/asg_beam_reference.py restates the ASG search and
tests/beam_lexicon_reference.py the CTC search with a lexicon: float64, tuples for prefixes, one utterance at a time.
Nothing here uses gtn_applications_amd.lexicon or its packed trie: the lexicon is a dict from RAW spelling tuple
(replabels packed in, never the garbage) to word id, the position inside a word is the tuple of non-garbage labels
since the last word end, checked against the set of the spellings' proper prefixes, and the LM is
beam_lm_reference.ArpaLM over word ids (word v is label v, the blank is V) or None.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after the final drop and </s> up to the
first one not returned -- and the number of merged extensions."""
import math

from asg_beam_reference import candidates, transition
from beam_lexicon_reference import is_prefix_free, proper_prefixes
from beam_lm_reference import EOS
from beam_reference import NEG, clean, lae


def segment(lexicon, garbage, labels):
    """(word ids, the non-garbage labels since the last word end) of a raw class sequence with the garbage transparent,
    None if it leaves the lexicon"""
    inside, words, part = proper_prefixes(lexicon), [], ()
    for c in labels:
        if c == garbage:
            continue
        part += (c,)
        if part in lexicon:
            words.append(lexicon[part])
            part = ()
        elif part not in inside:
            return None
    return words, part


def beam_search(x, Wt, W, K, nbest, lexicon, garbage, lm, alpha, omega, beta, score_eos, logz=None, on_frame=None):
    """asg_beam_reference.beam_search with the additions of section 24.  lexicon: {raw spelling tuple: word id},
    prefix-free; garbage: the transparent class or None; lm: an ArpaLM over word ids or None.  Returns (hyps, margin,
    merges): hyps = nbest pairs (raw class tuple, score), the score minus logz if given; ranks beyond what is left
    after the last frame are ((), -inf).  on_frame(t, beam, cand, extension, merged, entries): called in every frame
    with the ranked beam [(prefix, p, part, history)], the candidates, the extension function, the merged flags and
    the sorted entries -- for a test that has to know a situation occurred."""
    inside = proper_prefixes(lexicon)
    beam = [((), 0.0, (), lm.start if lm else None)]  # (prefix, p, labels since the last word, LM history), ranked
    margin, merges = math.inf, 0
    for t, raw in enumerate(x):
        row = clean(raw)
        cand = candidates(row, K)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        n = len(beam)
        # rule 4: the stays add nothing and keep node and state, for the garbage as for any other class
        stay = [NEG] * n
        last_pos = [None] * n
        for i, (pre, p, _, _) in enumerate(beam):
            if pre and pre[-1] in pos:
                last_pos[i] = pos[pre[-1]]
                stay[i] = (row[pre[-1]] + transition(Wt, pre[-1], pre[-1])) + p

        def extension(i, c):
            """rule 3: (e, labels since the last word, next history) of i + c; e = -inf: it does not exist"""
            pre, p, part, hist = beam[i]
            ac = (row[c] + transition(Wt, pre[-1] if pre else None, c)) + p
            if ac == NEG:
                return NEG, None, None
            if garbage is not None and c == garbage:
                return ac, part, hist
            part = part + (c,)
            if part in lexicon:  # the class completes a word
                l, nxt = lm.step(hist, lexicon[part]) if lm else (0.0, None)
                if l == NEG:
                    return NEG, None, None
                return ac + ((alpha * l + omega) + beta), (), nxt
            if part in inside:
                return ac + beta, part, hist
            return NEG, None, None

        merged = [[False] * len(cand) for _ in range(n)]
        for j, pj in enumerate(h[0] for h in beam):
            if last_pos[j] is None:
                continue
            for i, pi in enumerate(h[0] for h in beam):
                if len(pi) + 1 == len(pj) and pi == pj[:-1]:
                    stay[j] = lae(stay[j], extension(i, pj[-1])[0])
                    merged[i][last_pos[j]] = True
                    merges += 1
                    break
        entries = [(stay[i], i, beam[i][0], beam[i][2], beam[i][3]) for i in range(n)]
        for i in range(n):
            pre = beam[i][0]
            for p, (c, _) in enumerate(cand):
                if not (pre and pre[-1] == c) and not merged[i][p]:
                    e, part, nxt = extension(i, c)
                    entries.append((e, n + i * len(cand) + p, pre + (c,), part, nxt))
        entries = [e for e in entries if e[0] > NEG]
        entries.sort(key=lambda e: (-e[0], e[1]))
        if on_frame is not None:
            on_frame(t, beam, cand, extension, merged, entries)
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [(pre, p, part, hist) for p, _, pre, part, hist in entries[:W]]
        if not beam:
            break
    # rule 5: a rank inside a word is dropped, </s>, the ranks again
    final = []
    for r, (pre, p, part, hist) in enumerate(beam):
        if part:
            continue
        s = p
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


def brute_force(x, Wt, lexicon, garbage, lm, alpha, omega, beta, score_eos):
    """[(raw class tuple, score)] by rule 6: asg_beam_reference.brute_force's mass of every collapsed raw sequence over
    all C^T frame paths, those kept that walk the lexicon (garbage transparent) back to a word end, re-scored with
    alpha LM(words) + omega #words + beta #(non-garbage classes) and the </s> term; best first"""
    from asg_beam_reference import brute_force as masses

    out = []
    for pre, mass in masses(x, Wt):
        at = segment(lexicon, garbage, pre)
        if at is None or at[1] or mass == NEG:
            continue
        words = at[0]
        s = mass + omega * len(words) + beta * sum(1 for c in pre if c != garbage)
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


def raw_lexicon(words_tokens, num_replabels):
    """{raw spelling: word id} of words given as token index lists (separator included): rule 1, written out here
    rather than taken from the package -- a run of n equal tokens is groups of up to 1 + R: the token shifted by R,
    then, for a group of s >= 2, the replabel s - 2"""
    R, out = num_replabels, {}
    for v, toks in enumerate(words_tokens):
        s, k = [], 0
        while k < len(toks):
            n = 1
            while k + n < len(toks) and toks[k + n] == toks[k] and n < 1 + R:
                n += 1
            s.append(toks[k] + R)
            if n >= 2:
                s.append(n - 2)
            k += n
        out[tuple(s)] = v
    assert len(out) == len(words_tokens) and is_prefix_free(out)
    return out
