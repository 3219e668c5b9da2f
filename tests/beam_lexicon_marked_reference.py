"""The CTC and Transducer prefix beam searches with a START-MARKED lexicon and a word-level n-gram LM (include/wfl.h:
wfl_ctc_beam_search_lexicon_marked, wfl_transducer_beam_search_lexicon_marked) restated in plain
Python from the rules: float64, tuples for prefixes, one utterance at a time.  Nothing here uses
gtn_applications_amd.lexicon or its packed trie: the lexicon is a dict from spelling tuple to word id (several spellings
may name one word, a spelling may be a proper prefix of another), the position of a hypothesis is the tuple of labels
since its current word began (empty: the empty prefix alone), and the LM is beam_lm_reference.ArpaLM over word ids (word
v is label v, the blank is V) or None.

One function serves both criteria: Wt None and forced False are CTC's rules (every transition weight 0, both masses into
an extension unless it repeats the last label), which is rule 7 of section 25.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after the last frame's terms up to the
first one not returned -- and the number of merged extensions."""
import math

from beam_lm_reference import EOS
from beam_reference import NEG, candidates, clean, lae, row_lse
from transducer_beam_reference import weight


def starts(lexicon):
    """R: the classes that begin a word"""
    return {s[0] for s in lexicon}


def is_start_marked(lexicon):
    """the one condition of rule 1: no class that begins a word occurs inside one"""
    return not (starts(lexicon) & {c for s in lexicon for c in s[1:]})


def positions(lexicon):
    """every non-empty prefix of a spelling, the spellings included: where a hypothesis inside or at the end of a word
    may stand"""
    return {s[:k] for s in lexicon for k in range(1, len(s) + 1)}


def segment(lexicon, labels):
    """(the COMPLETED words, the labels of the current word) of a label sequence, None if it leaves the lexicon: a word
    is completed by the label that begins the next"""
    R, at, words, part = starts(lexicon), positions(lexicon), [], ()
    for c in labels:
        if c in R:
            if part:
                if part not in lexicon:
                    return None
                words.append(lexicon[part])
            part = (c,)
        else:
            part += (c,)
            if len(part) == 1 or part not in at:
                return None
    return words, part


def words_of(lexicon, labels):
    """the words of a label sequence by rule 5 -- the pending word counts if its spelling is complete --, None if the
    sequence leaves the lexicon or ends inside a word"""
    seg = segment(lexicon, labels)
    if seg is None or (seg[1] and seg[1] not in lexicon):
        return None
    return seg[0] + ([lexicon[seg[1]]] if seg[1] else [])


def beam_search(x, blank, W, K, nbest, lexicon, lm, alpha, omega, beta, score_eos, normalize=False, Wt=None, forced=False,
                logz=None):
    """x: the [T, C] scores of one utterance.  lexicon: {spelling tuple: word id}, start-marked; lm: an ArpaLM over word
    ids or None.  Returns (hyps, margin, merges): hyps = nbest pairs (label tuple, score) -- the score minus the rows'
    log-sum-exps if `normalize`, minus logz if given --; ranks beyond what is left after the last frame are ((), -inf)."""
    R, at = starts(lexicon), positions(lexicon)
    beam = [((), 0.0, NEG, (), lm.start if lm else None)]  # (prefix, pb, pnb, labels of the current word, LM history)
    margin, merges, norm = math.inf, 0, 0.0
    for t, raw in enumerate(x):
        row = clean(raw)
        norm += row_lse(row)
        cand = candidates(row, blank, K)  # (by acoustic score alone)
        pos = {c: p for p, (c, _) in enumerate(cand)}
        brow = None if t == 0 else blank  # the state behind pb: the start in frame 0, the blank from frame 1 on
        n = len(beam)
        no_extension = forced and t == 0

        def extension(i, c):
            """rule 3: (e, labels of the current word, next history) of i + c; e = -inf: it does not exist"""
            pre, pb, pnb, part, hist = beam[i]
            if no_extension:
                return NEG, None, None
            m = pb + weight(Wt, brow, c)
            if not forced and pre and pre[-1] != c:
                m = lae(m, pnb + weight(Wt, pre[-1], c))
            ac = row[c] + m
            if ac == NEG:
                return NEG, None, None
            if c not in R:  # inside a word: the arc of the current node
                if not part or part + (c,) not in at:
                    return NEG, None, None
                return ac + beta, part + (c,), hist
            if not part:  # the first word of the empty prefix
                return ac + beta, (c,), hist
            if part not in lexicon:  # a new word behind an unfinished one
                return NEG, None, None
            l, nxt = lm.step(hist, lexicon[part]) if lm else (0.0, None)
            if l == NEG:
                return NEG, None, None
            return ac + ((alpha * l + omega) + beta), (c,), nxt

        # the stays add no term and keep position and history
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
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [e[2:] for e in entries[:W]]
        if not beam:
            break
    # rule 5: the empty sequence as it is, a complete pending word's term, anything else dropped; </s>; the ranks again
    final = []
    for r, (pre, pb, pnb, part, hist) in enumerate(beam):
        s = pb if forced else lae(pb, pnb)
        if s == NEG:
            continue
        if part:
            if part not in lexicon:
                continue
            l, hist = lm.step(hist, lexicon[part]) if lm else (0.0, None)
            if l == NEG:
                continue
            s += alpha * l + omega
        if score_eos and lm:
            l, _ = lm.step(hist, EOS)
            if l == NEG:
                continue
            s += alpha * l
        final.append((s, r, pre))
    final.sort(key=lambda e: (-e[0], e[1]))
    for r in range(min(nbest, len(final) - 1)):
        margin = min(margin, final[r][0] - final[r + 1][0])
    sub = (norm if normalize else 0.0) if logz is None else logz
    hyps = [(pre, s - sub) for s, _, pre in final[:nbest]]
    hyps += [((), NEG)] * (nbest - len(hyps))
    return hyps, margin, merges


def brute_force(x, blank, lexicon, lm, alpha, omega, beta, score_eos, Wt=None, forced=False, ctc=False):
    """[(label tuple, score)] by rule 6: the mass of every label sequence over all C^T frame paths -- grouped by
    collapsed sequence (ctc: beam_reference.brute_force) or by the sequence the token graph spells
    (transducer_beam_reference.brute_force) --, those kept that segment under rule 1 and end at a terminal node (or are
    empty), re-scored with alpha LM(words) + omega #words + beta #labels and the </s> term; best first"""
    if ctc:
        from beam_reference import brute_force as ctc_masses

        masses = ctc_masses(x, blank)
    else:
        from transducer_beam_reference import brute_force as tok_masses

        masses = tok_masses(x, Wt, blank, forced)
    out = []
    for pre, mass in masses:
        words = words_of(lexicon, pre)
        if words is None or mass == NEG:
            continue
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


def random_lexicon(rs, C, blank, V, max_len, n_starts, two_spellings=False):
    """{spelling: word id} of seeded random words over C classes: the first n_starts classes that are not the blank begin
    words, the others continue them; 1 .. max_len labels; built so that some words are proper prefixes of others (every
    word's prefixes that begin with a start class are candidates); with two_spellings word 0 gets a second spelling"""
    classes = [c for c in range(C) if c != blank]
    R, inner = classes[:n_starts], classes[n_starts:]
    lexicon = {}
    for _ in range(100 * V):
        if len(lexicon) >= V:
            break
        s = (R[rs.randint(len(R))],) + tuple(inner[rs.randint(len(inner))] for _ in range(rs.randint(max_len))) if inner \
            else (R[rs.randint(len(R))],)
        for k in (len(s), 1 + rs.randint(len(s))):  # the word and one of its prefixes: not prefix-free
            if s[:k] not in lexicon and len(lexicon) < V:
                lexicon[s[:k]] = len(lexicon)
    assert len(lexicon) == V, "not enough different words at this size"
    if two_spellings:
        for _ in range(1000):
            s = (R[rs.randint(len(R))],) + tuple(inner[rs.randint(len(inner))] for _ in range(1 + rs.randint(max_len)))
            if s not in lexicon:
                lexicon[s] = 0
                break
    return lexicon
