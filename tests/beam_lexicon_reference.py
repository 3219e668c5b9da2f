"""The CTC prefix beam search with a lexicon and a word-level n-gram LM (include/wfl.h: wfl_ctc_beam_search_lexicon;
DESIGN.md section 20) restated in plain Python, as tests/beam_lm_reference.py restates the search with a token LM:
float64, tuples for prefixes, one utterance at a time.  Nothing here uses gtn_applications_amd.lexicon or its packed
trie: the lexicon is a dict from spelling tuple to word id, the position inside a word is the tuple of labels since the
last word end, checked against the set of the spellings' proper prefixes, and the LM is beam_lm_reference.ArpaLM over
word ids (word v is label v, the blank is V) or None."""
import math

from beam_lm_reference import EOS
from beam_reference import NEG, candidates, clean, lae, row_lse


def proper_prefixes(lexicon):
    """every proper prefix of a spelling, the empty one included: the positions a hypothesis may stand at"""
    return {s[:k] for s in lexicon for k in range(len(s))}


def is_prefix_free(lexicon):
    return not (set(lexicon) & proper_prefixes(lexicon))


def segment(lexicon, labels):
    """(word ids, the labels since the last word end) of a label sequence, None if it leaves the lexicon"""
    inside, words, part = proper_prefixes(lexicon), [], ()
    for c in labels:
        part += (c,)
        if part in lexicon:
            words.append(lexicon[part])
            part = ()
        elif part not in inside:
            return None
    return words, part


def beam_search(x, blank, W, K, nbest, lexicon, lm, alpha, omega, beta, score_eos, normalize=False):
    """beam_reference.beam_search with the additions of section 20.  lexicon: {spelling tuple: word id}, prefix-free;
    lm: an ArpaLM over word ids or None.  Returns (hyps, margin, merges) alike; the margin also covers the ranks after
    the final drop and </s>."""
    inside = proper_prefixes(lexicon)
    beam = [((), 0.0, NEG, (), lm.start if lm else None)]  # (prefix, pb, pnb, labels since the last word, LM history)
    margin, merges, norm = math.inf, 0, 0.0
    for raw in x:
        row = clean(raw)
        norm += row_lse(row)
        cand = candidates(row, blank, K)  # (by acoustic score alone)
        pos = lambda c: next((p for p, (cc, _) in enumerate(cand) if cc == c), None)
        n = len(beam)
        tot = [lae(pb, pnb) for _, pb, pnb, _, _ in beam]
        stay_pb = [row[blank] + tot[i] for i in range(n)]
        stay_pnb = [NEG] * n
        last_pos = [None] * n
        for i, (pre, pb, pnb, _, _) in enumerate(beam):
            if pre:
                last_pos[i] = pos(pre[-1])
                if last_pos[i] is not None:
                    stay_pnb[i] = row[pre[-1]] + pnb

        def extension(i, c):
            """(e, labels since the last word, next history) of i + c; e = -inf: it does not exist"""
            pre, pb, _, part, hist = beam[i]
            e = row[c] + (pb if pre and pre[-1] == c else tot[i])
            if e == NEG:
                return NEG, None, None
            part = part + (c,)
            if part in lexicon:  # the label completes a word
                l, nxt = lm.step(hist, lexicon[part]) if lm else (0.0, None)
                if l == NEG:
                    return NEG, None, None
                return e + ((alpha * l + omega) + beta), (), nxt
            if part in inside:
                return e + beta, part, hist
            return NEG, None, None

        merged = [[False] * len(cand) for _ in range(n)]
        for j, pj in enumerate(h[0] for h in beam):
            if last_pos[j] is None:
                continue
            for i, pi in enumerate(h[0] for h in beam):
                if len(pi) + 1 == len(pj) and pi == pj[:-1]:
                    stay_pnb[j] = lae(stay_pnb[j], extension(i, pj[-1])[0])
                    merged[i][last_pos[j]] = True
                    merges += 1
                    break
        entries = [(lae(stay_pb[i], stay_pnb[i]), i, beam[i][0], stay_pb[i], stay_pnb[i], beam[i][3], beam[i][4])
                   for i in range(n)]
        for i in range(n):
            for p, (c, _) in enumerate(cand):
                if c != blank and not merged[i][p]:
                    e, part, nxt = extension(i, c)
                    entries.append((e, n + i * len(cand) + p, beam[i][0] + (c,), NEG, e, part, nxt))
        entries = [e for e in entries if e[0] != NEG]
        entries.sort(key=lambda e: (-e[0], e[1]))
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [e[2:] for e in entries[:W]]
        if not beam:
            break
    final = []
    for r, (pre, pb, pnb, part, hist) in enumerate(beam):
        if part:
            continue  # (it ends inside a word)
        s = lae(pb, pnb)
        if score_eos and lm:
            l, _ = lm.step(hist, EOS)
            if l == NEG:
                continue
            s += alpha * l
        final.append((s, r, pre))
    final.sort(key=lambda e: (-e[0], e[1]))
    for r in range(min(nbest, len(final) - 1)):
        margin = min(margin, final[r][0] - final[r + 1][0])
    hyps = [(pre, s - norm if normalize else s) for s, _, pre in final[:nbest]]
    hyps += [((), NEG)] * (nbest - len(hyps))
    return hyps, margin, merges


def random_lexicon(rs, C, blank, V, max_len, sep=None):
    """{spelling: word id} of V different seeded random words of 1 .. max_len labels (never the blank, never `sep`),
    each followed by the separator class `sep` if there is one -- prefix-free then by construction; without one, words
    are drawn until the set is prefix-free, from the start again where short words have left no room for V of them"""
    letters = [c for c in range(C) if c != blank and c != sep]
    for _ in range(1000):
        lexicon = {}
        for _ in range(50 * V):
            s = tuple(letters[rs.randint(len(letters))] for _ in range(1 + rs.randint(max_len)))
            s += () if sep is None else (sep,)
            if s not in lexicon and is_prefix_free({**lexicon, s: 0}):
                lexicon[s] = len(lexicon)
            if len(lexicon) == V:
                return lexicon
    raise AssertionError("not enough different words at this size")
