"""The CTC prefix beam search with an n-gram LM and a length bonus (include/wfl.h: wfl_ctc_beam_search_lm; DESIGN.md
section 18) restated in plain Python, as tests/beam_reference.py restates the search without them: float64, tuples for
prefixes, one utterance at a time -- and the LM as a dict of grams read from ARPA text by the few lines below, walked by
the textbook back-off rule.  Nothing here uses gtn_applications_amd.lm: the loader, its packed acceptor and the kernel's
lookups are what this is the expectation of.

ArpaLM.step(history, label) works on class labels: history is the tuple of the last labels (with "<s>" in front where
the sentence start is still in reach), label a class index or EOS."""
import math

from beam_reference import NEG, candidates, clean, lae, row_lse

EOS, BOS = "</s>", "<s>"
LN10 = math.log(10.0)


class ArpaLM:
    """grams: {tuple of labels: (ln p, ln back-off)} over class indices, BOS and EOS; order: the file's"""

    def __init__(self, text, tokens, blank):
        label = {tok: (i if i < blank else i + 1) for i, tok in enumerate(tokens)}
        label[BOS], label[EOS] = BOS, EOS
        self.grams, self.order, n = {}, 0, 0
        for line in text.split("\n"):
            line = line.strip()
            if line.endswith("-grams:"):
                n = int(line[1:line.index("-")])
                self.order = max(self.order, n)  # (the file's order, even where its last section is empty)
            elif n and line and not line.startswith("\\"):
                f = line.split()
                if all(w in label for w in f[1:n + 1]):
                    bo = float(f[n + 1]) * LN10 if len(f) > n + 1 else 0.0
                    self.grams[tuple(label[w] for w in f[1:n + 1])] = (float(f[0]) * LN10, bo)
        self.start = (BOS,) if (BOS,) in self.grams and self.order > 1 else ()

    def state(self, gram):
        """the longest suffix of the gram, at most order - 1 long, that is a gram itself: the history that stays"""
        for k in range(min(len(gram), self.order - 1), 0, -1):
            if gram[len(gram) - k:] in self.grams:
                return gram[len(gram) - k:]
        return ()

    def step(self, hist, c):
        """(ln weight, next history) of label c after hist; (-inf, None) if not even the unigram exists"""
        acc = 0.0
        while True:
            g = hist + (c,)
            if g in self.grams:
                return acc + self.grams[g][0], self.state(g)
            if not hist:
                return NEG, None
            acc += self.grams[hist][1]
            hist = hist[1:]

    def score(self, labels, eos=True):
        total, hist = 0.0, self.start
        for c in list(labels) + ([EOS] if eos else []):
            w, hist = self.step(hist, c)
            if hist is None:
                return NEG
            total += w
        return total


def beam_search(x, blank, W, K, nbest, lm, alpha, beta, score_eos, normalize=False):
    """beam_reference.beam_search with the additions of section 18.  Returns (hyps, margin, merges) alike; the margin
    also covers the ranks after </s>."""
    beam = [((), 0.0, NEG, lm.start)]  # (prefix, pb, pnb, LM history), ranked
    margin, merges, norm = math.inf, 0, 0.0
    for raw in x:
        row = clean(raw)
        norm += row_lse(row)
        cand = candidates(row, blank, K)  # (by acoustic score alone)
        pos = lambda c: next((p for p, (cc, _) in enumerate(cand) if cc == c), None)
        n = len(beam)
        tot = [lae(pb, pnb) for _, pb, pnb, _ in beam]
        stay_pb = [row[blank] + tot[i] for i in range(n)]
        stay_pnb = [NEG] * n
        last_pos = [None] * n
        for i, (pre, pb, pnb, _) in enumerate(beam):
            if pre:
                last_pos[i] = pos(pre[-1])
                if last_pos[i] is not None:
                    stay_pnb[i] = row[pre[-1]] + pnb

        def extension(i, c):
            """(e, next history) of i + c; e = -inf: it does not exist"""
            pre, pb, _, hist = beam[i]
            e = row[c] + (pb if pre and pre[-1] == c else tot[i])
            if e == NEG:
                return NEG, None
            l, nxt = lm.step(hist, c)
            return (NEG, None) if l == NEG else (e + (alpha * l + beta), nxt)

        merged = [[False] * len(cand) for _ in range(n)]
        for j, (pj, _, _, _) in enumerate(beam):
            if last_pos[j] is None:
                continue
            for i, (pi, _, _, _) in enumerate(beam):
                if len(pi) + 1 == len(pj) and pi == pj[:-1]:
                    stay_pnb[j] = lae(stay_pnb[j], extension(i, pj[-1])[0])
                    merged[i][last_pos[j]] = True
                    merges += 1
                    break
        entries = [(lae(stay_pb[i], stay_pnb[i]), i, beam[i][0], stay_pb[i], stay_pnb[i], beam[i][3]) for i in range(n)]
        for i in range(n):
            for p, (c, _) in enumerate(cand):
                if c != blank and not merged[i][p]:
                    e, nxt = extension(i, c)
                    entries.append((e, n + i * len(cand) + p, beam[i][0] + (c,), NEG, e, nxt))
        entries = [e for e in entries if e[0] != NEG]
        entries.sort(key=lambda e: (-e[0], e[1]))
        if len(entries) > W:
            margin = min(margin, entries[W - 1][0] - entries[W][0])
        beam = [(pre, pb, pnb, hist) for _, _, pre, pb, pnb, hist in entries[:W]]
        if not beam:
            break
    final = []
    for r, (pre, pb, pnb, hist) in enumerate(beam):
        s = lae(pb, pnb)
        if score_eos:
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


def random_arpa(rs, tokens, order, keep, eos=True):
    """ARPA text of a seeded random LM over `tokens`: every unigram, and each higher gram whose
    history and suffix are in the file with probability `keep`; log10 weights in [-3, -0.1], back-offs in [-1, 0]."""
    words = list(tokens) + ([EOS] if eos else [])
    levels = [[(BOS,)] + [(w,) for w in words]]
    for n in range(2, order + 1):
        prev, level = set(levels[-1]), []
        for h in levels[-1]:
            if h[-1] == EOS:
                continue
            for w in words:
                g = h + (w,)
                if g[1:] in prev and rs.rand() < keep:
                    level.append(g)
        levels.append(level)
    out = ["\\data\\"] + [f"ngram {n + 1}={len(level)}" for n, level in enumerate(levels)] + [""]
    for n, level in enumerate(levels):
        out.append(f"\\{n + 1}-grams:")
        for g in level:
            line = f"{-0.1 - 2.9 * rs.rand():.6f}\t{' '.join(g)}"
            if n + 1 < len(levels) and g[-1] != EOS:
                line += f"\t{-rs.rand():.6f}"
            out.append(line)
        out.append("")
    return "\n".join(out + ["\\end\\", ""])
