"""The CTC prefix beam search with an n-gram LM and a length bonus (include/wfl.h: wfl_ctc_beam_search_lm; DESIGN.md
section 18) restated in plain Python, as tests/beam_reference.py restates the search without them: float64, tuples for
prefixes, one utterance at a time -- and the LM as a dict of grams read from ARPA text by the few lines below, walked by
the textbook back-off rule.  Nothing here uses gtn_applications_amd.lm: the loader, its packed acceptor and the kernel's
lookups are what this is the expectation of.

ArpaLM.step(history, label) works on class labels: history is the tuple of the last labels (with "<s>" in front where
the sentence start is still in reach), label a class index or EOS."""
import math

from beam_reference import NEG, search

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


def token_lm_rules(lm, alpha, beta, score_eos):
    """(start, extend, finish) of a search with an LM over the labels: the state is (LM history,); a label adds
    alpha l + beta, a label the LM cannot follow does not exist; </s> adds alpha l after the last frame"""

    def extend(state, pre, c):
        l, nxt = lm.step(state[0], c)
        return None if l == NEG else (alpha * l + beta, (nxt,))

    def finish(state, s):
        if score_eos:
            l, _ = lm.step(state[0], EOS)
            if l == NEG:
                return None
            s += alpha * l
        return s

    return (lm.start,), extend, finish


def beam_search(x, blank, W, K, nbest, lm, alpha, beta, score_eos, normalize=False):
    """beam_reference.beam_search with the additions of section 18.  Returns (hyps, margin, merges) alike; the margin
    also covers the ranks after </s>."""
    return search(x, blank, W, K, nbest, *token_lm_rules(lm, alpha, beta, score_eos), normalize=normalize)


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
