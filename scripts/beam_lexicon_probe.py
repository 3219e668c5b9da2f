"""Per-call time of CTC.beam_search with a lexicon and a word-level n-gram LM beside the same search with a token-level LM,
at the benchmark's decode shape (B=128, T=1000, C=100), on a GPU.

    python scripts/beam_lexicon_probe.py                  beam widths 1, 16, 64 at 32 classes per frame, both inputs
    python scripts/beam_lexicon_probe.py --config 16,32 --input noise --calls 3 --warmup 1 --rounds 1
        one configuration only: the target of a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/beam_lexicon_probe.py --config ...
        (scripts/kstats.py prints the averages; the lexicon call's beam launch is beam_search_kernel<NT, wfl::BeamLex>)

Lexicon: `--words` seeded random words of 1 to 4 of the 98 letters, each ending in the separator class 98 (the blank is
99).  Word LM: a seeded random trigram over the words in the manner of scripts/beam_lm_probe.py -- every unigram,
`--keep` of the bigrams, and of the trigrams whose parts are in the file -- loaded through
NGramLM.from_arpa(path, words, blank=len(words)).  lm_weight 0.8, word_bonus 0.6, length_bonus 0.3, </s> scored.
Inputs: white noise (scripts/beam_probe.py's), and emissions peaked on an alignment that spells 30 lexicon words.  The
token-LM call is scripts/beam_lm_probe.py's (its trigram over the 99 tokens, weight 0.8, bonus 0.5).

The two calls alternate in one process -- token LM, lexicon, token LM, lexicon, ... -- so that clocks and neighbours
drift under both alike; a call ends on the host with its results, so the host clock around it is its time.  Reported
per call form: the median over all timed calls, and the spread (min, max); for the lexicon call also the number of
utterances that decode to at least one word."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gtn_applications_amd.criterions.ctc import CTC  # noqa: E402
from gtn_applications_amd.lexicon import Lexicon  # noqa: E402
from gtn_applications_amd.lm import NGramLM  # noqa: E402
from scripts.beam_lm_probe import random_trigram  # noqa: E402
from scripts.beam_probe import inputs  # noqa: E402


def random_lexicon(C, blank, sep, V, seed):
    rs = np.random.RandomState(seed)
    letters = [c for c in range(C) if c not in (blank, sep)]
    spellings = set()
    while len(spellings) < V:
        spellings.add(tuple(letters[i] for i in rs.randint(len(letters), size=1 + rs.randint(4))) + (sep,))
    return Lexicon(sorted(spellings), C, blank)


def random_word_trigram(V, keep, seed):
    """NGramLM over V word ids: every unigram, each bigram with probability `keep`, each trigram whose history and suffix
    are in the file with probability `keep`; log10 weights in [-3, -0.1], back-offs in [-1, 0]"""
    rs = np.random.RandomState(seed)
    names = [f"w{v}" for v in range(V)]
    words = names + ["</s>"]
    levels = [[("<s>",)] + [(w,) for w in words]]
    follow = {}  # history word -> the words that follow it in a bigram
    pairs = [(h, w) for h in ["<s>"] + names for w in np.array(words)[rs.rand(len(words)) < keep]]
    for h, w in pairs:
        follow.setdefault(h, []).append(w)
    levels.append(pairs)
    levels.append([(h, m, w) for h, m in pairs if m != "</s>" for w in follow.get(m, []) if rs.rand() < keep])
    lines = ["\\data\\"] + [f"ngram {n + 1}={len(level)}" for n, level in enumerate(levels)] + [""]
    for n, level in enumerate(levels):
        lines.append(f"\\{n + 1}-grams:")
        for g in level:
            bo = f"\t{-rs.rand():.6f}" if n < 2 and g[-1] != "</s>" else ""
            lines.append(f"{-0.1 - 2.9 * rs.rand():.6f}\t{' '.join(g)}{bo}")
        lines.append("")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe_words.arpa")
        with open(path, "w") as f:
            f.write("\n".join(lines + ["\\end\\", ""]))
        return NGramLM.from_arpa(path, names, V)


def spelled(B, T, C, blank, lex, seed):
    """emissions peaked on an alignment of 30 lexicon words per utterance: every label on a run of frames of its own,
    blank frames between the runs, +8 on white noise"""
    rs = np.random.RandomState(seed)
    x = rs.randn(B, T, C).astype(np.float32)
    for b in range(B):
        labels = [c for v in rs.randint(lex.num_words, size=30) for c in lex.spellings[v]]
        cuts = np.sort(rs.choice(np.arange(1, T), size=2 * len(labels), replace=False))
        frames = np.full(T, blank)
        for i, lab in enumerate(labels):
            frames[cuts[2 * i]:cuts[2 * i + 1]] = lab
        x[b, np.arange(T), frames] += 8.0
    return torch.from_numpy(x).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--C", type=int, default=100)
    ap.add_argument("--configs", default="1,32 16,32 64,32", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="both", choices=["both", "lexicon", "lm"], help="which call form (for a kernel trace)")
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--keep", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=5, help="timed calls of each form per round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "beam_lexicon_probe needs a GPU"
    blank, sep = a.C - 1, a.C - 2
    crit = CTC(blank=blank, use_pt=False)
    lex = random_lexicon(a.C, blank, sep, a.words, seed=2)
    word_lm = random_word_trigram(a.words, a.keep, seed=3)
    token_lm = random_trigram(a.C, blank, 0.05, seed=1)
    for pack in (lex, word_lm, token_lm):
        pack.on_device("cuda")
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    data = {"noise": inputs(a.B, a.T, a.C, blank)["noise"], "peaked": spelled(a.B, a.T, a.C, blank, lex, seed=4)}
    data = {k: v for k, v in data.items() if a.input in ("both", k)}
    print(f"B={a.B} T={a.T} C={a.C} blank={blank}; lexicon: {lex.num_words} words, {lex.num_nodes} nodes, {lex.num_arcs} arcs; "
          f"word LM order {word_lm.order}: {word_lm.num_states} states, {word_lm.num_arcs} arcs; token LM: "
          f"{token_lm.num_states} states, {token_lm.num_arcs} arcs; {a.warmup} warm-up + {a.rounds} x {a.calls} alternating "
          f"timed calls of each form; ms per call: median (min .. max)")
    for name, x in data.items():
        for W, K in configs:
            forms = {"lm": lambda: crit.beam_search(x, beam_size=W, classes_per_frame=K, lm=token_lm, lm_weight=0.8,
                                                    length_bonus=0.5),
                     "lexicon": lambda: crit.beam_search(x, beam_size=W, classes_per_frame=K, lexicon=lex, word_bonus=0.6,
                                                         lm=word_lm, lm_weight=0.8, length_bonus=0.3)}
            forms = {k: f for k, f in forms.items() if a.only in ("both", k)}
            results = {k: f() for k, f in forms.items()}
            for _ in range(a.warmup):
                for f in forms.values():
                    f()
            ms = {k: [] for k in forms}
            for _ in range(a.rounds * a.calls):
                for k, f in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            line = f"{name:7s} W={W:2d} K={K:2d}  " + "   ".join(
                f"{k:7s} {statistics.median(v):8.3f} ({min(v):8.3f} .. {max(v):8.3f})" for k, v in ms.items())
            if "lexicon" in forms:
                line += f"   (words in {sum(len(p) > 0 for p in results['lexicon'])} of {a.B})"
            if len(forms) == 2:
                line += f"   lexicon / lm {statistics.median(ms['lexicon']) / statistics.median(ms['lm']):5.2f}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
