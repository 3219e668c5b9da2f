"""Per-call time of CTC.beam_search with a START-MARKED lexicon beside the same search with the
end-marked lexicon of the same vocabulary and beside the token-LM search, at the benchmark's decode shape (B=128,
T=1000, C=100), on a GPU.  scripts/beam_lexicon_probe.py's protocol with a third call form.

    python scripts/beam_lexicon_marked_probe.py                     beam widths 1, 16, 64 at 32 classes per frame, both inputs
    python scripts/beam_lexicon_marked_probe.py --only existing     the token-LM and end-marked calls alone: what a parent
                                                                    checkout can run too (it needs nothing of section 26)

Vocabulary: beam_lexicon_probe's `--words` seeded random words of 1 to 4 of the 98 letters.  End-marked: each followed
by the separator class 98.  Start-marked: the separator moved to the front of the word -- the same number of words,
nodes and labels per word; class 98 begins every word and occurs in none.  Word LM, constants and the token-LM call:
beam_lexicon_probe's.  Inputs: the same white noise for every form; and emissions peaked on an alignment that spells the
same 30 words per utterance in the form's own convention, on the same frames ("w |" against "| w": the peaks of a word
move by one run).

The forms alternate in one process -- token LM, end-marked, start-marked, token LM, ... -- so that clocks and
neighbours drift under all alike; a call ends on the host with its results, so the host clock around it is its time.
Reported per form: the median over all timed calls (15 by default) and the spread (min, max); for the lexicon forms
also the number of utterances that decode to at least one word."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gtn_applications_amd.criterions.ctc import CTC  # noqa: E402
from gtn_applications_amd.lexicon import Lexicon  # noqa: E402
from scripts.beam_lexicon_probe import random_lexicon, random_word_trigram, spelled  # noqa: E402
from scripts.beam_lm_probe import random_trigram  # noqa: E402
from scripts.beam_probe import inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--C", type=int, default=100)
    ap.add_argument("--configs", default="1,32 16,32 64,32", help="beam,classes pairs")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="all", choices=["all", "existing", "marked"])
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--keep", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=5, help="timed calls of each form per round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "beam_lexicon_marked_probe needs a GPU"
    blank, sep = a.C - 1, a.C - 2
    crit = CTC(blank=blank, use_pt=False)
    end = random_lexicon(a.C, blank, sep, a.words, seed=2)
    word_lm = random_word_trigram(a.words, a.keep, seed=3)
    token_lm = random_trigram(a.C, blank, 0.05, seed=1)
    lexicons = {"end": end}
    if a.only != "existing":  # (word v of both lexicons is the same word: the word LM serves both)
        lexicons["start"] = Lexicon([(sep,) + tuple(s[:-1]) for s in end.spellings], a.C, blank, boundary="start")
    for pack in list(lexicons.values()) + [word_lm, token_lm]:
        pack.on_device("cuda")
    configs = [tuple(int(v) for v in c.split(",")) for c in a.configs.split()]
    noise = inputs(a.B, a.T, a.C, blank)["noise"]
    data = {"noise": {k: noise for k in ("lm", "end", "start")}}
    data["peaked"] = {k: spelled(a.B, a.T, a.C, blank, lex, seed=4) for k, lex in lexicons.items()}
    data["peaked"]["lm"] = data["peaked"]["end"]
    data = {k: v for k, v in data.items() if a.input in ("both", k)}
    print(f"B={a.B} T={a.T} C={a.C} blank={blank}; " +
          "; ".join(f"{k}-marked lexicon: {lex.num_words} words, {lex.num_nodes} nodes, {lex.num_arcs} arcs"
                    for k, lex in lexicons.items()) +
          f"; word LM order {word_lm.order}: {word_lm.num_states} states, {word_lm.num_arcs} arcs; token LM: "
          f"{token_lm.num_states} states, {token_lm.num_arcs} arcs; {a.warmup} warm-up + {a.rounds} x {a.calls} alternating "
          f"timed calls of each form; ms per call: median (min .. max)")
    for name, xs in data.items():
        for W, K in configs:
            def lexicon_call(kind):
                return lambda: crit.beam_search(xs[kind], beam_size=W, classes_per_frame=K, lexicon=lexicons[kind], word_bonus=0.6,
                                                lm=word_lm, lm_weight=0.8, length_bonus=0.3)

            forms = {}
            if a.only != "marked":
                forms["lm"] = lambda: crit.beam_search(xs["lm"], beam_size=W, classes_per_frame=K, lm=token_lm, lm_weight=0.8,
                                                       length_bonus=0.5)
            for kind in lexicons:
                if kind == "start" or a.only != "marked":
                    forms[kind] = lexicon_call(kind)
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
                f"{k:5s} {statistics.median(v):8.3f} ({min(v):8.3f} .. {max(v):8.3f})" for k, v in ms.items())
            line += "   words in " + ", ".join(f"{k} {sum(len(p) > 0 for p in results[k])}" for k in lexicons if k in forms)
            line += f" of {a.B}"
            if "start" in forms and "end" in forms:
                line += f"   start / end {statistics.median(ms['start']) / statistics.median(ms['end']):5.2f}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
