"""Per-call time of CTC.beam_search and CTC.errors(beam_size=) at a shape where the call is host-bound (default B=1, T=16,
C=32, W=4, K=4), on a GPU: what the checks and the argument plumbing in front of the launch cost, and nothing else shows.

    python scripts/beam_plan_probe.py            plain, with a token LM, with a lexicon and its word LM; both calls

The LMs and the lexicon are scripts/beam_lm_probe.py's and scripts/beam_lexicon_probe.py's at this C (50 words); the
input is white noise.  Each line is one loop of `--calls` calls behind `--warmup`, the host clock around it (a call ends
on the host with its results).  One process per measurement: an A/B runs this in fresh processes of each tree in turn."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gtn_applications_amd import metrics as M  # noqa: E402
from gtn_applications_amd.criterions.ctc import CTC  # noqa: E402
from scripts.beam_lexicon_probe import random_lexicon, random_word_trigram  # noqa: E402
from scripts.beam_lm_probe import random_trigram  # noqa: E402
from scripts.beam_probe import per_call_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--C", type=int, default=32)
    ap.add_argument("--W", type=int, default=4)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--words", type=int, default=50)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "beam_plan_probe needs a GPU"
    blank, sep = a.C - 1, a.C - 2
    crit = CTC(blank=blank, use_pt=False)
    lex = random_lexicon(a.C, blank, sep, a.words, seed=2)
    forms = {"plain": {},
             "lm": dict(lm=random_trigram(a.C, blank, 0.05, seed=1), lm_weight=0.8, length_bonus=0.5),
             "lexicon": dict(lexicon=lex, word_bonus=0.6, lm=random_word_trigram(a.words, 0.05, seed=3), lm_weight=0.8,
                             length_bonus=0.3)}
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.randn(a.B, a.T, a.C).astype(np.float32)).cuda()
    targets = [rs.randint(0, a.C - 2, size=4).tolist() for _ in range(a.B)]
    counter = M.ErrorCounter(wordsep=sep)
    print(f"B={a.B} T={a.T} C={a.C} blank={blank} W={a.W} K={a.K}; {a.warmup} warm-up + {a.calls} timed calls; ms per call")
    for name, kw in forms.items():
        calls = {"beam_search": lambda: crit.beam_search(x, beam_size=a.W, classes_per_frame=a.K, **kw),
                 "errors": lambda: crit.errors(x, targets, counter, beam_size=a.W, classes_per_frame=a.K, **kw)}
        for call, fn in calls.items():
            print(f"{name:8s} {call:12s} {per_call_ms(fn, a.warmup, a.calls):8.4f}", flush=True)


if __name__ == "__main__":
    main()
