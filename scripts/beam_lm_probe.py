"""Per-call time of CTC.beam_search with an n-gram LM beside the same search without one, at the benchmark's decode shape
(B=128, T=1000, C=100), on a GPU.

    python scripts/beam_lm_probe.py                    beam widths 1, 16, 64 at 32 classes per frame, both inputs
    python scripts/beam_lm_probe.py --config 16,32 --input noise --calls 3 --warmup 1 --rounds 1
        one configuration only: the target of a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/beam_lm_probe.py --config ...
        (scripts/kstats.py prints the averages; the LM call's beam launch is beam_search_kernel<NT, wfl::BeamLm>)

Inputs: scripts/beam_probe.py's (white noise; emissions peaked on a random alignment).  The LM is a seeded random
trigram over the 99 tokens, written as ARPA text and loaded through NGramLM.from_arpa: every unigram, 5 % of the bigrams,
5 % of the trigrams whose parts are in the file.  lm_weight 0.8, length_bonus 0.5, </s> scored.

The two calls alternate in one process -- no-LM, LM, no-LM, LM, ... -- so that clocks and neighbours drift under both
alike; a call ends on the host with its results, so the host clock around it is its time.  Reported per call form: the
median over all timed calls, and the spread (min, max).  Results: profiles/beam_search_lm.txt."""
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
from gtn_applications_amd.lm import NGramLM  # noqa: E402
from scripts.beam_probe import inputs  # noqa: E402


def random_trigram(C, blank, keep, seed):
    """NGramLM over the classes but the blank: every unigram, each bigram / trigram (whose history and suffix are in the
    file) with probability `keep`; log10 weights in [-3, -0.1], back-offs in [-1, 0]"""
    rs = np.random.RandomState(seed)
    tokens = [f"t{i}" for i in range(C - 1)]
    words = tokens + ["</s>"]
    levels = [[("<s>",)] + [(w,) for w in words]]
    for _ in (2, 3):
        prev = set(levels[-1])
        levels.append([h + (w,) for h in levels[-1] if h[-1] != "</s>" for w in words
                       if h[1:] + (w,) in prev and rs.rand() < keep])
    lines = ["\\data\\"] + [f"ngram {n + 1}={len(level)}" for n, level in enumerate(levels)] + [""]
    for n, level in enumerate(levels):
        lines.append(f"\\{n + 1}-grams:")
        for g in level:
            bo = f"\t{-rs.rand():.6f}" if n < 2 and g[-1] != "</s>" else ""
            lines.append(f"{-0.1 - 2.9 * rs.rand():.6f}\t{' '.join(g)}{bo}")
        lines.append("")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.arpa")
        with open(path, "w") as f:
            f.write("\n".join(lines + ["\\end\\", ""]))
        return NGramLM.from_arpa(path, tokens, blank)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--C", type=int, default=100)
    ap.add_argument("--configs", default="1,32 16,32 64,32", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="both", choices=["both", "lm", "plain"], help="which call form (for a kernel trace)")
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--calls", type=int, default=5, help="timed calls of each form per round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "beam_lm_probe needs a GPU"
    blank = a.C - 1
    crit = CTC(blank=blank, use_pt=False)
    lm = random_trigram(a.C, blank, a.keep, seed=1)
    lm.on_device("cuda")
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    data = {k: v for k, v in inputs(a.B, a.T, a.C, blank).items() if a.input in ("both", k)}
    print(f"B={a.B} T={a.T} C={a.C} blank={blank}; LM order {lm.order}: {lm.num_states} states, {lm.num_arcs} arcs; "
          f"{a.warmup} warm-up + {a.rounds} x {a.calls} alternating timed calls of each form; ms per call: median (min .. max)")
    for name, x in data.items():
        for W, K in configs:
            forms = {"plain": lambda: crit.beam_search(x, beam_size=W, classes_per_frame=K),
                     "lm": lambda: crit.beam_search(x, beam_size=W, classes_per_frame=K, lm=lm, lm_weight=0.8, length_bonus=0.5)}
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
                f"{k:5s} {statistics.median(v):8.3f} ({min(v):8.3f} .. {max(v):8.3f})" for k, v in ms.items())
            if len(forms) == 2:
                differ = sum(p.tolist() != q.tolist() for p, q in zip(results["plain"], results["lm"]))
                line += f"   lm / plain {statistics.median(ms['lm']) / statistics.median(ms['plain']):5.2f}" \
                        f"   (best differs in {differ} of {a.B})"
            print(line, flush=True)


if __name__ == "__main__":
    main()
