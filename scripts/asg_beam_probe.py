"""Per-call time of ASG.beam_search beside ASG.viterbi and beside CTC.beam_search on the same emissions and options, at
the benchmark's decode shape (B=128, T=1000, C=100), on a GPU.

    python scripts/asg_beam_probe.py                    every (beam width, classes per frame) of --configs, both inputs
    python scripts/asg_beam_probe.py --config 16,32 --only asg --input noise --calls 3 --runs 1
        one configuration, one search only: for a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/asg_beam_probe.py --config ...
        (scripts/kstats.py prints the averages per kernel)

The criterion is ASG(97 tokens, 2 replabels, garbage): 100 classes, the garbage last; its transitions are 0.1 N(0,1).
Inputs: scripts/beam_probe.py's -- white noise N(0,1), and emissions peaked (+8) on a random alignment of 44 labels
with the garbage class (CTC: the blank) between them.  Three times per configuration: ASG.beam_search (the search, the
mapping of the results and the denominator logz for its normalised scores), the search alone (engine.asg_beam_search
with normalize=False: the three launches), and CTC.beam_search with the blank where ASG has its garbage.  A call ends on
the host with its results, so the host clock around `calls` calls is the per-call time.  Results:
profiles/asg_beam_search.txt."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from beam_probe import inputs, per_call_ms  # noqa: E402
from gtn_applications_amd import engine as E  # noqa: E402
from gtn_applications_amd.criterions.asg import ASG  # noqa: E402
from gtn_applications_amd.criterions.ctc import CTC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--configs", default="1,32 16,32 64,64", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="all", choices=["all", "asg", "ctc"])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "asg_beam_probe needs a GPU"
    asg = ASG(97, num_replabels=2, use_garbage=True).cuda()
    C, last = asg.N, asg.N - 1
    with torch.no_grad():
        asg.transitions.copy_(torch.from_numpy((0.1 * np.random.RandomState(1).randn(C + 1, C)).astype(np.float32)))
    Wt = asg.transitions.detach().contiguous()
    ctc = CTC(blank=last, use_pt=False)
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    data = {k: v for k, v in inputs(a.B, a.T, C, last).items() if a.input in ("both", k)}
    fmt = lambda ms: "  ".join(f"{v:8.3f}" for v in ms)
    print(f"B={a.B} T={a.T} C={C} garbage = blank = {last}; {a.warmup} warm-up + {a.calls} timed calls, {a.runs} runs; ms per call")
    for name, x in data.items():
        if a.only != "ctc":
            greedy = asg.viterbi(x)
            ms = [per_call_ms(lambda: asg.viterbi(x), a.warmup, max(a.calls, 20)) for _ in range(a.runs)]
            print(f"{name:7s} ASG.viterbi                        {fmt(ms)}")
        for W, K in configs:
            kw = dict(beam_size=W, classes_per_frame=K)
            med = {}
            if a.only != "ctc":
                best = asg.beam_search(x, **kw)
                differ = sum(p.tolist() != g.tolist() for p, g in zip(best, greedy))
                ms = [per_call_ms(lambda: asg.beam_search(x, **kw), a.warmup, a.calls) for _ in range(a.runs)]
                print(f"{name:7s} ASG.beam_search W={W:2d} K={K:2d}         {fmt(ms)}   (differs from viterbi in {differ} of {a.B})")
                ms = [per_call_ms(lambda: E.asg_beam_search(x, Wt, W, K, normalize=False), a.warmup, a.calls) for _ in range(a.runs)]
                med["asg"] = sorted(ms)[len(ms) // 2]
                print(f"{name:7s}   the search alone W={W:2d} K={K:2d}      {fmt(ms)}")
            if a.only != "asg":
                ms = [per_call_ms(lambda: ctc.beam_search(x, **kw), a.warmup, a.calls) for _ in range(a.runs)]
                med["ctc"] = sorted(ms)[len(ms) // 2]
                print(f"{name:7s} CTC.beam_search W={W:2d} K={K:2d}         {fmt(ms)}")
            if len(med) == 2:
                print(f"{name:7s}   ASG search alone / CTC W={W:2d} K={K:2d}  {med['asg'] / med['ctc']:8.2f}")


if __name__ == "__main__":
    main()
