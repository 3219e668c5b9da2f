"""Per-call time of Transducer.beam_search beside CTC.beam_search on the same emissions and options, at the benchmark's
decode shape (B=128, T=1000, C=101: 100 tokens and the blank), on a GPU.

    python scripts/transducer_beam_probe.py              every (beam width, classes per frame) of --configs, both inputs
    python scripts/transducer_beam_probe.py --config 16,32 --only bigram-optional --input noise --calls 3 --runs 1
        one configuration, one search only: for a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/transducer_beam_probe.py --config ...
        (scripts/kstats.py prints the averages per kernel)

The criteria are Transducer(100 single-grapheme tokens, blank last) with the bigram transition model (ngram=2,
parameters 0.1 N(0,1)) in both searched token graphs -- blank="optional" without repeats and blank="forced" -- and the
forced graph without a model (the optional graph without one IS the CTC search).  Inputs: scripts/beam_probe.py's --
white noise N(0,1), and emissions peaked (+8) on a random alignment of 44 labels with the blank between them.  Twice per
criterion and configuration: Transducer.beam_search (the operands of the route, the normaliser and the search) and the
search alone (engine.transducer_beam_search on those operands with normalize=False: the three launches); beside them
CTC.beam_search with the same blank.  A call ends on the host with its results, so the host clock around `calls` calls
is the per-call time; the median of the runs goes into the ratio.  Results: profiles/transducer_beam_search.txt."""
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
from gtn_applications_amd.criterions.ctc import CTC  # noqa: E402
from gtn_applications_amd.criterions.transducer import Transducer  # noqa: E402

KINDS = {"bigram-optional": (2, dict(blank="optional", allow_repeats=False)), "bigram-forced": (2, dict(blank="forced")),
         "plain-forced": (0, dict(blank="forced"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--configs", default="1,32 16,32 64,64", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="all", choices=["all", "ctc"] + list(KINDS))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "transducer_beam_probe needs a GPU"
    tokens = [chr(0x100 + i) for i in range(a.tokens)]
    g2i = {t: i for i, t in enumerate(tokens)}
    C, blank = a.tokens + 1, a.tokens
    crits = {}
    for name, (ngram, kw) in KINDS.items():
        if a.only in ("all", name):
            crit = Transducer(tokens, g2i, ngram=ngram, **kw).cuda()
            if ngram:
                with torch.no_grad():
                    n = crit.transition_params.numel()
                    crit.transition_params.copy_(torch.from_numpy((0.1 * np.random.RandomState(1).randn(n)).astype(np.float32)))
            crits[name] = crit
    ctc = CTC(blank=blank, use_pt=False)
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    data = {k: v for k, v in inputs(a.B, a.T, C, blank).items() if a.input in ("both", k)}
    fmt = lambda ms: "  ".join(f"{v:8.3f}" for v in ms)
    median = lambda ms: sorted(ms)[len(ms) // 2]
    print(f"B={a.B} T={a.T} C={C} blank = {blank}; {a.warmup} warm-up + {a.calls} timed calls, {a.runs} runs; ms per call")
    for name, x in data.items():
        for W, K in configs:
            kw = dict(beam_size=W, classes_per_frame=K)
            base = None
            if a.only in ("all", "ctc"):
                ms = [per_call_ms(lambda: ctc.beam_search(x, **kw), a.warmup, a.calls) for _ in range(a.runs)]
                base = median(ms)
                print(f"{name:7s} CTC.beam_search                 W={W:2d} K={K:2d}  {fmt(ms)}")
            for kind, crit in crits.items():
                plan, route = crit._beam_plan(x, "probe", W, K, 1)
                xe, Wt = crit._beam_inputs(x, route)
                greedy = crit.viterbi(x)
                best = crit.beam_search(x, **kw)
                differ = sum(p.tolist() != g.tolist() for p, g in zip(best, greedy))
                ms = [per_call_ms(lambda: crit.beam_search(x, **kw), a.warmup, a.calls) for _ in range(a.runs)]
                print(f"{name:7s} {kind:15s} .beam_search    W={W:2d} K={K:2d}  {fmt(ms)}   (differs from viterbi in {differ} of {a.B})")
                ms = [per_call_ms(lambda: E.transducer_beam_search(xe, Wt, blank, plan.forced, W, K, normalize=False), a.warmup,
                                  a.calls) for _ in range(a.runs)]
                ratio = f"   {median(ms) / base:5.2f} x CTC" if base else ""
                print(f"{name:7s} {kind:15s} search alone    W={W:2d} K={K:2d}  {fmt(ms)}{ratio}")


if __name__ == "__main__":
    main()
