"""Per-call time of Transducer.beam_search(merge_spellings=True) beside the unmerged search on the same emissions and
options, at the benchmark's word-piece shape (B=128, T=1000, C=1001: benchmarks/word_pieces_tokens_1000.txt and the blank),
on a GPU -- and what the merging changes in the result.

    python scripts/transducer_merged_beam_probe.py              every (beam width, classes per frame) of --configs, both inputs
    python scripts/transducer_merged_beam_probe.py --config 16,32 --only bigram-optional --input noise --calls 3 --runs 1
        one configuration, one criterion only: for a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/transducer_merged_beam_probe.py --config ...

The criteria are Transducer(the 1000 word pieces, blank last) with the bigram transition model (ngram=2, parameters 0.1
N(0,1)) and without a model, in both searched token graphs.  Inputs: scripts/beam_probe.py's -- white noise N(0,1), and
emissions peaked (+8) on a random alignment of 44 labels with the blank between them.  Per criterion and configuration,
merged and unmerged in the same run: Transducer.beam_search (the operands of the route, the normaliser and the search)
and the search alone (engine.transducer_beam_search on those operands with normalize=False: the three launches).  A call
ends on the host with its results, so the host clock around `calls` calls is the per-call time; the median of the runs
goes into the ratio merged / unmerged.  Per input also: the share of utterances whose best spelling differs from the
spelling of the unmerged search's best sequence, and the mean gain in score where the two agree.
Results: profiles/transducer_merged_beam_search.txt."""
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
from gtn_applications_amd.criterions.transducer import Transducer  # noqa: E402

KINDS = {"bigram-optional": (2, dict(blank="optional", allow_repeats=False)), "bigram-forced": (2, dict(blank="forced")),
         "plain-optional": (0, dict(blank="optional", allow_repeats=False)), "plain-forced": (0, dict(blank="forced"))}


def word_pieces():
    with open(os.path.join(ROOT, "benchmarks", "word_pieces_tokens_1000.txt")) as f:
        tokens = sorted(l.strip() for l in f)
    return tokens, {g: i for i, g in enumerate(sorted(set(c for t in tokens for c in t)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--configs", default="1,32 16,32 64,64", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="all", choices=["all"] + list(KINDS))
    ap.add_argument("--search", default="both", choices=["both", "merged", "unmerged"], help="(for a kernel trace)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "transducer_merged_beam_probe needs a GPU"
    tokens, g2i = word_pieces()
    C, blank = len(tokens) + 1, len(tokens)
    crits = {}
    for name, (ngram, kw) in KINDS.items():
        if a.only in ("all", name):
            crit = Transducer(tokens, g2i, ngram=ngram, **kw).cuda()
            if ngram:
                with torch.no_grad():
                    n = crit.transition_params.numel()
                    crit.transition_params.copy_(torch.from_numpy((0.1 * np.random.RandomState(1).randn(n)).astype(np.float32)))
            crits[name] = crit
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    data = {k: v for k, v in inputs(a.B, a.T, C, blank).items() if a.input in ("both", k)}
    fmt = lambda ms: "  ".join(f"{v:8.3f}" for v in ms)
    median = lambda ms: sorted(ms)[len(ms) // 2]
    timed = lambda fn: [per_call_ms(fn, a.warmup, a.calls) for _ in range(a.runs)]
    spelt = lambda crit, p: tuple(g for v in p.tolist() for g in crit.token_spellings[v])
    print(f"B={a.B} T={a.T} C={C} blank = {blank}; {a.warmup} warm-up + {a.calls} timed calls, {a.runs} runs; ms per call")
    for name, x in data.items():
        for W, K in configs:
            kw = dict(beam_size=W, classes_per_frame=K)
            for kind, crit in crits.items():
                plan, route = crit._beam_plan(x, "probe", W, K, 1)
                table = crit._spelling(plan, "probe")
                xe, Wt = crit._beam_inputs(x, route)
                base = {}
                for which in ("unmerged", "merged"):
                    if a.search not in ("both", which):
                        continue
                    m = which == "merged"
                    ms = timed(lambda: crit.beam_search(x, merge_spellings=m, **kw))
                    base[which, "call"] = median(ms)
                    print(f"{name:7s} {kind:15s} {which:8s} .beam_search  W={W:2d} K={K:2d}  {fmt(ms)}")
                    ms = timed(lambda: E.transducer_beam_search(xe, Wt, blank, plan.forced, W, K, normalize=False,
                                                                spelling=table if m else None))
                    base[which, "search"] = median(ms)
                    print(f"{name:7s} {kind:15s} {which:8s} search alone  W={W:2d} K={K:2d}  {fmt(ms)}")
                if a.search != "both":
                    continue
                mh, msc = crit.beam_search(x, return_scores=True, merge_spellings=True, **kw)
                uh, usc = crit.beam_search(x, return_scores=True, **kw)
                same = [spelt(crit, p) == spelt(crit, q) for p, q in zip(mh, uh)]
                gain = [float(msc[b, 0] - usc[b, 0]) for b in range(a.B) if same[b] and usc[b, 0] > -np.inf]
                print(f"{name:7s} {kind:15s} merged / unmerged     W={W:2d} K={K:2d}  call {base['merged', 'call'] / base['unmerged', 'call']:5.2f} x  "
                      f"search alone {base['merged', 'search'] / base['unmerged', 'search']:5.2f} x   best spelling differs in "
                      f"{a.B - sum(same)} of {a.B}; mean gain where it agrees {np.mean(gain) if gain else float('nan'):.4f} "
                      f"(max {max(gain) if gain else float('nan'):.4f})")


if __name__ == "__main__":
    main()
