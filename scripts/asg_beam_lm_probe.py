"""Per-call time of ASG.beam_search with a token-level n-gram LM beside the same search without one, at the decode shape of
scripts/asg_beam_probe.py (B=128, T=1000, C=100), on a GPU.

    python scripts/asg_beam_lm_probe.py                  beam widths 1, 16, 64 at 32 classes per frame, both inputs
    python scripts/asg_beam_lm_probe.py --config 16,32 --input noise --form lm --calls 3 --warmup 1
        one configuration, one call form: the target of a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/asg_beam_lm_probe.py --config ...
        (scripts/kstats.py prints the averages; the LM call's beam launch is beam_search_kernel<NT, wfl::BeamAsgLm>, the
        plain call's beam_search_kernel<NT, wfl::BeamAsg>)

The criterion is ASG(97 tokens, 2 replabels, garbage): 100 classes, the garbage last; its transitions are 0.1 N(0,1).
Inputs: scripts/beam_probe.py's -- white noise N(0,1), and emissions peaked (+8) on a random alignment of 44 labels with
the garbage class between them.  The LM is a seeded random trigram over the 97 tokens, written as ARPA text and read by
ASG.token_lm: every unigram, `--keep` of the bigrams, and of the trigrams whose parts are in the file.  lm_weight 0.8,
length_bonus 0.5, </s> scored.

The two calls alternate in one process -- plain, LM, plain, LM, ... -- so that clocks and neighbours drift under both
alike; a call ends on the host with its results, so the host clock around it is its time.  Reported per call form: the
median over all timed calls, and the spread (min, max); beside the ratio, CTC's LM-to-plain ratio at the same (W, K, input)
from profiles/beam_search_lm.txt.  Results: profiles/asg_beam_search_lm.txt."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from beam_probe import inputs  # noqa: E402
from gtn_applications_amd.criterions.asg import ASG  # noqa: E402
from transducer_beam_lm_probe import CTC_RATIO, random_trigram_text  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--configs", default="1,32 16,32 64,32", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--form", default="both", choices=["both", "lm", "plain"], help="which call form (for a kernel trace)")
    ap.add_argument("--keep", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=15, help="timed calls of each form")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "asg_beam_lm_probe needs a GPU"
    tokens = [f"t{i}" for i in range(97)]
    asg = ASG(len(tokens), num_replabels=2, use_garbage=True).cuda()
    C, last = asg.N, asg.N - 1
    with torch.no_grad():
        asg.transitions.copy_(torch.from_numpy((0.1 * np.random.RandomState(1).randn(C + 1, C)).astype(np.float32)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.arpa")
        with open(path, "w") as f:
            f.write(random_trigram_text(tokens, a.keep, seed=1))
        lm = asg.token_lm(path, tokens)
    lm.on_device("cuda")
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    data = {k: v for k, v in inputs(a.B, a.T, C, last).items() if a.input in ("both", k)}
    print(f"B={a.B} T={a.T} C={C} = 97 tokens + 2 replabels + garbage {last}; LM order {lm.order}: {lm.num_states} states, "
          f"{lm.num_arcs} arcs; {a.warmup} warm-up + {a.calls} alternating timed calls of each form; ms per call: median (min .. max)")
    for name, x in data.items():
        for W, K in configs:
            forms = {"plain": lambda: asg.beam_search(x, beam_size=W, classes_per_frame=K),
                     "lm": lambda: asg.beam_search(x, beam_size=W, classes_per_frame=K, token_lm=lm, lm_weight=0.8, length_bonus=0.5)}
            forms = {k: f for k, f in forms.items() if a.form in ("both", k)}
            results = {k: f() for k, f in forms.items()}
            for _ in range(a.warmup):
                for f in forms.values():
                    f()
            ms = {k: [] for k in forms}
            for _ in range(a.calls):
                for k, f in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            line = f"{name:7s} W={W:2d} K={K:2d}  " + "   ".join(
                f"{k:5s} {statistics.median(v):8.3f} ({min(v):8.3f} .. {max(v):8.3f})" for k, v in ms.items())
            if len(forms) == 2:
                differ = sum(p.tolist() != q.tolist() for p, q in zip(results["plain"], results["lm"]))
                repeats = sum(int((p[1:] == p[:-1]).sum()) for p in results["lm"])
                ctc = CTC_RATIO.get((name, W, K))
                line += f"   lm / plain {statistics.median(ms['lm']) / statistics.median(ms['plain']):5.2f}" \
                        f"   (CTC's: {'%.2f' % ctc if ctc else 'not measured'}; best differs in {differ} of {a.B}; " \
                        f"{repeats} repeated tokens in the LM call's results)"
            print(line, flush=True)


if __name__ == "__main__":
    main()
