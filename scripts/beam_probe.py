"""Per-call time of CTC.beam_search beside CTC.viterbi at the benchmark's decode shape (B=128, T=1000, C=100), on a GPU.

    python scripts/beam_probe.py                      every (beam width, classes per frame) of --configs, both inputs
    python scripts/beam_probe.py --config 16,32       one configuration only: for a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/beam_probe.py --config 16,32 --calls 3
        (scripts/kstats.py prints the averages: beam_candidates_kernel / beam_search_kernel / beam_write_kernel)

Inputs: white noise N(0,1), and emissions peaked (+8) on a random alignment of random 44-label targets with 8 frames
per utterance moved to another class.  A call ends on the host with its results, so the host clock around `calls` calls
is the per-call time; the warm-up calls run every shape first.  Results: profiles/beam_search.txt."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gtn_applications_amd.criterions.ctc import CTC  # noqa: E402


def inputs(B, T, C, blank, seed=0):
    rs = np.random.RandomState(seed)
    noise = rs.randn(B, T, C).astype(np.float32)
    peaked = rs.randn(B, T, C).astype(np.float32)
    for b in range(B):
        target = rs.randint(0, C - 1, size=44)
        cuts = np.sort(rs.choice(np.arange(1, T), size=2 * 44, replace=False))
        frames = np.full(T, blank)
        for i, lab in enumerate(target):
            frames[cuts[2 * i]:cuts[2 * i + 1]] = lab
        moved = rs.choice(T, size=8, replace=False)
        frames[moved] = rs.randint(0, C, size=8)
        peaked[b, np.arange(T), frames] += 8.0
    return {"noise": torch.from_numpy(noise).cuda(), "peaked": torch.from_numpy(peaked).cuda()}


def per_call_ms(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--C", type=int, default=100)
    ap.add_argument("--configs", default="1,32 1,64 16,32 16,64 64,32 64,64", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "beam_probe needs a GPU"
    blank = a.C - 1
    crit = CTC(blank=blank, use_pt=False)
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    data = {k: v for k, v in inputs(a.B, a.T, a.C, blank).items() if a.input in ("both", k)}
    print(f"B={a.B} T={a.T} C={a.C} blank={blank}; {a.warmup} warm-up + {a.calls} timed calls, {a.runs} runs; ms per call")
    for name, x in data.items():
        greedy = crit.viterbi(x)
        ms = [per_call_ms(lambda: crit.viterbi(x), a.warmup, max(a.calls, 20)) for _ in range(a.runs)]
        print(f"{name:7s} viterbi                      " + "  ".join(f"{v:8.3f}" for v in ms))
        for W, K in configs:
            best = crit.beam_search(x, beam_size=W, classes_per_frame=K)
            differ = sum(p.tolist() != g.tolist() for p, g in zip(best, greedy))
            ms = [per_call_ms(lambda: crit.beam_search(x, beam_size=W, classes_per_frame=K), a.warmup, a.calls)
                  for _ in range(a.runs)]
            print(f"{name:7s} beam_search W={W:2d} K={K:2d}       " + "  ".join(f"{v:8.3f}" for v in ms) +
                  f"   (differs from greedy in {differ} of {a.B})")


if __name__ == "__main__":
    main()
