"""CTC's per-utterance input lengths (criterions/ctc.py `input_lengths`) at the benchmark shape -- B=128, T=1000, C=100,
L=44, emissions that are a producer's output: this tree and a build of the parent commit alternating in ONE GPU call,
four runs each (the tree that goes first alternates too), every run a fresh process.

    python scripts/ctc_lengths_ab.py --parent DIR [--out FILE]     DIR: a checkout of the parent commit, built in place

Per run, ms per call, synchronised at the end of the timed loop:
    step                      loss = CTC(x * 1, targets); loss.backward()       both trees: must be unchanged
    step(lengths)             the same with lengths uniform in [T/2, T]          this tree
    viterbi / errors          with and without the lengths                       (the parent: without)
1. the step without lengths: the difference of the medians against the spread (max - min) of the parent's own runs;
2. the step with lengths against the same tree's step without;
3. viterbi and errors with and without lengths.
`--worker` is the measuring process (it imports the package of the tree it runs in)."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def worker(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch

    from gtn_applications_amd.criterions import ctc

    try:
        from gtn_applications_amd import ErrorCounter
    except ImportError:
        ErrorCounter = None

    rs = np.random.RandomState(0)
    B, T, C, L = 128, 1000, 100, 44
    crit = ctc.CTC(blank=C - 1, use_pt=False)
    leaf = torch.from_numpy(rs.randn(B, T, C).astype(np.float32)).cuda().requires_grad_(True)
    targets = [torch.tensor(rs.randint(0, C - 1, size=L).tolist()) for _ in range(B)]
    lengths = rs.randint(T // 2, T + 1, size=B).tolist()
    has_lengths = hasattr(ctc, "check_input_lengths")  # (the parent: no lengths)

    def timed(fn, n=60, warm=10):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def step(*extra):
        leaf.grad = None
        crit(leaf * 1.0, targets, *extra).backward()

    row = {"step": timed(step)}
    x = leaf.detach()
    row["viterbi"] = timed(lambda: crit.viterbi(x), n=200, warm=20)
    counter = ErrorCounter() if ErrorCounter is not None else None
    if counter is not None:
        row["errors"] = timed(lambda: crit.errors(x, targets, counter), n=200, warm=20)
    if has_lengths:
        row["step(lengths)"] = timed(lambda: step(lengths))
        row["step again"] = timed(step)  # (the same process, after the calls with lengths)
        row["viterbi(lengths)"] = timed(lambda: crit.viterbi(x, lengths), n=200, warm=20)
        row["errors(lengths)"] = timed(lambda: crit.errors(x, targets, counter, lengths), n=200, warm=20)
        pad = sum(T - n for n in lengths)
        assert float(leaf.grad.abs().sum()) > 0
        step(lengths)
        torch.cuda.synchronize()
        zero = sum(int((leaf.grad[b, n:] != 0).sum()) for b, n in enumerate(lengths))
        assert zero == 0, zero
        row["pad_frames"] = pad
    print("ROW " + json.dumps(row), flush=True)


def run(tree):
    """one measuring process in `tree`; a failing worker ends the comparison"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree], cwd=tree, capture_output=True,
                         text=True, timeout=600)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit(f"worker in {tree} ended with {out.returncode}: nothing more is started")
    return [json.loads(l[4:]) for l in out.stdout.splitlines() if l.startswith("ROW ")][0]


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit, built in place")
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree))
    runs = {"new": [], "parent": []}
    for k in range(args.runs):  # alternating, and the tree that goes first alternates too
        order = ["new", "parent"] if args.parent else ["new"]
        for which in order if k % 2 == 0 else order[::-1]:
            runs[which].append(run(ROOT if which == "new" else os.path.abspath(args.parent)))
            print(f"run {k + 1}: {which} done", flush=True)
    lines = ["CTC module step, viterbi and errors at B=128 T=1000 C=100 L=44 (producer-output emissions), ms per call;",
             f"lengths uniform in [T/2, T] ({runs['new'][0].get('pad_frames')} pad frames of 128000)"]

    def series(which, what):
        vals = [r[what] for r in runs[which] if what in r]
        if vals:
            lines.append(f"  {which:<6} {what:<18} {'  '.join(f'{v:.4f}' for v in vals)}   (median {median(vals):.4f}, "
                         f"spread {max(vals) - min(vals):.4f})")
        return vals

    for what in ("step", "step again", "step(lengths)", "viterbi", "viterbi(lengths)", "errors", "errors(lengths)"):
        for which in ("parent", "new"):
            series(which, what)
    if args.parent:
        p, n = [r["step"] for r in runs["parent"]], [r["step"] for r in runs["new"]]
        diff, spread = median(n) - median(p), max(p) - min(p)
        verdict = "inside" if abs(diff) <= spread else "OUTSIDE"
        lines.append(f"1. step without lengths: median new - median parent = {diff:+.4f} ms, the parent's own spread is "
                     f"{spread:.4f} ms: {verdict} the spread")
    n, w = [r["step"] for r in runs["new"]], [r["step(lengths)"] for r in runs["new"]]
    lines.append(f"2. step with lengths - step without, this tree: {median(w) - median(n):+.4f} ms of {median(n):.4f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
