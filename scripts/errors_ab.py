"""criterion.errors() (decode and error counts on the device, csrc/error_kernels.hip) against what a training step spends
on its metric otherwise: this tree and a build of the parent commit alternating in ONE GPU call, three runs each, every
run a fresh process.

    python scripts/errors_ab.py --parent DIR [--out FILE]     DIR: a checkout of the parent commit, built in place

Per workload (the benchmark shapes: CTC B=128 T=1000 C=100 L=44; ASG the same with 98 tokens + 1 replabel + garbage;
Transducer B=64 T=800 with the 1000 word pieces) and per input (white noise; emissions peaked on a random alignment of the
targets with a few frames flipped), ms per call, synchronised:
    parent viterbi(x)                 the least the parent spends before any metric exists
    viterbi(x)                        this tree: must be unchanged
    errors(x, targets, counter)       decode + count on the device, 4 integers to the host
    counter(viterbi(x), targets)      the predictions to the host and back
`--worker` is the measuring process (it imports the package of the tree it runs in)."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKLOADS = ("ctc", "asg", "transducer")
INPUTS = ("noise", "peaked")
FLIPS = 8  # frames per utterance moved to another class in the peaked input


def worker(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch

    from gtn_applications_amd.criterions import asg, ctc, transducer

    try:
        from gtn_applications_amd import ErrorCounter
    except ImportError:  # the parent: no metric
        ErrorCounter = None

    def alignment(rs, rows, T, filler):
        out = np.full((len(rows), T), filler, np.int64)
        for b, row in enumerate(rows):
            cuts = np.sort(rs.choice(np.arange(1, T), size=2 * len(row), replace=False))
            for k, v in enumerate(row):
                out[b, cuts[2 * k]:cuts[2 * k + 1]] = v
        return out

    def emissions(rs, kind, frames, C):
        B, T = frames.shape
        if kind == "noise":
            return torch.from_numpy(rs.randn(B, T, C).astype(np.float32)).cuda()
        lab = frames.copy()
        for b in range(B):
            for t in rs.choice(T, size=FLIPS, replace=False):
                lab[b, t] = (lab[b, t] + 1 + rs.randint(C - 1)) % C
        x = 0.1 * rs.randn(B, T, C).astype(np.float32)
        x[np.arange(B)[:, None], np.arange(T)[None, :], lab] += 8.0
        return torch.from_numpy(x).cuda()

    def timed(fn, n=40, warm=8):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def cases():
        rs = np.random.RandomState(0)
        B, T, C, L = 128, 1000, 100, 44
        # CTC: 99 tokens + blank; token 0 is the word separator
        toks = [chr(0x100 + i) for i in range(C - 1)]
        rows = [rs.randint(0, C - 1, size=L).tolist() for _ in range(B)]
        yield "ctc", ctc.CTC(blank=C - 1, use_pt=False), (toks, toks, toks[0]), [torch.tensor(r) for r in rows], \
            lambda kind: emissions(rs, kind, alignment(rs, rows, T, C - 1), C)
        # ASG: 98 tokens + 1 replabel + garbage (bench.py --workload asg); no label twice in a row in the alignment
        m = asg.ASG(C - 2, 1, True).cuda()
        with torch.no_grad():
            m.transitions.copy_(torch.randn(C + 1, C, generator=torch.Generator().manual_seed(7)))
        toks = [chr(0x100 + i) for i in range(C - 2)]
        rows = [[int(v) for v in (rs.permutation(C - 2).tolist() * 2)[:L]] for _ in range(B)]
        yield "asg", m, (toks, toks, toks[0]), [torch.tensor(r) for r in rows], \
            lambda kind: emissions(rs, kind, alignment(rs, [[v + 1 for v in r] for r in rows], T, C - 1), C)
        # Transducer: the 1000 word pieces, 15 pieces per utterance spelled in graphemes (bench.py --workload transducer)
        with open(os.path.join(root, "benchmarks", "word_pieces_tokens_1000.txt")) as f:
            pieces = sorted(l.strip() for l in f)
        graphemes = sorted(set(c for t in pieces for c in t))
        g2i = {g: i for i, g in enumerate(graphemes)}
        B, T = 64, 800
        rnd = random.Random(0)
        piece_rows = [[rnd.randrange(len(pieces)) for _ in range(15)] for _ in range(B)]
        rows = [[g2i[c] for p in r for c in pieces[p]] for r in piece_rows]
        sep = max(graphemes, key=lambda g: sum(t.startswith(g) for t in pieces))  # (what most pieces begin with)
        m = transducer.Transducer(pieces, g2i, blank="optional", allow_repeats=False, reduction="mean")
        yield "transducer", m, (pieces, graphemes, sep), [torch.tensor(r) for r in rows], \
            lambda kind: emissions(rs, kind, alignment(rs, piece_rows, T, len(pieces)), len(pieces) + 1)

    for name, crit, tables, targets, make in cases():
        counter = ErrorCounter(*tables) if ErrorCounter is not None else None
        for kind in INPUTS:
            x = make(kind)
            row = {"workload": name, "input": kind, "viterbi": timed(lambda: crit.viterbi(x))}
            if counter is not None:
                fused, split = crit.errors(x, targets, counter), counter(crit.viterbi(x), targets)
                assert fused == split, (fused, split)
                row["counts"] = list(fused)
                row["errors"] = timed(lambda: crit.errors(x, targets, counter))
                row["counter(viterbi)"] = timed(lambda: counter(crit.viterbi(x), targets))
            print("ROW " + json.dumps(row), flush=True)


def run(tree):
    """one measuring process in `tree`; a failing worker ends the comparison"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree], cwd=tree, capture_output=True,
                         text=True, timeout=900)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit(f"worker in {tree} ended with {out.returncode}: nothing more is started")
    return [json.loads(l[4:]) for l in out.stdout.splitlines() if l.startswith("ROW ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit, built in place")
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.tree))
    runs = {"new": [], "parent": []}
    for k in range(args.runs):  # alternating
        runs["new"].append(run(ROOT))
        print(f"run {k + 1}: this tree done", flush=True)
        if args.parent:
            runs["parent"].append(run(os.path.abspath(args.parent)))
            print(f"run {k + 1}: parent done", flush=True)
    lines = []

    def series(which, k, what):
        vals = [r[k][what] for r in runs[which]]
        return f"{'  '.join(f'{v:.4f}' for v in vals)}   (min {min(vals):.4f}, max {max(vals):.4f})", vals

    for k, first in enumerate(runs["new"][0]):
        lines.append(f"{first['workload']} / {first['input']}   (tokens_dist, words_dist, n_tokens, n_words) = {tuple(first['counts'])}")
        got = {}
        if args.parent:
            text, got["parent viterbi"] = series("parent", k, "viterbi")
            lines.append(f"  parent viterbi(x)               ms per call: {text}")
        for what, label in (("viterbi", "viterbi(x)"), ("errors", "errors(x, targets, counter)"), ("counter(viterbi)", "counter(viterbi(x), targets)")):
            text, got[what] = series("new", k, what)
            lines.append(f"  {label:<30}  ms per call: {text}")
        if args.parent:
            e, p = got["errors"], got["parent viterbi"]
            verdict = "every run of errors() is faster than every run of" if max(e) < min(p) else (
                "every run of errors() is SLOWER than every run of" if min(e) > max(p) else "errors() is within the spread of")
            lines.append(f"  -> {verdict} the parent's bare viterbi() (medians {sorted(e)[len(e) // 2]:.4f} vs {sorted(p)[len(p) // 2]:.4f} ms)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
