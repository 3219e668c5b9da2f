"""Bit-for-bit A/B of the lattice engine between two builds of libwfl.so (GPU; seconds per case).

    python scripts/lattice_ab_bits.py --parent /path/to/parent/libwfl.so [--out profiles/tail_layout_ab_bits.txt]

For each case a fresh child process per build (WFL_LIB_PATH; the parent's library must carry the soname libwfl.so so that
the C++ operators bind to it too), each under its own time limit; the first child that fails ends the run.  The parent
runs twice: where it reproduces its own bytes the new build must match them, where it does not (atomic accumulation
order) the table says so and the RESULT line names the fields: this script does not check them, the suite's parity tests
against the float64 oracle are their bar.  Compared: loss, log Z, sweep formats, dx (and the gradient of learnable weights;
the best paths and their scores in the tropical case) -- a child that cannot get at one of them fails.  Inputs: the case
builders of the tests named in CASES."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
# name: (what it reaches, environment of the child)
CASES = {
    "a_asg_banded": ("banded probability sweep, band_grad_kernel: ASG force alignment B=3 T=40 C=9", {}),
    "b_transducer_nested_T48": ("256-thread sweeps, gradient beside them: test_gpu_transducer_modes 'nested', T=48", {}),
    "c_transducer_nested_T96_mitm": ("the same, meeting in the middle: T=96", {"WFL_LATTICE_MITM": "2"}),
    "d_backoff_bigram": ("general probability sweep, certificate: test_gpu_ngram back-off fixture B=2 T=30", {}),
    "e_ctc_260_labels": ("CTC target of 260 labels through the lattice engine B=2 T=300 C=20", {}),
    "f_ctc_260_labels_log": ("case e in the log domain", {"WFL_LATTICE_DOMAIN": "log"}),
    "g1_backoff_streamed_lds": ("case d, streamed sweeps, states in LDS", {"WFL_LATTICE_STREAMED": "1"}),
    "g2_backoff_streamed_global": ("case d, streamed sweeps, states in global memory", {"WFL_LATTICE_STREAMED": "2"}),
    "h_asg_tropical": ("tropical sweep and backtrace: case a", {}),
}


def _engine_case(name):
    import numpy as np
    import torch

    from gtn_applications_amd import engine as E

    rs = np.random.RandomState(11)
    if name.startswith(("a_", "h_")):
        B, T, C, lens = 3, 40, 9, (7, 1, 12)
        pack_of = lambda tg, dev: E.PackedLattice.asg_force_align(tg.flat, tg.offsets, C, dev)  # noqa: E731
    else:
        B, T, C, lens = 2, 300, 20, (260, 40)
        pack_of = lambda tg, dev: E.PackedLattice.ctc(tg.flat, tg.offsets, C - 1, C, dev)  # noqa: E731
    x = torch.tensor(rs.randn(B, T, C).astype(np.float32), device="cuda")
    targets = [rs.randint(0, C - 1, size=n).tolist() for n in lens]
    pack = pack_of(E.targets_on_device(targets, x.device), x.device)
    if name.startswith("h_"):
        paths, scores = E.lattice_viterbi(x, pack)
        return {"logz": scores.cpu().numpy(), "paths": np.concatenate([[-2] if p is None else np.append(p, -1) for p in paths])}
    st = E.lattice_forward(x, pack, log_softmax=True)
    fmt = E.lattice_formats(st).cpu().numpy()
    dx = torch.zeros_like(x)
    coef = torch.full((B,), 1.0 / B, device="cuda")
    E.lattice_grad(st, coef, dx=dx)
    return {"loss": -st.logz.sum().cpu().numpy(), "logz": st.logz.cpu().numpy(), "fmt": fmt, "dx": dx.cpu().numpy()}


def _criterion_case(name):
    import numpy as np
    import torch

    from gtn_applications_amd import engine as E

    if name[0] in "bc":
        import test_gpu_transducer_modes as TM

        T = 48 if name[0] == "b" else 96
        targets = TM._random_targets(TM.SETS["nested"][1], (T - 4, T - 8), 4)
        crit = TM._criterion("nested", "optional", "mean")
        C = len(TM.SETS["nested"][0]) + 1
        x = np.random.RandomState(4).randn(len(targets), T, C).astype(np.float32)
    else:
        from gtn_applications_amd import graph as G
        from gtn_applications_amd.criterions import transducer as TR

        lit = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_literals.json")))["backoff_transitions"]
        N, T, B = lit["N"], 30, 2
        g = G.Graph(True)
        for n in range(8):
            g.add_node(n in lit["start"], n in lit["accept"])
        for a in lit["arcs"]:
            g.add_arc(*a)
        rs = np.random.RandomState(5)
        crit = TR.Transducer([(n,) for n in range(N)], {n: n for n in range(N)}, blank="optional", allow_repeats=False,
                             transitions=g, reduction="mean")
        x = rs.randn(B, T, N + 1).astype(np.float32)
        targets = [rs.randint(0, N, size=rs.randint(5, 12)).tolist() for _ in range(B)]
        with torch.no_grad():
            crit.transition_params.copy_(torch.from_numpy((0.3 * rs.randn(crit.transition_params.numel())).astype(np.float32)))
        crit.cuda()
        crit.tokens.arc_sort(True)
    xg = torch.tensor(x, device="cuda", requires_grad=True)
    tt = [torch.tensor(t) for t in targets]
    if name[0] in "bc":
        loss, sides = crit(xg, tt), ("num",)
    else:  # the general lattice path for numerator and denominator (test_gpu_ngram: none of the module's short cuts)
        loss = TR.TransducerLossFunction.apply(xg, tt, crit.tokens, crit.lexicon, crit.transition_params, crit.transitions,
                                               crit.reduction)
        sides = ("num", "den")
    out = {}
    for side in sides:  # the sweeps' states: the step must have kept them
        st = getattr(loss.grad_fn.aux, side)
        torch.cuda.synchronize()
        out[side + "_logz"] = st.logz.detach().cpu().numpy().copy()
        out[side + "_fmt"] = E.lattice_formats(st).cpu().numpy().copy()
    loss.backward()
    out["loss"], out["dx"] = loss.detach().cpu().numpy(), xg.grad.cpu().numpy()
    tp = getattr(crit, "transition_params", None)
    if tp is not None and tp.grad is not None:
        out["dparams"] = tp.grad.cpu().numpy()
    return out


def child(name, dump):
    import numpy as np

    out = _engine_case(name) if name[0] in "aefh" else _criterion_case(name)
    np.savez(dump, **{k: np.ascontiguousarray(v) for k, v in out.items()})


def digests(path):
    import numpy as np

    with np.load(path) as z:
        return {k: hashlib.sha256(z[k].tobytes()).hexdigest()[:16] + f" {z[k].dtype}{list(z[k].shape)}" for k in z.files}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libwfl.so built from the parent commit (soname libwfl.so); required but for --child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--child", default=None)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.dump)
    if not a.parent or not os.path.exists(a.parent):
        ap.error("--parent: the library built from the parent commit is required")
    lines = ["case | what | parent reproduces itself | new == parent | fields (sha256/16, dtype, shape; * = differs)"]
    ok, unchecked = True, []
    for name, (what, env) in CASES.items():
        got = {}
        for tag, lib in (("parent1", a.parent), ("parent2", a.parent), ("new", None)):
            e = dict(os.environ, **env)
            e.pop("WFL_LIB_PATH", None)
            if lib:
                e["WFL_LIB_PATH"] = os.path.abspath(lib)
            dump = os.path.join(a.tmp, f"ab_{name}_{tag}.npz")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--dump", dump], env=e, cwd=ROOT,
                                   timeout=a.limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                print(f"{name} / {tag}: child killed at its time limit of {a.limit} s", flush=True)
                return 3
            if r.returncode != 0:  # nothing more is started; 1: a Python error of the child, 2: anything else (a fault on the device)
                print(f"{name} / {tag}: child failed with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
                return 1 if r.returncode == 1 else 2
            got[tag] = digests(dump)
        same = {k: got["parent1"][k] == got["parent2"][k] for k in got["parent1"]}
        match = {k: got["new"].get(k) == got["parent1"][k] for k in got["parent1"]}
        held = all(match[k] for k in same if same[k]) and set(got["new"]) == set(got["parent1"])
        ok = ok and held
        unchecked += [f"{name}:{k}" for k in same if not same[k]]
        fields = "; ".join(f"{k} {got['new'].get(k)}" + ("" if match[k] else " *") + ("" if same[k] else " (parent differs from itself)")
                           for k in got["parent1"])
        lines.append(f"{name} | {what} | {'yes' if all(same.values()) else 'NO: ' + ','.join(k for k in same if not same[k])} | "
                     f"{'yes' if all(match.values()) else 'NO: ' + ','.join(k for k in match if not match[k])} | {fields}")
        print(lines[-1], flush=True)
    lines.append("RESULT: " + ("the new build matches the parent's bytes wherever the parent reproduces its own" if ok
                               else "MISMATCH where the parent reproduces itself"))
    lines.append("NOT CHECKED HERE (the parent differs from itself; bar: the suite's parity tests against the float64 oracle): "
                 + (", ".join(unchecked) or "nothing"))
    print(lines[-2])
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
