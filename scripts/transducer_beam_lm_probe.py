"""Per-call time of Transducer.beam_search with a token-level n-gram LM beside the same search without one, at the
decode shape of scripts/transducer_beam_probe.py (B=128, T=1000) over the 1000 word pieces of
benchmarks/word_pieces_tokens_1000.txt and the blank (C=1001), on a GPU.

    python scripts/transducer_beam_lm_probe.py           beam widths 1, 16, 64 at 32 classes per frame, both inputs, both graphs
    python scripts/transducer_beam_lm_probe.py --config 16,32 --input noise --only forced --calls 3 --warmup 1
        one configuration only: the target of a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/transducer_beam_lm_probe.py --config ...
        (scripts/kstats.py prints the averages; the LM call's beam launch is beam_search_kernel<NT, wfl::BeamTokLm>, the
        plain call's beam_search_kernel<NT, wfl::BeamTok>)

The criteria are Transducer(the 1000 pieces, blank last) with the bigram transition model (ngram=2, parameters 0.1 N(0,1))
in both searched token graphs -- blank="optional" without repeats and blank="forced".  Inputs: scripts/beam_probe.py's
(white noise; emissions peaked on a random alignment).  The LM is a seeded random trigram over the 1000 pieces, written
as ARPA text and read by Transducer.token_lm: every unigram, `--keep` of the bigrams, and of the trigrams whose parts are
in the file.  lm_weight 0.8, length_bonus 0.5, </s> scored.

The two calls alternate in one process -- plain, LM, plain, LM, ... -- so that clocks and neighbours drift under both
alike; a call ends on the host with its results, so the host clock around it is its time.  Reported per call form: the
median over all timed calls, and the spread (min, max); beside the ratio, CTC's LM-to-plain ratio at the same (W, K, input)
from profiles/beam_search_lm.txt.  Results: profiles/transducer_beam_search_lm.txt."""
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
from gtn_applications_amd.criterions.transducer import Transducer  # noqa: E402

KINDS = {"optional": dict(blank="optional", allow_repeats=False), "forced": dict(blank="forced")}
# profiles/beam_search_lm.txt, section 1: CTC.beam_search(lm=) / CTC.beam_search() at B=128, T=1000, C=100
CTC_RATIO = {("noise", 1, 32): 1.03, ("noise", 16, 32): 1.00, ("noise", 64, 32): 1.32,
             ("peaked", 1, 32): 1.08, ("peaked", 16, 32): 3.34, ("peaked", 64, 32): 1.60}


def pieces(n):
    """(tokens, grapheme -> index): the benchmark's word pieces for n = 1000, n single-grapheme tokens otherwise"""
    if n == 1000:
        with open(os.path.join(ROOT, "benchmarks", "word_pieces_tokens_1000.txt")) as f:
            tokens = sorted(l.rstrip("\n") for l in f if l.rstrip("\n"))
    else:
        tokens = [chr(0x100 + i) for i in range(n)]
    return tokens, {g: i for i, g in enumerate(sorted(set(c for t in tokens for c in t)))}


def random_trigram_text(tokens, keep, seed):
    """ARPA text over `tokens`: every unigram, each bigram / trigram (whose history and suffix are in the file) with
    probability `keep`; log10 weights in [-3, -0.1], back-offs in [-1, 0]"""
    rs = np.random.RandomState(seed)
    words = list(tokens) + ["</s>"]
    levels = [[("<s>",)] + [(w,) for w in words]]
    for _ in (2, 3):
        prev = set(levels[-1])
        level = []
        for h in levels[-1]:
            if h[-1] == "</s>":
                continue
            picked = np.nonzero(rs.rand(len(words)) < keep)[0]  # (one draw per history: a million pairs at 1000 pieces)
            level += [h + (words[i],) for i in picked if h[1:] + (words[i],) in prev]
        levels.append(level)
    lines = ["\\data\\"] + [f"ngram {n + 1}={len(level)}" for n, level in enumerate(levels)] + [""]
    for n, level in enumerate(levels):
        lines.append(f"\\{n + 1}-grams:")
        for g in level:
            bo = f"\t{-rs.rand():.6f}" if n < 2 and g[-1] != "</s>" else ""
            lines.append(f"{-0.1 - 2.9 * rs.rand():.6f}\t{' '.join(g)}{bo}")
        lines.append("")
    return "\n".join(lines + ["\\end\\", ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--tokens", type=int, default=1000)
    ap.add_argument("--configs", default="1,32 16,32 64,32", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="both", choices=["both"] + list(KINDS), help="which token graph")
    ap.add_argument("--form", default="both", choices=["both", "lm", "plain"], help="which call form (for a kernel trace)")
    ap.add_argument("--keep", type=float, default=0.005)
    ap.add_argument("--calls", type=int, default=15, help="timed calls of each form")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "transducer_beam_lm_probe needs a GPU"
    tokens, g2i = pieces(a.tokens)
    C, blank = a.tokens + 1, a.tokens
    crits = {}
    for name, kw in KINDS.items():
        if a.only in ("both", name):
            crit = Transducer(tokens, g2i, ngram=2, **kw).cuda()
            with torch.no_grad():
                n = crit.transition_params.numel()
                crit.transition_params.copy_(torch.from_numpy((0.1 * np.random.RandomState(1).randn(n)).astype(np.float32)))
            crits[name] = crit
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.arpa")
        with open(path, "w") as f:
            f.write(random_trigram_text(tokens, a.keep, seed=1))
        lm = next(iter(crits.values())).token_lm(path)
    lm.on_device("cuda")
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    data = {k: v for k, v in inputs(a.B, a.T, C, blank).items() if a.input in ("both", k)}
    print(f"B={a.B} T={a.T} C={C} blank={blank}; bigram transitions; LM order {lm.order}: {lm.num_states} states, "
          f"{lm.num_arcs} arcs; {a.warmup} warm-up + {a.calls} alternating timed calls of each form; ms per call: median (min .. max)")
    for name, x in data.items():
        for kind, crit in crits.items():
            for W, K in configs:
                forms = {"plain": lambda: crit.beam_search(x, beam_size=W, classes_per_frame=K),
                         "lm": lambda: crit.beam_search(x, beam_size=W, classes_per_frame=K, token_lm=lm, lm_weight=0.8,
                                                        length_bonus=0.5)}
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
                line = f"{name:7s} {kind:8s} W={W:2d} K={K:2d}  " + "   ".join(
                    f"{k:5s} {statistics.median(v):8.3f} ({min(v):8.3f} .. {max(v):8.3f})" for k, v in ms.items())
                if len(forms) == 2:
                    differ = sum(p.tolist() != q.tolist() for p, q in zip(results["plain"], results["lm"]))
                    ctc = CTC_RATIO.get((name, W, K))
                    line += f"   lm / plain {statistics.median(ms['lm']) / statistics.median(ms['plain']):5.2f}" \
                            f"   (CTC's: {'%.2f' % ctc if ctc else 'not measured'}; best differs in {differ} of {a.B})"
                print(line, flush=True)


if __name__ == "__main__":
    main()
