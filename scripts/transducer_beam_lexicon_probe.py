"""Per-call time of Transducer.beam_search with a lexicon and a word-level n-gram LM, in both searched token graphs,
beside the plain Transducer.beam_search and beside CTC.beam_search(lexicon=) on the same emissions, at the benchmark's
decode shape (B=128, T=1000, C=101: 100 single-grapheme tokens and the blank), on a GPU.

    python scripts/transducer_beam_lexicon_probe.py       beam widths 1, 16, 64 at 32 classes per frame, both inputs
    python scripts/transducer_beam_lexicon_probe.py --config 16,32 --input peaked --only optional --calls 3 --warmup 1
        one configuration, one call form: the target of a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/transducer_beam_lexicon_probe.py --config ...
        (the lexicon calls' beam launch is beam_search_kernel<NT, wfl::BeamTokLex>, the plain one's <NT, wfl::BeamTok>, the
        CTC one's <NT, wfl::BeamLex>)

The criteria are Transducer(100 single-grapheme tokens, blank last) with the bigram transition model (ngram=2,
parameters 0.1 N(0,1): scripts/transducer_beam_probe.py's) with blank="optional" without repeats and with
blank="forced".  Lexicon: scripts/beam_lexicon_probe.py's -- `--words` seeded random words of 1 to 4 of the 99 letters,
each ending in the separator token 99 --, built by Transducer.word_lexicon; the CTC call takes the same trie (blank
100).  Word LM: that script's seeded random trigram.  lm_weight 0.8, word_bonus 0.6, length_bonus 0.3, </s> scored.
Inputs: white noise N(0,1), and emissions peaked (+8) on an alignment that spells 30 lexicon words, every token on a run
of frames of its own with blank frames between the runs (an alignment of both token graphs).

The call forms alternate in one process -- plain, optional, forced, ctc, plain, ... -- so that clocks and neighbours
drift under all alike; a call ends on the host with its results, so the host clock around it is its time.  Reported per
call form: the median over all timed calls and the spread (min .. max); for the lexicon calls also the number of
utterances that decode to at least one word.  Results: profiles/transducer_beam_search_lexicon.txt."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gtn_applications_amd.criterions.ctc import CTC  # noqa: E402
from gtn_applications_amd.criterions.transducer import Transducer  # noqa: E402
from scripts.beam_lexicon_probe import random_word_trigram, spelled  # noqa: E402

KINDS = {"optional": dict(blank="optional", allow_repeats=False), "forced": dict(blank="forced")}


def random_words(tokens, V, seed):
    """V different words of 1 to 4 of the tokens but the last (the separator), as strings"""
    rs = np.random.RandomState(seed)
    words = set()
    while len(words) < V:
        words.add("".join(tokens[i] for i in rs.randint(len(tokens) - 1, size=1 + rs.randint(4))))
    return sorted(words)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--configs", default="1,32 16,32 64,32", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="all", choices=["all", "plain", "optional", "forced", "ctc"],
                    help="one call form (for a kernel trace)")
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--keep", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=15, help="timed calls of each form")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "transducer_beam_lexicon_probe needs a GPU"
    tokens = [chr(0x100 + i) for i in range(100)]
    g2i = {t: i for i, t in enumerate(tokens)}
    C, blank = 101, 100
    crits = {}
    for kind, kw in KINDS.items():
        crit = Transducer(tokens, g2i, ngram=2, **kw).cuda()
        with torch.no_grad():
            n = crit.transition_params.numel()
            crit.transition_params.copy_(torch.from_numpy((0.1 * np.random.RandomState(1).randn(n)).astype(np.float32)))
        crits[kind] = crit
    ctc = CTC(blank=blank, use_pt=False)
    lex = crits["optional"].word_lexicon(random_words(tokens, a.words, seed=2), wordsep=tokens[-1])
    assert (lex.num_classes, lex.blank) == (C, blank)
    word_lm = random_word_trigram(a.words, a.keep, seed=3)
    for pack in (lex, word_lm):
        pack.on_device("cuda")
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    noise = torch.from_numpy(np.random.RandomState(0).randn(a.B, a.T, C).astype(np.float32)).cuda()
    data = {"noise": noise, "peaked": spelled(a.B, a.T, C, blank, lex, seed=4)}
    data = {k: v for k, v in data.items() if a.input in ("both", k)}
    print(f"B={a.B} T={a.T} C={C} blank = {blank}; lexicon: {lex.num_words} words, {lex.num_nodes} nodes, "
          f"{lex.num_arcs} arcs; word LM order {word_lm.order}: {word_lm.num_states} states, {word_lm.num_arcs} arcs; "
          f"{a.warmup} warm-up + {a.calls} alternating timed calls of each form; ms per call: median (min .. max)")
    opts = dict(lexicon=lex, lm=word_lm, lm_weight=0.8, word_bonus=0.6, length_bonus=0.3)
    for name, x in data.items():
        for W, K in configs:
            forms = {"plain": lambda: crits["optional"].beam_search(x, beam_size=W, classes_per_frame=K),
                     "optional": lambda: crits["optional"].beam_search(x, beam_size=W, classes_per_frame=K, **opts),
                     "forced": lambda: crits["forced"].beam_search(x, beam_size=W, classes_per_frame=K, **opts),
                     "ctc": lambda: ctc.beam_search(x, beam_size=W, classes_per_frame=K, **opts)}
            forms = {k: f for k, f in forms.items() if a.only in ("all", k)}
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
                f"{k:8s} {statistics.median(v):8.3f} ({min(v):8.3f} .. {max(v):8.3f})" for k, v in ms.items())
            for kind in KINDS:
                if kind in forms:
                    line += f"   ({kind}: words in {sum(len(p) > 0 for p in results[kind])} of {a.B}"
                    for k in ("plain", "ctc"):
                        if k in forms:
                            line += f", / {k} {statistics.median(ms[kind]) / statistics.median(ms[k]):5.2f}"
                    line += ")"
            print(line, flush=True)


if __name__ == "__main__":
    main()
