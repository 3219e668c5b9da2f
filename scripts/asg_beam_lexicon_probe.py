"""Per-call time of ASG.beam_search with a lexicon and a word-level n-gram LM beside the plain ASG.beam_search and beside
CTC.beam_search(lexicon=) on the same emissions, at the benchmark's decode shape (B=128, T=1000, 100 classes), on a GPU.

    python scripts/asg_beam_lexicon_probe.py              beam widths 1, 16, 64 at 32 classes per frame, both inputs
    python scripts/asg_beam_lexicon_probe.py --config 16,32 --input noise --only lexicon --calls 3 --warmup 1
        one configuration, one call form: the target of a kernel trace in a run of its own,
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/asg_beam_lexicon_probe.py --config ...
        (the lexicon call's beam launch is beam_search_kernel<NT, wfl::BeamAsgLex>, the plain one's <NT, wfl::BeamAsg>)

The criterion is ASG(97 tokens, 2 replabels, garbage): 100 raw classes, the garbage last; transitions 0.1 N(0,1).
Lexicon: scripts/beam_lexicon_probe.py's -- `--words` seeded random words of 1 to 4 of the 96 letters, each ending in
the separator token 96 --, built by ASG.lexicon (so doubled letters are spelled with replabels); the CTC call takes the
same trie with the blank where ASG has its garbage.  Word LM: that script's seeded random trigram.  lm_weight 0.8,
word_bonus 0.6, length_bonus 0.3, </s> scored.  Inputs: white noise N(0,1), and emissions peaked (+8) on an alignment
that spells 30 lexicon words in raw classes with the garbage between the runs.

The three calls alternate in one process -- plain, lexicon, CTC lexicon, plain, ... -- so that clocks and neighbours
drift under all alike; a call ends on the host with its results, so the host clock around it is its time.  Reported per
call form: the median over all timed calls and the spread (min .. max); for the ASG lexicon call also the number of
utterances that decode to at least one word.  Results: profiles/asg_beam_search_lexicon.txt."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gtn_applications_amd.criterions.asg import ASG  # noqa: E402
from gtn_applications_amd.criterions.ctc import CTC  # noqa: E402
from scripts.beam_lexicon_probe import random_word_trigram  # noqa: E402


def random_words(letters, V, seed):
    rs = np.random.RandomState(seed)
    words = set()
    while len(words) < V:
        words.add(tuple(int(i) for i in rs.randint(letters, size=1 + rs.randint(4))))
    return sorted(words)


def spelled(B, T, C, garbage, lex, seed):
    """emissions peaked on an alignment of 30 lexicon words per utterance in raw classes: every class on a run of frames
    of its own, garbage frames between the runs, +8 on white noise"""
    rs = np.random.RandomState(seed)
    x = rs.randn(B, T, C).astype(np.float32)
    for b in range(B):
        labels = [c for v in rs.randint(lex.num_words, size=30) for c in lex.spellings[v]]
        cuts = np.sort(rs.choice(np.arange(1, T), size=2 * len(labels), replace=False))
        frames = np.full(T, garbage)
        for i, lab in enumerate(labels):
            frames[cuts[2 * i]:cuts[2 * i + 1]] = lab
        x[b, np.arange(T), frames] += 8.0
    return torch.from_numpy(x).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--configs", default="1,32 16,32 64,32", help="beam,classes pairs")
    ap.add_argument("--config", default=None, help="one beam,classes pair (for a kernel trace)")
    ap.add_argument("--input", default="both", choices=["both", "noise", "peaked"])
    ap.add_argument("--only", default="all", choices=["all", "plain", "lexicon", "ctc"], help="one call form (for a kernel trace)")
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--keep", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=15, help="timed calls of each form")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "asg_beam_lexicon_probe needs a GPU"
    asg = ASG(97, num_replabels=2, use_garbage=True).cuda()
    C, garbage = asg.N, asg.garbage_idx
    with torch.no_grad():
        asg.transitions.copy_(torch.from_numpy((0.1 * np.random.RandomState(1).randn(C + 1, C)).astype(np.float32)))
    ctc = CTC(blank=garbage, use_pt=False)
    lex = asg.lexicon(random_words(96, a.words, seed=2), list(range(97)), wordsep=96, split=list)
    assert (lex.num_classes, lex.blank) == (C, garbage)  # (the CTC call takes the same trie: its blank is the garbage)
    word_lm = random_word_trigram(a.words, a.keep, seed=3)
    for pack in (lex, word_lm):
        pack.on_device("cuda")
    configs = [tuple(int(v) for v in c.split(",")) for c in ([a.config] if a.config else a.configs.split())]
    noise = torch.from_numpy(np.random.RandomState(0).randn(a.B, a.T, C).astype(np.float32)).cuda()
    data = {"noise": noise, "peaked": spelled(a.B, a.T, C, garbage, lex, seed=4)}
    data = {k: v for k, v in data.items() if a.input in ("both", k)}
    print(f"B={a.B} T={a.T} C={C} garbage = blank = {garbage}; lexicon: {lex.num_words} words, {lex.num_nodes} nodes, "
          f"{lex.num_arcs} arcs; word LM order {word_lm.order}: {word_lm.num_states} states, {word_lm.num_arcs} arcs; "
          f"{a.warmup} warm-up + {a.calls} alternating timed calls of each form; ms per call: median (min .. max)")
    opts = dict(lexicon=lex, lm=word_lm, lm_weight=0.8, word_bonus=0.6, length_bonus=0.3)
    for name, x in data.items():
        for W, K in configs:
            forms = {"plain": lambda: asg.beam_search(x, beam_size=W, classes_per_frame=K),
                     "lexicon": lambda: asg.beam_search(x, beam_size=W, classes_per_frame=K, **opts),
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
                f"{k:7s} {statistics.median(v):8.3f} ({min(v):8.3f} .. {max(v):8.3f})" for k, v in ms.items())
            if "lexicon" in forms:
                line += f"   (words in {sum(len(p) > 0 for p in results['lexicon'])} of {a.B})"
                for k in ("plain", "ctc"):
                    if k in forms:
                        line += f"   lexicon / {k} {statistics.median(ms['lexicon']) / statistics.median(ms[k]):5.2f}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
