"""The ASG prefix beam search with a token-level n-gram LM and a length bonus (include/wfl.h: wfl_asg_beam_search_lm;
DESIGN.md section 29) restated in plain Python, as tests/asg_beam_reference.py restates the ASG search and
tests/beam_lm_reference.py the CTC search with an LM: float64, tuples for prefixes, one utterance at a time.  Nothing
here uses gtn_applications_amd.lm or its packed acceptor: the LM is beam_lm_reference.ArpaLM over the N tokens (token i
is label i, built with blank = N), walked by the textbook back-off rule.

The LM reads exactly what the mapped write launch emits -- asg_beam_reference.unpack(raw, garbage, R) --, one raw class
at a time: a hypothesis carries (LM history, rep), rep the token a replabel right behind the prefix would repeat or -1.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after </s> up to the first one not
returned -- and the number of merged extensions."""
from asg_beam_reference import search, unpack
from beam_lm_reference import EOS
from beam_reference import NEG


def emitted(rep, c, garbage, R):
    """rule 1: (the LM labels raw class c emits behind a prefix with `rep`, rep behind it)"""
    if garbage is not None and c == garbage:
        return [], rep
    if c >= R:
        return [c - R], c - R
    if rep >= 0:
        return [rep] * (c + 1), -1
    return [], -1  # (a replabel at the start or behind another replabel: the write launch emits nothing either)


def rules(lm, alpha, beta, score_eos, garbage, R):
    """(start, extend, finish) for asg_beam_reference.search: the state is (LM history, rep)"""

    def extend(state, pre, c):  # rules 1 and 2
        hist, rep = state
        labels, rep = emitted(rep, c, garbage, R)
        term = 0.0
        for u in labels:
            l, hist = lm.step(hist, u)
            if l == NEG:
                return None
            term = term + (alpha * l + beta)
        return term, (hist, rep)

    def finish(state, s):  # rule 4
        if score_eos:
            l, _ = lm.step(state[0], EOS)
            if l == NEG:
                return None
            s += alpha * l
        return s

    return (lm.start, -1), extend, finish


def beam_search(x, Wt, W, K, nbest, lm, alpha, beta, score_eos, garbage, R, logz=None, on_frame=None):
    """asg_beam_reference.beam_search with the additions of section 29.  lm: an ArpaLM over the N = C - R - (garbage is
    not None) tokens; garbage: the garbage class or None; R: the number of replabels.  Returns (hyps, margin, merges):
    hyps = nbest pairs (raw class tuple, score), the score minus logz if given; ranks beyond what is left after the last
    frame are ((), -inf).  on_frame(t, beam, cand, extension, merged, entries): called in every frame with the ranked
    beam [(prefix, p, history, rep)], the candidates, the extension function, the merged flags and the sorted entries --
    for a test that has to know a situation occurred."""
    return search(x, Wt, W, K, nbest, *rules(lm, alpha, beta, score_eos, garbage, R), logz=logz, on_frame=on_frame)


def frame_bound(beam, cand, extension, merged, entries, W):
    """rule 7: the bound of a frame as the kernel forms it -- the W-th best of one key per hypothesis of a full beam: its
    stay entry (merged extension included: what `entries` holds) or, where its last label is no candidate, its first own
    extension with its real term, -inf where that does not exist; -inf for a beam that is not full"""
    if len(beam) < W:
        return NEG
    classes = [c for c, _ in cand]
    stays = {e[1]: e[0] for e in entries if e[1] < len(beam)}
    keys = []
    for i, h in enumerate(beam):
        pre = h[0]
        if pre and pre[-1] in classes:
            keys.append(stays.get(i, NEG))
            continue
        own = [c for q, c in enumerate(classes) if not merged[i][q]]
        keys.append(extension(i, own[0])[0] if own else NEG)
    return sorted(keys, reverse=True)[W - 1]


def brute_force(x, Wt, lm, alpha, beta, score_eos, garbage, R):
    """[(raw class tuple, score)] by rule 5, never through the frame loop: asg_beam_reference.brute_force's mass of every
    collapsed raw sequence over all C^T frame paths, re-scored with alpha lm.score(unpack(l)) + beta len(unpack(l)) (the
    </s> term inside lm.score); a sequence the LM cannot follow is left out; best first (ties: the sequence that sorts
    first)"""
    from asg_beam_reference import brute_force as masses

    out = []
    for pre, mass in masses(x, Wt):
        if mass == NEG:
            continue
        mapped = unpack(pre, garbage, R)
        l = lm.score(mapped, eos=score_eos)
        if l == NEG:
            continue
        out.append((pre, mass + alpha * l + beta * len(mapped)))
    return sorted(out, key=lambda e: (-e[1], e[0]))
