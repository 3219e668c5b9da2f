"""The Transducer prefix beam search with a token-level n-gram LM and a length bonus (include/wfl.h:
wfl_transducer_beam_search_lm) restated in plain Python, as tests/transducer_beam_reference.py
restates the Transducer search and tests/beam_lm_reference.py the CTC search with an LM: float64, tuples for prefixes,
one utterance at a time.  Nothing here uses gtn_applications_amd.lm or its packed acceptor: the LM is
beam_lm_reference.ArpaLM over class labels, walked by the textbook back-off rule.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after the topology's drop and </s> up to
the first one not returned -- and the number of merged extensions."""
from beam_lm_reference import EOS, token_lm_rules
from beam_reference import NEG, search


def beam_search(x, Wt, blank, forced, W, K, nbest, lm, alpha, beta, score_eos, logz=None, on_frame=None):
    """transducer_beam_reference.beam_search with the additions of section 28.  lm: an ArpaLM over the classes.  Returns
    (hyps, margin, merges): hyps = nbest pairs (token tuple, score), the score minus logz if given; ranks beyond what is
    left after the last frame are ((), -inf).  on_frame(t, beam, cand, extension, merged, entries): called in every
    frame with the ranked beam [(prefix, pb, pnb, history)], the candidates, the extension function, the merged flags
    and the sorted live entries -- for a test that has to know a situation occurred."""
    rules = token_lm_rules(lm, alpha, beta, score_eos)
    return search(x, blank, W, K, nbest, *rules, Wt=Wt, forced=forced, logz=logz, on_frame=on_frame)


def brute_force(x, Wt, blank, forced, lm, alpha, beta, score_eos):
    """[(token tuple, score)]: transducer_beam_reference.brute_force's mass of every token sequence over all C^T frame
    paths the token graph accepts, re-scored with alpha LM(tokens) + beta #tokens and the </s> term; a sequence the LM
    cannot follow is left out; best first (ties: the sequence that sorts first)"""
    from transducer_beam_reference import brute_force as masses

    out = []
    for pre, mass in masses(x, Wt, blank, forced):
        if mass == NEG:
            continue
        hist, total, dead = lm.start, 0.0, False
        for c in list(pre) + ([EOS] if score_eos else []):
            l, hist = lm.step(hist, c)
            if l == NEG:
                dead = True
                break
            total += l
        if dead:
            continue
        out.append((pre, mass + alpha * total + beta * len(pre)))
    return sorted(out, key=lambda e: (-e[1], e[0]))
