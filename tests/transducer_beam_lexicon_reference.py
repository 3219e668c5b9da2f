"""The Transducer prefix beam search with a lexicon and a word-level n-gram LM (include/wfl.h:
wfl_transducer_beam_search_lexicon) restated in plain Python, as tests/transducer_beam_reference.py
restates the Transducer search and tests/beam_lexicon_reference.py the CTC search with a lexicon: float64, tuples for
prefixes, one utterance at a time.  Nothing here uses gtn_applications_amd.lexicon or its packed trie: the lexicon is a
dict from token tuple to word id, the position inside a word is the tuple of tokens since the last word end, checked
against the set of the spellings' proper prefixes, and the LM is beam_lm_reference.ArpaLM over word ids (word v is label
v, the blank is V) or None.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after the final drop and </s> up to the
first one not returned -- and the number of merged extensions."""
from beam_lexicon_reference import lexicon_rules, segment
from beam_lm_reference import EOS
from beam_reference import NEG, search


def beam_search(x, Wt, blank, forced, W, K, nbest, lexicon, lm, alpha, omega, beta, score_eos, logz=None, on_frame=None):
    """transducer_beam_reference.beam_search with the additions of section 25.  lexicon: {token tuple: word id},
    prefix-free; lm: an ArpaLM over word ids or None.  Returns (hyps, margin, merges): hyps = nbest pairs (token tuple,
    score), the score minus logz if given; ranks beyond what is left after the last frame are ((), -inf).
    on_frame(t, beam, cand, extension, merged, entries): called in every frame with the ranked beam [(prefix, pb, pnb,
    part, history)], the candidates, the extension function, the merged flags and the sorted live entries -- for a test
    that has to know a situation occurred."""
    rules = lexicon_rules(lexicon, lm, alpha, omega, beta, score_eos)
    return search(x, blank, W, K, nbest, *rules, Wt=Wt, forced=forced, logz=logz, on_frame=on_frame)


def brute_force(x, Wt, blank, forced, lexicon, lm, alpha, omega, beta, score_eos):
    """[(token tuple, score)] by rule 6: transducer_beam_reference.brute_force's mass of every token sequence over all
    C^T frame paths the token graph accepts, those kept that segment into lexicon words, re-scored with alpha LM(words) +
    omega #words + beta #tokens and the </s> term; best first"""
    from transducer_beam_reference import brute_force as masses

    out = []
    for pre, mass in masses(x, Wt, blank, forced):
        at = segment(lexicon, pre)
        if at is None or at[1] or mass == NEG:
            continue
        words = at[0]
        s = mass + omega * len(words) + beta * len(pre)
        if lm:
            hist, total, dead = lm.start, 0.0, False
            for v in words + ([EOS] if score_eos else []):
                l, hist = lm.step(hist, v)
                if l == NEG:
                    dead = True
                    break
                total += l
            if dead:
                continue
            s += alpha * total
        out.append((pre, s))
    return sorted(out, key=lambda e: (-e[1], e[0]))
