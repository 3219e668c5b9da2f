"""The ASG prefix beam search with a lexicon and a word-level n-gram LM (include/wfl.h: wfl_asg_beam_search_lexicon;
DESIGN.md section 24) restated in plain Python, as tests/asg_beam_reference.py restates the ASG search and
tests/beam_lexicon_reference.py the CTC search with a lexicon: float64, tuples for prefixes, one utterance at a time.
Nothing here uses gtn_applications_amd.lexicon or its packed trie: the lexicon is a dict from RAW spelling tuple
(replabels packed in, never the garbage) to word id, the position inside a word is the tuple of non-garbage labels
since the last word end, checked against the set of the spellings' proper prefixes, and the LM is
beam_lm_reference.ArpaLM over word ids (word v is label v, the blank is V) or None.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after the final drop and </s> up to the
first one not returned -- and the number of merged extensions."""
from asg_beam_reference import search
from beam_lexicon_reference import is_prefix_free, proper_prefixes
from beam_lm_reference import EOS
from beam_reference import NEG


def segment(lexicon, garbage, labels):
    """(word ids, the non-garbage labels since the last word end) of a raw class sequence with the garbage transparent,
    None if it leaves the lexicon"""
    inside, words, part = proper_prefixes(lexicon), [], ()
    for c in labels:
        if c == garbage:
            continue
        part += (c,)
        if part in lexicon:
            words.append(lexicon[part])
            part = ()
        elif part not in inside:
            return None
    return words, part


def beam_search(x, Wt, W, K, nbest, lexicon, garbage, lm, alpha, omega, beta, score_eos, logz=None, on_frame=None):
    """asg_beam_reference.beam_search with the additions of section 24.  lexicon: {raw spelling tuple: word id},
    prefix-free; garbage: the transparent class or None; lm: an ArpaLM over word ids or None.  Returns (hyps, margin,
    merges): hyps = nbest pairs (raw class tuple, score), the score minus logz if given; ranks beyond what is left
    after the last frame are ((), -inf).  on_frame(t, beam, cand, extension, merged, entries): called in every frame
    with the ranked beam [(prefix, p, part, history)], the candidates, the extension function, the merged flags and
    the sorted entries -- for a test that has to know a situation occurred."""
    inside = proper_prefixes(lexicon)

    def extend(state, pre, c):  # rule 3
        part, hist = state
        if garbage is not None and c == garbage:
            return 0.0, state
        part = part + (c,)
        if part in lexicon:  # the class completes a word
            l, nxt = lm.step(hist, lexicon[part]) if lm else (0.0, None)
            return None if l == NEG else ((alpha * l + omega) + beta, ((), nxt))
        return (beta, (part, hist)) if part in inside else None

    def finish(state, s):  # rule 5: a rank inside a word is dropped, </s>
        part, hist = state
        if part:
            return None
        if score_eos and lm:
            l, _ = lm.step(hist, EOS)
            if l == NEG:
                return None
            s += alpha * l
        return s

    return search(x, Wt, W, K, nbest, ((), lm.start if lm else None), extend, finish, logz=logz, on_frame=on_frame)


def brute_force(x, Wt, lexicon, garbage, lm, alpha, omega, beta, score_eos):
    """[(raw class tuple, score)] by rule 6: asg_beam_reference.brute_force's mass of every collapsed raw sequence over
    all C^T frame paths, those kept that walk the lexicon (garbage transparent) back to a word end, re-scored with
    alpha LM(words) + omega #words + beta #(non-garbage classes) and the </s> term; best first"""
    from asg_beam_reference import brute_force as masses

    out = []
    for pre, mass in masses(x, Wt):
        at = segment(lexicon, garbage, pre)
        if at is None or at[1] or mass == NEG:
            continue
        words = at[0]
        s = mass + omega * len(words) + beta * sum(1 for c in pre if c != garbage)
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


def raw_lexicon(words_tokens, num_replabels):
    """{raw spelling: word id} of words given as token index lists (separator included): rule 1, written out here
    rather than taken from the package -- a run of n equal tokens is groups of up to 1 + R: the token shifted by R,
    then, for a group of s >= 2, the replabel s - 2"""
    R, out = num_replabels, {}
    for v, toks in enumerate(words_tokens):
        s, k = [], 0
        while k < len(toks):
            n = 1
            while k + n < len(toks) and toks[k + n] == toks[k] and n < 1 + R:
                n += 1
            s.append(toks[k] + R)
            if n >= 2:
                s.append(n - 2)
            k += n
        out[tuple(s)] = v
    assert len(out) == len(words_tokens) and is_prefix_free(out)
    return out
