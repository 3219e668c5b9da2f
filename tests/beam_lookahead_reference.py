"""The lexicon searches of CTC and the Transducer with word-LM look-ahead inside words (include/wfl.h: the four
wfl_*_beam_search_lexicon*_lookahead entries) restated in plain Python from the rules: float64,
tuples for prefixes, one utterance at a time, every operation of a term rounded on its own as Python rounds it.  Nothing
here uses gtn_applications_amd.lexicon or its packed trie: the lexicon is a dict from spelling tuple to word id -- end-
marked (prefix-free) or start-marked --, the position of a hypothesis is the tuple of labels of its current word, and the
look-ahead is a dict from that tuple to a score.  The LM is beam_lm_reference.ArpaLM over word ids.

One function serves CTC and both Transducer topologies, as beam_lexicon_marked_reference's does: Wt None and forced
False are CTC's rules.  It never skips a lookup: every extension's term is formed, so the device's prune bound is
compared against a search without one."""
from beam_lexicon_marked_reference import positions, starts
from beam_lexicon_reference import proper_prefixes
from beam_lm_reference import EOS
from beam_reference import NEG, search


def node_look(lexicon, scores, marked):
    """{labels of the current word: the best score of the words that can still be completed from there}: 0 for the empty
    tuple; end-marked the non-empty proper prefixes of the spellings, start-marked every non-empty prefix, the spellings
    included.  scores[v]: the score of word v."""
    look = {(): 0.0}
    for s, v in lexicon.items():
        for k in range(1, len(s) + (1 if marked else 0)):
            look[s[:k]] = max(look.get(s[:k], NEG), scores[v])
    return look


def unigram_scores(lm, V):
    """scores[v] of lookahead="unigram": the LM's step from its empty history, a word without one the smallest of the
    others (lm: an ArpaLM whose step((), v) is the unigram's)"""
    u = [lm.step((), v)[0] for v in range(V)]
    low = min(s for s in u if s != NEG)
    return [low if s == NEG else s for s in u]


def lookahead_rules(lexicon, lm, look, alpha, omega, beta, score_eos, marked):
    """(start, extend, finish) of a lexicon search with look-ahead: the state is (labels of the current word, LM
    history).  Rule 1: a label inside a word adds alpha (look[to] - look[from]) + beta, from the root look is 0; rule 2
    (end-marked) and rule 3 (start-marked): the word's step is settled against what its node has paid, and a
    start-marked word's first label pays its own node's look-ahead on top; rule 4: after the last frame a rank inside
    a word is dropped -- start-marked: unless its spelling is complete, then settled alike --, then </s>"""
    R = starts(lexicon) if marked else set()
    at = positions(lexicon) if marked else proper_prefixes(lexicon)

    def extend(state, pre, c):
        part, hist = state
        if not marked:
            to = part + (c,)
            if to in lexicon:  # rule 2: the word's step settled against what its node has paid
                l, nxt = lm.step(hist, lexicon[to]) if lm else (0.0, None)
                return None if l == NEG else ((alpha * (l - look[part]) + omega) + beta, ((), nxt))
            return (alpha * (look[to] - look[part]) + beta, (to, hist)) if to in at else None  # rule 1
        if c not in R:  # rule 1, inside a start-marked word
            if not part or part + (c,) not in at:
                return None
            return alpha * (look[part + (c,)] - look[part]) + beta, (part + (c,), hist)
        if not part:  # rule 1 from the root, whose look-ahead is 0
            return alpha * (look[(c,)] - 0.0) + beta, ((c,), hist)
        if part not in lexicon:
            return None
        l, nxt = lm.step(hist, lexicon[part]) if lm else (0.0, None)
        if l == NEG:
            return None
        return ((alpha * (l - look[part]) + omega) + beta) + alpha * look[(c,)], ((c,), nxt)  # rule 3

    def finish(state, s):  # rule 4
        part, hist = state
        if part:
            if not marked or part not in lexicon:
                return None
            l, hist = lm.step(hist, lexicon[part]) if lm else (0.0, None)
            if l == NEG:
                return None
            s += alpha * (l - look[part]) + omega
        if score_eos and lm:
            l, _ = lm.step(hist, EOS)
            if l == NEG:
                return None
            s += alpha * l
        return s

    return ((), lm.start if lm else None), extend, finish


def beam_search(x, blank, W, K, nbest, lexicon, lm, look, alpha, omega, beta, score_eos, marked=False, normalize=False,
                Wt=None, forced=False, logz=None):
    """x: the [T, C] scores of one utterance.  lexicon: {spelling tuple: word id}; lm: an ArpaLM over word ids; look:
    node_look()'s dict.  Returns (hyps, margin, merges) as the other restatements do: hyps = nbest pairs (label tuple,
    score) -- minus the rows' log-sum-exps if `normalize`, minus logz if given --, ((), -inf) beyond what is left; the
    smallest selection margin; the number of merged extensions."""
    rules = lookahead_rules(lexicon, lm, look, alpha, omega, beta, score_eos, marked)
    return search(x, blank, W, K, nbest, *rules, Wt=Wt, forced=forced, normalize=normalize, logz=logz)
