"""The CTC and Transducer prefix beam searches with a START-MARKED lexicon and a word-level n-gram LM (include/wfl.h:
wfl_ctc_beam_search_lexicon_marked, wfl_transducer_beam_search_lexicon_marked) restated in plain
Python from the rules: float64, tuples for prefixes, one utterance at a time.  Nothing here uses
gtn_applications_amd.lexicon or its packed trie: the lexicon is a dict from spelling tuple to word id (several spellings
may name one word, a spelling may be a proper prefix of another), the position of a hypothesis is the tuple of labels
since its current word began (empty: the empty prefix alone), and the LM is beam_lm_reference.ArpaLM over word ids (word
v is label v, the blank is V) or None.

One function serves both criteria: Wt None and forced False are CTC's rules (every transition weight 0, both masses into
an extension unless it repeats the last label), which is rule 7 of section 25.

beam_search() reports what a comparison needs to know, as the other references do: the smallest selection margin --
kept against first dropped entry in every frame, and between consecutive ranks after the last frame's terms up to the
first one not returned -- and the number of merged extensions."""
from beam_lm_reference import EOS
from beam_reference import NEG, search


def starts(lexicon):
    """R: the classes that begin a word"""
    return {s[0] for s in lexicon}


def is_start_marked(lexicon):
    """the one condition of rule 1: no class that begins a word occurs inside one"""
    return not (starts(lexicon) & {c for s in lexicon for c in s[1:]})


def positions(lexicon):
    """every non-empty prefix of a spelling, the spellings included: where a hypothesis inside or at the end of a word
    may stand"""
    return {s[:k] for s in lexicon for k in range(1, len(s) + 1)}


def segment(lexicon, labels):
    """(the COMPLETED words, the labels of the current word) of a label sequence, None if it leaves the lexicon: a word
    is completed by the label that begins the next"""
    R, at, words, part = starts(lexicon), positions(lexicon), [], ()
    for c in labels:
        if c in R:
            if part:
                if part not in lexicon:
                    return None
                words.append(lexicon[part])
            part = (c,)
        else:
            part += (c,)
            if len(part) == 1 or part not in at:
                return None
    return words, part


def words_of(lexicon, labels):
    """the words of a label sequence by rule 5 -- the pending word counts if its spelling is complete --, None if the
    sequence leaves the lexicon or ends inside a word"""
    seg = segment(lexicon, labels)
    if seg is None or (seg[1] and seg[1] not in lexicon):
        return None
    return seg[0] + ([lexicon[seg[1]]] if seg[1] else [])


def marked_lexicon_rules(lexicon, lm, alpha, omega, beta, score_eos):
    """(start, extend, finish) of a search with a start-marked lexicon: the state is (labels of the current word, LM
    history).  Rule 3: a label that begins no word continues the current one along the spellings and adds beta; one that
    begins a word adds beta behind the empty prefix, behind a complete spelling that word's (alpha l + omega) + beta,
    and does not exist behind an unfinished one.  Rule 5: after the last frame the empty sequence as it is, a complete
    pending word's alpha l + omega, anything else dropped; then </s>'s alpha l"""
    R, at = starts(lexicon), positions(lexicon)

    def extend(state, pre, c):
        part, hist = state
        if c not in R:  # inside a word: the arc of the current node
            return (beta, (part + (c,), hist)) if part and part + (c,) in at else None
        if not part:  # the first word of the empty prefix
            return beta, ((c,), hist)
        if part not in lexicon:  # a new word behind an unfinished one
            return None
        l, nxt = lm.step(hist, lexicon[part]) if lm else (0.0, None)
        return None if l == NEG else ((alpha * l + omega) + beta, ((c,), nxt))

    def finish(state, s):
        part, hist = state
        if part:
            if part not in lexicon:
                return None
            l, hist = lm.step(hist, lexicon[part]) if lm else (0.0, None)
            if l == NEG:
                return None
            s += alpha * l + omega
        if score_eos and lm:
            l, _ = lm.step(hist, EOS)
            if l == NEG:
                return None
            s += alpha * l
        return s

    return ((), lm.start if lm else None), extend, finish


def beam_search(x, blank, W, K, nbest, lexicon, lm, alpha, omega, beta, score_eos, normalize=False, Wt=None, forced=False,
                logz=None):
    """x: the [T, C] scores of one utterance.  lexicon: {spelling tuple: word id}, start-marked; lm: an ArpaLM over word
    ids or None.  Returns (hyps, margin, merges): hyps = nbest pairs (label tuple, score) -- the score minus the rows'
    log-sum-exps if `normalize`, minus logz if given --; ranks beyond what is left after the last frame are ((), -inf)."""
    rules = marked_lexicon_rules(lexicon, lm, alpha, omega, beta, score_eos)
    return search(x, blank, W, K, nbest, *rules, Wt=Wt, forced=forced, normalize=normalize, logz=logz)


def brute_force(x, blank, lexicon, lm, alpha, omega, beta, score_eos, Wt=None, forced=False, ctc=False):
    """[(label tuple, score)] by rule 6: the mass of every label sequence over all C^T frame paths -- grouped by
    collapsed sequence (ctc: beam_reference.brute_force) or by the sequence the token graph spells
    (transducer_beam_reference.brute_force) --, those kept that segment under rule 1 and end at a terminal node (or are
    empty), re-scored with alpha LM(words) + omega #words + beta #labels and the </s> term; best first"""
    if ctc:
        from beam_reference import brute_force as ctc_masses

        masses = ctc_masses(x, blank)
    else:
        from transducer_beam_reference import brute_force as tok_masses

        masses = tok_masses(x, Wt, blank, forced)
    out = []
    for pre, mass in masses:
        words = words_of(lexicon, pre)
        if words is None or mass == NEG:
            continue
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


def random_lexicon(rs, C, blank, V, max_len, n_starts, two_spellings=False):
    """{spelling: word id} of seeded random words over C classes: the first n_starts classes that are not the blank begin
    words, the others continue them; 1 .. max_len labels; built so that some words are proper prefixes of others (every
    word's prefixes that begin with a start class are candidates); with two_spellings word 0 gets a second spelling"""
    classes = [c for c in range(C) if c != blank]
    R, inner = classes[:n_starts], classes[n_starts:]
    lexicon = {}
    for _ in range(100 * V):
        if len(lexicon) >= V:
            break
        s = (R[rs.randint(len(R))],) + tuple(inner[rs.randint(len(inner))] for _ in range(rs.randint(max_len))) if inner \
            else (R[rs.randint(len(R))],)
        for k in (len(s), 1 + rs.randint(len(s))):  # the word and one of its prefixes: not prefix-free
            if s[:k] not in lexicon and len(lexicon) < V:
                lexicon[s[:k]] = len(lexicon)
    assert len(lexicon) == V, "not enough different words at this size"
    if two_spellings:
        for _ in range(1000):
            s = (R[rs.randint(len(R))],) + tuple(inner[rs.randint(len(inner))] for _ in range(1 + rs.randint(max_len)))
            if s not in lexicon:
                lexicon[s] = 0
                break
    return lexicon
