"""The CTC prefix beam search with a lexicon and a word-level n-gram LM (include/wfl.h: wfl_ctc_beam_search_lexicon;
DESIGN.md section 20) restated in plain Python, as tests/beam_lm_reference.py restates the search with a token LM:
float64, tuples for prefixes, one utterance at a time.  Nothing here uses gtn_applications_amd.lexicon or its packed
trie: the lexicon is a dict from spelling tuple to word id, the position inside a word is the tuple of labels since the
last word end, checked against the set of the spellings' proper prefixes, and the LM is beam_lm_reference.ArpaLM over
word ids (word v is label v, the blank is V) or None."""
from beam_lm_reference import EOS
from beam_reference import NEG, search


def proper_prefixes(lexicon):
    """every proper prefix of a spelling, the empty one included: the positions a hypothesis may stand at"""
    return {s[:k] for s in lexicon for k in range(len(s))}


def is_prefix_free(lexicon):
    return not (set(lexicon) & proper_prefixes(lexicon))


def segment(lexicon, labels):
    """(word ids, the labels since the last word end) of a label sequence, None if it leaves the lexicon"""
    inside, words, part = proper_prefixes(lexicon), [], ()
    for c in labels:
        part += (c,)
        if part in lexicon:
            words.append(lexicon[part])
            part = ()
        elif part not in inside:
            return None
    return words, part


def lexicon_rules(lexicon, lm, alpha, omega, beta, score_eos):
    """(start, extend, finish) of a search with an end-marked (prefix-free) lexicon: the state is (labels since the last
    word, LM history); a label inside a word adds beta, the one that completes a word (alpha l + omega) + beta, any
    other does not exist; after the last frame a rank inside a word is dropped and </s> adds alpha l"""
    inside = proper_prefixes(lexicon)

    def extend(state, pre, c):
        part, hist = state
        part = part + (c,)
        if part in lexicon:  # the label completes a word
            l, nxt = lm.step(hist, lexicon[part]) if lm else (0.0, None)
            return None if l == NEG else ((alpha * l + omega) + beta, ((), nxt))
        return (beta, (part, hist)) if part in inside else None

    def finish(state, s):
        part, hist = state
        if part:
            return None  # (it ends inside a word)
        if score_eos and lm:
            l, _ = lm.step(hist, EOS)
            if l == NEG:
                return None
            s += alpha * l
        return s

    return ((), lm.start if lm else None), extend, finish


def beam_search(x, blank, W, K, nbest, lexicon, lm, alpha, omega, beta, score_eos, normalize=False):
    """beam_reference.beam_search with the additions of section 20.  lexicon: {spelling tuple: word id}, prefix-free;
    lm: an ArpaLM over word ids or None.  Returns (hyps, margin, merges) alike; the margin also covers the ranks after
    the final drop and </s>."""
    rules = lexicon_rules(lexicon, lm, alpha, omega, beta, score_eos)
    return search(x, blank, W, K, nbest, *rules, normalize=normalize)


def random_lexicon(rs, C, blank, V, max_len, sep=None):
    """{spelling: word id} of V different seeded random words of 1 .. max_len labels (never the blank, never `sep`),
    each followed by the separator class `sep` if there is one -- prefix-free then by construction; without one, words
    are drawn until the set is prefix-free, from the start again where short words have left no room for V of them"""
    letters = [c for c in range(C) if c != blank and c != sep]
    for _ in range(1000):
        lexicon = {}
        for _ in range(50 * V):
            s = tuple(letters[rs.randint(len(letters))] for _ in range(1 + rs.randint(max_len)))
            s += () if sep is None else (sep,)
            if s not in lexicon and is_prefix_free({**lexicon, s: 0}):
                lexicon[s] = len(lexicon)
            if len(lexicon) == V:
                return lexicon
    raise AssertionError("not enough different words at this size")
