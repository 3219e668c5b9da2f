"""Lexicons for CTC.beam_search (host-side data preparation, like lm.py): the vocabulary a grapheme or word-piece CTC
model may emit, as a trie over the words' spellings.

A Lexicon is the packed trie of include/wfl.h (wfl_lexicon): a CSR of nodes with the root at
node 0; node n owns the arcs [arc_ptr[n], arc_ptr[n+1]) = (arc_label, arc_next) with strictly ascending labels;
arc_next >= 0 is an inner node, arc_next = -(v+1) completes word v and leads back to the root; no leaves are stored.
Nodes are numbered breadth first, the children of a node in label order.

The lexicon must be prefix-free -- no spelling is a proper prefix of another and no two words share one -- so that a
label sequence has at most one segmentation into words: the search merges hypotheses by their prefix, and the trie node
and LM state of a hypothesis must be functions of it.  Spellings that end in a separator class (a grapheme model's word
separator) are prefix-free by construction.

The word LM convention.  A word-level LM needs no class of its own: word v is LM label v, so
`NGramLM.from_arpa(path, words, blank=len(words))` is a back-off acceptor over word ids -- V + 1 "classes", index V the
blank that is never used, and </s> the label V + 1 = lm.num_classes.  check_word_lm() verifies exactly that where the
two objects meet.

The second boundary convention (boundary="start").  Word pieces carry the word boundary at the
START of a word ("_the", "_the" + "re"): a word has no separator behind it, a word may be a proper prefix of another and
may have several spellings, so such a vocabulary is not prefix-free.  A label sequence still has one segmentation if no
class that begins a word also occurs inside one -- the one condition of a start-marked lexicon: a word has ended where
the next begins, or where the utterance ends.  Its pack is wfl_lexicon_marked: the same CSR with the leaves stored and
every arc_next a node, node_word[n] the word whose spelling ends at node n (-1: none) and start_node[c] the root's child
by class c (-1: c begins no word).  During the search a hypothesis is ranked without the LM term of its last, unfinished
word.

Word-LM look-ahead.  Lexicon.lookahead(word_scores) pushes the best score of the words below a
trie node up to that node (node_look; 0 at the root) and returns the prepared LexiconLookahead -- wfl_lexicon_lookahead:
the array and the ranges the search's prune bound is formed from, checked once by libwfl, uploaded once per device;
Lexicon.unigram_lookahead(lm) is that of the word LM's unigram scores, built once per (lexicon, lm) pair.  The searches
pay lm_weight * node_look provisionally on the way down a word and settle it where the word ends."""
import ctypes
import weakref

import numpy as np

from . import _native as N


class Lexicon:
    """spellings[v]: the non-empty sequence of emission classes that spells word v (separator classes included);
    num_classes: the C of the emissions, blank among them.  ValueError for an empty list, an empty spelling, a class
    outside [0, C), the blank in a spelling, or a pair of words that breaks prefix-freeness (both are named).
    words: optional names of the words, for messages.
    boundary="start": a start-marked lexicon (the module's docstring).  word_of[k]: the word of spelling k (default k),
    which is how a word gets several spellings; words then names the word ids.  ValueError for an empty spelling, the
    blank or a class outside [0, C) in a spelling, two words with one spelling, a word id without a spelling, or a class
    that both begins a word and occurs inside one (the two words that show it are named)."""

    def __init__(self, spellings, num_classes, blank, words=None, boundary="end", word_of=None):
        if boundary not in ("end", "start"):
            raise ValueError(f"Lexicon: boundary {boundary!r} is neither 'end' nor 'start'")
        self.boundary = boundary
        if boundary == "start":
            self._init_start(spellings, num_classes, blank, words, word_of)
            return
        if word_of is not None:
            raise ValueError("Lexicon: word_of needs boundary='start' (an end-marked lexicon is prefix-free: a word has "
                             "one spelling)")
        self.num_classes, self.blank = int(num_classes), int(blank)
        spellings = [tuple(int(c) for c in s) for s in spellings]
        if not spellings:
            raise ValueError("Lexicon: no words")
        if words is not None and len(list(words)) != len(spellings):
            raise ValueError("Lexicon: as many names as spellings are needed")
        self.word_names = None if words is None else list(words)
        name = (lambda v: repr(self.word_names[v])) if self.word_names is not None else (lambda v: f"word {v}")
        if self.num_classes < 1 or not 0 <= self.blank < self.num_classes:
            raise ValueError(f"Lexicon: {self.num_classes} classes, blank {self.blank}")
        hint = "; spellings that end in a separator class are prefix-free by construction"
        children = [{}]  # node -> {label: child node, or ~v for the arc that completes word v}
        for v, s in enumerate(spellings):
            if not s:
                raise ValueError(f"Lexicon: {name(v)} has an empty spelling")
            for c in s:
                if not 0 <= c < self.num_classes:
                    raise ValueError(f"Lexicon: {name(v)} is spelled with class {c}, outside [0, {self.num_classes})")
                if c == self.blank:
                    raise ValueError(f"Lexicon: {name(v)} is spelled with the blank {c}")
            node = 0
            for c in s[:-1]:
                nxt = children[node].get(c)
                if nxt is None:
                    nxt = children[node][c] = len(children)
                    children.append({})
                elif nxt < 0:
                    raise ValueError(f"Lexicon: the spelling of {name(~nxt)} is a proper prefix of that of {name(v)}: "
                                     f"the lexicon is not prefix-free{hint}")
                node = nxt
            nxt = children[node].get(s[-1])
            if nxt is not None and nxt < 0:
                raise ValueError(f"Lexicon: {name(~nxt)} and {name(v)} have the same spelling: a word has one spelling "
                                 f"and a spelling one word{hint}")
            if nxt is not None:
                while nxt >= 0:  # (any word below: the first arc of every node on the way)
                    nxt = children[nxt][min(children[nxt])]
                raise ValueError(f"Lexicon: the spelling of {name(v)} is a proper prefix of that of {name(~nxt)}: "
                                 f"the lexicon is not prefix-free{hint}")
            children[node][s[-1]] = ~v
        self.spellings = spellings
        # breadth first from the root, children in label order
        order, number = [0], {0: 0}
        for n in order:
            for c in sorted(children[n]):
                k = children[n][c]
                if k >= 0:
                    number[k] = len(order)
                    order.append(k)
        arc_ptr, arc_label, arc_next = [0], [], []
        for n in order:
            for c in sorted(children[n]):
                k = children[n][c]
                arc_label.append(c)
                arc_next.append(number[k] if k >= 0 else -(~k + 1))
            arc_ptr.append(len(arc_label))
        self.arc_ptr = np.asarray(arc_ptr, dtype=np.int32)
        self.arc_label = np.asarray(arc_label, dtype=np.int32)
        self.arc_next = np.asarray(arc_next, dtype=np.int32)
        self.num_nodes, self.num_arcs, self.num_words = len(order), len(arc_label), len(spellings)
        desc = N.Lexicon(self.num_nodes, self.num_arcs, self.num_words, 0, self.arc_ptr.ctypes.data,
                         self.arc_label.ctypes.data, self.arc_next.ctypes.data)
        if N.lib.wfl_lexicon_check(ctypes.byref(desc), self.num_classes, self.blank) != N.WFL_OK:
            raise ValueError(f"Lexicon: {N.last_error()}")
        self._arcs = [{int(arc_label[a]): int(arc_next[a]) for a in range(arc_ptr[n], arc_ptr[n + 1])}
                      for n in range(self.num_nodes)]
        self._on_device = {}
        self._unigram_lookahead = weakref.WeakKeyDictionary()  # lm -> its LexiconLookahead

    def _init_start(self, spellings, num_classes, blank, words, word_of):
        self.num_classes, self.blank = int(num_classes), int(blank)
        spellings = [tuple(int(c) for c in s) for s in spellings]
        if not spellings:
            raise ValueError("Lexicon: no words")
        word_of = list(range(len(spellings))) if word_of is None else [int(v) for v in word_of]
        if len(word_of) != len(spellings):
            raise ValueError("Lexicon: word_of names one word per spelling")
        V = max(word_of) + 1 if words is None else len(list(words))
        self.word_names = None if words is None else list(words)
        name = (lambda v: repr(self.word_names[v])) if self.word_names is not None else (lambda v: f"word {v}")
        if self.num_classes < 1 or not 0 <= self.blank < self.num_classes:
            raise ValueError(f"Lexicon: {self.num_classes} classes, blank {self.blank}")
        for v in word_of:
            if not 0 <= v < V:
                raise ValueError(f"Lexicon: word_of names word {v}, outside [0, {V})")
        for v in sorted(set(range(V)) - set(word_of)):
            raise ValueError(f"Lexicon: {name(v)} has no spelling")
        children, node_word = [{}], [-1]  # node -> {label: child node}; node -> the word that ends there
        first, inner = {}, {}  # class -> the first word it begins / it occurs inside
        for s, v in zip(spellings, word_of):
            if not s:
                raise ValueError(f"Lexicon: {name(v)} has an empty spelling")
            for c in s:
                if not 0 <= c < self.num_classes:
                    raise ValueError(f"Lexicon: {name(v)} is spelled with class {c}, outside [0, {self.num_classes})")
                if c == self.blank:
                    raise ValueError(f"Lexicon: {name(v)} is spelled with the blank {c}")
            first.setdefault(s[0], v)
            for c in s[1:]:
                inner.setdefault(c, v)
            node = 0
            for c in s:
                nxt = children[node].get(c)
                if nxt is None:
                    nxt = children[node][c] = len(children)
                    children.append({})
                    node_word.append(-1)
                node = nxt
            if node_word[node] >= 0:
                raise ValueError(f"Lexicon: {name(node_word[node])} and {name(v)} have the same spelling: a spelling is "
                                 f"that of one word" if node_word[node] != v else
                                 f"Lexicon: {name(v)} is given the same spelling twice")
            node_word[node] = v
        for c in sorted(set(first) & set(inner)):
            raise ValueError(f"Lexicon: class {c} begins {name(first[c])} and occurs inside {name(inner[c])}: in a "
                             f"start-marked lexicon no class that begins a word occurs inside one")
        self.spellings, self.word_of = spellings, word_of
        # breadth first from the root, children in label order
        order, number = [0], {0: 0}
        for n in order:
            for c in sorted(children[n]):
                number[children[n][c]] = len(order)
                order.append(children[n][c])
        arc_ptr, arc_label, arc_next = [0], [], []
        for n in order:
            for c in sorted(children[n]):
                arc_label.append(c)
                arc_next.append(number[children[n][c]])
            arc_ptr.append(len(arc_label))
        start = [-1] * self.num_classes
        for c, k in children[0].items():
            start[c] = number[k]
        self.arc_ptr = np.asarray(arc_ptr, dtype=np.int32)
        self.arc_label = np.asarray(arc_label, dtype=np.int32)
        self.arc_next = np.asarray(arc_next, dtype=np.int32)
        self.node_word = np.asarray([node_word[n] for n in order], dtype=np.int32)
        self.start_node = np.asarray(start, dtype=np.int32)
        self.num_nodes, self.num_arcs, self.num_words = len(order), len(arc_label), V
        desc = self.marked_desc()
        if N.lib.wfl_lexicon_marked_check(ctypes.byref(desc), self.num_classes, self.blank) != N.WFL_OK:
            raise ValueError(f"Lexicon: {N.last_error()}")
        self._arcs = [{int(arc_label[a]): int(arc_next[a]) for a in range(arc_ptr[n], arc_ptr[n + 1])}
                      for n in range(self.num_nodes)]
        self._on_device = {}
        self._unigram_lookahead = weakref.WeakKeyDictionary()  # lm -> its LexiconLookahead

    def marked_desc(self):
        """the wfl_lexicon_marked of a start-marked lexicon's host arrays (they must outlive it)"""
        trie = N.Lexicon(self.num_nodes, self.num_arcs, self.num_words, 0, self.arc_ptr.ctypes.data,
                         self.arc_label.ctypes.data, self.arc_next.ctypes.data)
        return N.LexiconMarked(trie, self.node_word.ctypes.data, self.start_node.ctypes.data)

    @classmethod
    def from_words(cls, words, tokens, blank, wordsep=None, split=None, boundary="end", splits=None):
        """words: strings; tokens: the model's tokens in class order without the blank, blank: its class index, so token
        i is class i below the blank and i + 1 from it on (the convention of NGramLM.from_arpa).  A word is split into
        its characters, or by split(word) -> list of tokens (word pieces); with `wordsep` that token's class ends every
        spelling.  ValueError names a word with a piece that is no token.
        boundary="start": a start-marked lexicon; the marker is part of the pieces, so `wordsep` is refused;
        splits(word) -> a list of decompositions, each a list of pieces: every one becomes a spelling of the word."""
        if boundary not in ("end", "start"):
            raise ValueError(f"Lexicon.from_words: boundary {boundary!r} is neither 'end' nor 'start'")
        if boundary == "start" and wordsep is not None:
            raise ValueError("Lexicon.from_words: with boundary='start' the word boundary is part of the pieces: no wordsep")
        if splits is not None and boundary != "start":
            raise ValueError("Lexicon.from_words: splits (several decompositions of a word) needs boundary='start'")
        if splits is not None and split is not None:
            raise ValueError("Lexicon.from_words: split gives one decomposition per word, splits several: give one of them")
        tokens, blank = list(tokens), int(blank)
        if not 0 <= blank <= len(tokens):
            raise ValueError(f"Lexicon.from_words: blank {blank} is outside [0, {len(tokens)}]")
        if len(set(tokens)) != len(tokens):
            raise ValueError("Lexicon.from_words: a token appears twice")
        label = {tok: (i if i < blank else i + 1) for i, tok in enumerate(tokens)}
        if wordsep is not None and wordsep not in label:
            raise ValueError(f"Lexicon.from_words: the word separator {wordsep!r} is not one of the model's tokens")
        words = list(words)
        spellings, word_of = [], []
        for v, w in enumerate(words):
            ways = [list(w) if split is None else list(split(w))] if splits is None else [list(d) for d in splits(w)]
            for pieces in ways:
                for p in pieces:
                    if p not in label:
                        raise ValueError(f"Lexicon.from_words: {p!r} of {w!r} is not one of the model's tokens")
                spellings.append([label[p] for p in pieces] + ([label[wordsep]] if wordsep is not None else []))
                word_of.append(v)
        if boundary == "start":
            return cls(spellings, len(tokens) + 1, blank, words=words, boundary="start", word_of=word_of)
        return cls(spellings, len(tokens) + 1, blank, words=words)

    # ------------------------------------------------------------------------------------------------------------
    def walk(self, labels):
        """(word ids, node): the one segmentation of the label sequence into words and the trie node it ends in (0:
        at a word boundary); None if the sequence leaves the trie.  A start-marked lexicon (DESIGN.md section 26 rule
        5): a word ends where the next begins or, if the node is terminal, with the sequence -- the last word counts
        then; node 0 is the empty sequence alone."""
        found, node = [], 0
        if self.boundary == "start":
            for c in labels:
                c = int(c)
                if 0 <= c < self.num_classes and self.start_node[c] >= 0:
                    if node != 0:
                        if self.node_word[node] < 0:
                            return None
                        found.append(int(self.node_word[node]))
                    node = int(self.start_node[c])
                else:
                    node = self._arcs[node].get(c) if node != 0 else None
                    if node is None:
                        return None
            if node != 0 and self.node_word[node] >= 0:
                found.append(int(self.node_word[node]))
            return found, node
        for c in labels:
            nxt = self._arcs[node].get(int(c))
            if nxt is None:
                return None
            if nxt < 0:
                found.append(-(nxt + 1))
                node = 0
            else:
                node = nxt
        return found, node

    def words(self, labels):
        """the word ids of a label sequence that is a sequence of whole words; ValueError otherwise"""
        at = self.walk(labels)
        if at is None:
            raise ValueError("Lexicon.words: the labels leave the lexicon")
        if at[1] != 0 and (self.boundary == "end" or self.node_word[at[1]] < 0):
            raise ValueError("Lexicon.words: the labels end inside a word")
        return at[0]

    def on_device(self, device):
        """the operators' DeviceLexicon (csrc/torch_ops.cpp) of this pack on `device`: `.ints` int32 [arc_ptr |
        arc_label | arc_next] there and the wfl_lexicon that points into it; a start-marked lexicon's [node_word |
        start_node] behind them, and the wfl_lexicon_marked.  Uploaded once per device and kept, as NGramLM.on_device
        keeps its pack."""
        import torch

        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"Lexicon.on_device: {device} is not a GPU")
        index = torch.cuda.current_device() if device.index is None else device.index
        held = self._on_device.get(index)
        if held is None:
            marked = self.boundary == "start"
            ints = np.concatenate([self.arc_ptr, self.arc_label, self.arc_next] + ([self.node_word, self.start_node] if marked else []))
            held = self._on_device[index] = N.ops.DeviceLexicon(torch.from_numpy(ints).to(torch.device("cuda", index)),
                                                                self.num_nodes, self.num_arcs, self.num_words,
                                                                self.num_classes if marked else 0)
        return held


    def lookahead(self, word_scores):
        """The LexiconLookahead of the word scores u[v] (float64 [num_words], finite, natural logs): node_look[0] = 0,
        otherwise node_look[n] = max u[v] over the words that can still be completed from node n -- the completing arcs
        in the subtree of n, or for a start-marked lexicon the terminal nodes in it, n included.
        One pass from the leaves up: the breadth-first numbering puts children behind their parents.  ValueError for a
        wrong length or an entry that is not finite."""
        try:
            u = np.ascontiguousarray(word_scores, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"Lexicon.lookahead: the word scores must be numbers, got {type(word_scores).__name__}") from None
        if u.ndim != 1 or u.shape[0] != self.num_words:
            raise ValueError(f"Lexicon.lookahead: one score per word is needed -- [{self.num_words}] --, got {list(u.shape)}")
        if not np.isfinite(u).all():
            v = int(np.flatnonzero(~np.isfinite(u))[0])
            raise ValueError(f"Lexicon.lookahead: the score of word {v} is {u[v]}, not finite")
        look = np.full(self.num_nodes, -np.inf)
        marked = self.boundary == "start"
        for n in range(self.num_nodes - 1, -1, -1):
            best = u[self.node_word[n]] if marked and self.node_word[n] >= 0 else -np.inf
            for a in range(int(self.arc_ptr[n]), int(self.arc_ptr[n + 1])):
                m = int(self.arc_next[a])
                best = max(best, look[m] if m >= 0 else u[-(m + 1)])
            look[n] = best
        look[0] = 0.0
        return LexiconLookahead(self, look)

    def unigram_lookahead(self, lm):
        """lookahead() of the word LM's unigram scores (lm.unigram_scores(): lookahead="unigram"), built once per
        (lexicon, lm) pair and kept.  A word whose entry is -inf takes the smallest finite entry among the words;
        ValueError if no word has a finite entry, or if lm is no word LM of this lexicon."""
        held = self._unigram_lookahead.get(lm)
        if held is None:
            check_word_lm(self, lm, "Lexicon.unigram_lookahead")
            u = lm.unigram_scores()[:self.num_words].copy()
            finite = np.isfinite(u)
            if not finite.any():
                raise ValueError("Lexicon.unigram_lookahead: the lm has a finite unigram score for none of the words")
            u[~finite] = u[finite].min()
            held = self._unigram_lookahead[lm] = self.lookahead(u)
        return held


class LexiconLookahead:
    """The prepared word-LM look-ahead of a lexicon (wfl_lexicon_lookahead): `lexicon`, node_look
    float64 [num_nodes] and the ranges the search's prune bound is formed from -- (arc_min, arc_max) of node_look[m] -
    node_look[n] over the inner arcs, (end_min, end_max) of node_look over the nodes where a word can complete,
    (start_min, start_max) of node_look over the root's children (start-marked; 0, 0 otherwise).  Checked once, here, by
    libwfl's wfl_lexicon_lookahead_check (wfl_lexicon_marked_lookahead_check), which writes the ranges: ValueError for a
    wrong length, an entry that is not finite, a root that is not 0.  Lexicon.lookahead() builds one from word scores."""

    RANGES = ("arc_min", "arc_max", "end_min", "end_max", "start_min", "start_max")

    def __init__(self, lexicon, node_look):
        if not isinstance(lexicon, Lexicon):
            raise ValueError(f"LexiconLookahead: lexicon must be a lexicon.Lexicon, got {type(lexicon).__name__}")
        self.lexicon = lexicon
        try:
            self.node_look = np.ascontiguousarray(node_look, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("LexiconLookahead: node_look must be numbers") from None
        if self.node_look.ndim != 1 or self.node_look.shape[0] != lexicon.num_nodes:
            raise ValueError(f"LexiconLookahead: node_look must be [{lexicon.num_nodes}], one entry per node of the lexicon, "
                             f"got {list(self.node_look.shape)}")
        desc = N.LexiconLookahead(self.node_look.ctypes.data, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        if lexicon.boundary == "start":
            lex = lexicon.marked_desc()
            rc = N.lib.wfl_lexicon_marked_lookahead_check(ctypes.byref(lex), ctypes.byref(desc))
        else:
            lex = N.Lexicon(lexicon.num_nodes, lexicon.num_arcs, lexicon.num_words, 0, lexicon.arc_ptr.ctypes.data,
                            lexicon.arc_label.ctypes.data, lexicon.arc_next.ctypes.data)
            rc = N.lib.wfl_lexicon_lookahead_check(ctypes.byref(lex), ctypes.byref(desc))
        if rc != N.WFL_OK:
            raise ValueError(f"LexiconLookahead: {N.last_error()}")
        for name in self.RANGES:
            setattr(self, name, float(getattr(desc, name)))
        self._on_device = {}

    def on_device(self, device):
        """the operators' DeviceLookahead (csrc/torch_ops.cpp) on `device`: node_look there and the ranges.  Uploaded once
        per device and kept, as Lexicon.on_device keeps its pack."""
        import torch

        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"LexiconLookahead.on_device: {device} is not a GPU")
        index = torch.cuda.current_device() if device.index is None else device.index
        held = self._on_device.get(index)
        if held is None:
            held = self._on_device[index] = N.ops.DeviceLookahead(
                torch.from_numpy(self.node_look).to(torch.device("cuda", index)), *(getattr(self, name) for name in self.RANGES))
        return held


def check_lookahead(lookahead, lexicon, lm, merge_spellings, what):
    """The LexiconLookahead of a search's `lookahead` keyword, or None for None; ValueError otherwise (`what`: the call it
    was given to).  "unigram": lexicon.unigram_lookahead(lm); a LexiconLookahead of this lexicon: itself; anything else:
    the explicit word scores u[v], lexicon.lookahead's.  It needs both a lexicon and its word LM."""
    if lookahead is None:
        return None
    if merge_spellings:
        raise ValueError(f"{what}: lookahead is the lexicon search's, merge_spellings has no lexicon")
    if not isinstance(lexicon, Lexicon) or lm is None:
        raise ValueError(f"{what}: lookahead needs a lexicon and its word lm")
    check_word_lm(lexicon, lm, what)
    try:
        if isinstance(lookahead, str):
            if lookahead != "unigram":
                raise ValueError(f"lookahead {lookahead!r} is neither None, 'unigram' nor an array of word scores")
            return lexicon.unigram_lookahead(lm)
        if isinstance(lookahead, LexiconLookahead):
            if lookahead.lexicon is not lexicon:
                raise ValueError("the LexiconLookahead was prepared for another lexicon")
            return lookahead
        return lexicon.lookahead(lookahead)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None


def check_word_lm(lexicon, lm, what):
    """ValueError unless `lm` (an lm.NGramLM) follows the word LM convention above for `lexicon`"""
    V = lexicon.num_words
    if lm.num_classes != V + 1 or lm.blank != V:
        raise ValueError(f"{what}: with a lexicon the lm is a word LM over its {V} words -- num_classes {V + 1}, blank {V} "
                         f"(NGramLM.from_arpa(path, words, blank=len(words))) --, this one has num_classes "
                         f"{lm.num_classes}, blank {lm.blank}")
