"""Token-level n-gram language models for CTC.beam_search (host-side data preparation, like transitions_builder.py).

An NGramLM is the back-off acceptor of include/wfl.h (wfl_ngram_lm) over the emission classes of a
CTC model: state s has arcs (label, next, w) with strictly ascending labels and an optional back-off (bo_next, bo_w);
labels are class indices, never the blank, and label C stands for </s>; weights are float64 natural logs.

    step(s, c): acc = 0; look c up among the arcs of s; found: (acc + w, next); no back-off: (-inf, None);
                otherwise acc += bo_w[s], s = bo_next[s], look again.

NGramLM.from_arpa() builds one from an ARPA file by the format's definition: `\\data\\`, `ngram N=count` lines, one
`\\N-grams:` section per order of lines `log10(p) w1 .. wN [log10(back-off)]`, `\\end\\`.  The states are the empty
history and every gram of an order below the file's that does not end in </s>; the arc of a gram leaves the state of its
first N-1 words and enters the longest suffix of the gram that is a state; a state backs off to the state of its words
without the first.  The pack is checked once, by libwfl's wfl_ngram_lm_check, when the object is built -- the kernels
trust only packs that passed it."""
import bisect
import ctypes
import math

import numpy as np

from . import _native as N

MAX_ORDER = 8  # a back-off chain has at most wfl.h's WFL_NGRAM_LM_MAX_BACKOFF = 8 links: orders 1..8 stay below it
_LN10 = math.log(10.0)


class NGramLM:
    """The packed acceptor.  num_classes: the C of the emissions it scores, blank among them; the arrays as in
    wfl_ngram_lm (arc_ptr [S+1], arc_label / arc_next / arc_w [A], bo_next / bo_w [S], bo_next -1 for none).
    Raises ValueError if wfl_ngram_lm_check refuses the pack."""

    def __init__(self, num_classes, blank, arc_ptr, arc_label, arc_next, arc_w, bo_next, bo_w, start=0, order=None,
                 tokens=None):
        self.num_classes, self.blank, self.start = int(num_classes), int(blank), int(start)
        self.arc_ptr = np.ascontiguousarray(arc_ptr, dtype=np.int32)
        self.arc_label = np.ascontiguousarray(arc_label, dtype=np.int32)
        self.arc_next = np.ascontiguousarray(arc_next, dtype=np.int32)
        self.arc_w = np.ascontiguousarray(arc_w, dtype=np.float64)
        self.bo_next = np.ascontiguousarray(bo_next, dtype=np.int32)
        self.bo_w = np.ascontiguousarray(bo_w, dtype=np.float64)
        S, A = self.bo_next.shape[0], self.arc_label.shape[0]
        if any(a.ndim != 1 for a in (self.arc_ptr, self.arc_label, self.arc_next, self.arc_w, self.bo_next, self.bo_w)) or \
                self.arc_ptr.shape[0] != S + 1 or self.arc_next.shape[0] != A or self.arc_w.shape[0] != A or \
                self.bo_w.shape[0] != S:
            raise ValueError(f"NGramLM: the arrays do not describe {S} states and {A} arcs")
        self.num_states, self.num_arcs = S, A
        self.step_min = self.step_max = 0.0
        desc = self._desc(*(a.ctypes.data for a in (self.arc_ptr, self.arc_label, self.arc_next, self.arc_w, self.bo_next,
                                                     self.bo_w)))
        if N.lib.wfl_ngram_lm_check(ctypes.byref(desc), self.num_classes, self.blank) != N.WFL_OK:
            raise ValueError(f"NGramLM: {N.last_error()}")
        # the bounds of step() the search prunes lookups with: the check computes them from the pack it accepted
        self.step_min, self.step_max = float(desc.step_min), float(desc.step_max)
        if order is None:  # 1 + the longest back-off chain (the check bounded it)
            order = 1
            for s in range(S):
                d = 1
                while self.bo_next[s] >= 0:
                    s, d = int(self.bo_next[s]), d + 1
                order = max(order, d)
        self.order = int(order)
        self.tokens = None if tokens is None else list(tokens)
        self._on_device = {}

    def _desc(self, arc_ptr, arc_label, arc_next, arc_w, bo_next, bo_w):
        return N.NgramLm(self.num_states, self.num_arcs, self.start, 0, self.step_min, self.step_max, arc_ptr, arc_label,
                         arc_next, arc_w, bo_next, bo_w)

    # ------------------------------------------------------------------------------------------------------------
    def step(self, state, label):
        """(log weight, next state) of `label` (a class index, or num_classes for </s>) from `state`: the rule above;
        (-inf, None) if no state of the back-off chain has the arc"""
        acc, s = 0.0, int(state)
        while True:
            lo, hi = int(self.arc_ptr[s]), int(self.arc_ptr[s + 1])
            a = lo + bisect.bisect_left(self.arc_label[lo:hi].tolist(), label)
            if a < hi and self.arc_label[a] == label:
                return acc + float(self.arc_w[a]), int(self.arc_next[a])
            if self.bo_next[s] < 0:
                return -math.inf, None
            acc, s = acc + float(self.bo_w[s]), int(self.bo_next[s])

    def class_of(self, token):
        if self.tokens is None or token not in self.tokens:
            raise ValueError(f"NGramLM: {token!r} is not one of the model's tokens")
        i = self.tokens.index(token)
        return i if i < self.blank else i + 1

    def score(self, labels, eos=True):
        """float64 natural log of P(labels [</s>] | <s>): the sum of step() along the labels from the start state.
        labels: class indices, or a string of space-separated tokens (an LM loaded with its token list)."""
        if isinstance(labels, str):
            labels = [self.class_of(w) for w in labels.split()]
        total, s = 0.0, self.start
        for c in list(labels) + ([self.num_classes] if eos else []):
            c = int(c)
            if not 0 <= c <= self.num_classes or c == self.blank:
                raise ValueError(f"NGramLM.score: label {c} is not a class the model scores")
            w, s = self.step(s, c)
            if s is None:
                return -math.inf
            total += w
        return total

    def unigram_scores(self):
        """float64 [num_classes]: entry v is step(base, v)[0], base the state reached from `start` by following bo_next
        until there is no back-off (the empty history of from_arpa) -- the back-off weights on the way are not counted;
        the blank's entry, and that of a label without an arc there, is -inf.  What lookahead="unigram" smears over a
        lexicon's trie."""
        base = self.start
        while self.bo_next[base] >= 0:  # (the check bounded the chain)
            base = int(self.bo_next[base])
        scores = np.full(self.num_classes, -math.inf)
        lo, hi = int(self.arc_ptr[base]), int(self.arc_ptr[base + 1])
        labels = self.arc_label[lo:hi]
        keep = labels < self.num_classes  # (not </s>; the blank has no arc)
        scores[labels[keep]] = self.arc_w[lo:hi][keep]
        return scores

    def on_device(self, device):
        """the operators' DeviceLm (csrc/torch_ops.cpp) of this pack on `device`: `.ints` int32 [arc_ptr | arc_label |
        arc_next | bo_next] and `.weights` float64 [arc_w | bo_w] there, and the wfl_ngram_lm that points into them.
        Uploaded once per device and kept (the cache is a plain dict: two threads that make their first call for a
        device at the same time may both upload, and one copy is dropped -- harmless)"""
        import torch

        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"NGramLM.on_device: {device} is not a GPU")
        index = torch.cuda.current_device() if device.index is None else device.index
        held = self._on_device.get(index)
        if held is None:
            ints = np.concatenate([self.arc_ptr, self.arc_label, self.arc_next, self.bo_next])
            weights = np.concatenate([self.arc_w, self.bo_w])
            dev = torch.device("cuda", index)
            held = self._on_device[index] = N.ops.DeviceLm(torch.from_numpy(ints).to(dev), torch.from_numpy(weights).to(dev),
                                                           self.num_states, self.num_arcs, self.start, self.step_min,
                                                           self.step_max)
        return held

    # ------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, path, tokens, blank, bos="<s>", eos="</s>", unk="<unk>"):
        """tokens: the model's tokens in class order without the blank (the convention of --tokens), blank: its class
        index, so token i is class i below the blank and i + 1 from it on.  A token without a unigram takes the arcs
        of `unk` if the file has one (the arcs are duplicated per class), otherwise ValueError names it.  ARPA words
        that are no tokens are dropped with every gram that contains them.  ValueError, with the line, for a file
        that is not ARPA: no \\data\\, a section whose size is not the declared one, a gram of the wrong length, a
        number that is none, a gram whose history or suffix (the gram without its last / first word) is absent."""
        tokens = list(tokens)
        blank = int(blank)
        if not 0 <= blank <= len(tokens):
            raise ValueError(f"NGramLM.from_arpa: blank {blank} is outside [0, {len(tokens)}]")
        if len(set(tokens)) != len(tokens):
            raise ValueError("NGramLM.from_arpa: a token appears twice")
        for special in (bos, eos):
            if special in tokens:
                raise ValueError(f"NGramLM.from_arpa: {special!r} is a token")
        C = len(tokens) + 1
        grams, order = _read_arpa(path)
        unigrams = {g[0] for g in grams[0]}
        classes = {w: [] for w in unigrams}
        for i, tok in enumerate(tokens):
            word = tok if tok in unigrams else unk
            if word not in unigrams:
                raise ValueError(f"NGramLM.from_arpa: {path} has no unigram for token {tok!r} and no {unk!r}")
            classes[word].append(i if i < blank else i + 1)

        def kept(g):
            n = len(g)
            for k, w in enumerate(g):
                if w == bos:
                    if k != 0:
                        return False
                elif w == eos:
                    if k != n - 1:
                        return False
                elif not classes.get(w):
                    return False
            return True

        table = [{g: v for g, v in level.items() if kept(g)} for level in grams]  # gram -> (log10 p, log10 bo, line)
        for n in range(1, order):
            for g, (_, _, line) in table[n].items():
                if g[:-1] not in table[n - 1]:
                    raise ValueError(f"{path}:{line}: the history {' '.join(g[:-1])!r} of this gram is absent")
                if g[1:] not in table[n - 1]:
                    raise ValueError(f"{path}:{line}: the suffix {' '.join(g[1:])!r} of this gram is absent")
        state = {(): 0}
        for n in range(order - 1):
            for g in table[n]:
                if g[-1] != eos:
                    state[g] = len(state)
        S = len(state)
        arcs = [[] for _ in range(S)]
        for n in range(order):
            for g, (p, _, line) in table[n].items():
                if g == (bos,):
                    continue  # (a history, never a label)
                src = state[g[:-1]]
                if g[-1] == eos:
                    labels, nxt = [C], 0
                else:
                    labels = classes[g[-1]]
                    nxt = next(state[g[len(g) - k:]] for k in range(min(len(g), order - 1), -1, -1) if g[len(g) - k:] in state)
                arcs[src] += [(c, nxt, p * _LN10, line) for c in labels]
        arc_ptr, arc_label, arc_next, arc_w = [0], [], [], []
        for a in arcs:
            a.sort()
            for (c, _, _, _), (d, _, _, line) in zip(a, a[1:]):
                if c == d:
                    raise ValueError(f"{path}:{line}: this gram is in the file twice")
            arc_label += [c for c, _, _, _ in a]
            arc_next += [x for _, x, _, _ in a]
            arc_w += [w for _, _, w, _ in a]
            arc_ptr.append(len(arc_label))
        bo_next, bo_w = [-1] * S, [0.0] * S
        for g, s in state.items():
            if g:
                bo_next[s], bo_w[s] = state[g[1:]], table[len(g) - 1][g][1] * _LN10
        return cls(C, blank, arc_ptr, arc_label, arc_next, arc_w, bo_next, bo_w, start=state.get((bos,), 0), order=order,
                   tokens=tokens)


def _read_arpa(path):
    """([{gram tuple: (log10 p, log10 back-off or 0, line)} per order], order).  ValueError with the line otherwise."""
    def bad(line, what):
        return ValueError(f"{path}:{line}: {what}")

    with open(path) as f:
        lines = f.read().split("\n")
    at = 0
    while at < len(lines) and lines[at].strip() != "\\data\\":
        at += 1
    if at == len(lines):
        raise bad(len(lines), "no \\data\\ section")
    at += 1
    counts = []
    while at < len(lines) and lines[at].strip().startswith("ngram"):
        body = lines[at].strip()[len("ngram"):].split("=")
        try:
            n, count = int(body[0]), int(body[1])
        except (ValueError, IndexError):
            raise bad(at + 1, "not an `ngram N=count` line") from None
        if n != len(counts) + 1 or count < 0:
            raise bad(at + 1, f"`ngram {len(counts) + 1}=count` expected")
        counts.append(count)
        at += 1
    if not counts:
        raise bad(at + 1, "no `ngram N=count` line after \\data\\")
    if len(counts) > MAX_ORDER:
        raise bad(at, f"order {len(counts)} is more than the {MAX_ORDER} an NGramLM takes")
    grams = []
    for n in range(1, len(counts) + 1):
        while at < len(lines) and not lines[at].strip():
            at += 1
        if at == len(lines) or lines[at].strip() != f"\\{n}-grams:":
            raise bad(at + 1, f"\\{n}-grams: expected")
        header = at + 1
        at += 1
        level = {}
        while at < len(lines) and lines[at].strip() and not lines[at].strip().startswith("\\"):
            fields = lines[at].split()
            if len(fields) not in (n + 1, n + 2):
                raise bad(at + 1, f"a {n}-gram line has {n + 1} or {n + 2} fields, this one {len(fields)}")
            try:
                p = float(fields[0])
                bo = float(fields[n + 1]) if len(fields) == n + 2 else 0.0
            except ValueError:
                raise bad(at + 1, "a probability or back-off that is no number") from None
            if p != p or bo != bo or p == math.inf or bo == math.inf:
                raise bad(at + 1, "a probability or back-off that is NaN or +inf")
            g = tuple(fields[1:n + 1])
            if g in level:
                raise bad(at + 1, "this gram is in the file twice")
            level[g] = (p, bo, at + 1)
            at += 1
        if len(level) != counts[n - 1]:
            raise bad(header, f"{len(level)} {n}-grams in the section, {counts[n - 1]} declared")
        grams.append(level)
    while at < len(lines) and not lines[at].strip():
        at += 1
    if at == len(lines) or lines[at].strip() != "\\end\\":
        raise bad(at + 1, "\\end\\ expected")
    return grams, len(counts)
