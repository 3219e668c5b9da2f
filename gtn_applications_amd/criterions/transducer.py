"""Transducer criterion -- counterpart of /root/reference/criterions/transducer.py.

Graph factories (`make_*_graph`), the `Transducer` module and `TransducerLossFunction` keep the
reference's names, arguments and error behaviour (transducer.py:15-348).  The small per-utterance
graph algebra (target o lexicon, tokens o decompositions, transitions o alignments;
transducer.py:265-281) runs in the C++ host library; everything that touches the [B,T,C] emissions
-- `intersect(emissions, .)`, `forward_score`, `viterbi_path`, `backward`
(transducer.py:283-288,321-336,216-221) -- runs on the lattice engine kernels.
"""
import collections
import ctypes
import itertools
import numbers
import os
import threading

import math

import numpy as np
import torch

from .. import _native as N
from .. import engine as E
from .. import graph as G
from .. import metrics as M


def make_scalar_graph(weight):
    """transducer.py:15-20."""
    scalar = G.Graph()
    scalar.add_node(True)
    scalar.add_node(False, True)
    scalar.add_arc(0, 1, 0, 0, weight)
    return scalar


def make_chain_graph(sequence):
    """transducer.py:23-29."""
    seq = [int(s) for s in sequence]
    graph = G.Graph(False)
    n = len(seq)
    graph.add_nodes([1] + [0] * n, [0] * n + [1] if n else [0])
    if n:
        idx = np.arange(n, dtype=np.int32)
        graph.add_arcs(idx, idx + 1, np.asarray(seq, dtype=np.int32))
    return graph


def make_transitions_graph(ngram, num_tokens, calc_grad=False):
    """transducer.py:32-58: dense n-gram transition model; </s> is reached by epsilon arcs."""
    transitions = G.Graph(calc_grad)
    transitions.add_node(True, ngram == 1)
    state_map = {(): 0}
    for n in range(1, ngram):  # histories that still include <s>
        for state in itertools.product(range(num_tokens), repeat=n):
            state_map[state] = transitions.add_node(False, ngram == 1)
            transitions.add_arc(state_map[state[:-1]], state_map[state], state[-1])
    src, dst, lab = [], [], []
    for state in itertools.product(range(num_tokens), repeat=ngram):
        src.append(state_map[state[:-1]]), dst.append(state_map[state[1:]]), lab.append(state[-1])
    transitions.add_arcs(src, dst, lab)
    if ngram > 1:
        end_idx = transitions.add_node(False, True)
        idx = np.arange(end_idx, dtype=np.int32)
        transitions.add_arcs(idx, np.full(end_idx, end_idx, np.int32), np.full(end_idx, G.epsilon, np.int32))
    return transitions


def make_lexicon_graph(word_pieces, graphemes_to_idx):
    """transducer.py:61-75: letters -> word pieces."""
    graph = G.Graph(False)
    graph.add_node(True, True)
    for i, wp in enumerate(word_pieces):
        prev = 0
        for letter in wp[:-1]:
            n = graph.add_node()
            graph.add_arc(prev, n, graphemes_to_idx[letter], G.epsilon)
            prev = n
        graph.add_arc(prev, 0, graphemes_to_idx[wp[-1]], i)
    graph.arc_sort()
    return graph


def make_token_graph(token_list, blank="none", allow_repeats=True):
    """transducer.py:78-123: emission labels -> tokens (one or more frames per token)."""
    if not allow_repeats and blank != "optional":
        raise ValueError("Must use blank='optional' if disallowing repeats.")
    ntoks = len(token_list)
    graph = G.Graph(False)
    graph.add_node(True, True)
    graph.add_nodes([0] * ntoks, [int(blank != "forced")] * ntoks)
    if blank != "none":
        graph.add_node()
        graph.add_arc(0, ntoks + 1, ntoks, G.epsilon)  # blank index is assumed to be last (ntoks)
        graph.add_arc(ntoks + 1, 0, G.epsilon)
    entry = (ntoks + 1) if blank == "forced" else 0
    arcs = []  # (src, dst, ilabel, olabel) in the reference's insertion order
    for i in range(ntoks):
        arcs.append((entry, i + 1, i, i))
        arcs.append((i + 1, i + 1, i, G.epsilon))
        if allow_repeats:
            if blank == "forced":  # token -> blank only
                arcs.append((i + 1, ntoks + 1, ntoks, G.epsilon))
            else:  # token -> blank and every token
                arcs.append((i + 1, 0, G.epsilon, G.epsilon))
        else:  # token -> blank and every OTHER token
            arcs.append((i + 1, ntoks + 1, ntoks, G.epsilon))
            arcs.extend((i + 1, j + 1, j, j) for j in range(ntoks) if j != i)
    src, dst, il, ol = (np.fromiter((a[k] for a in arcs), dtype=np.int32, count=len(arcs)) for k in range(4))
    graph.add_arcs(src, dst, il, ol)
    return graph


def make_kernel_graph(x, blank_idx, blank_optional, spike=False, calc_grad=False):
    """transducer.py:351-367."""
    g = G.Graph(calc_grad)
    g.add_node(True, len(x) == 0)  # start in blank
    g.add_arc(0, 0, blank_idx)
    for i, c in enumerate(x):
        last = (i + 1) == len(x)
        g.add_node(False, blank_optional and last)
        g.add_node(False, last)
        g.add_arc(2 * i, 2 * i + 1, c)
        if not spike:
            g.add_arc(2 * i + 1, 2 * i + 1, c)
        g.add_arc(2 * i + 1, 2 * i + 2, blank_idx)
        g.add_arc(2 * i + 2, 2 * i + 2, blank_idx)
        if i > 0 and blank_optional and x[i - 1] != c:
            g.add_arc(2 * i - 1, 2 * i + 1, c)
    g.arc_sort(True)
    g.arc_sort()
    return g


# alignment graphs per (tokens, lexicon, transitions, target) and packed batches: content-keyed LRUs
_ALIGN_CACHE = E.LRU(4096)
_PACK_CACHE = E.LRU(32)
# One batch is packed at a time (the cache, the staging ring and the packer's host pool are shared between the caller's
# thread and the prefetch thread of Transducer.prepare)
_PACK_LOCK = threading.RLock()
_PREP = {"pool": None, "streams": {}}


class PreparedTargets:
    """A batch of targets whose alignment acceptors are being (or have been) built, packed and uploaded ahead of the
    step that uses them: what `Transducer.prepare(targets)` returns and `Transducer.forward(inputs, prepared)` accepts
    in the place of the target list.  The per-batch host work of the criterion (the graph algebra of
    transducer.py:262-281 for every utterance: ~0.3 ms at the benchmark's size) then runs on a side thread while the
    previous step is on the GPU -- what a DataLoader's prefetch does for the inputs."""

    __slots__ = ("targets", "future", "B")

    def __init__(self, targets, future, B):
        self.targets, self.future, self.B = targets, future, B

    def result(self):
        return self.future.result()

    def __len__(self):
        return self.B


def _pack_entry(targets, tokens, lexicon, transitions, C, dev, reduction):
    """(cache key, flat labels info) of a batch and its cache entry (built if it is not there): the per-sample graph
    algebra of transducer.py:262-281 for the whole batch -- one native call, threaded over the utterances like the
    reference's gtn.parallel_for (transducer.py:296) -- and the asynchronous upload on the CURRENT stream."""
    flat, offsets, lens = E.flatten_any(targets)
    B = len(lens)
    key = ("num", flat.tobytes(), tuple(lens), id(tokens), id(lexicon), id(transitions), C, dev.index)
    full_key = key + (reduction == "mean",)
    with _PACK_LOCK:
        if full_key not in _PACK_CACHE.data:
            N.lib.wfl_host_pool_wake()  # (new targets: the packer's threads are awake by the time its job is submitted)

        def build():
            if reduction == "mean":  # transducer.py:302-305: normalise by the (grapheme) target length
                sc = np.array([1.0 / n if n > 0 else 1.0 for n in lens], dtype=np.float32)
            else:
                sc = np.ones(B, dtype=np.float32)
            # (loss scale, +scale/B, -scale/B) travel with the packed batch: one asynchronous upload, no kernels
            pack = E.PackedLattice.transducer_batch(tokens, lexicon, transitions, flat, offsets, C, dev,
                                                    extra=np.concatenate([sc, sc / B, -sc / B]))
            fac = pack.extra
            return pack, fac[:B], fac[B:2 * B], fac[2 * B:], (tokens, lexicon, transitions)

        entry = _PACK_CACHE.get(full_key, build)
    return B, entry


def _prepare(targets, tokens, lexicon, transitions, C, dev, reduction):
    """_pack_entry on the prefetch thread, its upload on a stream of its own (the step that uses the pack orders itself
    behind the pack's event)."""
    if _PREP["pool"] is None:
        import concurrent.futures

        _PREP["pool"] = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="wfl-prepare")
    stream = _PREP["streams"].get(dev.index)
    if stream is None:
        stream = _PREP["streams"][dev.index] = torch.cuda.Stream(device=dev)

    def job():
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            return _pack_entry(targets, tokens, lexicon, transitions, C, dev, reduction)

    return _PREP["pool"].submit(job)


def _zero_weight_view(graph):
    """Structure of `graph` with all arc weights 0: learnable weights are added on the device."""
    a = graph.arrays()
    g = G.Graph(False)
    g.add_nodes(a["start"], a["accept"])
    g.add_arcs(a["src"], a["dst"], a["ilabel"], a["olabel"])
    return g


def _alignment_graph(target, tokens, lexicon, transitions, direct=False):
    """transducer.py:265-281: every frame-level alignment of every decomposition of `target` into
    tokens, optionally intersected with the transition model.  Returns (graph, weight ids).
    direct=True: the alignments written down without the composition where the token graph allows it
    (G.token_alignments -- what the native batch packer does; isomorphic, not identical)."""
    key = (tuple(target), id(tokens), id(lexicon), id(transitions), bool(direct))

    def build():
        tgt = make_chain_graph(target)
        tokens_target = G.remove(G.project_output(G.compose(tgt, lexicon)))
        ali = G.token_alignments(tokens, tokens_target) if direct else None
        if ali is None:
            ali = G.project_input(G.remove(G.compose(tokens, tokens_target)))
        if transitions is None:
            return ali, None, (tokens, lexicon)
        ali, from_trans, _ = G.compose(transitions, ali, provenance=True)
        return ali, from_trans, (tokens, lexicon, transitions)  # keep operands alive: ids stay unique

    return _ALIGN_CACHE.get(key, build)[:2]


# WFL_DENSE_NGRAM=0: the bigram normaliser through the general lattice sweep (A/B tests, measurements)
_DENSE_NGRAM = os.environ.get("WFL_DENSE_NGRAM", "1") != "0"


class Transducer(torch.nn.Module):
    """A generic transducer loss (transducer.py:126-234).

    tokens: list of iterables (strings, tuples, ...) -- the model's output units.
    graphemes_to_idx: grapheme -> integer index.
    ngram: order of the learned token-level transition model (0: none).
    transitions: alternatively a ready transition graph (its arcs become `transition_params`).
    blank: 'none' | 'optional' | 'forced'.   allow_repeats: allow the same token twice in a row.
    """

    def __init__(self, tokens, graphemes_to_idx, ngram=0, transitions=None, blank="none",
                 allow_repeats=True, reduction="none"):
        super(Transducer, self).__init__()
        if blank not in ["optional", "forced", "none"]:
            raise ValueError("Invalid value specificed for blank. Must be in ['optional', 'forced', 'none']")
        self.tokens = make_token_graph(tokens, blank=blank, allow_repeats=allow_repeats)
        self.lexicon = make_lexicon_graph(tokens, graphemes_to_idx)
        self._num_emission_classes = len(tokens) + int(blank != "none")  # (width of the emissions: prepare())
        # the graphemes every token spells, as indices: what beam_search(merge_spellings=True) identifies hypotheses by
        # (plain attributes, no buffers: the state_dict is what it was)
        self.token_spellings = [tuple(graphemes_to_idx[g] for g in wp) for wp in tokens]
        self._spelling_table = None
        # the tokens as tuples of their elements: what word_lexicon() compares the pieces of a word against (plain too)
        self._token_pieces = [tuple(wp) for wp in tokens]
        # the tokens as they were given, in class order: what token_lm() names the classes of an ARPA file by (plain too)
        self._token_names = list(tokens)
        self._has_blank = blank != "none"
        self.ngram = ngram
        if ngram > 0 and transitions is not None:
            raise ValueError("Only one of ngram and transitions may be specified")
        if ngram > 0:
            transitions = make_transitions_graph(ngram, len(tokens) + int(blank != "none"), True)
        if transitions is not None:
            # the arc weights of the graph are replaced by the parameters on every call
            # (transducer.py:255-256), so only its structure matters
            self.transitions = _zero_weight_view(transitions)
            self.transitions.arc_sort()
            self.transition_params = torch.nn.Parameter(torch.zeros(self.transitions.num_arcs()))
        else:
            self.transitions = None
            self.transition_params = None
        self.reduction = reduction

    def prepare(self, targets, device=None):
        """Start building, packing and uploading the alignment acceptors of a batch the criterion will see later -- on a
        side thread and a stream of its own; returns at once.  Hand the result to forward() in the place of `targets`:

            nxt = criterion.prepare(next_targets)        # e.g. right after the step's launches, or in the loader's collate
            loss = criterion(emissions, cur); loss.backward(); ...; cur = nxt

        (reference: transducer.py:262-281 runs this per step, inside forward.)  `device`: where the emissions will
        live (default: the current device)."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.tokens.arc_sort(True)
        C = self._num_emission_classes
        graph = None
        if self.transitions is not None:
            graph = _dispatch(self.transitions, C, self.transition_params.numel()).numerator
        return PreparedTargets(targets, _prepare(targets, self.tokens, self.lexicon, graph, C, dev, self.reduction),
                               len(targets))

    @E.on_input_device
    def forward(self, inputs, targets):
        self.tokens.arc_sort(True)
        if self.transitions is None:
            # transducer.py:186-187 applies log_softmax here; the engine fuses it into the gather
            # (forward) and the gradient rows (backward) instead of materialising [B,T,C] twice
            return E.make_eager(_FusedLogSoftmaxTransducerLoss.apply(inputs, targets, self.tokens, self.lexicon, None,
                                                                     None, self.reduction))
        return TransducerLoss(inputs, targets, self.tokens, self.lexicon, self.transition_params,
                              self.transitions, self.reduction)

    def _device_decode(self, C):
        self.tokens.arc_sort()  # (the order the host decode looks at the graph in, below)
        return _token_decode_plan(self.tokens, C)

    def _decode_plan(self, outputs):
        """What viterbi() and errors() decode, after the best frame-level path (under the transition model if any):
        ("emissions", x, drop, bias, flags) / ("paths", frames, drop, flags): the device decode's operands;
        ("host", labels, offsets): frame labels on the host, for wfl_transducer_decode_batch."""
        B, T, C = outputs.shape
        dev = E.require_gpu()
        x = E.as_device_f32(outputs.detach(), dev)
        kind = "none"
        if self.transitions is not None:
            params = E.as_device_f32(self.transition_params.detach(), dev)
            kind = _dispatch(self.transitions, C, params.numel()).kind
        if kind == "general":
            pack = _transitions_pack(self.transitions, B, C, dev)
            arc_paths, _ = E.lattice_viterbi(x, pack, weights=params)
            olab = self.transitions.arrays()["olabel"]
            # gtn.remove of the back-off arcs (transducer.py:218), for the whole batch at once
            lens = np.fromiter((0 if p is None else len(p) for p in arc_paths), np.int64, B)
            arcs = np.concatenate([p for p in arc_paths if p is not None and len(p)] or [np.zeros(0, np.int32)])
            labs = olab[arcs]
            keep = labs != G.epsilon
            offsets = np.zeros(B + 1, np.int64)
            np.cumsum(np.bincount(np.repeat(np.arange(B), lens)[keep], minlength=B), out=offsets[1:])
            return "host", np.ascontiguousarray(labs[keep], dtype=np.int32), offsets
        # (drop, flags) of the device decode, or None: the host decodes (a token graph that is not make_token_graph's,
        # labels outside its alphabet, emissions that came from the host)
        plan = self._device_decode(C) if outputs.is_cuda and B > 0 and T > 0 else None
        if kind == "bigram":
            # the fully connected recursion of the dense engine in the max-plus semiring (as the normaliser of the
            # loss takes its log-semiring one): its best state per frame IS the label path, no epsilon to remove
            frames = E.dense_viterbi(*_bigram_dense_operands(x, params, C))
            if plan is not None:
                return "paths", frames, plan[0], plan[1]
        else:
            if plan is not None:
                # argmax (of x + p under the unigram model), collapse and drop in one pass over x on the device
                return "emissions", x, plan[0], params if kind == "unigram" else None, plan[1]
            # viterbi_path of the bare emissions graph: per frame, the first maximal label -- of x + p under the
            # unigram model (one node, one self-loop per token)
            frames = E.row_argmax(x + params if kind == "unigram" else x)
        return "host", frames.cpu().numpy().reshape(-1), np.arange(B + 1, dtype=np.int64) * T

    def viterbi(self, outputs):
        """transducer.py:199-234: best frame-level path (under the transition model if any), then
        the shortest token sequence that path can transduce to."""
        plan = self._decode_plan(outputs)
        if plan[0] == "paths":
            return E.decode_paths(plan[1], plan[2], flags=plan[3])
        if plan[0] == "emissions":
            return E.decode_emissions(plan[1], plan[2], bias=plan[3], flags=plan[4])
        return self._host_decode(plan[1], plan[2])

    def _host_decode(self, labels, offsets):
        self.tokens.arc_sort()
        # one native call for the batch (the reference's gtn.parallel_for over process(b), transducer.py:232);
        # ambiguous decodings: the shortest wins (transducer.py:226-228)
        out, out_off = G.transducer_decode_batch(self.tokens, labels, offsets)
        flat = torch.from_numpy(out)  # (int32: torch.IntTensor, as transducer.py:233)
        return list(torch.split(flat, np.diff(out_off).tolist()))  # (views of one tensor: one call instead of B slices + clones)

    def _beam_plan(self, outputs, what, beam_size, classes_per_frame, nbest, lexicon=None, lm=None, lm_weight=1.0,
                   length_bonus=0.0, lm_eos=True, word_bonus=0.0, lookahead=None, token_lm=None):
        """The arguments of a beam search, checked before anything needs a device: (the E.TransducerBeamPlan of the
        options -- with a lexicon the E.TransducerLexiconBeamPlan; with a token_lm the E.TransducerLmBeamPlan, whose
        scalars lm_weight, length_bonus and lm_eos then are; with neither every keyword of the two must be at its
        default --, the transition model's kind: "none", "unigram" or "bigram")"""
        E.check_beam_outputs(outputs, what)
        self.tokens.arc_sort()
        n = ctypes.c_int()
        mode = N.lib.wfl_graph_token_kind(self.tokens._h, ctypes.byref(n))
        if mode not in (N.TOKENS_FORCED, N.TOKENS_OPTIONAL_NO_REPEATS):
            graph = {N.TOKENS_NONE: 'blank="none"', N.TOKENS_OPTIONAL: 'blank="optional" with repeats'}.get(mode, "this token graph")
            raise NotImplementedError(
                f"{what}: {graph} is ambiguous -- a frame path spells more than one token sequence (a repeated token "
                "multiplies alignments, so the sum over alignments favours [a, a, ...] over [a]), and a prefix search "
                'over it is no decoder; blank="optional" with allow_repeats=False and blank="forced" are searched')
        C = n.value + 1
        if outputs.shape[2] != C:
            raise ValueError(f"{what}: outputs have {outputs.shape[2]} classes, the criterion has {n.value} tokens and the blank")
        kind = "none"
        if self.transitions is not None:
            kind = _dispatch(self.transitions, C, self.transition_params.numel()).kind
            if kind == "general":
                raise NotImplementedError(f"{what}: the transition model is neither make_transitions_graph(1, C) nor "
                                          "(2, C): only no model, the unigram and the bigram model are searched")
        if token_lm is not None:
            if lexicon is not None:
                raise NotImplementedError(
                    f"{what}: token_lm together with a lexicon -- a token-level LM and a word LM over the same hypothesis "
                    "are two LM states and two terms per extension: a search of its own; give one of them")
            if lm is not None:
                raise ValueError(f"{what}: lm is the word LM of a lexicon; with token_lm there is none")
            if lookahead is not None:
                raise ValueError(f"{what}: lookahead needs a lexicon and its word lm, not a token_lm")
            if isinstance(word_bonus, bool) or not isinstance(word_bonus, numbers.Real) or float(word_bonus) != 0.0:
                raise ValueError(f"{what}: word_bonus needs a lexicon, got {word_bonus!r}")
            plan = E.TransducerLmBeamPlan.checked(C, n.value, mode == N.TOKENS_FORCED, beam_size, classes_per_frame, nbest,
                                                  token_lm, lm_weight, length_bonus, lm_eos, what)
        elif lexicon is None:
            if lookahead is not None:
                raise ValueError(f"{what}: lookahead needs a lexicon and its word lm")
            E.refuse_without_lexicon(what, lm, lm_weight, length_bonus, lm_eos, word_bonus, "a Transducer")
            plan = E.TransducerBeamPlan.checked(C, n.value, mode == N.TOKENS_FORCED, beam_size, classes_per_frame, nbest, what)
        else:
            plan = E.TransducerLexiconBeamPlan.checked(C, n.value, mode == N.TOKENS_FORCED, beam_size, classes_per_frame, nbest,
                                                       lexicon, lm, lm_weight, word_bonus, length_bonus, lm_eos, what,
                                                       lookahead=lookahead)
        return plan, kind

    def word_lexicon(self, words, wordsep=None, split=None, boundary="end", splits=None):
        """The lexicon.Lexicon of `words` for beam_search(lexicon=): a trie over sequences of the
        module's own tokens, for (n_tokens + 1, n_tokens) -- the emission classes and the blank of a token graph with a
        blank, which the module must have.  A word is split into its characters, or by split(word) into pieces; each
        piece must be one of the module's tokens, compared as tuple(piece) against tuple(token); with `wordsep` that
        token ends every spelling.  split= fixes ONE decomposition per word: the other decompositions of the same
        graphemes into word pieces are not in the trie.  ValueError names a word and its piece that is no token.
        boundary="start" (DESIGN.md section 26): a start-marked lexicon -- word pieces that carry the word boundary at
        the start of a word, words that are prefixes of one another; no wordsep then, and splits(word) -> a list of
        decompositions gives a word several spellings, each a hypothesis of its own in the search.
        (`Transducer.lexicon` is the criterion's token-to-grapheme graph, hence the name.)"""
        what = "Transducer.word_lexicon"
        if not self._has_blank:
            raise ValueError(f'{what}: blank="none" has no class for the blank a Lexicon is built around, and no beam search')
        if boundary not in ("end", "start"):
            raise ValueError(f"{what}: boundary {boundary!r} is neither 'end' nor 'start'")
        if boundary == "start" and wordsep is not None:
            raise ValueError(f"{what}: with boundary='start' the word boundary is part of the pieces: no wordsep")
        if splits is not None and boundary != "start":
            raise ValueError(f"{what}: splits (several decompositions of a word) needs boundary='start'")
        if splits is not None and split is not None:
            raise ValueError(f"{what}: split gives one decomposition per word, splits several: give one of them")
        index = {}
        for i, tok in enumerate(self._token_pieces):
            index.setdefault(tok, i)
        sep = None
        if wordsep is not None:
            sep = index.get(tuple(wordsep))
            if sep is None:
                raise ValueError(f"{what}: the word separator {wordsep!r} is not one of the module's tokens")
        words = list(words)
        spellings, word_of = [], []
        for v, w in enumerate(words):
            ways = [list(w) if split is None else list(split(w))] if splits is None else [list(d) for d in splits(w)]
            for pieces in ways:
                ids = []
                for piece in pieces:
                    i = index.get(tuple(piece))
                    if i is None:
                        raise ValueError(f"{what}: {piece!r} of {w!r} is not one of the module's tokens")
                    ids.append(i)
                spellings.append(ids + ([sep] if sep is not None else []))
                word_of.append(v)
        from ..lexicon import Lexicon

        n = len(self._token_pieces)
        if boundary == "start":
            return Lexicon(spellings, n + 1, n, words=words, boundary="start", word_of=word_of)
        return Lexicon(spellings, n + 1, n, words=words)

    def token_lm(self, path, bos="<s>", eos="</s>", unk="<unk>"):
        """The lm.NGramLM of an ARPA file over the module's own tokens for beam_search(token_lm=):
        NGramLM.from_arpa(path, the module's tokens in class order, blank=n_tokens) -- the emission classes and the
        blank of a token graph with a blank, which the module must have.  The ARPA file names a token as the module was
        given it."""
        if not self._has_blank:
            raise ValueError('Transducer.token_lm: blank="none" has no class for the blank an NGramLM is built around, and '
                             "no beam search")
        from ..lm import NGramLM

        return NGramLM.from_arpa(path, self._token_names, blank=len(self._token_names), bos=bos, eos=eos, unk=unk)

    @staticmethod
    def words(lexicon, labels):
        """The word ids of a token sequence that beam_search(lexicon=) returned: lexicon.words(labels)"""
        labels = labels.tolist() if hasattr(labels, "tolist") else list(labels)
        return lexicon.words([int(v) for v in labels])

    def _spelling(self, plan, what):
        """The E.Spelling of the plan's classes (the tokens' spellings, the blank's none), checked once and kept: ValueError
        for a token that spells nothing or more than E.SPELL_MAX graphemes.  Needs no device."""
        held = self._spelling_table
        rows = list(self.token_spellings)
        if held is None or held[0] != rows:
            for i, s in enumerate(rows):
                if not 1 <= len(s) <= E.SPELL_MAX:
                    raise ValueError(f"{what}: token {i} spells {len(s)} graphemes, merge_spellings takes tokens of 1 to "
                                     f"{E.SPELL_MAX}")
            table = E.Spelling.checked(rows[:plan.blank] + [None] + rows[plan.blank:], plan.blank, what)
            held = self._spelling_table = (rows, table)
        E.check_spelling(held[1], plan, what)
        return held[1]

    @staticmethod
    def _merge_flag(merge_spellings, what, lexicon=None, token_lm=None):
        if not isinstance(merge_spellings, (bool, np.bool_)):
            raise ValueError(f"{what}: merge_spellings must be True or False, got {merge_spellings!r}")
        if merge_spellings and token_lm is not None:
            raise NotImplementedError(
                f"{what}: merge_spellings=True with a token_lm -- the merged search sums the token sequences that spell the "
                "same graphemes into one hypothesis, while the LM's score and state depend on the token sequence: the "
                "members of a merged hypothesis carry different LM terms")
        if merge_spellings and lexicon is not None:
            raise NotImplementedError(
                f"{what}: merge_spellings=True with a lexicon -- the merged search identifies a hypothesis by the graphemes "
                "it spells, so one hypothesis stands for several token prefixes, while the trie node (and with it the LM "
                "state) is a function of the token prefix: the members of a merged hypothesis stand at different nodes")
        return bool(merge_spellings)

    def _beam_inputs(self, outputs, kind):
        """(emissions, transitions or None) of the search, as the routes of the loss form them (_dispatch): float32,
        contiguous, on the emissions' GPU or the required one (no host path)"""
        dev = outputs.device if outputs.is_cuda else E.require_gpu()
        x = outputs.detach().to(device=dev, dtype=torch.float32).contiguous()
        if kind == "none":
            return x, None
        params = E.as_device_f32(self.transition_params.detach(), dev).reshape(-1)
        if kind == "unigram":
            return x + params, None  # (_unigram_route)
        xd, Wd = _bigram_dense_operands(x, params, x.shape[2])
        return xd, Wd.contiguous()

    @E.on_input_device
    def beam_search(self, outputs, beam_size=16, classes_per_frame=None, nbest=1, return_scores=False,
                    merge_spellings=False, lexicon=None, lm=None, lm_weight=1.0, length_bonus=0.0, lm_eos=True, word_bonus=0.0,
                    lookahead=None, token_lm=None):
        """Transducer prefix beam search (an addition: the reference has viterbi() only).  viterbi() gives the best frame
        path; the criterion scores a token sequence by the sum over all its alignments, and this returns the token
        sequences it rates highest (DESIGN.md section 22 has the rules; csrc/beam_kernels.hip runs them, in float64).
        Per frame the `classes_per_frame` classes of highest emission score (default min(C, 32)) and the blank extend a
        hypothesis; `beam_size` (1..64) hypotheses survive a frame.  Only the unambiguous token graphs are searched --
        blank="optional" with allow_repeats=False, and blank="forced" --, with no transition model or the unigram or
        bigram one (`ngram` 0, 1, 2); everything else raises NotImplementedError.  Returns token indices with the blank
        dropped, in viterbi()'s dtype: nbest == 1: B CPU tensors; otherwise a list of `nbest` such tensors per utterance,
        best first (a rank beyond the result is empty).  return_scores: also a float64 CPU tensor [B, nbest]: the log
        mass of the token sequence's alignments that the beam kept, minus the normaliser of the loss (-inf for an empty
        rank).  For tokens that are single graphemes that is minus the criterion's loss of that target where nothing was
        pruned.  With word pieces the loss also sums over the other decompositions of the same graphemes, so the score
        is a lower bound of minus the loss; two token sequences that spell the same graphemes are separate hypotheses
        unless `merge_spellings`.
        merge_spellings=True: hypotheses are identified by the graphemes they spell (and their
        last token), and the masses of all decompositions of those graphemes into tokens are summed inside the beam
        launch.  A returned sequence is then a REPRESENTATIVE -- one token sequence that spells the result --, and the
        score belongs to its spelling: the kept log mass of every alignment of every decomposition, minus the
        normaliser -- minus the criterion's loss of that grapheme target where nothing was pruned, a lower bound
        otherwise, and never below the score of any single decomposition.  No two ranks spell the same graphemes.  The
        return types do not change.  A token that spells nothing, or more than 64 graphemes, raises ValueError.
        B == 0 or T == 0: empty sequences with score 0, no device needed.
        lexicon: a lexicon.Lexicon built by self.word_lexicon() -- only sequences of its words are
        returned (every result is a whole number of words; self.words(lexicon, labels) names them), and lm (optional) is
        a word LM over its word ids (NGramLM.from_arpa(path, words, blank=len(words))).  A token adds length_bonus, a
        completed word lm_weight * step(s, word) + word_bonus on top, and lm_eos lm_weight * step(s, </s>) after the last
        frame; the scores include these terms.  With word pieces a lexicon built with split= fixes one decomposition per
        word: the score is the kept mass of that token sequence's alignments, a lower bound of minus the loss as
        without a lexicon, and the criterion's other decompositions of the same graphemes are not searched.  A lexicon
        with merge_spellings=True raises NotImplementedError.  Without a lexicon the call is what it was, and lm,
        lm_weight, length_bonus, lm_eos and word_bonus must be at their defaults (ValueError).  B == 0 or T == 0 with a
        lexicon: the empty sequence, scored by the LM's </s> alone.  A start-marked lexicon (word_lexicon(...,
        boundary="start"), DESIGN.md section 26: word pieces that carry the word boundary at the start of a word, words
        that are prefixes of one another, several spellings of a word through splits=) is taken as it is: a word ends
        where the next begins or with the utterance, two spellings of the same words are separate hypotheses, and a
        hypothesis is ranked without the LM term of its last, unfinished word until then.  lookahead (DESIGN.md section
        27; it needs a lexicon and an lm): "unigram" or an array of one finite score per word -- lm_weight times the best
        score of the words below a trie node is paid provisionally while a word is being spelled and settled where the
        word ends, so that a narrow beam ranks a hypothesis by the word the LM wants; unpruned the results are those
        without it.
        token_lm: an lm.NGramLM over the module's own classes (self.token_lm(path) reads one from
        an ARPA file; num_classes == n_tokens + 1, blank == n_tokens) -- shallow fusion with an n-gram LM over the tokens
        themselves: no vocabulary, and words that no lexicon lists.  lm_weight, length_bonus and lm_eos are then its
        scalars, as in CTC.beam_search(lm=) without a lexicon: a token c behind LM state s adds lm_weight * step(s, c) +
        length_bonus, lm_eos lm_weight * step(s, </s>) after the last frame; the scores include these terms.  `lm`
        remains the word LM of a lexicon: lm=, word_bonus or lookahead with a token_lm raise ValueError, a token_lm with a
        lexicon or with merge_spellings=True NotImplementedError.  B == 0 or T == 0 with a token_lm: the empty sequence,
        scored by the LM's </s> alone.  No input lengths."""
        what = "Transducer.beam_search"
        plan, kind = self._beam_plan(outputs, what, beam_size, classes_per_frame, nbest, lexicon, lm, lm_weight, length_bonus,
                                     lm_eos, word_bonus, lookahead, token_lm)
        # (the plan knows its search; merging by spelling is the plain plan's, with the tokens' Spelling)
        merged = {"spelling": self._spelling(plan, what)} if self._merge_flag(merge_spellings, what, lexicon, token_lm) else {}
        if outputs.shape[0] == 0 or outputs.shape[1] == 0:
            hyps, scores = plan.no_frames(outputs.shape[0], torch.int32)
        else:
            x, Wt = self._beam_inputs(outputs, kind)
            with torch.cuda.device(x.device), torch.no_grad():
                hyps, scores = plan.search(x, Wt, True, torch.int32, **merged)
        if plan.nbest == 1:
            hyps = [h[0] for h in hyps]
        return (hyps, scores) if return_scores else hyps

    @E.on_input_device
    def errors(self, outputs, targets, counter, *, beam_size=None, classes_per_frame=None, merge_spellings=False, lexicon=None,
               lm=None, lm_weight=1.0, length_bonus=0.0, lm_eos=True, word_bonus=0.0, lookahead=None, token_lm=None):
        """compute_edit_distance(self.viterbi(outputs), targets, preprocessor) (train.py:74-87, 278-284) as
        (tokens_dist, words_dist, n_tokens, n_words), with `counter` a metrics.ErrorCounter: where viterbi() decodes on
        the device the count runs behind the same decode and the predictions never reach the host.  `beam_size` (an
        addition): the predictions are beam_search(outputs, beam_size, classes_per_frame)'s instead, counted behind the
        beam launches on their device buffers; `classes_per_frame` and `merge_spellings` (beam_search's: the predictions
        are the representatives of the best spellings) need a beam_size.  lexicon, lm, lm_weight, length_bonus, lm_eos,
        word_bonus, lookahead: beam_search's, with a beam_size: the predictions are those of the search with a lexicon.
        token_lm: beam_search's, with a beam_size: the predictions are those of the search with a token-level LM."""
        merge = self._merge_flag(merge_spellings, "Transducer.errors", lexicon, token_lm)
        if beam_size is None and lookahead is not None:
            raise ValueError("Transducer.errors: lookahead needs a beam_size")
        if beam_size is None and token_lm is not None:
            raise ValueError("Transducer.errors: token_lm needs a beam_size")
        if beam_size is None:
            if classes_per_frame is not None or merge:
                raise ValueError("Transducer.errors: classes_per_frame and merge_spellings need a beam_size")
            if lexicon is not None:
                raise ValueError("Transducer.errors: lexicon needs a beam_size")
            E.refuse_without_lexicon("Transducer.errors", lm, lm_weight, length_bonus, lm_eos, word_bonus, "a Transducer")
        else:
            plan, kind = self._beam_plan(outputs, "Transducer.errors", beam_size, classes_per_frame, 1, lexicon, lm, lm_weight,
                                         length_bonus, lm_eos, word_bonus, lookahead, token_lm)
            merged = {"spelling": self._spelling(plan, "Transducer.errors")} if merge else {}
            counter.check_hypothesis_labels(plan.C - 1, "Transducer.errors")  # (the blank is never a label of a result)
            if outputs.shape[0] == 0 or outputs.shape[1] == 0:
                return counter([h[0] for h in plan.no_frames(outputs.shape[0], torch.int32)[0]], targets)
            x, Wt = self._beam_inputs(outputs, kind)
            with torch.cuda.device(x.device), torch.no_grad():
                return counter.totals(M.plan_errors(counter, targets, x, plan, Wt, **merged))
        C = outputs.shape[2]
        dplan = self._device_decode(C)
        # (a blank in the last column is never emitted)
        counter.check_hypothesis_labels(C - 1 if dplan is not None and dplan[0] == C - 1 else C, "Transducer.errors")
        with torch.no_grad():
            plan = self._decode_plan(outputs)
            if plan[0] == "paths":
                return counter.totals(M.decode_paths_errors(counter, targets, plan[1], plan[2], flags=plan[3]))
            if plan[0] == "emissions":
                return counter.totals(M.decode_emissions_errors(counter, targets, plan[1], plan[2], bias=plan[3], flags=plan[4]))
            return counter(self._host_decode(plan[1], plan[2]), targets)


def _token_decode_plan(tokens, C):
    """(drop, flags) with which the device decode (wfl_decode_emissions / wfl_decode_paths) transduces frame labels below
    C through `tokens` exactly as wfl_transducer_decode_batch does -- collapse repeats, drop the blank, within what the
    graph accepts (csrc/graph.cpp::token_decode) --, or None: `tokens` is none of make_token_graph's four graphs, or
    labels below C lie outside its alphabet (the host composes those)."""
    n = ctypes.c_int()
    mode = N.lib.wfl_graph_token_kind(tokens._h, ctypes.byref(n))
    if mode < 0:
        return None
    blank = None if mode == N.TOKENS_NONE else n.value
    if C > n.value + (blank is not None):
        return None
    if blank is not None and blank >= C:  # (emissions without a column for the blank)
        if mode == N.TOKENS_FORCED:
            return None
        blank = None
    return blank, N.DECODE_BLANK_SEPARATED if mode == N.TOKENS_FORCED else 0


def _dense_unigram(transitions, C):
    """True iff `transitions` is make_transitions_graph(1, C) (transducer.py:32-58 with ngram = 1): one start + accept
    node with a self-loop per token, arc i labelled i."""
    if transitions.num_nodes() != 1 or transitions.num_arcs() != C:
        return False
    a = transitions.arrays()
    idx = np.arange(C)
    return bool(a["start"][0] and a["accept"][0] and (a["src"] == 0).all() and (a["dst"] == 0).all()
                and (a["ilabel"] == idx).all() and (a["olabel"] == idx).all())


def _dense_bigram(transitions, C):
    """True iff `transitions` has exactly the structure of make_transitions_graph(2, C) (transducer.py:32-58): start
    node 0, one node per previous token, C start arcs, C x C bigram arcs `prev a -> cur b` at arc C + a C + b, and
    an epsilon arc from every node to the accepting end node.  Its normaliser
    forward_score(intersect(emissions, transitions)) (transducer.py:286-288) is then the fully connected recursion of
    the dense engine (csrc/dense_kernels.hip) with W[0] = start scores, W[1+b][a] = bigram score and the end
    arcs' scores added to the last frame -- instead of the general lattice sweep with (C+1) C^2 arcs."""
    if transitions.num_nodes() != C + 2 or transitions.num_arcs() != C + C * C + C + 1:
        return False
    a = transitions.arrays()
    idx = np.arange(C, dtype=np.int64)
    ab = np.arange(C * C, dtype=np.int64)
    eps = np.arange(C + 1, dtype=np.int64)
    s, d, il, ol = (np.asarray(a[k]) for k in ("src", "dst", "ilabel", "olabel"))
    n0, n1 = C, C + C * C
    st, ac = np.flatnonzero(np.asarray(a["start"])), np.flatnonzero(np.asarray(a["accept"]))  # (per-node flags)
    return bool(st.tolist() == [0] and ac.tolist() == [C + 1]
                and (s[:n0] == 0).all() and (d[:n0] == 1 + idx).all() and (il[:n0] == idx).all() and (ol[:n0] == idx).all()
                and (s[n0:n1] == 1 + ab // C).all() and (d[n0:n1] == 1 + ab % C).all() and (il[n0:n1] == ab % C).all()
                and (ol[n0:n1] == ab % C).all()
                and (s[n1:] == eps).all() and (d[n1:] == C + 1).all() and (il[n1:] == G.epsilon).all() and (ol[n1:] == G.epsilon).all())


def _bigram_numerator_graph(transitions, C):
    """The transition graph the NUMERATOR's alignments are intersected with when the Transducer carries the dense
    bigram model (_bigram_route).  make_transitions_graph(2, C) reaches its accepting node through one epsilon arc per
    history (transducer.py:32-58), so every alignment acceptor ends in an epsilon arc -- and an acceptor with an epsilon
    arc is swept in the log domain by the general kernels (0.37 + 0.22 ms at the n-gram benchmark's shape against
    0.05 + 0.07 for the same acceptor without it).  That arc's score depends on the LAST emitted label only (node 1 + c
    after label c), so it is the dense normaliser's trick again: the end arcs' scores ride on the last frame's emissions
    and the graph loses its epsilon arcs -- every node accepts instead.  The remaining arcs are laid out like the dense
    engine's matrix W [(C+1), C] row-major (include/wfl.h): arc c = start -> c, arc (1 + b) C + a = bigram a -> b, so that
    numerator and normaliser read their weights from ONE tensor, as ASG's do."""
    a = transitions.arrays()
    idx = np.arange(C, dtype=np.int32)
    prev = np.tile(idx, C)    # a: fastest
    cur = np.repeat(idx, C)   # b
    src = np.concatenate([np.zeros(C, np.int32), 1 + prev])
    dst = np.concatenate([1 + idx, 1 + cur])
    lab = np.concatenate([idx, cur])
    g = G.Graph(False)
    g.add_nodes(np.asarray(a["start"]), np.ones(C + 2, dtype=np.asarray(a["accept"]).dtype))
    g.add_arcs(src, dst, lab, lab)
    return g


# What a transition graph is, structurally, for C emission classes.  kind: "unigram" (make_transitions_graph(1, C)),
# "bigram" (make_transitions_graph(2, C)) or "general"; numerator: the graph the numerator's alignments are intersected
# with -- None for the unigram model (its scores are added to the emissions: _unigram_route), _bigram_numerator_graph for
# the bigram model, the graph itself otherwise.
_TransitionModel = collections.namedtuple("_TransitionModel", "kind numerator")
_MODELS = E.LRU(64)


def _transition_model(transitions, C):
    """The _TransitionModel of (transitions, C): classified arc by arc once, then looked up."""
    def build():
        if _dense_unigram(transitions, C):
            model = _TransitionModel("unigram", None)
        elif _dense_bigram(transitions, C):
            model = _TransitionModel("bigram", _bigram_numerator_graph(transitions, C))
        else:
            model = _TransitionModel("general", transitions)
        return model, transitions  # (holds the graph: its id stays unique)

    return _MODELS.get((id(transitions), C), build)[0]


def _dispatch(transitions, C, num_params):
    """The _TransitionModel the loss, prepare() and viterbi() of a criterion with `transitions` act on: the graph's own
    where a dense route may take it -- the WFL_DENSE_NGRAM switch is on and there is one parameter per arc -- and the
    general one otherwise."""
    model = _transition_model(transitions, C)
    if model.kind != "general" and not (_DENSE_NGRAM and num_params == transitions.num_arcs()):
        return _TransitionModel("general", transitions)
    return model


def _numerator_entry(targets, tokens, lexicon, graph, C, dev, reduction, B):
    """The packed alignment acceptors of a batch (their cache entry): from a PreparedTargets handle if it was made for
    this criterion and device, else packed here."""
    if isinstance(targets, PreparedTargets):
        nb, entry = targets.result()
        pack = entry[0]
        if pack.desc.B != B or pack.device != dev or entry[4] != (tokens, lexicon, graph):
            # prepared for other emissions (another device, another criterion): pack again, here
            nb, entry = _pack_entry(targets.targets, tokens, lexicon, graph, C, dev, reduction)
    else:
        nb, entry = _pack_entry(targets, tokens, lexicon, graph, C, dev, reduction)
    if nb != B:
        raise ValueError(f"got {nb} targets for a batch of {B}")
    pack = entry[0]
    if pack.order_behind_upload():
        # uploaded on another stream (the prefetch thread's, or an earlier step's): its memory stays this stream's too
        pack._blob.record_stream(torch.cuda.current_stream())
    return entry


def _bigram_dense_operands(x, params, C):
    """(emissions with the end arcs' scores on the last frame, W [(C+1), C] of the dense engine) for the bigram
    transition model: params = [start C | bigram a -> b at C + a C + b | end arcs of nodes 0 .. C]"""
    n1 = C + C * C
    Wd = torch.cat([params[:C].view(1, C), params[C:n1].view(C, C).t()], dim=0)
    xd = x.clone()
    xd[:, -1, :] += params[n1 + 1:]
    return xd, Wd


def _bigram_route(inputs, targets, tokens, lexicon, transition_params, numerator, reduction):
    """TransducerLoss with the dense bigram model as the ASG step it is; `numerator`: the model's numerator graph
    (_bigram_numerator_graph).  Emissions with the end arcs' scores on the last frame and the matrix W of the dense
    engine are formed from `transition_params` (_bigram_dense_operands), and ASGLoss (one native call:
    csrc/torch_ops.cpp::asg_forward) does the rest."""
    from . import asg as _asg

    B, T, C = inputs.shape
    dev = E.require_gpu()
    with torch.cuda.device(dev):
        pack, scale, cpos, cneg, _ = _numerator_entry(targets, tokens, lexicon, numerator, C, dev, reduction, B)
    return _BigramAsAsg.apply(inputs, transition_params, _asg.PackedNumerator(pack, scale, cpos, cneg, B))


class _BigramAsAsg(torch.autograd.Function):
    """_bigram_route's step as ONE autograd node: the operands of the ASG step from (emissions, transition_params) --
    three small torch ops -- the ASG step on them (asg.Step: csrc/torch_ops.cpp::asg_forward), and in backward its
    two gradients mapped back to the caller's tensors.  (Spelled with differentiable torch ops around ASGLoss the step
    carried eight more autograd nodes: ~0.1 ms of host time where the step is host-bound.)"""

    @staticmethod
    @E.on_input_device
    def forward(ctx, inputs, transition_params, packed):
        from . import asg as _asg

        B, T, C = inputs.shape
        dev = E.require_gpu()
        xd, Wd = _bigram_dense_operands(E.as_device_f32(inputs.detach(), dev),
                                        E.as_device_f32(transition_params.detach(), dev).reshape(-1), C)
        # (requires_grad tells the step which gradients it will be asked for -- the end arcs' gradient is the last frame's
        # rows of the emission gradient, so the parameters alone ask for that too; its early gradients are not offered)
        xd.requires_grad_(inputs.requires_grad or transition_params.requires_grad)
        Wd.requires_grad_(transition_params.requires_grad)
        ctx.bigram = (C, inputs.device, transition_params.device, transition_params.shape)
        loss, ctx.step = _asg.Step.forward(xd, Wd, packed, "none")
        return loss if inputs.is_cuda else loss.cpu()

    @staticmethod
    @E.on_input_device
    def backward(ctx, grad_output):
        C, in_dev, par_dev, par_shape = ctx.bigram
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dxd, dWd = ctx.step.backward(grad_output, need_x or need_p, need_p)
        dp = None
        if need_p:
            # the end arcs' scores rode on the last frame's emissions: their gradient is that frame's rows, summed
            # (the emission gradient is computed for it even when the caller's emissions ask for none)
            end = dxd[:, -1, :].sum(dim=0)
            dp = torch.cat([dWd[0], dWd[1:].t().reshape(-1), end.new_zeros(1), end]).reshape(par_shape)
        return E.on_device_of(dxd if need_x else None, in_dev), E.on_device_of(dp, par_dev), None


def _transitions_pack(transitions, B, C, device):
    key = ("den", id(transitions), B, C, device.index)

    def build():
        wid = np.arange(transitions.num_arcs(), dtype=np.int32)
        return E.PackedLattice.from_graphs([transitions], C, device, wids=[wid], B=B, shared=True), transitions

    return _PACK_CACHE.get(key, build)[0]


# what TransducerLossFunction.forward leaves on its node for backward: the emissions, the transition parameters (None
# without transitions), the LatticeStates of numerator and normaliser (None without transitions), the gradient factors
_Saved = collections.namedtuple("_Saved", "x params num den cpos cneg")

# the launch groups of a step without a transition model, in the order csrc/torch_ops.cpp::lattice_loss_forward takes
# their timing events
_PHASES = ("lattice_gather", "lattice_chain")


class TransducerLossFunction(torch.autograd.Function):
    """transducer.py:237-343, the general path: the numerator's alignments intersected with `transitions` as they are
    and both forward scores on the lattice engine, whatever the transition model (TransducerLoss is what routes the dense
    n-gram models elsewhere).  Backward finds the forward's state on the node as `ctx.aux`, a _Saved."""

    @staticmethod
    @E.on_input_device
    def forward(ctx, inputs, targets, tokens, lexicon, transition_params=None, transitions=None,
                reduction="none"):
        return TransducerLossFunction._forward(ctx, False, inputs, targets, tokens, lexicon, transition_params,
                                               transitions, reduction)

    @staticmethod
    def _forward(ctx, log_softmax, inputs, targets, tokens, lexicon, transition_params, transitions, reduction):
        B, T, C = inputs.shape
        if transitions is not None and transition_params is None:
            raise ValueError("Specified transitions, but not transition params.")
        if T == 0:
            raise ValueError("TransducerLoss: empty emissions (T == 0)")
        dev = E.require_gpu()
        x = E.as_device_f32(inputs.detach(), dev)
        params = E.as_device_f32(transition_params.detach(), dev) if transitions is not None else None
        pack, scale, cpos, cneg, _ = _numerator_entry(targets, tokens, lexicon, transitions, C, dev, reduction, B)
        need_grad = inputs.requires_grad or (transition_params is not None and transition_params.requires_grad)
        if transitions is None:
            # gather, sweeps, loss reduction and join in one native call (csrc/torch_ops.cpp::lattice_loss_forward).
            # The emission gradient is the whole backward pass here: the sweeps' launch computes it for grad_output = 1
            # as it goes when it can (in_launch), backward scales it and patches what is left.
            want_dx = inputs.requires_grad and _IN_LAUNCH_GRAD
            phases = E.phase_events("transducer", _PHASES)  # (None: no launch group of this step is timed)
            (loss, xg, al, be, lz, lse, dx_early), in_launch = N.ops.lattice_loss_forward(
                x, ctypes.addressof(pack.desc), pack.ints, pack.floats, scale, cneg, bool(log_softmax), want_dx, need_grad,
                phases or [])
            num = E.LatticeState()
            num.pack, num.T, num.C, num.weights, num.bptr = pack, T, C, None, None
            num.xg, num.alpha, num.beta, num.logz = xg, al, be, lz
            num.x, num.row_lse = (x if log_softmax else None), lse
            ctx.aux = _Saved(x, None, num, None, cpos, cneg)
            ctx.devices = (inputs.device, None)
            early = E.EarlyGrads((inputs,), (dx_early,), lambda gout, bufs: E.lattice_grad_rest(
                num, cneg, gout, bufs[0])) if in_launch else None
            E.hold_early(ctx, early, in_launch and E.may_hand_over(inputs))
            return loss if inputs.is_cuda else loss.cpu()
        # normaliser: forward_score(emissions o transitions), transducer.py:286-288, independent of the numerator sweep:
        # forked onto a second stream so that the two overlap
        with E.side_stream(dev) as fork:
            den = E.lattice_forward(x, _transitions_pack(transitions, B, C, dev), weights=params, need_beta=need_grad)
        num = E.lattice_forward(x, pack, weights=params, need_beta=need_grad, log_softmax=log_softmax)
        fork.join(den.xg, den.alpha, den.beta, den.logz)
        loss = E.reduce_loss(den.logz, scale, 1.0, minus=num.logz)
        ctx.aux = _Saved(x, params, num, den, cpos, cneg)
        E.hold_early(ctx, None, False)
        ctx.devices = (inputs.device, transition_params.device)
        return loss if inputs.is_cuda else loss.cpu()

    @staticmethod
    @E.on_input_device
    def backward(ctx, grad_output):
        E.check_not_released(ctx)
        # the launch of the sweeps wrote the gradient for grad_output = 1: scaled in place, then the rows of the utterances
        # that launch did not serve.  A second pass over a retained graph finds the buffer gone and recomputes below.
        early = ctx.early.claim(grad_output) if ctx.early is not None else None
        if early is not None:
            return E.on_device_of(early[0], ctx.devices[0]), None, None, None, None, None, None
        x, params, num, den, cpos, cneg = ctx.aux
        gout = E.as_device_f32(grad_output.detach().reshape(1), x.device)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.zeros_like(params) if (params is not None and ctx.needs_input_grad[4]) else None
        if dx is not None or dW is not None:
            E.lattice_grad(num, cneg, coef_w=cneg, gout=gout, dx=dx, accumulate=False, dW=dW)
            if den is not None:
                E.lattice_grad(den, cpos, coef_w=cpos, gout=gout, dx=dx, accumulate=True, dW=dW)
        return E.on_device_of(dx, ctx.devices[0]), None, None, None, E.on_device_of(dW, ctx.devices[1]), None, None


class _FusedLogSoftmaxTransducerLoss(TransducerLossFunction):
    """TransducerLoss(log_softmax(inputs), ...) without transitions, as one operator: the gather
    subtracts the rows' log-sum-exp, the gradient kernel differentiates through it."""

    @staticmethod
    @E.on_input_device
    def forward(ctx, inputs, targets, tokens, lexicon, transition_params=None, transitions=None,
                reduction="none"):
        return TransducerLossFunction._forward(ctx, True, inputs, targets, tokens, lexicon, transition_params,
                                               transitions, reduction)


_IN_LAUNCH_GRAD = os.environ.get("WFL_TRANSDUCER_IN_LAUNCH_GRAD", "1") != "0"  # (0: gradient in backward -- A/B, tests)


def _unigram_route(inputs, targets, tokens, lexicon, transition_params, reduction):
    """TransducerLoss with the unigram model (make_transitions_graph(1, C): one node, a self-loop per label) as the
    transition-free step on other emissions.  Every arc with label c carries p_c in numerator and
    normaliser alike, so with x' = x + p the normaliser is  sum_t logsumexp_c x'[t]  and the loss is the negated
    numerator score of log_softmax(x') -- the fused log_softmax criterion (one native call, the gradient beside the
    sweeps); autograd sums the emission gradient over (b, t) into `transition_params`."""
    x = inputs if inputs.dtype == torch.float32 else inputs.float()
    p = transition_params.to(device=x.device, dtype=torch.float32)
    return E.make_eager(_FusedLogSoftmaxTransducerLoss.apply(x + p, targets, tokens, lexicon, None, None, reduction))


def TransducerLoss(inputs, targets, tokens, lexicon, transition_params=None, transitions=None, reduction="none"):
    """transducer.py:346 (`TransducerLoss = TransducerLossFunction.apply`): same call, same result -- the dense n-gram
    models by their own routes (_dispatch)."""
    if transitions is not None and transition_params is not None and inputs.dim() == 3 and inputs.shape[1] > 0:
        model = _dispatch(transitions, inputs.shape[2], transition_params.numel())
        if model.kind == "unigram":
            return _unigram_route(inputs, targets, tokens, lexicon, transition_params, reduction)
        if model.kind == "bigram":
            return _bigram_route(inputs, targets, tokens, lexicon, transition_params, model.numerator, reduction)
    return E.make_eager(TransducerLossFunction.apply(inputs, targets, tokens, lexicon, transition_params, transitions,
                                                     reduction))


# -------------------------------------------------------------------------------------------------
# ConvTransduce1D (transducer.py:370-556)
# -------------------------------------------------------------------------------------------------
class _KernelTable:
    """Device description of a lexicon for csrc/conv_kernels.hip (layout: include/wfl.h).  Arc ids
    follow the insertion order of make_kernel_graph, which is also the layout of `kernel_params`
    (transducer.py:474-483 hands consecutive slices of it to the kernels' arc weights)."""

    def __init__(self, lexicon, blank_optional, spike):
        self.lexicon = [tuple(int(c) for c in tok) for tok in lexicon]
        self.blank_optional, self.spike = bool(blank_optional), bool(spike)
        tab = np.zeros((len(self.lexicon), 36), dtype=np.int32)
        ns = 0 if spike else 1
        n = 0
        for k, tok in enumerate(self.lexicon):
            if len(tok) > 15:
                raise ValueError(f"ConvTransduce1D: lexicon entry {k} has {len(tok)} sub-tokens (limit 15)")
            tab[k, 0] = len(tok)
            tab[k, 34] = n  # arc 0 -> 0
            n += 1
            for i, c in enumerate(tok):
                tab[k, 2 + i] = c
                tab[k, 18 + i] = n
                skip = i > 0 and blank_optional and tok[i - 1] != c
                if skip:
                    tab[k, 1] |= 1 << i
                n += 3 + ns + int(skip)
        self.table, self.num_arcs = tab, n
        toks = [c for tok in self.lexicon for c in tok]
        self.min_tok, self.max_tok = (min(toks), max(toks)) if toks else (0, 0)  # checked against C in the forward
        self.flags = (N.CONV_SPIKE if spike else 0) | (N.CONV_BLANK_OPTIONAL if blank_optional else 0)
        self._dev = {}

    def on(self, device):
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = torch.from_numpy(self.table).to(device)
        return t

    def check_classes(self, C):
        """Every sub-token and the blank index must name one of a row's C classes: the kernels index a window's LDS
        copy with them, unchecked (the reference scores an entry with a label no emission carries -inf: DESIGN.md 3.4)."""
        blank = self.blank_idx
        if not 0 <= blank < C:
            raise ValueError(f"ConvTransduce1D: blank_idx {blank} is outside the input's {C} classes")
        if self.min_tok < 0 or self.max_tok >= C:
            k, c = next((k, c) for k, tok in enumerate(self.lexicon) for c in tok if not 0 <= c < C)
            raise ValueError(f"ConvTransduce1D: lexicon entry {k} {self.lexicon[k]} has sub-token {c}, outside the "
                             f"input's {C} classes")


class ConvTransduce1DFunction(torch.autograd.Function):
    """transducer.py:461-552.  `kernels` is the lexicon table built by ConvTransduce1D (a list of
    kernel graphs made by make_kernel_graph is accepted too and converted).  Unlike the reference
    there is no process-global CTX_GRAPHS: everything backward needs lives on `ctx` (re-entrant)."""

    @classmethod
    def apply(cls, inputs, kernels, kernel_size, stride, kernel_params=None, viterbi=False):
        # The backward keeps the window and its gradient rows in LDS, twice the forward's bytes: a shape only the
        # forward has room for is refused before the forward runs, not in the middle of autograd.  (Asked here: inside
        # forward() grad mode is off and ctx.needs_input_grad ignores torch.no_grad().)
        if (torch.is_grad_enabled() and inputs.dim() == 3
                and any(t is not None and t.requires_grad for t in (inputs, kernel_params))):
            C = inputs.shape[2]
            if 1 <= kernel_size <= 16 and 2 * kernel_size * C * 4 > N.lib.wfl_conv_lds_limit():  # (conv_check's test)
                raise N.WflUnsupported(N.ERR_UNSUPPORTED, f"conv_grad: window of {kernel_size} frames x {C} classes "
                                                          "does not fit LDS")
        return super().apply(inputs, kernels, kernel_size, stride, kernel_params, viterbi)

    @staticmethod
    @E.on_input_device
    def forward(ctx, inputs, kernels, kernel_size, stride, kernel_params=None, viterbi=False):
        B, T, C = inputs.shape
        if T < kernel_size:  # padding should be done outside of this function (transducer.py:468-470)
            raise ValueError(f"Input ({T}) too short for kernel ({kernel_size})")
        if not isinstance(kernels, _KernelTable):
            raise TypeError("ConvTransduce1DFunction: pass the ConvTransduce1D module's kernel table")
        kernels.check_classes(C)
        dev = E.require_gpu()
        x = E.as_device_f32(inputs.detach(), dev)
        params = E.as_device_f32(kernel_params.detach(), dev) if kernel_params is not None else None
        if params is not None and params.numel() != kernels.num_arcs:
            raise ValueError(f"kernel_params has {params.numel()} entries, the kernels have {kernels.num_arcs} arcs")
        tab = kernels.on(dev)
        K = tab.shape[0]
        blank = kernels.blank_idx
        Tout = (T - kernel_size) // stride + 1
        out = torch.empty((B, Tout, K), dtype=torch.float32, device=dev)
        sr = N.SEMIRING_TROPICAL if viterbi else N.SEMIRING_LOG
        N.check(N.lib.wfl_conv_forward(E.ptr(x), B, T, C, E.ptr(tab), K, kernel_size, stride, blank, kernels.flags,
                                       E.ptr(params), sr, E.ptr(out), E.stream_ptr()))
        ctx.aux = (x, params, tab, kernels, kernel_size, stride, sr)
        ctx.devices = (inputs.device, None if kernel_params is None else kernel_params.device)
        return out if inputs.is_cuda else out.to(inputs.device)

    @staticmethod
    @E.on_input_device
    def backward(ctx, grad_output):
        x, params, tab, kernels, kernel_size, stride, sr = ctx.aux
        B, T, C = x.shape
        delta = E.as_device_f32(grad_output.detach(), x.device)
        dx = torch.empty_like(x)
        dparams = torch.zeros_like(params) if (params is not None and ctx.needs_input_grad[4]) else None
        N.check(N.lib.wfl_conv_grad(E.ptr(x), B, T, C, E.ptr(tab), tab.shape[0], kernel_size, stride,
                                    kernels.blank_idx, kernels.flags, E.ptr(params), sr, E.ptr(delta), E.ptr(dx),
                                    E.ptr(dparams), E.stream_ptr()))
        return E.on_device_of(dx, ctx.devices[0]), None, None, None, E.on_device_of(dparams, ctx.devices[1]), None


class ConvTransduce1D(torch.nn.Module):
    """A 1D convolutional transducer layer (transducer.py:370-457): every lexicon entry is a small
    alignment graph over the previous layer's tokens, slid over the input like a convolution."""

    def __init__(self, lexicon, kernel_size, stride, blank_idx, blank_optional=True, learn_params=False,
                 scale="none", normalize="none", viterbi=False, spike=False):
        super().__init__()
        self.normalize = normalize
        self.viterbi = viterbi
        if scale == "none":
            self.scale = 1.0
        elif scale == "sqrt":
            self.scale = math.sqrt(kernel_size)
        elif scale == "linear":
            self.scale = kernel_size
        else:
            raise ValueError(f"Unknown scale {scale}")
        if normalize not in ["none", "pre", "post"]:
            raise ValueError(f"Unknown normalization {normalize}")
        self.kernel_size = kernel_size
        assert self.kernel_size % 2 != 0, "Use an odd kernel size for easy padding."
        self.stride = stride

        def size_with_rep(token):
            return len(token) + sum(t1 == t2 for t1, t2 in zip(token[:-1], token[1:]))

        min_kernel_size = max(size_with_rep(l) for l in lexicon)
        if kernel_size < min_kernel_size:
            raise ValueError(f"Kernel size needed of at least {min_kernel_size}.")
        self.kernels = _KernelTable(lexicon, blank_optional, spike)
        self.kernels.blank_idx = int(blank_idx)
        self.kernel_params = None
        if learn_params:
            self.kernel_params = torch.nn.Parameter(torch.zeros(self.kernels.num_arcs))

    @E.on_input_device
    def forward(self, inputs):
        # inputs are of shape [B, T, C]
        pad = self.kernel_size // 2
        inputs = torch.nn.functional.pad(inputs, (0, 0, pad, pad))
        if self.normalize == "pre":
            inputs = torch.nn.functional.log_softmax(inputs, dim=2)
        outputs = ConvTransduce1DFunction.apply(inputs, self.kernels, self.kernel_size, self.stride,
                                                self.kernel_params, self.viterbi)
        outputs = outputs / self.scale
        if self.normalize == "post":
            outputs = torch.nn.functional.softmax(outputs, dim=2)
        if self.normalize == "pre":
            outputs = outputs.exp()
        return outputs
