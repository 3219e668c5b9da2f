"""ASG criterion -- counterpart of /root/reference/criterions/asg.py.

loss_b = forward_score(emissions o transitions) - forward_score(force_align o transitions o emissions)
(asg.py:111-115).  The denominator runs on the dense-transition kernels (csrc/dense_kernels.hip),
the numerator on the lattice engine with arcs that index the (C+1) x C transition matrix; the
reference's per-sample rebuild of the C^2-arc transitions graph (asg.py:54-69,103) disappears: the
transitions tensor is the graph.
"""
import ctypes
import itertools
import numbers
import os

import torch

from .. import _native as N
from .. import engine as E
from .. import graph as G
from .. import metrics as M


def pack_replabels(tokens, num_replabels):
    """asg.py:13-32: replace runs of a repeated token by a "repeat k times" label."""
    if all(isinstance(t, list) for t in tokens):
        return [pack_replabels(t, num_replabels) for t in tokens]
    assert isinstance(tokens, list)
    out, run, prev = [], 0, -1
    for tok in tokens:
        if tok == prev and run < num_replabels:
            run += 1
            continue
        if run > 0:
            out.append(run - 1)
            run = 0
        out.append(tok + num_replabels)
        prev = tok
    if run > 0:
        out.append(run - 1)
    return out


def unpack_replabels(tokens, num_replabels):
    """asg.py:35-49: inverse of pack_replabels."""
    if all(isinstance(t, list) for t in tokens):
        return [unpack_replabels(t, num_replabels) for t in tokens]
    assert isinstance(tokens, list)
    out, prev = [], -1
    for tok in tokens:
        if tok >= num_replabels:
            out.append(tok - num_replabels)
            prev = tok
        elif prev != -1:
            out.extend([prev - num_replabels] * (tok + 1))
            prev = -1
    return out


def pack_targets_batch(targets, num_replabels, garbage_idx):
    """ASG.forward's target preparation (asg.py:201-208: pack_replabels per target, then a garbage label between and
    around the labels) for a whole batch of 1-D CPU tensors as array operations; returns a list of B int64 tensors
    (views of one).  A run of n equal labels becomes groups of up to 1 + num_replabels: the label (shifted by
    num_replabels), then -- for a group of s >= 2 -- the replabel s - 2."""
    import numpy as np

    B = len(targets)
    lens = np.fromiter((t.numel() for t in targets), np.int64, B)
    total = int(lens.sum())
    flat = torch.cat([t.reshape(-1) for t in targets]).to(torch.int64).numpy() if total else np.zeros(0, np.int64)
    R, P = num_replabels, num_replabels + 1
    starts = np.zeros(B, dtype=np.int64)
    np.cumsum(lens[:-1], out=starts[1:])
    rows = np.repeat(np.arange(B), lens)
    if total:
        brk = np.ones(total, dtype=bool)
        brk[1:] = flat[1:] != flat[:-1]
        brk[starts[lens > 0]] = True
        run_start = np.flatnonzero(brk)
        run_id = np.cumsum(brk) - 1
        pos = (np.arange(total) - run_start[run_id]) % P          # position inside the group
        run_end = np.empty(total, dtype=bool)                      # last element of its run
        run_end[:-1] = brk[1:]
        run_end[-1] = True
        is_label = pos == 0
        is_rep = (pos >= 1) & (run_end | (pos == P - 1))            # last element of a group of >= 2
        keep = is_label | is_rep
        vals = np.where(is_label, flat + R, pos - 1)[keep]
        out_rows = rows[keep]
        out_lens = np.bincount(out_rows, minlength=B).astype(np.int64)
    else:
        vals, out_lens = np.zeros(0, np.int64), np.zeros(B, np.int64)
    if garbage_idx is not None:  # [g, t0, g, t1, ..., g]
        new_lens = 2 * out_lens + 1
        new_starts = np.zeros(B, dtype=np.int64)
        np.cumsum(new_lens[:-1], out=new_starts[1:])
        res = np.full(int(new_lens.sum()), garbage_idx, dtype=np.int64)
        if len(vals):
            old_starts = np.zeros(B, dtype=np.int64)
            np.cumsum(out_lens[:-1], out=old_starts[1:])
            r = np.repeat(np.arange(B), out_lens)
            res[new_starts[r] + 2 * (np.arange(len(vals)) - old_starts[r]) + 1] = vals
        vals, out_lens = res, new_lens
    return list(torch.split(torch.from_numpy(np.ascontiguousarray(vals, dtype=np.int64)), out_lens.tolist()))


def collapse_and_unpack(paths, garbage_idx, num_replabels):
    """asg.py:228-234 for a whole batch (numpy [B,T] label paths): repeats collapsed, the garbage label dropped,
    replabels unpacked (unpack_replabels above: a replabel r right behind a label repeats that label r + 1 times, any
    other replabel is dropped) -- as array operations instead of a Python loop over 128 x 1000 labels.
    Returns a list of B torch.IntTensor."""
    import numpy as np

    B = paths.shape[0]
    if isinstance(paths, torch.Tensor):
        # on the device: the same collapse as five small launches, and only what survives it travels to the host
        keep = torch.ones_like(paths, dtype=torch.bool)
        if paths.shape[1] > 1:
            keep[:, 1:] = paths[:, 1:] != paths[:, :-1]
        if garbage_idx is not None:
            keep &= paths != garbage_idx
        lens = keep.sum(dim=1).cpu().numpy()
        flat = paths[keep].cpu().numpy()
    else:
        flat, lens = E.collapse_rows(paths, drop=garbage_idx)
    R = num_replabels
    is_lab = flat >= R
    prev_lab = np.zeros(len(flat), dtype=bool)
    prev_lab[1:] = is_lab[:-1]
    starts = np.zeros(B, dtype=np.int64)
    np.cumsum(lens[:-1], out=starts[1:])
    prev_lab[starts[lens > 0]] = False  # (a row's first token has no predecessor)
    prev_tok = np.roll(flat, 1)
    counts = np.where(is_lab, 1, np.where(prev_lab, flat + 1, 0)).astype(np.int64)
    values = np.where(is_lab, flat, prev_tok) - R
    out = np.repeat(values, counts).astype(np.int32)
    rows = np.repeat(np.arange(B), lens)
    out_lens = np.bincount(rows, weights=counts, minlength=B).astype(np.int64)
    return E.split_rows(out, out_lens, torch.int32)


# the step's launch groups, in the order csrc/torch_ops.cpp::asg_forward takes their timing events
_PHASES = ("lattice_gather", "lattice_chain", "lattice_grad", "dense_chain", "dense_grad")


def max_classes():
    """Largest class count the ASG kernels accept (wfl_dense_max_classes: an index-width bound, 16384 -- up to
    wfl_dense_on_chip_classes() the transition matrix is private to a workgroup, beyond it is streamed from L2 by the
    batched per-frame product of csrc/dense_wide.h).  The reference has no limit (asg.py:198-199)."""
    return int(N.lib.wfl_dense_max_classes())


_EARLY_GRAD = os.environ.get("WFL_ASG_EARLY_GRAD", "1") != "0"  # (0: the gradient kernels in backward -- A/B, tests)


class PackedNumerator:
    """A numerator lattice packed elsewhere, in the place of ASGLoss's `targets`: acceptors whose learnable arc weights
    index `transitions` row-major, with the loss factors (scale, +scale/B, -scale/B) that travel with them.  What the
    Transducer with the bigram transition model hands over (criterions/transducer.py::_bigram_route): its loss IS
    forward_score(emissions o transitions) - forward_score(emissions o alignments o transitions), the ASG step."""

    __slots__ = ("pack", "scale", "cpos", "cneg", "B")

    def __init__(self, pack, scale, cpos, cneg, B):
        self.pack, self.scale, self.cpos, self.cneg, self.B = pack, scale, cpos, cneg, B


def _gated_factors(tg, reduction, T):
    """E.loss_factors(tg, reduction) for emissions of T frames: (scale, +scale/B, -scale/B).  An utterance no alignment
    fits whatever the scores -- a target longer than T, an empty target (asg.py:75-77: no accepting node) -- has loss
    +inf by the numerator's log Z, and DESIGN.md section 4 promises it a gradient of exactly zero: the dense gradient
    kernels weigh the denominator's posteriors by cpos[b] without looking at the numerator, so its two coefficients are
    zeros here (scale stays: the loss is +inf).  Known before any launch, from the staged lengths; decided once per
    (batch, reduction, T) -- a batch without such an utterance gets the views E.loss_factors hands out, untouched."""
    key = ("asg_factors", reduction, T)
    hit = tg.cache.get(key)
    if hit is None:
        hit = E.loss_factors(tg, reduction)
        dead = [n == 0 or n > T for n in tg.lens]
        if any(dead):
            live = torch.tensor([0.0 if d else 1.0 for d in dead], dtype=torch.float32, device=hit[1].device)
            hit = (hit[0], hit[1] * live, hit[2] * live)
        tg.cache[key] = hit
    return hit


class ASGLossFunction(torch.autograd.Function):
    @staticmethod
    def create_transitions_graph(transitions, calc_grad=False):
        """asg.py:54-69 as a host graph: arc ids are the row-major index into transitions
        [(C+1), C] (row 0: start -> i, row 1+i: j -> i).  Used when a Transducer is given ASG
        transitions (tests/transducer_test.py:474-481); the ASG loss itself never builds it."""
        import numpy as np

        C = transitions.shape[1]
        assert transitions.shape == (C + 1, C)
        g = G.Graph(calc_grad)
        g.add_nodes([1] + [0] * C, [0] + [1] * C)
        i = np.repeat(np.arange(C, dtype=np.int32), C)
        j = np.tile(np.arange(C, dtype=np.int32), C)
        src = np.concatenate([np.zeros(C, np.int32), j + 1])
        dst = np.concatenate([np.arange(1, C + 1, dtype=np.int32), i + 1])
        lab = np.concatenate([np.arange(C, dtype=np.int32), i])
        g.add_arcs(src, dst, lab, lab, transitions.detach().cpu().contiguous().view(-1).numpy())
        return g

    @staticmethod
    def create_force_align_graph(target):
        """asg.py:72-81 as a host graph (API parity)."""
        g = G.Graph(False)
        g.add_node(True)
        L = len(target)
        for l in range(1, L + 1):
            g.add_node(False, l == L)
            g.add_arc(l - 1, l, target[l - 1])
            g.add_arc(l, l, target[l - 1])
        g.arc_sort(True)
        return g

    @staticmethod
    @E.on_input_device
    def forward(ctx, inputs, transitions, targets, reduction="none"):
        loss, step = Step.forward(inputs, transitions, targets, reduction)
        ctx.aux = step
        E.hold_early(ctx, step.early, step.early is not None)
        return loss

    @staticmethod
    @E.on_input_device
    def backward(ctx, grad_output):
        E.check_not_released(ctx)
        return (*ctx.aux.backward(grad_output, ctx.needs_input_grad[0], ctx.needs_input_grad[1]), None, None)


class Step:
    """One ASG step without an autograd node of its own -- what ASGLossFunction wraps, and what the Transducer's bigram
    route runs inside its node (criterions/transducer.py::_BigramAsAsg): forward() launches and returns the loss with
    the state backward() needs."""

    __slots__ = ("x", "W", "fcc", "cpos", "dx_num", "dw_num", "fork", "devices", "early")

    @classmethod
    def forward(cls, inputs, transitions, targets, reduction):
        B, T, C = inputs.shape
        if reduction not in ("none", "mean"):  # asg.py:120-121
            raise ValueError("invalid value for reduction '" + str(reduction) + "'")
        if tuple(transitions.shape) != (C + 1, C):
            raise ValueError(f"transitions must be [{C + 1}, {C}], got {tuple(transitions.shape)}")
        if T == 0:
            raise ValueError("ASGLoss: empty emissions (T == 0)")
        dev = E.require_gpu()
        self = cls()
        x = self.x = E.as_device_f32(inputs.detach(), dev)
        W = self.W = E.as_device_f32(transitions.detach(), dev)
        if isinstance(targets, PackedNumerator):
            if targets.B != B:
                raise ValueError(f"got {targets.B} targets for a batch of {B}")
            pack, scale, cpos, cneg = targets.pack, targets.scale, targets.cpos, targets.cneg
        else:
            tg = E.targets_on_device(targets, dev)
            if tg.B != B:
                raise ValueError(f"got {tg.B} targets for a batch of {B}")
            scale, cpos, cneg = _gated_factors(tg, reduction, T)
            pack = tg.cache.get(("asg_fal", C))
            if pack is None:
                pack = tg.cache[("asg_fal", C)] = E.PackedLattice.asg_force_align(tg.flat, tg.offsets, C, dev)
        need_dx, need_dw = inputs.requires_grad, transitions.requires_grad
        need_grad = need_dx or need_dw
        # Every launch of the step in one native call (csrc/torch_ops.cpp::asg_forward): ~60 us of host time instead of
        # the ~200 the same sequence costs spelled in Python (what a step costs at a training batch of 8, where the
        # kernels take less than that).  The numerator (force-aligned lattice) and the denominator (fully connected)
        # sweeps are independent and both latency-bound: the numerator runs on a second stream, its gradient (for
        # grad_output = 1) right behind its sweeps, still under the denominator's.
        # `early`: the denominator's gradient right behind its sweeps as well, for grad_output = 1 (with the numerator's
        # as its addend): between the forward and the backward kernels of a step the GPU otherwise waits ~30 us for the
        # host to come back through the autograd engine.  `loss.backward()` takes the two buffers as they are
        # (E.EagerLoss.backward has who gets them how); should the engine run the node after all, backward scales
        # them by grad_output.
        early = need_grad and _EARLY_GRAD and all(E.may_hand_over(t) and t.device == x.device
                                                  for t in (inputs, transitions) if t.requires_grad)
        fork = E.side_stream(dev)
        pack.order_behind_upload(fork.side)  # (a cached pack uploaded on a third stream)
        phases = E.phase_events("asg", _PHASES)  # (None: no launch group of this step is timed)
        loss, da, db, dz, ws, self.dx_num, self.dw_num, dx, dW = N.ops.asg_forward(
            x, W, ctypes.addressof(pack.desc), pack.ints, pack.floats, scale, cpos, cneg, need_dx, need_dw, early,
            fork.side.cuda_stream, phases or [])
        fcc = self.fcc = E.DenseState()
        fcc.B, fcc.T, fcc.C, fcc.alpha, fcc.beta, fcc.logz, fcc.ws = B, T, C, da, db, dz, ws
        self.cpos, self.fork = cpos, fork if need_grad else None
        self.devices = (inputs.device, transitions.device)
        self.early = E.EarlyGrads((inputs, transitions), (dx, dW)) if early else None
        return (loss if inputs.is_cuda else loss.cpu()), self

    def backward(self, grad_output, need_dx, need_dw):
        """-> (dx, dW) on the operands' devices, None for one not needed: the buffers of the forward launches, scaled
        in place; a second pass over a retained graph finds them used and recomputes"""
        grads = self.early.claim(grad_output, (need_dx, need_dw)) if self.early is not None else None
        if grads is None:
            x, W, cpos, dx_num, dw_num = self.x, self.W, self.cpos, self.dx_num, self.dw_num
            gout = E.as_device_f32(grad_output.detach().reshape(1), x.device)
            dx = torch.empty_like(x) if need_dx and dx_num is not None else None
            dW = torch.empty_like(W) if need_dw and dw_num is not None else None
            if dx is not None or dW is not None:
                self.fork.join(dx_num, dw_num)
                # + posteriors of the fully connected graph, - posteriors of the force-aligned one (asg.py:158-168)
                E.dense_grad(x, W, self.fcc, cpos, coef_w=cpos, gout=gout, dx=dx, accumulate=False, dW=dW,
                             addend=dx_num if dx is not None else None, dW_addend=dw_num if dW is not None else None)
            grads = dx, dW
        return E.on_device_of(grads[0], self.devices[0]), E.on_device_of(grads[1], self.devices[1])


def ASGLoss(*args):
    """asg.py:183 (`ASGLoss = ASGLossFunction.apply`): same call, same result."""
    return E.make_eager(ASGLossFunction.apply(*args))


def _refuse_lookahead(what, lookahead):
    if lookahead is not None:
        raise NotImplementedError(
            f"{what}: lookahead (word-LM look-ahead inside words, DESIGN.md section 27) is for CTC and the Transducer -- "
            "ASG's stay entries look one extension up per hypothesis for their prune bound, and what look-ahead does to "
            "that bound is a question of its own")


class ASG(torch.nn.Module):
    def __init__(self, num_classes, num_replabels=1, use_garbage=True):
        super(ASG, self).__init__()
        self.num_classes = num_classes
        self.num_replabels = num_replabels
        assert self.num_replabels > 0
        self.garbage_idx = (num_classes + num_replabels) if use_garbage else None
        self.N = num_classes + num_replabels + int(use_garbage)
        limit = max_classes()
        if self.N > limit:  # (16384: the (N+1) x N matrix alone would be a gigabyte)
            raise NotImplementedError(
                f"ASG with {self.N} classes (tokens + replabels + garbage): the dense-transition kernels take at most {limit}")
        self.transitions = torch.nn.Parameter(torch.zeros(self.N + 1, self.N))

    @E.on_input_device
    def forward(self, inputs, targets):
        if len(targets) and all(type(t) is torch.Tensor and not t.is_cuda for t in targets):
            # (what train.py hands over: the whole batch as array operations -- row by row in Python this preparation cost
            # more host time than the step's kernels take at a training batch)
            targets = pack_targets_batch(targets, self.num_replabels, self.garbage_idx)
            return ASGLoss(inputs, self.transitions, targets, "mean")
        targets = [pack_replabels(t.tolist(), self.num_replabels) for t in targets]
        if self.garbage_idx is not None:  # a garbage token between (and around) the labels: asg.py:203-208
            for idx, tgt in enumerate(targets):
                interleaved = [self.garbage_idx] * (2 * len(tgt) + 1)
                interleaved[1::2] = tgt
                targets[idx] = interleaved
        return ASGLoss(inputs, self.transitions, targets, "mean")

    def _best_paths(self, outputs):
        """(label paths [B,T] int32 on the device, whether viterbi() and errors() decode them there)"""
        B, T, C = outputs.shape
        assert C == self.N, "Wrong number of classes in output."
        dev = E.require_gpu()
        x = E.as_device_f32(outputs.detach(), dev)
        W = E.as_device_f32(self.transitions.detach(), dev)
        return E.dense_viterbi(x, W), outputs.is_cuda and B > 0

    def viterbi(self, outputs):
        """asg.py:211-237: best label sequence under emissions + transitions, repeats collapsed,
        garbage dropped, replabels unpacked."""
        paths, on_device = self._best_paths(outputs)
        if on_device:
            # collapse, garbage and replabels on the device: only the labels that survive travel (csrc/decode_kernels.hip)
            return E.decode_paths(paths, self.garbage_idx, self.num_replabels)
        return collapse_and_unpack(paths, self.garbage_idx, self.num_replabels)

    def _beam_plan(self, outputs, what, beam_size, classes_per_frame, nbest, lexicon=None, lm=None, lm_weight=1.0,
                   length_bonus=0.0, lm_eos=True, word_bonus=0.0, lookahead=None, token_lm=None):
        """The arguments of a beam search, checked before anything needs a device: the E.AsgBeamPlan of the options, with
        a lexicon the E.AsgLexiconBeamPlan; with a token_lm the E.AsgLmBeamPlan, whose scalars lm_weight, length_bonus
        and lm_eos then are; with neither every keyword of the two must be at its default"""
        E.check_beam_outputs(outputs, what)
        if outputs.shape[2] != self.N:
            raise ValueError(f"{what}: outputs have {outputs.shape[2]} classes, the criterion has {self.N}")
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
            return E.AsgLmBeamPlan.checked(self.N, beam_size, classes_per_frame, nbest, self.garbage_idx, self.num_replabels,
                                           token_lm, lm_weight, length_bonus, lm_eos, what)
        if lexicon is None:
            E.refuse_without_lexicon(what, lm, lm_weight, length_bonus, lm_eos, word_bonus, "an ASG")
            return E.AsgBeamPlan.checked(self.N, beam_size, classes_per_frame, nbest, what)
        return E.AsgLexiconBeamPlan.checked(self.N, beam_size, classes_per_frame, nbest, self.garbage_idx, lexicon, lm,
                                            lm_weight, word_bonus, length_bonus, lm_eos, what)

    def lexicon(self, words, tokens, wordsep=None, split=None):
        """The lexicon.Lexicon of `words` for beam_search(lexicon=): a trie over the RAW class
        sequences the criterion trains on.  tokens: the model's num_classes tokens in class order (token i is raw class
        i + num_replabels); a word is split into its characters, or by split(word) -> list of tokens; with `wordsep`
        that token ends every spelling.  A spelling is pack_replabels(token indices, num_replabels): "aa|" with one
        replabel is [a + 1, 0, sep + 1].  The garbage class is never spelled: the search treats it as transparent.  The
        Lexicon is built for (N, garbage) where the module has a garbage class, else for (N + 1, N): a phantom class that
        is never a label stands in for the blank a Lexicon wants.  ValueError names a word with a piece that is no token,
        and two words where the last token of one equals the first token of the other: the criterion packs a target as a
        whole, so that pair would be packed across the word boundary and no trie over single words spells it."""
        tokens = list(tokens)
        what = "ASG.lexicon"
        if len(tokens) != self.num_classes:
            raise ValueError(f"{what}: {len(tokens)} tokens for a criterion of {self.num_classes} classes")
        if len(set(tokens)) != len(tokens):
            raise ValueError(f"{what}: a token appears twice")
        index = {tok: i for i, tok in enumerate(tokens)}
        if wordsep is not None and wordsep not in index:
            raise ValueError(f"{what}: the word separator {wordsep!r} is not one of the model's tokens")
        words = list(words)
        pieces_of = []
        for w in words:
            pieces = list(w) if split is None else list(split(w))
            for p in pieces:
                if p not in index:
                    raise ValueError(f"{what}: {p!r} of {w!r} is not one of the model's tokens")
            pieces = [index[p] for p in pieces] + ([index[wordsep]] if wordsep is not None else [])
            if not pieces:
                raise ValueError(f"{what}: {w!r} has an empty spelling")
            pieces_of.append(pieces)
        first = {}
        for w, pieces in zip(words, pieces_of):
            first.setdefault(pieces[0], w)
        for w, pieces in zip(words, pieces_of):
            if pieces[-1] in first:
                raise ValueError(f"{what}: {w!r} ends in the token {tokens[pieces[-1]]!r} that {first[pieces[-1]]!r} starts "
                                 f"with: replabels would pack the pair across the word boundary, which a lexicon of single "
                                 f"words cannot spell; spellings that end in a separator (wordsep) no word starts with "
                                 f"satisfy this by construction")
        from ..lexicon import Lexicon

        spellings = [pack_replabels(pieces, self.num_replabels) for pieces in pieces_of]
        if self.garbage_idx is not None:
            return Lexicon(spellings, self.N, self.garbage_idx, words=words)
        return Lexicon(spellings, self.N + 1, self.N, words=words)

    def token_lm(self, path, tokens, bos="<s>", eos="</s>", unk="<unk>"):
        """The lm.NGramLM of an ARPA file over the model's tokens for beam_search(token_lm=):
        NGramLM.from_arpa(path, tokens, blank=len(tokens)).  tokens: the model's num_classes tokens in class order, as
        the ARPA file names them (token i is raw class i + num_replabels, and LM label i); the LM is built around a
        phantom blank num_classes that is never a label.  The LM never sees a replabel or the garbage: it reads what
        beam_search returns."""
        tokens = list(tokens)
        if len(tokens) != self.num_classes:
            raise ValueError(f"ASG.token_lm: {len(tokens)} tokens for a criterion of {self.num_classes} classes")
        from ..lm import NGramLM

        return NGramLM.from_arpa(path, tokens, blank=len(tokens), bos=bos, eos=eos, unk=unk)

    def words(self, lexicon, labels):
        """The word ids of a label sequence that beam_search(lexicon=) returned (mapped: garbage dropped, replabels
        unpacked): lexicon.words of the sequence packed again.  No word ends in a token a word starts with (lexicon()
        checks that), so packing the whole sequence packs every word as the lexicon spells it."""
        labels = labels.tolist() if hasattr(labels, "tolist") else list(labels)
        return lexicon.words(pack_replabels([int(v) for v in labels], self.num_replabels))

    def _beam_inputs(self, outputs):
        """(emissions, transitions): float32, contiguous, on the emissions' GPU or the required one (no host path)"""
        dev = outputs.device if outputs.is_cuda else E.require_gpu()
        return (outputs.detach().to(device=dev, dtype=torch.float32).contiguous(),
                E.as_device_f32(self.transitions.detach(), dev))

    @E.on_input_device
    def beam_search(self, outputs, beam_size=16, classes_per_frame=None, nbest=1, return_scores=False, lexicon=None, lm=None,
                    lm_weight=1.0, length_bonus=0.0, lm_eos=True, word_bonus=0.0, lookahead=None, token_lm=None):
        """ASG prefix beam search (an addition: the reference has viterbi() only).  viterbi() gives the best frame path
        under emissions + transitions; the criterion scores a label sequence by the sum over all its alignments (the
        force-align numerator, asg.py:72-115), and this returns the sequences it rates highest (DESIGN.md section 21 has
        the rules; csrc/beam_kernels.hip runs them, in float64).  Per frame the `classes_per_frame` classes of highest
        emission score (default min(N, 32)) extend a hypothesis; `beam_size` (1..64) hypotheses survive a frame.  A
        hypothesis whose last class is not among a frame's candidates lives on only through its extensions: ASG has
        no blank to wait in.  Returns what viterbi() returns -- garbage dropped, replabels unpacked, on the device --:
        nbest == 1: B int64 CPU tensors; otherwise a list of `nbest` such tensors per utterance, best first (a rank
        beyond the final beam is empty).  The search and its n-best list are over RAW class sequences (tokens shifted by
        the replabels, replabels, garbage), the criterion's own objects: two raw sequences can give the same output
        once the garbage is dropped, so an n-best list may name an output twice, each time with the probability of
        that raw sequence alone.  return_scores: also a float64 CPU tensor [B, nbest] of log-probabilities under the
        criterion -- the raw sequence's log mass minus the denominator (asg.py:114): minus the ASG loss of that raw
        sequence where the beam pruned none of its alignments, a lower bound of it otherwise --, -inf for an empty rank.  B == 0 or T == 0: empty sequences with score 0, no device needed.

        lexicon (an addition): a lexicon.Lexicon built by self.lexicon() -- only sequences of its
        words are returned, and lm (optional) is a word LM over its word ids (NGramLM.from_arpa(path, words,
        blank=len(words))).  A raw class other than the garbage adds length_bonus, a completed word lm_weight * step(s,
        word) + word_bonus on top, and lm_eos lm_weight * step(s, </s>) after the last frame; the scores include these
        terms.  The garbage class is transparent: it may stand anywhere between the classes of a word.  The search and
        the n-best list are still over raw sequences, and only the raw forms the criterion is trained on are returned: a
        word spelled `a a` is found as raw `a, replabel 0`, never as raw `a, garbage, a`, which unpacks to the same
        tokens but does not walk the trie.  Without a lexicon the call is what it was, and lm, lm_weight, length_bonus,
        lm_eos and word_bonus must be at their defaults (ValueError).  B == 0 or T == 0 with a lexicon: the empty
        sequence, scored by the LM's </s> alone.  lookahead (CTC's and the Transducer's): anything
        but None raises NotImplementedError, as a start-marked lexicon does.

        token_lm (an addition): an lm.NGramLM over the model's tokens (self.token_lm(path, tokens)
        reads one from an ARPA file; num_classes == self.num_classes + 1, blank == self.num_classes) -- lexicon-free
        decoding with a letter n-gram, shallow fusion inside the beam.  The LM reads exactly what this call returns: a
        token steps it once, a replabel k right behind a token steps it by that token k + 1 more times, the garbage and
        a replabel with nothing to repeat not at all.  lm_weight, length_bonus and lm_eos are then its scalars, as in
        CTC.beam_search(lm=): every LM step adds lm_weight * step(s, token) + length_bonus, lm_eos adds lm_weight *
        step(s, </s>) after the last frame; the scores include these terms.  The search and the n-best list are still
        over raw sequences: raw `a, garbage, a` and raw `a, replabel 0` return the same tokens, carry the same LM term
        and are two hypotheses, each with the mass of its own alignments, so an n-best list may name an output twice.
        `lm` remains the word LM of a lexicon: lm=, word_bonus or lookahead beside a token_lm raise ValueError, a
        token_lm with a lexicon NotImplementedError.  B == 0 or T == 0 with a token_lm: the empty sequence, scored by
        the LM's </s> alone.  Without token_lm the call is what it was."""
        if token_lm is None:
            _refuse_lookahead("ASG.beam_search", lookahead)
        plan = self._beam_plan(outputs, "ASG.beam_search", beam_size, classes_per_frame, nbest, lexicon, lm, lm_weight,
                               length_bonus, lm_eos, word_bonus, lookahead, token_lm)
        if outputs.shape[0] == 0 or outputs.shape[1] == 0:
            hyps, scores = plan.no_frames(outputs.shape[0])
        else:
            x, W = self._beam_inputs(outputs)
            with torch.cuda.device(x.device), torch.no_grad():
                hyps, scores = plan.search(x, W, True, self.garbage_idx, self.num_replabels)
        if plan.nbest == 1:
            hyps = [h[0] for h in hyps]
        return (hyps, scores) if return_scores else hyps

    @E.on_input_device
    def errors(self, outputs, targets, counter, *, beam_size=None, classes_per_frame=None, lexicon=None, lm=None,
               lm_weight=1.0, length_bonus=0.0, lm_eos=True, word_bonus=0.0, lookahead=None, token_lm=None):
        """compute_edit_distance(self.viterbi(outputs), targets, preprocessor) (train.py:74-87, 278-284) as
        (tokens_dist, words_dist, n_tokens, n_words), with `counter` a metrics.ErrorCounter: where viterbi() decodes on
        the device the count runs behind the same decode and the predictions never reach the host.  `beam_size` (an
        addition): the predictions are beam_search(outputs, beam_size, classes_per_frame)'s instead, counted behind the
        beam launches on their device buffers; `classes_per_frame` needs a beam_size.  lexicon, lm, lm_weight,
        length_bonus, lm_eos, word_bonus: beam_search's, with a beam_size: the predictions are those of the search with
        a lexicon.  lookahead: refused, as by beam_search.  token_lm: beam_search's, with a beam_size: the predictions
        are those of the search with a token-level LM."""
        if token_lm is None:
            _refuse_lookahead("ASG.errors", lookahead)
        elif beam_size is None:
            raise ValueError("ASG.errors: token_lm needs a beam_size")
        if beam_size is None:
            if classes_per_frame is not None:
                raise ValueError("ASG.errors: classes_per_frame needs a beam_size")
            if lexicon is not None:
                raise ValueError("ASG.errors: lexicon needs a beam_size")
            E.refuse_without_lexicon("ASG.errors", lm, lm_weight, length_bonus, lm_eos, word_bonus, "an ASG")
        else:
            plan = self._beam_plan(outputs, "ASG.errors", beam_size, classes_per_frame, 1, lexicon, lm, lm_weight,
                                   length_bonus, lm_eos, word_bonus, lookahead, token_lm)
            counter.check_hypothesis_labels(self.num_classes, "ASG.errors")
            if outputs.shape[0] == 0 or outputs.shape[1] == 0:
                return counter([h[0] for h in plan.no_frames(outputs.shape[0])[0]], targets)
            x, W = self._beam_inputs(outputs)
            with torch.cuda.device(x.device), torch.no_grad():
                return counter.totals(M.plan_errors(counter, targets, x, plan, W, self.garbage_idx, self.num_replabels))
        counter.check_hypothesis_labels(self.num_classes, "ASG.errors")
        with torch.no_grad():
            if not (outputs.is_cuda and outputs.shape[0] > 0):
                return counter(self.viterbi(outputs), targets)
            paths, _ = self._best_paths(outputs)
            return counter.totals(M.decode_paths_errors(counter, targets, paths, self.garbage_idx, self.num_replabels))
