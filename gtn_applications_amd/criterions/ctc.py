"""CTC criterion -- counterpart of /root/reference/criterions/ctc.py.

`CTCLossFunction.forward/backward`, `CTCLoss` and `CTC` keep the reference's signatures
(ctc.py:13-135).  Where the reference builds `gtn.intersect(g_emissions, g_criterion)` per sample
on host threads (ctc.py:38-65), this sends the whole batch through the CTC fast-path kernels
(csrc/ctc_kernels.hip; up to four target positions per lane) -- or, for targets longer than 255
labels, through the generic lattice engine (csrc/lattice_kernels.hip).  Both are HIP paths; there is no CPU path.
"""
import collections
import operator
import os

import numpy as np
import torch

from .. import _native as N
from .. import engine as E
from .. import graph as G
from .. import metrics as M


def check_input_lengths(input_lengths, B, T, what, keep_full=False):
    """The per-utterance input lengths of a padded batch as a tuple of B ints, or None when every utterance has all T
    frames (`input_lengths` None, or all equal to T: exactly the call without lengths).  `input_lengths`: B integers
    1 <= T_b <= T as a list, a tuple or a 1-D integer tensor -- a device tensor is read back, which costs one
    synchronisation.  ValueError naming the utterance otherwise; nothing here needs a device.  keep_full: lengths that
    all equal T are returned as they are -- for emissions that are not float32, which are taken WITH lengths only (the
    padded copy is what converts them), whatever the lengths of the batch at hand are."""
    if input_lengths is None:
        return None
    if isinstance(input_lengths, torch.Tensor):
        if input_lengths.dim() != 1:
            raise ValueError(f"{what}: input_lengths must be 1-D, got a tensor of {input_lengths.dim()} dimensions")
        if input_lengths.dtype.is_floating_point or input_lengths.dtype.is_complex or input_lengths.dtype == torch.bool:
            raise ValueError(f"{what}: input_lengths must be integers, got a {input_lengths.dtype} tensor")
        values = input_lengths.tolist()
    elif isinstance(input_lengths, (list, tuple)):
        values = list(input_lengths)
    else:
        raise ValueError(f"{what}: input_lengths must be a list, a tuple or a 1-D integer tensor, "
                         f"got {type(input_lengths).__name__}")
    if len(values) != B:
        raise ValueError(f"{what}: got {len(values)} input lengths for a batch of {B}")
    lens = []
    for b, v in enumerate(values):
        if isinstance(v, torch.Tensor) and v.dim() == 0 and not (v.dtype.is_floating_point or v.dtype == torch.bool):
            v = v.item()
        try:
            n = None if isinstance(v, bool) else operator.index(v)
        except TypeError:
            n = None
        if n is None:
            raise ValueError(f"{what}: the input length of utterance {b} is not an integer: {v!r}")
        if not 1 <= n <= T:
            raise ValueError(f"{what}: input length {n} of utterance {b} is outside [1, {T}]")
        lens.append(n)
    return None if not keep_full and all(n == T for n in lens) else tuple(lens)


class BlankLabelUnderLengths(ValueError):
    """CTCLossFunction.forward met input lengths and a target label equal to the blank index.  It is the autograd node
    and cannot widen its input; `targets` are the staged targets (labels inside [0, C)) for the caller that can."""

    def __init__(self, targets):
        super().__init__("CTCLossFunction: input_lengths with a target label equal to the blank index: call CTCLoss, "
                         "which gives such labels a column of their own")
        self.targets = targets


# ctx.aux of CTCLossFunction, per route.  "pipelined": one launch for loss and gradient (ctx.early holds that); "fast": the
# chains alone, no gradient asked; "lattice": the lattice engine, st its LatticeState.  coef: the gradient's factors
_Saved = collections.namedtuple("_Saved", "kind x coef tg blank lse st", defaults=(None,) * 4)


class CTCLossFunction(torch.autograd.Function):
    """`input_lengths` (padded batches; an addition to the reference's call): utterance b has the frames [0, T_b), the
    frames behind them are read as certain-blank frames -- 0 for the blank, -inf for every other class -- which are the
    identity of the CTC label graph ("Input lengths as certain-blank frames").  The training step of float32
    device emissions with targets of up to 63 labels substitutes them inside its launches (wfl_ctc_call.input_lengths);
    every other route runs unchanged on a copy of the emissions padded that way (wfl_ctc_pad_frames).  The pad rows of
    every gradient are set to exactly 0 (wfl_zero_pad_rows) before it is handed out.  Whenever `input_lengths` is passed, emissions of
    another floating dtype are taken too (the padded copy is float32, the gradient comes back in their dtype) -- also
    when all the lengths equal T; float32 emissions with such lengths take exactly the path without lengths.  The
    identity needs targets without the blank index among their labels: with lengths, such a target is refused here
    (BlankLabelUnderLengths, a ValueError) and served by CTCLoss and the CTC module, which catch that
    (_lengths_with_blank_labels)."""

    @staticmethod
    def create_ctc_graph(target, blank_idx):
        """ctc.py:15-29 as a host graph (API parity; the kernels never need it)."""
        g = G.Graph(False)
        L = len(target)
        S = 2 * L + 1
        for s in range(S):
            g.add_node(s == 0, s >= S - 2)
            label = target[(s - 1) // 2] if s % 2 else blank_idx
            g.add_arc(s, s, label)
            if s > 0:
                g.add_arc(s - 1, s, label)
            if s % 2 and s > 1 and label != target[(s - 1) // 2 - 1]:
                g.add_arc(s - 2, s, label)
        g.arc_sort(False)
        return g

    @staticmethod
    @E.on_input_device
    def forward(ctx, log_probs, targets, blank_idx=0, reduction="none", input_lengths=None):
        B, T, C = log_probs.shape
        if T == 0:
            raise ValueError("CTCLoss: empty emissions (T == 0)")
        if reduction not in ("none", "mean"):  # ctc.py:57-58
            raise ValueError("invalid value for reduction '" + str(reduction) + "'")
        lens = check_input_lengths(input_lengths, B, T, "CTCLoss", keep_full=log_probs.dtype != torch.float32)
        dev = E.require_gpu()
        if lens is None:
            x = E.as_device_f32(log_probs.detach(), dev)
        else:
            if not log_probs.dtype.is_floating_point:
                raise TypeError(f"expected a floating point tensor, got {log_probs.dtype}")
            x = log_probs.detach().to(device=dev, dtype=torch.float32).contiguous()
        tg = E.targets_on_device(targets, dev)
        if tg.B != B:
            raise ValueError(f"got {tg.B} targets for a batch of {B}")
        E.check_labels(tg, C, "CTCLoss")
        if not 0 <= int(blank_idx) < C:
            raise ValueError(f"CTCLoss: blank index {blank_idx} is outside [0, {C})")
        if lens is not None and tg.label_min <= int(blank_idx) <= tg.label_max and bool((tg.flat == int(blank_idx)).any()):
            # a certain-blank frame is the identity only while no LABEL state reads the blank's column (DESIGN.md
            # section 16): CTCLoss and the CTC module catch this and give such labels a column of their own -- with
            # the staged targets at hand, whose labels were checked against the caller's C just above
            raise BlankLabelUnderLengths(tg)
        need_grad, early = log_probs.requires_grad, None
        xlen = ctx.xlen = ctx.launch_xlen = None
        if lens is not None:
            xlen = ctx.xlen = E.input_lengths_on_device(lens, dev)
            if (need_grad and tg.max_len <= E.CTC_LENGTHS_MAX_LEN and E.ctc_fast_path_ok(tg.max_len, C)
                    and log_probs.is_cuda and log_probs.dtype == torch.float32):
                # the step's launches read the lengths themselves (wfl_ctc_call.input_lengths: the stagers of the
                # meet-in-the-middle launch, the log-domain chain and gradient bodies): no copy of the emissions
                ctx.launch_xlen = xlen
            else:
                # everything else -- longer targets, the lattice engine, no gradient, emissions that are not float32
                # or not on the device -- sweeps T frames of a copy whose pad rows are the identity frames; the chains,
                # the gradient blocks and the lattice engine score a -inf arc as the reference's intersect does
                x = E.ctc_pad_frames(x, xlen, int(blank_idx))
        if E.ctc_fast_path_ok(tg.max_len, C) and need_grad:
            # loss and gradient in ONE pipelined launch (gradient waves run behind the chains); backward
            # only applies the upstream scalar.  Like torch's own CTC, the gradient is produced eagerly.
            # The per-utterance factors (loss scale; gradient coefficient -scale/B) were uploaded with the targets.
            scale, coef = tg.addr("scale_" + reduction), tg.addr("cneg_" + reduction)
            dx = torch.empty_like(x)
            lse = E.row_lse(x) if ctx_log_softmax(ctx) else None
            _, _, loss = E.ctc_forward_backward(x, tg, int(blank_idx), coef, None, dx, loss_scale=scale, want_loss=True,
                                                lse=lse, shared_ws=True, xlen=ctx.launch_xlen)
            if xlen is not None:  # (the eager gradient: zeroed here, on the launch's stream, before anything can hand it out)
                E.zero_pad_rows(dx, xlen)
            ctx.aux = _Saved("pipelined", x, coef, tg, int(blank_idx), lse)
            early = E.EarlyGrads((log_probs,), (dx,))  # (for backward; not offered: the loss stays a plain tensor)
        elif ctx_log_softmax(ctx):
            raise RuntimeError("fused log_softmax CTC is only used on the pipelined path")
        elif E.ctc_fast_path_ok(tg.max_len, C):
            scale, _, coef = E.loss_factors(tg, reduction)
            ws, nll = E.ctc_forward(x, tg, int(blank_idx))
            loss = E.reduce_loss(nll, scale, 1.0)
            ctx.aux = _Saved("fast", x, coef, tg, int(blank_idx))
        else:
            pack = tg.cache.get(("ctc_lattice", int(blank_idx), C))
            if pack is None:
                pack = tg.cache[("ctc_lattice", int(blank_idx), C)] = E.PackedLattice.ctc(
                    tg.flat, tg.offsets, int(blank_idx), C, dev)
            scale, _, coef = E.loss_factors(tg, reduction)
            st = E.lattice_forward(x, pack, need_beta=need_grad)
            loss = E.reduce_loss(st.logz, scale, -1.0)
            ctx.aux = _Saved("lattice", x, coef, st=st)
        E.hold_early(ctx, early, False)
        ctx.in_device, ctx.in_dtype = log_probs.device, log_probs.dtype
        return loss if log_probs.is_cuda else loss.cpu()

    @staticmethod
    @E.on_input_device
    def backward(ctx, grad_output):
        sv = ctx.aux
        if sv.kind == "fast":
            raise RuntimeError("CTCLoss: backward through an input that did not require grad in forward")
        early = ctx.early.claim(grad_output) if ctx.early is not None else None  # (the eager gradient, scaled in place)
        if early is not None:
            dx = early[0]
        else:
            dx = torch.empty_like(sv.x)
            gout = E.as_device_f32(grad_output.detach().reshape(1), sv.x.device)
            if sv.kind == "pipelined":
                # a second backward through a retained graph: the eager gradient was handed out by the first one, so
                # run the same launch again -- with the same row log-sum-exps when the log_softmax is fused -- into a
                # fresh buffer, the upstream scalar applied by the kernel
                E.ctc_forward_backward(sv.x, sv.tg, sv.blank, sv.coef, gout, dx, lse=sv.lse, shared_ws=True,
                                       xlen=ctx.launch_xlen)
            else:
                E.lattice_grad(sv.st, sv.coef, gout=gout, dx=dx)
            if ctx.xlen is not None:
                E.zero_pad_rows(dx, ctx.xlen)
        if ctx.in_device.type != "cuda":
            dx = dx.to(ctx.in_device)
        if dx.dtype != ctx.in_dtype:  # (only with input lengths: other dtypes are rejected in forward)
            dx = dx.to(ctx.in_dtype)
        return dx, None, None, None, None


def ctx_log_softmax(ctx):
    return getattr(ctx, "fused_log_softmax", False)


class _FusedLogSoftmaxCTCLoss(CTCLossFunction):
    """CTCLoss(log_softmax(inputs), ...) as one operator (ctc.py:107 + ctc.py:122): the row log-sum-exps
    are computed once, subtracted where the chains gather their emissions, and the gradient rows
    start at -cf * softmax(inputs); only for the pipelined path (targets up to 255 labels, input
    requires grad) -- the module falls back to torch's log_softmax otherwise."""

    @staticmethod
    @E.on_input_device
    def forward(ctx, inputs, targets, blank_idx=0, reduction="none", input_lengths=None):
        ctx.fused_log_softmax = True
        return CTCLossFunction.forward(ctx, inputs, targets, blank_idx, reduction, input_lengths)


class _EagerLoss(torch.Tensor):
    """The scalar the C++ CTC node returns.  A plain tensor in every respect (no __torch_function__ dispatch) but one:
    `loss.backward()` with no arguments -- the call of ctc_benchmark.py:29-31 and of every training loop that uses the
    criterion's output as its loss -- does not run the criterion's own node on the autograd engine: the forward launch
    already computed the gradient, so for leaf emissions it is handed to their .grad directly, and for emissions that
    are a producer's output (a model's, train.py:262-266) the engine is started at THEIR edge with that gradient
    (csrc/torch_ops.cpp ctc_fast_backward: the ones_like fill, the trip through this node and the scale launch cost
    more host time than the step's kernels take).  Anything else -- a gradient argument, retain_graph, create_graph,
    inputs=, hooks on the loss (or on leaf emissions), anomaly mode, the loss used inside a larger expression, a torch
    other than the one the node was compiled against -- goes through torch.Tensor.backward / the engine."""

    __torch_function__ = torch._C._disabled_torch_function_impl

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        if (gradient is None and not retain_graph and not create_graph and inputs is None and fast_backward_enabled()
                and not torch.is_anomaly_enabled() and _NODE.ctc_fast_backward(self)):
            return None
        return torch.Tensor.backward(self, gradient, retain_graph, create_graph, inputs=inputs)


_FAST_BACKWARD = os.environ.get("WFL_CTC_FAST_BACKWARD", "1") != "0"  # (0: always the autograd engine -- A/B, tests)
_FAST_BACKWARD_OK = None


def fast_backward_enabled():
    """The short cut reads autograd structures through torch's C++ headers (Node hooks, AccumulateGrad, Engine::execute):
    it is only taken under the torch release the extension was compiled against -- any other falls back to
    torch.Tensor.backward, which is always correct (tests/test_host_library.py pins the fall-back)."""
    global _FAST_BACKWARD_OK
    if _FAST_BACKWARD_OK is None:
        _FAST_BACKWARD_OK = _NODE.built_for_torch() == torch_release(torch.__version__)
    return _FAST_BACKWARD and _FAST_BACKWARD_OK


def torch_release(version):
    """'2.10.0+rocm7.0' -> '2.10.0' (TORCH_VERSION in the headers carries no local build tag)."""
    return str(version).split("+")[0]


_NODE = N.ops  # the C++ autograd node of the pipelined step (csrc/torch_ops.cpp)


def _native_node():
    """The C++ autograd node of the pipelined step (_NODE: csrc/torch_ops.cpp, imported once by _native)."""
    return _NODE


@E.on_input_device
def _ctc_loss(log_probs, targets, blank_idx, reduction, fused_log_softmax, input_lengths=None):
    """CTCLossFunction.apply, with the hot case -- float32 device emissions that require grad, targets the fast
    kernels take -- routed through the C++ autograd node: same checks, same staging, same launch, but neither the
    forward nor the backward passes through Python's autograd.Function machinery (which costs more host time than
    the step's kernels take on the GPU at the benchmark shape).  A call with input lengths (a padded batch) goes
    through CTCLossFunction, which pads a copy and zeroes the gradient's pad rows around the same launches."""
    if input_lengths is not None and log_probs.dim() == 3:
        # checked before anything needs a device; lengths that all equal T are the call without lengths
        input_lengths = check_input_lengths(input_lengths, log_probs.shape[0], log_probs.shape[1], "CTCLoss",
                                            keep_full=log_probs.dtype != torch.float32)
    if input_lengths is not None:
        fn = _FusedLogSoftmaxCTCLoss if fused_log_softmax else CTCLossFunction
        try:
            return fn.apply(log_probs, targets, blank_idx, reduction, input_lengths)
        except BlankLabelUnderLengths as met:
            # (found by the node on the targets it staged and checked: lists, tensors or staged targets alike, and no
            # second pass over the labels for the batches without such a label)
            tg = met.targets
        return _lengths_with_blank_labels(log_probs, tg.flat, tg.offsets, int(blank_idx), reduction, fused_log_softmax,
                                          input_lengths)
    if (type(log_probs) is torch.Tensor and log_probs.is_cuda and log_probs.requires_grad
            and log_probs.dtype == torch.float32 and log_probs.dim() == 3 and log_probs.is_contiguous()
            and torch.is_grad_enabled() and log_probs.shape[1] > 0 and reduction in ("none", "mean")):
        lim = (int(blank_idx), reduction == "mean", fused_log_softmax, E.CTC_FAST_MAX_LEN, E.CTC_FAST_MAX_CLASSES,
               E.CTC_FAST_MAX_CLASSES_LONG)
        tok = None if E.PHASE_EVENTS is None else E._mark("ctc_step")
        lists = type(targets) in (list, tuple)
        # staging, upload, checks and launch in one native call (csrc/torch_ops.cpp)
        loss = _NODE.ctc_loss_lists(log_probs, targets, *lim) if tok is None and lists else None
        if loss is None:  # profiling, targets that call does not read, or not the hot case after all
            st = _NODE.stage_targets(targets, log_probs.device) if lists else None
            if st is None:
                st = E.targets_on_device(targets, log_probs.device)._st
            if tok is not None:  # (profiling: the event pair brackets the launch, not the staging)
                E._event_pool().append(tok[1])  # (recorded too early: take the start event again after the staging)
                tok = (tok[0], E._event())
            loss = _NODE.ctc_loss_staged(log_probs, st, *lim)
            E._done(tok)
        if loss is not None:
            loss.__class__ = _EagerLoss
            return loss
    fn = _FusedLogSoftmaxCTCLoss if fused_log_softmax else CTCLossFunction
    return fn.apply(log_probs, targets, blank_idx, reduction)


def _lengths_with_blank_labels(log_probs, flat, offsets, blank, reduction, fused_log_softmax, lens):
    """A padded batch whose targets hold the blank index as a LABEL.  In a certain-blank frame such a label's state has
    the finite score 0 as well, so the pad frames are no identity of its graph: paths move on, or wait, between a blank
    state and the blank-labelled state beside it, and where the target ends in such a label they are accepted -- Z grows
    (tests/test_ctc_lengths_host.py shows it on the oracle).  The labels get a column of their own
    instead -- class C, a copy of the blank's column, which a pad frame scores -inf like every other label -- and keep
    their place in the skip rule (they equal each other and no other label).  torch's cat and log_softmax carry the
    gradient back: the copy's into the blank's column, and through the normalisation when it was asked fused."""
    C = log_probs.shape[2]
    flat = np.asarray(flat)
    if flat.size and (int(flat.min()) < 0 or int(flat.max()) >= C):  # (the caller's C, not the widened row's)
        bad = int(flat.min()) if int(flat.min()) < 0 else int(flat.max())
        raise ValueError(f"CTCLoss: target label {bad} is outside [0, {C}) (emissions have {C} classes)")
    if fused_log_softmax:  # (a NaN is an impossible arc here as in the fused launch)
        log_probs = torch.nn.functional.log_softmax(log_probs.masked_fill(torch.isnan(log_probs), float("-inf")), dim=2)
    wide = torch.cat((log_probs, log_probs[:, :, blank:blank + 1]), dim=2)
    flat = np.where(flat == blank, C, flat)
    targets = [flat[offsets[b]:offsets[b + 1]].tolist() for b in range(len(offsets) - 1)]
    return CTCLossFunction.apply(wide, targets, blank, reduction, lens)


def CTCLoss(log_probs, targets, blank_idx=0, reduction="none", input_lengths=None):
    """ctc.py:96 (`CTCLoss = CTCLossFunction.apply`): same call, same result.  `input_lengths` (an addition: B integers
    1 <= T_b <= T, see check_input_lengths): the loss and gradient of the utterances log_probs[b, :T_b] -- the frames
    behind T_b of a padded batch do not count, their gradient rows are exactly 0; "mean" still divides by the target
    length.  None, or lengths that all equal T, is the call without them."""
    return _ctc_loss(log_probs, targets, blank_idx, reduction, False, input_lengths)


class CTC(torch.nn.Module):
    def __init__(self, blank, use_pt):
        super(CTC, self).__init__()
        self.blank = blank  # index of blank label
        self.use_pt = use_pt  # use torch.nn.functional.ctc_loss instead of the WFST engine

    @E.on_input_device
    def forward(self, inputs, targets, input_lengths=None):
        """ctc.py:106-122.  `input_lengths` (an addition, see CTCLoss): the frames of each utterance of a padded batch;
        with use_pt they go to torch's operator in place of [T] * B."""
        lens = None
        if input_lengths is not None:
            lens = check_input_lengths(input_lengths, inputs.shape[0], inputs.shape[1], "CTC",
                                       keep_full=inputs.dtype != torch.float32)
        if not self.use_pt and inputs.requires_grad and inputs.dtype == torch.float32 and \
                E.ctc_fast_path_ok(max((t.numel() for t in targets), default=0), inputs.shape[2]):
            return _ctc_loss(inputs, targets, self.blank, "mean", True, lens)
        log_probs = torch.nn.functional.log_softmax(inputs, dim=2)
        if self.use_pt:  # ctc.py:109-121
            return torch.nn.functional.ctc_loss(
                log_probs.permute(1, 0, 2), torch.cat(targets),
                [inputs.shape[1]] * inputs.shape[0] if lens is None else list(lens),
                [t.numel() for t in targets], blank=self.blank, zero_infinity=True,
            )
        return CTCLoss(log_probs, [t.tolist() for t in targets], self.blank, "mean", lens)

    def _device_decode(self, outputs):
        """(x, drop, flags) of the device decode viterbi() and errors() take, or None: the host decodes"""
        if (outputs.is_cuda and outputs.dtype == torch.float32 and outputs.dim() == 3 and outputs.numel() > 0
                and 0 <= self.blank < outputs.shape[2]):
            return outputs.detach().contiguous(), self.blank, N.DECODE_NAN_IS_MAX
        return None

    def viterbi(self, outputs, input_lengths=None):
        """Greedy decode (ctc.py:126-135): argmax, collapse repeats, drop blank.  `input_lengths` (an addition, see
        CTCLoss): row b is decoded as outputs[b, :T_b] -- a pad frame is a blank, which the collapse drops."""
        lens = None
        if input_lengths is not None:
            lens = check_input_lengths(input_lengths, outputs.shape[0], outputs.shape[1], "CTC.viterbi")
        plan = self._device_decode(outputs)
        if plan is not None:
            # argmax (torch.argmax's rule for NaNs), collapse and drop on the device: only the labels that survive travel
            if lens is None:
                return E.decode_emissions(plan[0], plan[1], flags=plan[2], dtype=torch.int64)
            with torch.cuda.device(outputs.device):  # (the lengths are staged through the current device's stream)
                xlen = E.input_lengths_on_device(lens, outputs.device)
                return E.decode_emissions(plan[0], plan[1], flags=plan[2], dtype=torch.int64, lengths=xlen)
        best = torch.argmax(outputs, dim=2).to("cpu").numpy()
        if lens is not None:
            for b, n in enumerate(lens):
                best[b, n:] = self.blank
        flat, kept = E.collapse_rows(best, drop=self.blank)  # (the whole batch at once: no loop over the rows)
        return E.split_rows(flat, kept, torch.int64)

    def _beam_plan(self, outputs, input_lengths, what, *options, lookahead=None):
        """The arguments of a beam search, checked before anything needs a device: (the E.BeamPlan of `options`, which
        are BeamPlan.checked's from beam_size to word_bonus, and of `lookahead`; lengths or None)"""
        E.check_beam_outputs(outputs, what)
        B, T, C = outputs.shape
        if C < 1:
            raise ValueError(f"{what}: outputs have no classes")
        plan = E.BeamPlan.checked(C, self.blank, *options, what, lookahead=lookahead)
        return plan, None if input_lengths is None else check_input_lengths(input_lengths, B, T, what)

    @staticmethod
    def _beam_emissions(outputs):
        """float32, contiguous, on a GPU: the tensor's own, or the required one (the criteria's rule: no host path)"""
        dev = outputs.device if outputs.is_cuda else E.require_gpu()
        return outputs.detach().to(device=dev, dtype=torch.float32).contiguous()

    @E.on_input_device
    def beam_search(self, outputs, beam_size=16, classes_per_frame=None, nbest=1, input_lengths=None, return_scores=False,
                    lm=None, lm_weight=1.0, length_bonus=0.0, lm_eos=True, lexicon=None, word_bonus=0.0, lookahead=None):
        """CTC prefix beam search (an addition: the reference has the greedy decode only).  viterbi() maximises over
        frame paths; this maximises over label sequences, whose probability is the sum over all their alignments
        (DESIGN.md section 17 has the rules; csrc/beam_kernels.hip runs them, in float64).  Per frame only the
        `classes_per_frame` best classes (default min(C, 32)) and the blank extend a hypothesis; `beam_size` (1..64)
        hypotheses survive a frame.  nbest == 1: B int64 CPU tensors, what viterbi() returns; otherwise a list of `nbest`
        such tensors per utterance, best first (a rank beyond the final beam is empty).  return_scores: also a float64
        CPU tensor [B, nbest] of log P(sequence | outputs[b, :T_b]) under log_softmax(outputs) -- the module's outputs
        are raw scores --, -inf for an empty rank.  `input_lengths`: see CTCLoss.  `lm`: an lm.NGramLM over this
        model's classes (NGramLM.from_arpa reads an ARPA file), fused into the search on the device (DESIGN.md section
        18): extending a hypothesis by a token adds lm_weight * log P_LM(token | history) + length_bonus to its score,
        a token the LM cannot follow the history with is never emitted, and with `lm_eos` every final hypothesis gets
        lm_weight * log P_LM(</s> | history) before the ranks are taken; the scores then include these terms.  Without
        an lm the call is what it was, and lm_weight, length_bonus, lm_eos must be left alone.  `lexicon`: a
        lexicon.Lexicon over this model's classes: only sequences of its words are returned (a
        hypothesis that ends inside a word is dropped after the last frame; nothing left: the empty sequence, -inf),
        `lm` is then a word-level LM over the lexicon's word ids (NGramLM.from_arpa(path, words, blank=len(words))), a
        completed word adds lm_weight * log P_LM(word | history) + word_bonus and every label length_bonus; the output
        is still the token labels, lexicon.words() gives the words.  A start-marked lexicon (Lexicon(...,
        boundary="start"), DESIGN.md section 26: word pieces that carry the word boundary at the start of a word, words
        that are prefixes of one another or have several spellings) is taken as it is: a word then ends where the next
        begins or with the utterance, and a hypothesis is ranked without the LM term of its last, unfinished word until
        then.  `word_bonus` needs a lexicon.  `lookahead` (it needs a lexicon and an lm): "unigram"
        or an array of one finite score per word -- the best score of the words below a trie node is paid provisionally,
        times lm_weight, while a word is being spelled and settled where the word ends, so that a narrow beam ranks a
        hypothesis by the word the LM wants; unpruned the results are those without it.  "unigram" takes
        lm.unigram_scores(), a word without one the smallest of the others.  CTC's search: ASG has
        its own (ASG.beam_search), the Transducer's token graphs have none."""
        plan, lens = self._beam_plan(outputs, input_lengths, "CTC.beam_search", beam_size, classes_per_frame, nbest, lm,
                                     lm_weight, length_bonus, lm_eos, lexicon, word_bonus, lookahead=lookahead)
        if outputs.shape[0] == 0 or outputs.shape[1] == 0:
            hyps, scores = plan.no_frames(outputs.shape[0])
        else:
            x = self._beam_emissions(outputs)
            with torch.cuda.device(x.device), torch.no_grad():
                xlen = None if lens is None else E.input_lengths_on_device(lens, x.device)
                hyps, scores = plan.search(x, xlen, normalize=True)
        if plan.nbest == 1:
            hyps = [h[0] for h in hyps]
        return (hyps, scores) if return_scores else hyps

    @E.on_input_device
    def errors(self, outputs, targets, counter, input_lengths=None, beam_size=None, classes_per_frame=None, lm=None,
               lm_weight=1.0, length_bonus=0.0, lm_eos=True, lexicon=None, word_bonus=0.0, lookahead=None):
        """compute_edit_distance(self.viterbi(outputs), targets, preprocessor) (train.py:74-87, 278-284) as
        (tokens_dist, words_dist, n_tokens, n_words), with `counter` a metrics.ErrorCounter: where viterbi() decodes on
        the device the count runs behind the same decode and the predictions never reach the host.  `input_lengths`
        (an addition, see CTCLoss): the predictions are viterbi(outputs, input_lengths)'s.  `beam_size` (an addition):
        the predictions are beam_search(outputs, beam_size, classes_per_frame, input_lengths=input_lengths)'s instead,
        counted behind the beam launch on its device buffers; `lm`, `lm_weight`, `length_bonus`, `lm_eos`, `lexicon`,
        `word_bonus`, `lookahead` are beam_search's and need a beam_size."""
        if beam_size is None:
            E.BeamPlan.refuse_without_beam(lm, lm_weight, length_bonus, lm_eos, lexicon, word_bonus, "CTC.errors",
                                           lookahead=lookahead)
        else:
            plan, lens = self._beam_plan(outputs, input_lengths, "CTC.errors", beam_size, classes_per_frame, 1, lm, lm_weight,
                                         length_bonus, lm_eos, lexicon, word_bonus, lookahead=lookahead)
            C = outputs.shape[2]
            counter.check_hypothesis_labels(C - 1 if self.blank == C - 1 else C, "CTC.errors")
            if outputs.shape[0] == 0 or outputs.shape[1] == 0:
                return counter([h[0] for h in plan.no_frames(outputs.shape[0])[0]], targets)
            x = self._beam_emissions(outputs)
            with torch.cuda.device(x.device), torch.no_grad():
                xlen = None if lens is None else E.input_lengths_on_device(lens, x.device)
                return counter.totals(M.plan_errors(counter, targets, x, plan, xlen))
        lens = None
        if input_lengths is not None:
            lens = check_input_lengths(input_lengths, outputs.shape[0], outputs.shape[1], "CTC.errors")
        C = outputs.shape[2]
        counter.check_hypothesis_labels(C - 1 if self.blank == C - 1 else C, "CTC.errors")  # (the blank is never emitted)
        with torch.no_grad():
            plan = self._device_decode(outputs)
            if plan is None:
                return counter(self.viterbi(outputs, lens), targets)
            xlen = None if lens is None else E.input_lengths_on_device(lens, outputs.device)
            return counter.totals(M.decode_emissions_errors(counter, targets, plan[0], plan[1], flags=plan[2], lengths=xlen))
