"""Device orchestration for the WFST loss engine: owns the torch-allocated buffers, the packed
lattices and the calls into libwfl.so.  torch is plumbing here (device memory + current stream);
all arithmetic happens in the HIP kernels behind the C ABI (include/wfl.h).
"""
import ctypes
import itertools
import math
import numbers
import operator
import sys
import threading
import weakref
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _native as N
from .lexicon import Lexicon, LexiconLookahead, check_lookahead, check_word_lm
from .lm import NGramLM

_F32 = torch.float32


_HAVE_GPU = None
_DEVICES = {}


def require_gpu():
    global _HAVE_GPU
    if _HAVE_GPU is None:  # (a visible GPU does not go away within a process)
        _HAVE_GPU = bool(torch.cuda.is_available())
    if not _HAVE_GPU:
        raise RuntimeError(
            "gtn_applications_amd: no ROCm GPU visible. The criteria run on HIP kernels only; "
            "there is deliberately no CPU fallback."
        )
    idx = torch.cuda.current_device()
    dev = _DEVICES.get(idx)
    if dev is None:
        dev = _DEVICES[idx] = torch.device("cuda", idx)
    return dev


def stream_ptr():
    # raw handle of torch's current stream on the current device (what current_stream().cuda_stream
    # returns, without building the Stream object: this sits on every launch).  Plain ints: ctypes converts them
    # for c_void_p parameters without a Python-level c_void_p object per argument.
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()) or None


def ptr(t):
    """device pointer argument: a tensor, a raw address (int) or None"""
    if t is None:
        return None
    return t if type(t) is int else t.data_ptr()


def as_device_f32(t, device):
    """float32, contiguous, on `device` (the reference reads raw float32 too: ctc.py:43-44)."""
    if t.dtype != _F32:
        raise TypeError(f"expected a float32 tensor, got {t.dtype}")
    if t.device != device:
        t = t.to(device)
    return t.contiguous()


def flatten_targets(targets):
    """list of int sequences (or 1-D tensors) -> (flat int32, offsets int64, lengths list)."""
    rows = [t.tolist() if hasattr(t, "tolist") else list(t) for t in targets]
    lens = [len(r) for r in rows]
    flat = np.fromiter(itertools.chain.from_iterable(rows), dtype=np.int32, count=sum(lens))
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return flat, offsets, lens


# bench.py sets this to a list to time the native launches of a step with HIP events recorded on the stream
# each launch goes to: entries are (phase name, start event, end event).  None (the default) costs one test.
PHASE_EVENTS = None
PHASE_ONLY = None  # optional set of phase names: the only ones recorded (bench.py's timed region records one)
PHASE_STRIDE = 1   # record every PHASE_STRIDE-th launch of a phase (an event pair costs the step ~10 us)
_PHASE_COUNT = {}


_EVENT_POOLS = {}  # device index -> timing events free for reuse (an event belongs to the device it was first recorded on)


def _event_pool():
    idx = torch.cuda.current_device()
    pool = _EVENT_POOLS.get(idx)
    if pool is None:
        pool = _EVENT_POOLS[idx] = []
    return pool


def prealloc_events(n):
    """bench.py: create the timing events of a timed region up front (hipEventCreate costs more than the record)"""
    pool = _event_pool()
    while len(pool) < n:
        pool.append(torch.cuda.Event(enable_timing=True))


def _event():
    pool = _event_pool()
    ev = pool.pop() if pool else torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


def on_input_device(fn):
    """Run a criterion entry point with the device of its first CUDA tensor argument current (the reference's
    criteria return results on the inputs' device whatever the current device is: ctc.py:69, asg.py:139).  Every
    per-device resource of the engine -- staging rings, workspaces, streams, timing events -- is looked up through
    the current device, so the switch is all it takes; nothing is done when it already is the current one."""
    def wrapped(*args, **kwargs):
        for a in args:
            if type(a) is torch.Tensor or isinstance(a, torch.Tensor):
                if a.is_cuda and a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)

    wrapped.__name__, wrapped.__doc__ = getattr(fn, "__name__", "wrapped"), fn.__doc__
    return wrapped


def phase_events(step, names):
    """The timing events of a step that issues every launch group of `names` in one native call (csrc/torch_ops.cpp:
    criterions/asg.py, transducer.py): a start and an end handle per group, 0 for a group not timed, which the call
    records around the group's launches -- or None when no group of THIS step is timed.  Under PHASE_STRIDE every
    PHASE_STRIDE-th step of `step` is, with all its groups that are due; each pair goes to PHASE_EVENTS, as _done does."""
    if PHASE_EVENTS is None or (PHASE_ONLY is not None and not any(n in PHASE_ONLY for n in names)):
        return None
    if PHASE_STRIDE > 1:
        key = "step:" + step
        k = _PHASE_COUNT[key] = _PHASE_COUNT.get(key, 0) + 1
        if k % PHASE_STRIDE:
            return None
    handles = []
    for name in names:
        if PHASE_ONLY is None or name in PHASE_ONLY:
            a, b = _event(), _event()  # (recorded once by _event: their HIP events exist; the call records them again)
            PHASE_EVENTS.append((name, a, b))
            handles += [a.cuda_event, b.cuda_event]
        else:
            handles += [0, 0]
    return handles


def _mark(name):
    if PHASE_EVENTS is None or (PHASE_ONLY is not None and name not in PHASE_ONLY):
        return None
    if PHASE_STRIDE > 1:
        k = _PHASE_COUNT[name] = _PHASE_COUNT.get(name, 0) + 1
        if k % PHASE_STRIDE:
            return None
    return name, _event()


def _done(tok):
    if tok is not None:
        PHASE_EVENTS.append((tok[0], tok[1], _event()))


def flatten_any(targets):
    """Targets as the criteria receive them -- a list of int sequences or of 1-D LongTensors (train.py hands over
    tensors, the benchmarks lists) -> (flat int32 array, offsets int64 [B+1], lengths).  Tensors are flattened
    with one torch.cat instead of B tolist() calls."""
    if len(targets) and all(type(t) is torch.Tensor and t.dim() == 1 and not t.is_cuda for t in targets):
        lens = [t.numel() for t in targets]
        flat = torch.cat(targets).to(torch.int32).numpy() if sum(lens) else np.zeros(0, np.int32)
        offsets = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        return flat, offsets, lens
    return flatten_targets(targets)


class LRU:
    def __init__(self, capacity=32):
        self.capacity = capacity
        self.data = OrderedDict()

    def get(self, key, make):
        hit = self.data.get(key)
        if hit is not None:
            self.data.move_to_end(key)
            return hit
        val = make()
        self.data[key] = val
        if len(self.data) > self.capacity:
            self.data.popitem(last=False)
        return val


class PackedLattice:
    """B acceptors in the flat device format of `wfl_lattice_desc`, resident in HBM."""

    def __init__(self, host_handle, device, extra=None, staged=None):
        """`extra`: optional float32 host array uploaded behind the float blob in the same copy (per-utterance loss
        factors); `self.extra` is its device view.  `staged` = (slot, buf, view): the packer already wrote the blobs
        into that staging slot (wfl_transducer_pack_batch_into)."""
        N.check_handle(host_handle)
        cuda = device is not None and device.type == "cuda"
        try:
            d = N.lib.wfl_lattice_host_desc(host_handle).contents
            self.desc = N.LatticeDesc.from_buffer_copy(d)
            ni, nf = int(d.int_words), int(d.float_words)
            ne = 0 if extra is None else int(extra.size)
            off_i = (4 * (nf + ne) + 15) & ~15  # [floats | extra | pad to 16 B | ints]: ONE buffer, one upload
            nbytes = off_i + 4 * max(ni, 1)
            external = staged is not None and N.lib.wfl_lattice_host_external(host_handle) == off_i
            if external:
                slot, buf, view = staged
                ring = _lattice_ring(device)
            elif cuda:
                # through a ring of reusable PINNED buffers and one asynchronous copy: a pageable copy is synchronous
                # (it would wait for everything queued on the stream before it -- the previous step's kernels), and
                # a fresh pinned allocation per batch costs a hipHostMalloc
                ring = _lattice_ring(device)
                if staged is not None:
                    ring.i -= 1  # (the slot offered to the packer was too small: take it again, grown)
                slot, buf, view = ring.next(nbytes, True)
            else:
                buf = torch.empty(nbytes, dtype=torch.uint8)
                view = buf.numpy()
            if nf and not external:
                ctypes.memmove(buf.data_ptr(), N.lib.wfl_lattice_host_floats(host_handle), 4 * nf)
            if ne:
                view[4 * nf:4 * (nf + ne)].view(np.float32)[:] = np.asarray(extra, dtype=np.float32).reshape(-1)
            if ni and not external:
                ctypes.memmove(buf.data_ptr() + off_i, N.lib.wfl_lattice_host_ints(host_handle), 4 * ni)
        finally:
            N.lib.wfl_lattice_host_free(host_handle)
        self.device = device
        self.max_wid = -1  # largest learnable-weight id of the arcs where the constructor knows it (from_graphs)
        self._host = None
        self._uploaded = None
        self._ordered = set()  # (streams order_behind_upload has ordered behind the upload)
        if cuda:
            blob = torch.empty(nbytes, dtype=torch.uint8, device=device)
            upload(blob, buf, nbytes)
            ev = ring.events[slot]
            if ev is None:
                ev = ring.events[slot] = torch.cuda.Event()
            ev.record()  # (the staging slot: reusable once this upload has read it)
            # the lattice's OWN event: packs are cached and may be used from another stream later, by which time the
            # slot's event may have been re-recorded on some other stream (order_behind_upload waits for this one)
            own = torch.cuda.Event()
            own.record()
            self._uploaded = (stream_ptr(), own)
        elif device is not None:
            blob = buf.to(device)
        else:
            blob = None
            self._host = (view[:4 * nf].view(np.float32).copy(), view[off_i:off_i + 4 * ni].view(np.int32).copy())
        self._blob = blob
        self.floats = blob[:4 * (nf + ne)].view(_F32) if blob is not None else None
        self.ints = blob[off_i:off_i + 4 * max(ni, 1)].view(torch.int32) if blob is not None else None
        self.extra = self.floats[nf:nf + ne] if (ne and blob is not None) else None
        self._n = (ni, nf)
        self._desc_ref = ctypes.byref(self.desc)

    def order_behind_upload(self, stream=None):
        """Before the pack is read on the current stream, or on `stream`, a side stream forked from it: that stream
        waits for the pack's upload if it was issued on neither -- a cached pack met again on another stream, one
        Transducer.prepare uploaded on its own.  Once per stream (the event is recorded once): True if it waited."""
        up = self._uploaded
        if up is None:
            return False
        cur = stream_ptr()
        key = cur if stream is None else (stream.cuda_stream or None)
        if up[0] in (cur, key) or key in self._ordered:
            return False
        (torch.cuda.current_stream() if stream is None else stream).wait_event(up[1])
        self._ordered.add(key)
        return True

    # host copies of the blobs (tests, diagnostics): kept when there is no device, fetched back otherwise
    @property
    def host_ints(self):
        return self._host[1] if self._host is not None else self.ints[:self._n[0]].cpu().numpy()

    @property
    def host_floats(self):
        return self._host[0] if self._host is not None else self.floats[:self._n[1]].cpu().numpy()

    # -- constructors ---------------------------------------------------------------------------
    @classmethod
    def from_graphs(cls, graphs, C, device, wids=None, B=None, shared=False):
        n = len(graphs)
        B = n if B is None else B
        handles = (ctypes.c_void_p * n)(*[g._h for g in graphs])
        keep = []
        wid_ptrs = None
        if wids is not None:
            arr = []
            for g, w in zip(graphs, wids):
                if w is None:
                    arr.append(None)
                    continue
                w = np.ascontiguousarray(w, dtype=np.int32)
                if w.size != g.num_arcs():
                    raise ValueError("weight-id array must have one entry per arc")
                keep.append(w)
                arr.append(w.ctypes.data)
            wid_ptrs = (ctypes.c_void_p * n)(*arr)
        h = N.lib.wfl_lattice_pack(handles, wid_ptrs, n, B, int(bool(shared)), int(C))
        pack = cls(h, device)
        pack.max_wid = max((int(w.max()) for w in keep if w.size), default=-1)
        return pack

    @classmethod
    def transducer_batch(cls, tokens, lexicon, transitions, flat, offsets, C, device, nthreads=0, extra=None):
        """Alignment acceptors of a whole batch, built and packed on the library's host thread pool
        (wfl_transducer_pack_batch: transducer.py:262-281 under gtn.parallel_for)."""
        flat = np.ascontiguousarray(flat, dtype=np.int32)
        if flat.size == 0:
            flat = np.zeros(1, np.int32)
        tr = None if transitions is None else transitions._h
        staged = None
        if device is not None and device.type == "cuda":
            # the packer writes the blobs straight into the pinned staging slot they are uploaded from
            ring = _lattice_ring(device)
            staged = ring.next(ring.nbytes, True)
            h = N.lib.wfl_transducer_pack_batch_into(tokens._h, lexicon._h, tr, flat.ctypes.data, offsets.ctypes.data,
                                                     len(offsets) - 1, int(C), int(nthreads), staged[1].data_ptr(),
                                                     staged[1].numel(), 0 if extra is None else int(extra.size))
        else:
            h = N.lib.wfl_transducer_pack_batch(tokens._h, lexicon._h, tr, flat.ctypes.data, offsets.ctypes.data,
                                                len(offsets) - 1, int(C), int(nthreads))
        return cls(h, device, extra, staged)

    @classmethod
    def ctc(cls, flat, offsets, blank, C, device):
        return cls(N.lib.wfl_lattice_pack_ctc(flat.ctypes.data, offsets.ctypes.data, len(offsets) - 1, blank, C), device)

    @classmethod
    def asg_force_align(cls, flat, offsets, C, device):
        return cls(N.lib.wfl_lattice_pack_asg_fal(flat.ctypes.data, offsets.ctypes.data, len(offsets) - 1, C), device)

    @classmethod
    def stc(cls, flat, offsets, star_idx, log_prob, C, device):
        return cls(
            N.lib.wfl_lattice_pack_stc(flat.ctypes.data, offsets.ctypes.data, len(offsets) - 1, star_idx, log_prob, C),
            device,
        )

    # -- host-side views (tests, Viterbi post-processing) -----------------------------------------
    def field(self, name, count):
        off = getattr(self.desc, name)
        src = self.host_floats if name in ("arc_w", "eps_w", "start_w", "accept_w") else self.host_ints
        return src[off:off + count]


def check_weight_ids(pack, weights, what):
    """The kernels index `weights` (and the gradient w.r.t. it) with the arcs' weight ids: an id beyond the tensor is a
    caller error, rejected before any kernel reads or adds there.  (raw addresses cannot be checked)"""
    if pack.max_wid >= 0 and isinstance(weights, torch.Tensor) and weights.numel() <= pack.max_wid:
        raise ValueError(f"{what}: weight id {pack.max_wid} is outside the {weights.numel()} learnable weights")


class LatticeState:
    """Everything the backward pass needs from a forward pass of the lattice engine."""

    __slots__ = ("pack", "T", "C", "xg", "alpha", "beta", "logz", "weights", "bptr", "x", "row_lse")


def lattice_diagnostics():
    """Counters of the gradient beside the sweeps (wfl_lattice_diagnostics): how often it was launched, how often its
    gate gave up (the call then fell back to the plain gradient for every row), the back-off state."""
    out = (ctypes.c_uint64 * 8)()
    N.check(N.lib.wfl_lattice_diagnostics(out, 8))
    names = ("launched", "gate_gave_up", "gate_ok", "skipped_in_backoff", "backoff_left", "env_serialised", "gate_spins", "fork")
    return dict(zip(names, (int(v) for v in out)))


def lattice_forward(x, pack, weights=None, need_beta=True, semiring=N.SEMIRING_LOG, log_softmax=False):
    """forward_score(intersect(emissions, A_b)) for every b: returns a LatticeState whose `logz`
    holds the per-utterance score (gtn call sites: ctc.py:50, asg.py:111, stc.py:86,
    transducer.py:283,287)."""
    B, T, C = x.shape
    d = pack.desc
    pack.order_behind_upload()
    if d.B != B:
        raise ValueError(f"lattice batch has {d.B} utterances, emissions have {B}")
    check_weight_ids(pack, weights, "lattice_forward")
    n_xg, n_ab = ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib.wfl_lattice_workspace(pack._desc_ref, T, ctypes.byref(n_xg), ctypes.byref(n_ab)))
    dev = x.device
    st = LatticeState()
    st.pack, st.T, st.C, st.weights = pack, T, C, weights
    st.xg = torch.empty(max(n_xg.value, 1), dtype=_F32, device=dev)
    st.alpha = torch.empty(max(n_ab.value, 1), dtype=_F32, device=dev)
    tropical = semiring == N.SEMIRING_TROPICAL
    st.beta = torch.empty(max(n_ab.value, 1), dtype=_F32, device=dev) if (need_beta and not tropical) else None
    st.bptr = torch.empty(max(n_ab.value, 1), dtype=torch.int32, device=dev) if tropical else None
    st.logz = torch.empty(B, dtype=_F32, device=dev)
    # log_softmax=True: x holds raw scores; the gather subtracts each row's log-sum-exp and the
    # gradient kernel differentiates through it (ctc.py:107, transducer.py:186-187 fused into the path)
    st.x = x if log_softmax else None
    st.row_lse = torch.empty((B, T), dtype=_F32, device=dev) if log_softmax else None
    s = stream_ptr()
    tag = "/shared" if d.shared else ""
    tok = _mark("lattice_gather" + tag)
    N.check(N.lib.wfl_lattice_gather(pack._desc_ref, ptr(pack.ints), ptr(x), T, C, ptr(st.xg), ptr(st.row_lse), s))
    _done(tok)
    tok = _mark("lattice_chain" + tag)
    N.check(
        N.lib.wfl_lattice_forward(
            pack._desc_ref, ptr(pack.ints), ptr(pack.floats), ptr(st.xg), T, ptr(weights), semiring,
            ptr(st.alpha), ptr(st.beta), ptr(st.bptr), ptr(st.logz), s,
        )
    )
    _done(tok)
    return st


def lattice_formats(st):
    """int32 [B] (device): how each utterance of a log-semiring forward pass was swept -- 1: fp64 probability domain
    (2: its sweeps met in the middle and left occupancies), 0: log domain (the certificate's repair: the two
    probability-domain sweeps disagreed about Z; an acceptor outside the lean sweeps' shape in the launch that has the
    gradient beside the sweeps; WFL_LATTICE_DOMAIN=log).  Diagnostics and tests (wfl_lattice_formats_offset)."""
    B = st.pack.desc.B
    pos = ctypes.c_int64()
    N.check(N.lib.wfl_lattice_formats_offset(st.pack._desc_ref, st.T, ctypes.byref(pos)))
    off = pos.value
    return st.alpha[off:off + B].view(torch.int32)


def lattice_grad(st, coef, coef_w=None, gout=None, dx=None, accumulate=False, dW=None):
    """Posteriors of the lattice -> dense emission gradient rows (and learnable-weight grads)."""
    p = st.pack
    check_weight_ids(p, dW, "lattice_grad")
    tok = _mark("lattice_grad" + ("/shared" if p.desc.shared else ""))
    N.check(
        N.lib.wfl_lattice_grad(
            p._desc_ref, ptr(p.ints), ptr(p.floats), ptr(st.xg), st.T, st.C, ptr(st.weights), ptr(st.alpha),
            ptr(st.beta), ptr(st.logz), ptr(coef), ptr(coef_w), ptr(gout), int(bool(accumulate)), ptr(st.x),
            ptr(st.row_lse), ptr(dx), ptr(dW), stream_ptr(),
        )
    )
    _done(tok)


def lattice_grad_rest(st, coef, gout, dx):
    """After a forward pass whose launch computed the emission gradient beside the sweeps (wfl_lattice_forward_grad):
    dx (already scaled by grad_output) gets the rows of the utterances the launch did not serve (wfl_lattice_grad_rest)."""
    p = st.pack
    tok = _mark("lattice_grad" + ("/shared" if p.desc.shared else ""))
    N.check(
        N.lib.wfl_lattice_grad_rest(
            p._desc_ref, ptr(p.ints), ptr(p.floats), ptr(st.xg), st.T, st.C, ptr(st.weights), ptr(st.alpha),
            ptr(st.beta), ptr(st.logz), ptr(coef), ptr(gout), ptr(st.x), ptr(st.row_lse), ptr(dx), stream_ptr(),
        )
    )
    _done(tok)


def lattice_viterbi(x, pack, weights=None):
    """viterbi_path(intersect(emissions, A_b)): list of numpy arrays of the caller's arc ids along
    the best path of each utterance (None if no accepting path), plus the best scores tensor."""
    B, T, C = x.shape
    st = lattice_forward(x, pack, weights, need_beta=False, semiring=N.SEMIRING_TROPICAL)
    stride = (T + 1) * max(1, pack.desc.max_levels) + 1
    path = torch.empty((B, stride), dtype=torch.int32, device=x.device)
    plen = torch.empty(B, dtype=torch.int32, device=x.device)
    N.check(
        N.lib.wfl_lattice_backtrace(
            pack._desc_ref, ptr(pack.ints), ptr(pack.floats), ptr(st.alpha), ptr(st.bptr), T, ptr(path), ptr(plen),
            stride, stream_ptr(),
        )
    )
    path, plen = path.cpu().numpy(), plen.cpu().numpy()
    return [None if plen[b] < 0 else path[b, :plen[b]].copy() for b in range(B)], st.logz


_SIDE_STREAMS = {}


def _order_after(waiter, signaller):
    """`waiter`'s later work after `signaller`'s earlier work.  torch's Stream.wait_stream creates and records an event
    per call; between the criteria's forked streams that record held the host for ~0.4 ms a call whenever the GPU had
    work queued (a Transducer step with a back-off model: 1.17 ms, 1.1 of them host, against 0.41 with the ring of
    device-scope events csrc/torch_ops.cpp keeps: wfl_order_event_flags) -- the host could not run ahead of the GPU."""
    N.ops.order_after(waiter.cuda_stream, signaller.cuda_stream, waiter.device.index)


class side_stream:
    """Run a block of launches on a second HIP stream that forks from / joins the current one: two
    independent latency-bound sweeps (ASG numerator and denominator) then share the GPU instead of
    queueing behind each other.  Tensors allocated inside must be passed to `keep()` so that the
    caching allocator knows the current stream uses them later."""

    def __init__(self, device):
        self.cur = torch.cuda.current_stream(device)
        key = device.index
        if key not in _SIDE_STREAMS:
            _SIDE_STREAMS[key] = torch.cuda.Stream(device)
        self.side = _SIDE_STREAMS[key]
        self.ctx = None

    def __enter__(self):
        _order_after(self.side, self.cur)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        return False

    def join(self, *tensors):
        """The current stream waits for everything launched on the side stream so far."""
        cur = torch.cuda.current_stream(self.side.device)
        _order_after(cur, self.side)
        for t in tensors:
            if t is not None:
                t.record_stream(cur)


class EagerLoss(torch.Tensor):
    """A scalar loss whose gradients the forward launches have already computed (for grad_output = 1).  A plain tensor
    in every respect but one: `loss.backward()` with no arguments -- the call of the reference's benchmarks
    (transducer_benchmark.py:47-49) and of a training loop that uses the criterion's output as its loss -- hands those
    buffers to the leaves' .grad without a trip through the autograd engine (its two thread hand-overs, the ones_like
    fill and the scale passes over [B, T, C] leave the GPU idle between the forward and the backward kernels) -- or,
    when an input is somebody's output, a parameter or a hooked leaf, starts the engine AT the inputs with those
    buffers as the root gradients (no ones_like, no trip through the criterion's node, no scale launches).  The
    autograd node offers them through `eager_take()` -> [(tensor, grad), ...] or None.  Anything else -- a gradient argument, retain_graph, create_graph, inputs=, anomaly mode, the loss
    inside a larger expression -- goes through torch.Tensor.backward / the engine, where the node scales the buffers
    by grad_output (in place, a launch that returns at once when grad_output is 1; a second pass over a retained graph
    recomputes)."""

    __torch_function__ = torch._C._disabled_torch_function_impl

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        node = self.grad_fn
        take = getattr(node, "eager_take", None)
        # (hooks on the loss itself -- register_hook, retain_grad -- and on its node only run inside the engine)
        if (take is not None and gradient is None and not retain_graph and not create_graph and inputs is None
                and self.dim() == 0 and not torch.is_anomaly_enabled() and not self._backward_hooks
                and not self.retains_grad and not getattr(node, "_wfl_hooked", False)):
            pairs = take()
            if pairs is not None:
                # the graph is spent, as after a pass of the engine without retain_graph: its buffers go, and a second
                # backward() raises instead of accumulating a recomputed gradient
                release_node(node)
                if all(plain_leaf(t) for t, _ in pairs):
                    for leaf, g in pairs:
                        if leaf.grad is None:
                            leaf.grad = g
                        else:
                            leaf.grad.add_(g)
                else:
                    # somebody's output (a model's, train.py:262-266), an nn.Parameter (DistributedDataParallel's
                    # reducer hangs on its AccumulateGrad node), a leaf with hooks: the autograd engine, started AT
                    # these tensors with the gradients the forward launches computed -- everything below them runs as
                    # under torch.Tensor.backward, only this node, the ones_like fill in front of it and its scale
                    # launches do not
                    torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
                return None
        return torch.Tensor.backward(self, gradient, retain_graph, create_graph, inputs=inputs)


class EarlyGrads:
    """The gradients the forward launches of a step wrote for grad_output = 1, until ONE backward claims them: the
    criterion's node under the autograd engine (claim) or EagerLoss.backward (take).  tensors: whose gradients; buffers:
    theirs, None where there is none; rest(gout, buffers): completes them behind the scaling (lattice_grad_rest)."""

    __slots__ = ("tensors", "buffers", "rest")

    def __init__(self, tensors, buffers, rest=None):
        self.tensors, self.buffers, self.rest = tensors, buffers, rest

    @property
    def dx(self):  # (the emission gradient's buffer, None once taken)
        return None if self.buffers is None else self.buffers[0]

    def claim(self, gout, want=None):
        """-> the buffers, scaled in place by grad_output `gout` (None: it is 1, no launch; wfl_scale returns at once when
        it is) and completed by `rest`.  want: a flag per buffer, None comes back for one not wanted, unscaled.  The
        first call takes them; every later one returns None: recompute."""
        bufs, self.buffers = self.buffers, None
        if bufs is None:
            return None
        if want is not None:
            bufs = tuple(b if w else None for b, w in zip(bufs, want))
        if gout is not None:
            live = [b for b in bufs if b is not None]
            gout = as_device_f32(gout.detach().reshape(1), live[0].device)
            for b in live:
                scale_inplace(b, gout)
        if self.rest is not None:
            self.rest(gout, bufs)
        return bufs

    def take(self):
        """EagerLoss.backward: -> [(tensor, grad), ...] with the buffers as they are; None if they are taken, or if a
        tensor cannot be handed its buffer (takes_grad) -- they stay claimable then."""
        if self.buffers is None:
            return None
        pairs = [(t, g) for t, g in zip(self.tensors, self.buffers) if g is not None]
        if not all(takes_grad(t, g) for t, g in pairs):
            return None
        if self.rest is None:
            self.claim(None)
        else:  # (it launches: on the buffers' device)
            with torch.cuda.device(pairs[0][1].device):
                self.claim(None)
        return pairs


def hold_early(ctx, early, offer):
    """forward() of a criterion: `early` (an EarlyGrads or None) on the autograd node, for backward to claim.  offer:
    EagerLoss.backward may take it too (ctx.eager_take) -- unless somebody registers a hook on the node, remembered as
    ctx._wfl_hooked: the engine runs those, EagerLoss.backward does not, so it must stand back.  The node offers no
    way to ask afterwards; the wrappers hold the node weakly (no cycle that would keep the forward's buffers alive)."""
    ctx.early = early
    if not offer:
        return
    ctx.eager_take = early.take
    ref = weakref.ref(ctx)
    ctx._wfl_hooked = False
    for name in ("register_hook", "register_prehook"):
        orig = getattr(type(ctx), name)

        def wrapped(fn, _orig=orig):
            node = ref()
            node._wfl_hooked = True
            return _orig(node, fn)

        setattr(ctx, name, wrapped)


def release_node(ctx):
    """After EagerLoss.backward handed the forward's gradients over: drop what backward would recompute from."""
    ctx._wfl_freed = True
    ctx.aux = None
    ctx.early = None
    ctx.eager_take = None


def check_not_released(ctx):
    """first line of backward(): the error torch raises for a second pass over a freed graph"""
    if getattr(ctx, "_wfl_freed", False):
        raise RuntimeError(
            "Trying to backward through the graph a second time (or directly access saved tensors after they have "
            "already been freed). Saved intermediate values of the graph are freed when you call .backward() or "
            "autograd.grad(). Specify retain_graph=True if you need to backward through the graph a second time.")


def plain_leaf(t):
    """May EagerLoss.backward write t.grad itself?  A plain leaf tensor that requires grad, on the device, without
    hooks -- and NOT an nn.Parameter: DistributedDataParallel (train.py:205-208 wraps criteria that have parameters)
    hangs its gradient all-reduce on the parameter's AccumulateGrad node, which only the autograd engine runs."""
    return (type(t) is torch.Tensor and t.is_leaf and t.requires_grad and t.is_cuda
            and not t._backward_hooks and not getattr(t, "_post_accumulate_grad_hooks", None))


def may_hand_over(t):
    """May EagerLoss.backward pass a gradient of t on itself -- to .grad if plain_leaf(t), else by starting the autograd
    engine at t?  Any float32 device tensor that requires grad (a model's output, an nn.Parameter, a leaf with hooks)."""
    return isinstance(t, torch.Tensor) and t.requires_grad and t.is_cuda and t.dtype == torch.float32


def takes_grad(t, g):
    """may_hand_over(t), and the gradient buffer g lives where t does (ASG transitions may sit on another GPU than the
    inputs: the engine running the criterion's node copies across; neither `t.grad = g` nor a root gradient may)"""
    return may_hand_over(t) and g.device == t.device and g.shape == t.shape and g.dtype == t.dtype


def make_eager(loss):
    """-> loss, as an EagerLoss if its autograd node offers `eager_take`"""
    if type(loss) is torch.Tensor and getattr(loss.grad_fn, "eager_take", None) is not None:
        loss.__class__ = EagerLoss
    return loss


def on_device_of(grad, device):
    """What a backward returns for a tensor that lives on `device`: the criteria compute on the GPU and accept CPU
    tensors, whose gradients go back to the host (None stays None)."""
    return grad if grad is None or device.type == "cuda" else grad.to(device)


def scale_inplace(v, s):
    """v *= s[0] on the device without a host sync (skipped by the kernel when s[0] == 1)."""
    N.check(N.lib.wfl_scale(ptr(v), v.numel(), ptr(s), stream_ptr()))
    return v


def reduce_loss(vals, scale, sign=1.0, out=None, minus=None):
    """out = (1/B) sum_b sign * scale[b] * (vals[b] - minus[b])   (ctc.py:68-69 and twins), on the device."""
    B = vals.numel()
    accumulate = out is not None
    if out is None:
        out = torch.empty((), dtype=_F32, device=vals.device)
    N.check(N.lib.wfl_reduce_loss(ptr(vals), ptr(minus), ptr(scale), B, float(sign), int(accumulate), ptr(out),
                                  stream_ptr()))
    return out


# -------------------------------------------------------------------------------------------------
# dense transitions
# -------------------------------------------------------------------------------------------------
class DenseState:
    __slots__ = ("alpha", "beta", "logz", "ws", "B", "T", "C")


def _dense_sizes(B, T, C):
    n, w = ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib.wfl_dense_workspace(B, T, C, ctypes.byref(n), ctypes.byref(w)))
    return n.value, w.value


def dense_forward(x, W, need_beta=True):
    B, T, C = x.shape
    st = DenseState()
    st.B, st.T, st.C = B, T, C
    st.alpha = torch.empty((B, T, C), dtype=_F32, device=x.device)
    st.beta = torch.empty((B, T, C), dtype=_F32, device=x.device) if need_beta else None
    st.logz = torch.empty(B, dtype=_F32, device=x.device)
    st.ws = torch.empty(_dense_sizes(B, T, C)[1], dtype=torch.uint8, device=x.device)
    tok = _mark("dense_chain")
    N.check(
        N.lib.wfl_dense_forward(ptr(x), ptr(W), B, T, C, N.SEMIRING_LOG, ptr(st.alpha), ptr(st.beta), None,
                                ptr(st.logz), ptr(st.ws), stream_ptr())
    )
    _done(tok)
    return st


def dense_flagged(st):
    """[B] bool: utterances the probability-domain sweeps handed to the log-domain kernels.  Beyond the on-chip class
    count (csrc/dense_wide.h: the frames of the whole batch are one product per frame) the verdict is the batch's, on W:
    every utterance or none.  (the workspace's layout is the library's: wfl_dense_workspace_field_c)"""
    B, T = st.B, st.T
    off, n = ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib.wfl_dense_workspace_field_c(B, T, st.C, N.DENSE_WS_FLAGS, ctypes.byref(off), ctypes.byref(n)))
    return st.ws[off.value:off.value + n.value].view(torch.int32).view(B, 2).ne(0).any(dim=1)


def dense_grad(x, W, st, coef, coef_w=None, gout=None, dx=None, accumulate=False, dW=None, addend=None, dW_addend=None):
    """dx / dW are OVERWRITTEN unless `accumulate`.  `addend` [B,T,C], `dW_addend` [(C+1),C]: terms added to dx / dW
    scaled by gout (gradients computed before gout was known)."""
    part = None
    if dW is not None:
        part = torch.empty(_dense_sizes(st.B, st.T, st.C)[0], dtype=_F32, device=x.device)
    tok = _mark("dense_grad")
    N.check(
        N.lib.wfl_dense_grad(ptr(x), ptr(W), st.B, st.T, st.C, ptr(st.alpha), ptr(st.beta), ptr(st.logz), ptr(coef),
                             ptr(coef_w), ptr(gout), int(bool(accumulate)), ptr(addend), ptr(dW_addend), ptr(dx),
                             ptr(dW), ptr(part), ptr(st.ws), stream_ptr())
    )
    _done(tok)


def dense_viterbi(x, W):
    B, T, C = x.shape
    alpha = torch.empty((B, T, C), dtype=_F32, device=x.device)
    bptr = None  # (no back-pointer buffer: include/wfl.h)
    path = torch.empty((B, T), dtype=torch.int32, device=x.device)
    N.check(N.lib.wfl_dense_viterbi(ptr(x), ptr(W), B, T, C, ptr(alpha), ptr(bptr), ptr(path),
                                    stream_ptr()))
    return path


# -------------------------------------------------------------------------------------------------
# CTC fast path
# -------------------------------------------------------------------------------------------------
def upload(dst, pinned, nbytes):
    """dst[:nbytes] (device uint8 tensor) = pinned[:nbytes] (pinned host uint8 tensor) on the current stream, by a
    kernel that reads the pinned buffer directly (wfl_upload): `copy_(non_blocking=True)` -- hipMemcpyAsync -- from
    pinned memory intermittently blocks the host until the stream has drained, which serialises host and GPU."""
    N.check(N.lib.wfl_upload(dst.data_ptr(), pinned.data_ptr(), int(nbytes), stream_ptr()))


class _StagingRing:
    """Pinned host buffers through which a batch's packed lattices reach the device in ONE asynchronous copy.  A slot is
    reused only after the copy that last read it has completed (event per slot)."""

    def __init__(self, slots=4, nbytes=1 << 22):
        self.bufs, self.views, self.events = [None] * slots, [None] * slots, [None] * slots
        self.i, self.nbytes = 0, nbytes

    def next(self, need, pinned):
        i = self.i = (self.i + 1) % len(self.bufs)
        if self.events[i] is not None:
            self.events[i].synchronize()
        buf = self.bufs[i]
        if buf is None or buf.numel() < need:
            n = max(self.nbytes, 1 << (int(need) - 1).bit_length())
            # every slot at once: a pinned allocation costs hundreds of microseconds -- slot by slot they would be
            # spread over the first steps of a run instead of being paid in the first one
            for k in range(len(self.bufs)):
                if self.bufs[k] is None or self.bufs[k].numel() < n:
                    if self.events[k] is not None:
                        self.events[k].synchronize()
                    self.bufs[k] = torch.empty(n, dtype=torch.uint8, pin_memory=pinned)
                    self.views[k] = self.bufs[k].numpy()
            buf = self.bufs[i]
        return i, buf, self.views[i]

    def __del__(self):
        # (freed with its thread: the buffers go back to torch's pinned pool, which must not hand them out while an
        # upload still reads them -- at interpreter exit nothing will)
        if not sys.is_finalizing():
            for ev in self.events:
                if ev is not None:
                    ev.synchronize()


_LATTICE_RINGS = threading.local()


def _lattice_ring(device):
    """The pinned staging ring of the lattice packers on `device` -- one PER HOST THREAD, freed with it: Transducer.prepare
    packs the next batch on a side thread while the caller's thread packs (ASG force alignment, Viterbi, CTC lattices)
    right after the loss; a ring's cursor, its `ring.i -= 1` retake and its per-slot events are not atomic, and two
    threads handed the same pinned slot would upload each other's bytes.  (The target stager's ring, csrc/torch_ops.cpp
    PinnedRing, is per device and only touched under the GIL without releasing it.)"""
    rings = getattr(_LATTICE_RINGS, "by_device", None)
    if rings is None:
        rings = _LATTICE_RINGS.by_device = {}
    ring = rings.get(device.index)
    if ring is None:
        ring = rings[device.index] = _StagingRing()
    return ring


_FACTORS = N.ops.FACTORS  # (the order of the per-utterance factor arrays behind the labels)


class CtcTargets:
    """Targets of a batch as the kernels want them, resident on the device: int64 offsets [B+1], int32 flat labels
    and the per-utterance loss / gradient factors of both reductions (scale_b = 1/len_b for "mean", 1 for "none";
    +-scale_b/B: ctc.py:53-58,87, asg.py:116-121,171-179) in ONE buffer filled on the host and uploaded with one
    asynchronous copy from pinned memory -- by the C++ operator's stager (csrc/torch_ops.cpp stage_targets; on the CPU:
    a host buffer, nothing uploaded).  A wrapper around its handle: a batch with the same content on the same device
    is the SAME object while the stager's 64-entry cache holds it, so `cache` (what callers derive from the batch:
    factor views, packed lattices) survives with it."""

    __slots__ = ("_st", "cache", "dev_buf", "B", "n", "max_len", "label_min", "label_max", "_lens")

    def __new__(cls, targets, device):
        st = N.ops.stage_targets(targets, device)
        if st is None:  # rows of numpy ints / ranges / tensors the stager does not read: normalise once, stage again
            st = N.ops.stage_targets([t.tolist() if hasattr(t, "tolist") else [int(v) for v in t] for t in targets],
                                     device)
            if st is None:
                raise TypeError("targets must be a sequence of int sequences or 1-D int tensors")
        tg = st.owner
        if tg is None:
            tg = st.owner = object.__new__(cls)
            tg._st, tg.cache, tg.dev_buf, tg._lens = st, {}, st.dev_buf, None
            tg.B, tg.n, tg.max_len, tg.label_min, tg.label_max = st.B, st.n, st.max_len, st.label_min, st.label_max
        return tg

    # host copies of the staged content
    @property
    def offsets(self):
        return self._st.offsets

    @property
    def flat(self):
        return self._st.flat

    @property
    def lens(self):
        if self._lens is None:
            self._lens = np.diff(self.offsets).tolist()
        return self._lens

    # raw device addresses (what the C ABI takes) and tensor views of the same memory
    def addr(self, what):
        base = self.dev_buf.data_ptr()
        if what == "offsets":
            return base
        if what == "flat":
            return base + self._st.off_flat
        return base + self._st.off_fac + 4 * self.B * _FACTORS.index(what)

    def factor(self, what):
        lo = self._st.off_fac + 4 * self.B * _FACTORS.index(what)
        return self.dev_buf[lo:lo + 4 * self.B].view(_F32)

    @property
    def dev_offsets(self):
        return self.dev_buf[:8 * (self.B + 1)].view(torch.int64)

    @property
    def dev_flat(self):
        off = self._st.off_flat
        return self.dev_buf[off:off + 4 * max(self.n, 1)].view(torch.int32)


_CTC_WS_SIZES = {}
CTC_LENGTHS_MAX_LEN = 63  # longest target whose launches read input lengths themselves (beyond: a padded copy)
CTC_FAST_MAX_LEN = 255  # longest target of the CTC fast path (four positions per lane); beyond: lattice engine
CTC_FAST_MAX_CLASSES = 16000  # widest emission row of the CTC fast path (compact gradient tiles: 8 x (4 KB + C bytes) of LDS) ...
CTC_FAST_MAX_CLASSES_LONG = 602  # ... and for targets of more than 63 labels (dense row tiles [17][C] per wave)


def check_labels(tg, C, what):
    """Labels must index the emission row: the reference's intersect would find no path (loss +inf);
    here an out-of-range label is a caller error and is rejected before any kernel indexes with it."""
    if tg.label_min < 0 or tg.label_max >= C:
        bad = tg.label_min if tg.label_min < 0 else tg.label_max
        raise ValueError(f"{what}: target label {bad} is outside [0, {C}) (emissions have {C} classes)")


def ctc_fast_path_ok(max_len, C):
    """Does the CTC fast path (csrc/ctc_kernels.hip) take this shape?  Otherwise: the generic lattice engine."""
    return max_len <= CTC_FAST_MAX_LEN and C <= (CTC_FAST_MAX_CLASSES if max_len <= 63 else CTC_FAST_MAX_CLASSES_LONG)
CTC_DEFAULT_FLAGS = 0  # (wfl_ctc_forward's flags: must be 0)


def ctc_forward(x, tg, blank, flags=None):
    B, T, C = x.shape
    key = (B, T, C, tg.max_len)
    n_ws = _CTC_WS_SIZES.get(key)
    if n_ws is None:
        n = ctypes.c_int64()
        N.check(N.lib.wfl_ctc_workspace(B, T, C, tg.max_len, ctypes.byref(n)))
        n_ws = _CTC_WS_SIZES[key] = n.value
    ws = torch.empty(n_ws, dtype=_F32, device=x.device)
    nll = torch.empty(B, dtype=_F32, device=x.device)
    if flags is None:
        flags = CTC_DEFAULT_FLAGS
    N.check(
        N.lib.wfl_ctc_forward(ptr(x), B, T, C, ptr(tg.dev_flat), ptr(tg.dev_offsets), tg.max_len, blank, flags,
                              ptr(ws), ptr(nll), stream_ptr())
    )
    return ws, nll


def row_lse(x):
    """[B,T] log-sum-exp over the classes of x [B,T,C] (the forward half of a fused log_softmax)."""
    B, T, C = x.shape
    out = torch.empty((B, T), dtype=_F32, device=x.device)
    N.check(N.lib.wfl_row_lse(ptr(x), B * T, C, ptr(out), stream_ptr()))
    return out


def collapse_rows(paths, drop=None):
    """The collapse every criterion's viterbi ends with (ctc.py:130-134, asg.py:228-233), for a whole batch at once:
    rows of `paths` (numpy [B,T] ints) with runs of equal labels reduced to one label, then the entries equal to `drop`
    removed.  Returns (flat values, row-major; lengths [B]) -- a Python loop over the rows costs milliseconds at a
    benchmark batch (128 rows of 1000 frames), this costs tens of microseconds."""
    import numpy as np

    B, T = paths.shape
    keep = np.ones((B, T), dtype=bool)
    if T > 1:
        np.not_equal(paths[:, 1:], paths[:, :-1], out=keep[:, 1:])
    if drop is not None:
        keep &= paths != drop
    return paths[keep], keep.sum(axis=1)


def split_rows(flat, lens, dtype):
    """list of B tensors (views of one CPU tensor of `dtype`) holding the rows of (flat, lens)"""
    t = torch.from_numpy(flat).to(dtype)
    return list(torch.split(t, [int(n) for n in lens]))


def row_argmax(x):
    """[B,T] int32: per frame the first maximal class of x [B,T,C] -- viterbi_path of the bare emissions graph
    (transducer.py:205-216 without transitions)."""
    B, T, C = x.shape
    out = torch.empty((B, T), dtype=torch.int32, device=x.device)
    N.check(N.lib.wfl_row_argmax(ptr(x), B * T, C, ptr(out), stream_ptr()))
    return out


def decode_chunk_frames():
    """Frames per chunk of the device decode (wfl_decode_chunk_frames): what crosses a chunk boundary is carried."""
    return int(N.lib.wfl_decode_chunk_frames())


def errors_chunk_steps():
    """Wavefront steps per LDS fill of the device error counts' distance launch (wfl_errors_chunk_steps): a strip's cell
    values and boundary column are carried across a fill."""
    return int(N.lib.wfl_errors_chunk_steps())


def decode_emissions(x, drop, bias=None, num_replabels=0, flags=0, dtype=torch.int32, lengths=None):
    """viterbi()'s decode from emissions, on the device (wfl_decode_emissions through csrc/torch_ops.cpp): per frame the
    first maximal class of x [B,T,C] (+ bias [C]), runs collapsed, `drop` (None: nothing) dropped, replabels unpacked.
    Returns B CPU tensors of `dtype` (int32 or int64), views of one tensor; only what survives the collapse leaves the
    device.  lengths (int32 [B] on x's device, input_lengths_on_device): utterance b ends at frame lengths[b]
    (wfl_decode_emissions_lengths)."""
    return N.ops.decode_emissions(x, bias, -1 if drop is None else int(drop), num_replabels, flags, dtype == torch.int64,
                                  lengths)


def decode_paths(paths, drop, num_replabels=0, flags=0, T=None, dtype=torch.int32):
    """The same decode from [B, >= T] int32 device label paths (wfl_dense_viterbi's): wfl_decode_paths."""
    T = paths.shape[1] if T is None else T
    return N.ops.decode_paths(paths, T, -1 if drop is None else int(drop), num_replabels, flags, dtype == torch.int64)


BEAM_MAX, BEAM_MAX_CLASSES = 64, 16384  # wfl_ctc_beam_search: beam width / classes per frame; classes in all


def beam_integer(v):
    """v as an int, or None where it is none: a bool (numpy's too), a float, a string"""
    try:
        return None if isinstance(v, (bool, np.bool_)) else operator.index(v)
    except TypeError:
        return None


def beam_widths(C, beam_size, classes_per_frame, nbest, what):
    """(beam, classes_per_frame, nbest) of a search over C classes within the limits of the beam kernel, or ValueError
    (`what`: the call they were given to).  classes_per_frame None: min(C, 32) -- a default, not a tuned value."""
    W = beam_integer(beam_size)
    if W is None or not 1 <= W <= BEAM_MAX:
        raise ValueError(f"{what}: beam_size must be an integer in [1, {BEAM_MAX}], got {beam_size!r}")
    K = min(C, 32) if classes_per_frame is None else beam_integer(classes_per_frame)
    if K is None or not 1 <= K <= min(C, BEAM_MAX):
        raise ValueError(f"{what}: classes_per_frame must be an integer in [1, {min(C, BEAM_MAX)}] for {C} classes, "
                         f"got {classes_per_frame!r}")
    n = beam_integer(nbest)
    if n is None or not 1 <= n <= W:
        raise ValueError(f"{what}: nbest must be an integer in [1, beam_size = {W}], got {nbest!r}")
    if C > BEAM_MAX_CLASSES:
        raise ValueError(f"{what}: {C} classes are more than the beam search takes ({BEAM_MAX_CLASSES})")
    return W, K, n


def beam_rows(flat, offsets, B, nbest, dtype=None):
    """hyps[b][r] of a beam op's (flat labels, offsets [B nbest + 1]): views of one CPU tensor, of `dtype` if given"""
    rows = (flat if dtype is None else flat.to(dtype)).split_with_sizes((offsets[1:] - offsets[:-1]).tolist())
    return [list(rows[b * nbest:(b + 1) * nbest]) for b in range(B)]


def beam_no_frames(B, nbest, dtype=torch.int64):
    """(hyps, scores) of a search over B utterances without a frame: every rank the empty sequence, with score 0"""
    hyps = [[torch.empty(0, dtype=dtype) for _ in range(nbest)] for _ in range(B)]
    return hyps, torch.zeros((B, nbest), dtype=torch.float64)


def check_beam_outputs(outputs, what):
    """ValueError unless `outputs` is what a criterion's beam search takes: a floating point [B, T, C] tensor"""
    if not isinstance(outputs, torch.Tensor) or outputs.dim() != 3:
        raise ValueError(f"{what}: outputs must be a [B, T, C] tensor")
    if not outputs.dtype.is_floating_point:
        raise ValueError(f"{what}: outputs must be a floating point tensor, got {outputs.dtype}")


# What the plans below check alike, each rule once (`what`: the call the arguments were given to).

def beam_finite(v, name, what):
    """v as a float, or ValueError unless it is a finite number: a Python or numpy number or a one-element tensor (a
    sweep over weights), never a bool or a string"""
    f = math.nan
    if not isinstance(v, (bool, np.bool_, str, bytes)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            pass
    if not math.isfinite(f):
        raise ValueError(f"{what}: {name} must be a finite number, got {v!r}")
    return f


def beam_lm_scalars(lm_weight, length_bonus, lm_eos, what, word_bonus=0.0):
    """(lm_weight, word_bonus, length_bonus, lm_eos) of an LM's terms as three floats and a bool, or ValueError: refused in
    this order"""
    weight, omega = beam_finite(lm_weight, "lm_weight", what), beam_finite(word_bonus, "word_bonus", what)
    bonus = beam_finite(length_bonus, "length_bonus", what)
    if not isinstance(lm_eos, (bool, np.bool_)):
        raise ValueError(f"{what}: lm_eos must be True or False, got {lm_eos!r}")
    return weight, omega, bonus, bool(lm_eos)


def check_built_for(built, noun, C, blank, what, need=None):
    """ValueError unless `built` -- `noun`: "the lm", "the token LM", "the lexicon", "the spelling table" -- was built for
    C classes with this blank (need: the message's words for what it must be; None: what the emissions have)"""
    if built.num_classes != C or built.blank != blank:
        raise ValueError(f"{what}: {noun} was built for {built.num_classes} classes with blank {built.blank}" +
                         (f", the emissions have {C} with blank {blank}" if need is None else f"; {need}"))


def refuse_without_lexicon(what, lm, lm_weight, length_bonus, lm_eos, word_bonus, search):
    """ValueError for a keyword of the lexicon search in a call without a lexicon: each must be at its default (`search`:
    "an ASG", "a Transducer")"""
    if lm is not None:
        raise ValueError(f"{what}: lm needs a lexicon (the lm of {search} search is a word LM)")
    for name, v, default in (("lm_weight", lm_weight, 1.0), ("length_bonus", length_bonus, 0.0), ("word_bonus", word_bonus, 0.0)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or float(v) != default:  # (numpy's numbers are Real too)
            raise ValueError(f"{what}: {name} needs a lexicon, got {v!r}")
    if lm_eos is not True:
        raise ValueError(f"{what}: lm_eos needs a lexicon, got {lm_eos!r}")


def beam_logz(x, Wt, normalize):
    """The denominator of normalised scores: logz [B] of dense_forward(x, Wt) on x's device, or None without transitions
    or without `normalize`"""
    if Wt is None or not normalize:
        return None
    with torch.cuda.device(x.device):  # (the denominator's launches go to the current device's stream)
        return dense_forward(x, Wt, need_beta=False).logz


def beam_preamble(plan, x, Wt, what, drop=None, num_replabels=0, spelling=None):
    """What the module-level searches of ASG and the Transducer do behind their plan: ValueError for transitions that are
    not [C + 1, C], a num_replabels or a drop (ASG's) out of range, a spelling (the Transducer's) that is not the plan's;
    then plan.no_frames' result where x has no frame, or None: the search runs"""
    if Wt is not None and tuple(Wt.shape) != (plan.C + 1, plan.C):
        raise ValueError(f"{what}: transitions must be [{plan.C + 1}, {plan.C}], got {tuple(Wt.shape)}")
    if not isinstance(num_replabels, int) or isinstance(num_replabels, bool) or num_replabels < 0:
        raise ValueError(f"{what}: num_replabels must be an integer >= 0, got {num_replabels!r}")
    if drop is not None and not -1 <= int(drop) < plan.C:
        raise ValueError(f"{what}: drop {drop} is outside [0, {plan.C})")
    if spelling is not None:
        check_spelling(spelling, plan, what)
    return plan.no_frames(x.shape[0]) if x.shape[0] == 0 or x.shape[1] == 0 else None


class _WithLookahead:
    """A lexicon plan whose search has word-LM look-ahead: the tuple is the plan's, .lookahead the
    prepared lexicon.LexiconLookahead that on_device() hands to the operators with it.  The plan's `checked` makes one."""

    def __new__(cls, plan, lookahead):
        self = super().__new__(cls, *plan)
        self.lookahead = lookahead
        return self


class BeamPlan(namedtuple(
        "BeamPlan", "C blank beam classes_per_frame nbest lm lm_weight length_bonus lm_eos lexicon word_bonus")):
    """The options of one CTC beam search over C classes, checked once (`checked`, the one constructor) and handed on whole:
    CTC.beam_search, CTC.errors(beam_size=) and ctc_beam_search build one plan per call, nothing behind them checks or
    lists the options again.  ints, floats, lm_eos a bool, lm an lm.NGramLM or None, lexicon a lexicon.Lexicon or None
    (lm is then its word LM).  Only on_device() and search() need a device.  lookahead: None, or the prepared
    lexicon.LexiconLookahead of a plan made with lookahead= -- not one of the tuple's fields, which
    are the options as they were: such a plan is a BeamPlanLookahead."""
    __slots__ = ()
    lookahead = None

    @classmethod
    def checked(cls, C, blank, beam_size, classes_per_frame, nbest, lm, lm_weight, length_bonus, lm_eos, lexicon, word_bonus,
                what, lookahead=None):
        """The plan of these arguments, within the limits of wfl_ctc_beam_search, or ValueError (`what`: the call they were
        given to).  classes_per_frame None: min(C, 32) -- a default, not a tuned value.  lm None: lm_weight and lm_eos at
        their defaults, and length_bonus unless there is a lexicon, whose search applies it to every label; an lm is built
        for these classes and this blank, or is the lexicon's word LM (the convention of lexicon.py).  lexicon None: no
        word_bonus.  Numbers: Python or numpy numbers, one-element tensors (a sweep over weights), never bools or strings.
        lookahead: None, "unigram" or the word scores u[v] (lexicon.check_lookahead); it needs a lexicon and an lm."""
        W, K, n = beam_widths(C, beam_size, classes_per_frame, nbest, what)
        if not 0 <= int(blank) < C:
            raise ValueError(f"{what}: blank index {blank} is outside [0, {C})")
        blank = int(blank)
        omega = beam_finite(word_bonus, "word_bonus", what)
        if lexicon is None:
            if omega != 0.0:
                raise ValueError(f"{what}: word_bonus needs a lexicon")
        elif not isinstance(lexicon, Lexicon):
            raise ValueError(f"{what}: lexicon must be a lexicon.Lexicon, got {type(lexicon).__name__}")
        else:
            check_built_for(lexicon, "the lexicon", C, blank, what)
        weight, _, bonus, lm_eos = beam_lm_scalars(lm_weight, length_bonus, lm_eos, what)
        if lm is None:
            if weight != 1.0 or (bonus != 0.0 and lexicon is None) or lm_eos is not True:
                raise ValueError(f"{what}: lm_weight, length_bonus and lm_eos need an lm" +
                                 ("" if lexicon is None else " (with a lexicon: lm_weight and lm_eos do)"))
        elif not isinstance(lm, NGramLM):
            raise ValueError(f"{what}: lm must be an lm.NGramLM, got {type(lm).__name__}")
        elif lexicon is not None:
            check_word_lm(lexicon, lm, what)
        else:
            check_built_for(lm, "the lm", C, blank, what)
        plan = cls(C, blank, W, K, n, lm, weight, bonus, lm_eos, lexicon, omega)
        look = check_lookahead(lookahead, lexicon, lm, False, what)
        return plan if look is None else BeamPlanLookahead(plan, look)

    @classmethod
    def refuse_without_beam(cls, lm, lm_weight, length_bonus, lm_eos, lexicon, word_bonus, what, lookahead=None):
        """ValueError for any of a beam search's keywords in a call that runs none: each must be at its default"""
        if lm is not None or lexicon is not None or lookahead is not None:
            raise ValueError(f"{what}: lm, lexicon and lookahead need a beam_size")
        cls.checked(1, 0, 1, None, 1, None, lm_weight, length_bonus, lm_eos, None, word_bonus, what)  # (only they can fail)

    def no_frames(self, B):
        """(hyps, scores) of search() for B utterances without a frame (B == 0 or T == 0), on the host: every rank is the
        empty sequence -- no word either --, the first scored by the LM's </s> alone"""
        if self.lm is None and self.lexicon is None:
            return beam_no_frames(B, self.nbest)
        return beam_lexicon_no_frames(B, self.nbest, self.lm, self.lm_weight, self.lm_eos)

    def on_device(self, device):
        """The plan as the operators take it (ops.BeamPlan, csrc/torch_ops.cpp), its lm and lexicon on `device` (their
        own per-device caches: nothing is uploaded twice)"""
        return N.ops.BeamPlan(blank=self.blank, beam=self.beam, classes_per_frame=self.classes_per_frame, nbest=self.nbest,
                              lm=None if self.lm is None else self.lm.on_device(device), lm_weight=self.lm_weight,
                              length_bonus=self.length_bonus, score_eos=self.lm_eos,
                              lexicon=None if self.lexicon is None else self.lexicon.on_device(device),
                              word_bonus=self.word_bonus,
                              lookahead=None if self.lookahead is None else self.lookahead.on_device(device))

    def search(self, x, lengths=None, normalize=True):
        """ctc_beam_search's (hyps, scores) for x: float32 [B,T,C] on a GPU, contiguous, C the plan's"""
        flat, offsets, scores = N.ops.ctc_beam_search(x, lengths, self.on_device(x.device), bool(normalize))
        return beam_rows(flat, offsets, x.shape[0], self.nbest), scores


class BeamPlanLookahead(_WithLookahead, BeamPlan):
    """A BeamPlan with look-ahead"""


def ctc_beam_search(x, blank, beam_size=16, classes_per_frame=None, nbest=1, lengths=None, normalize=True, lm=None,
                    lm_weight=1.0, length_bonus=0.0, lm_eos=True, lexicon=None, word_bonus=0.0, lookahead=None):
    """CTC prefix beam search on the device (wfl_ctc_beam_search through csrc/torch_ops.cpp; the rules: include/wfl.h,
    DESIGN.md section 17).  x: float32 [B,T,C] on a GPU, contiguous; lengths: int32 [B] on x's device
    (input_lengths_on_device) or None.  Returns (hyps, scores): hyps[b][r] the int64 CPU label tensor of rank r of
    utterance b (views of one tensor), scores float64 CPU [B, nbest] -- log mass of the sequence over the frames, minus
    the frames' log-sum-exps if `normalize`; a rank beyond the final beam is empty with score -inf.  Only the surviving
    labels and the scores leave the device.  lm: an lm.NGramLM -- the search of wfl_ctc_beam_search_lm (DESIGN.md section
    18): an extension by class c from LM state s adds lm_weight * step(s, c) + length_bonus, lm_eos adds lm_weight *
    step(s, </s>) after the last frame and ranks again; the scores include these terms.  lm None: the call it was.
    lexicon: a lexicon.Lexicon -- the search of wfl_ctc_beam_search_lexicon: only sequences of
    its words are returned, lm (if given) is the word LM over its word ids, a label adds length_bonus and a completed
    word lm_weight * step(s, word) + word_bonus on top.  A start-marked lexicon (lexicon.boundary == "start", DESIGN.md
    section 26) runs wfl_ctc_beam_search_lexicon_marked: the plan's DeviceLexicon carries the convention, and the word's
    term arrives with the next word's first label or after the last frame.  lexicon None: the call it was.  lookahead:
    "unigram" or word scores u[v] [num_words] -- the lexicon search with word-LM look-ahead inside words (DESIGN.md section
    27: wfl_ctc_beam_search_lexicon_lookahead and its start-marked sibling); it needs a lexicon and an lm; None: the call
    it was.  The options are one BeamPlan."""
    plan = BeamPlan.checked(x.shape[2], blank, beam_size, classes_per_frame, nbest, lm, lm_weight, length_bonus, lm_eos,
                            lexicon, word_bonus, "ctc_beam_search", lookahead=lookahead)
    return plan.search(x, lengths, normalize)


class AsgBeamPlan(namedtuple("AsgBeamPlan", "C beam classes_per_frame nbest")):
    """The options of one ASG beam search over C classes (tokens + replabels + garbage), checked once (`checked`, the one
    constructor) and handed on whole, as BeamPlan is for CTC: ASG.beam_search, ASG.errors(beam_size=) and asg_beam_search
    build one plan per call.  ASG has no blank, no input lengths and -- here -- no LM or lexicon, so four ints are all.
    Only search() and errors() need a device."""
    __slots__ = ()

    @classmethod
    def checked(cls, C, beam_size, classes_per_frame, nbest, what):
        """The plan of these arguments, within the limits of wfl_asg_beam_search, or ValueError (`what`: the call they
        were given to).  classes_per_frame None: min(C, 32) -- a default, not a tuned value.  Integers only, no bools."""
        C = beam_integer(C)
        if C is None or C < 1:
            raise ValueError(f"{what}: the emissions have no classes")
        return cls(C, *beam_widths(C, beam_size, classes_per_frame, nbest, what))

    def no_frames(self, B):
        """(hyps, scores) of search() for B utterances without a frame (B == 0 or T == 0), on the host: beam_no_frames's"""
        return beam_no_frames(B, self.nbest)

    def search(self, x, W, normalize=True, drop=None, num_replabels=0):
        """asg_beam_search's (hyps, scores) for x: float32 [B,T,C] on a GPU, contiguous, C the plan's; W: float32
        [C + 1, C] on x's device, contiguous"""
        flat, offsets, scores = N.ops.asg_beam_search(x, W, beam_logz(x, W, normalize), self.beam, self.classes_per_frame,
                                                      self.nbest, -1 if drop is None else int(drop), int(num_replabels))
        return beam_rows(flat, offsets, x.shape[0], self.nbest), scores


def asg_beam_search(x, Wt, beam_size=16, classes_per_frame=None, nbest=1, normalize=True, drop=None, num_replabels=0):
    """ASG prefix beam search on the device (wfl_asg_beam_search through csrc/torch_ops.cpp; the rules: include/wfl.h,
    DESIGN.md section 21).  x: float32 [B,T,C] on a GPU, contiguous; Wt: float32 [C + 1, C] on x's device, contiguous, the
    criterion's transitions (row 0: start -> c, row 1 + i: j -> i).  Returns (hyps, scores): hyps[b][r] the int64 CPU
    label tensor of rank r of utterance b (views of one tensor), scores float64 CPU [B, nbest] -- the log mass of the
    sequence's alignments, emissions plus transitions, minus the denominator logz_b of dense_forward(x, Wt) if
    `normalize`: then minus the ASG loss of that sequence (a lower bound of it where the beam pruned); a rank beyond the final beam is empty with score -inf.  With
    drop None and num_replabels 0 the sequences are the raw class sequences, which the scores are always of; otherwise
    `drop` is removed and replabels are unpacked on the way out (what ASG.viterbi does to a path).  Only the surviving
    labels and the scores leave the device.  The options are one AsgBeamPlan."""
    plan = AsgBeamPlan.checked(x.shape[2], beam_size, classes_per_frame, nbest, "asg_beam_search")
    return beam_preamble(plan, x, Wt, "asg_beam_search", drop, num_replabels) or plan.search(x, Wt, normalize, drop, num_replabels)


def beam_lexicon_terms(lexicon, want, need, lm, lm_weight, word_bonus, length_bonus, lm_eos, what):
    """What the lexicon searches of ASG and the Transducer check alike, or ValueError (`what`: the call the arguments
    were given to): lexicon a lexicon.Lexicon built for the (num_classes, blank) pair `want` (`need`: the message's words
    for what it must be); lm None or a word LM of it; the three numbers finite; lm_eos a bool; lm_weight and lm_eos at
    their defaults without an lm.  Returns (lm_weight, word_bonus, length_bonus, lm_eos) as floats and a bool."""
    if not isinstance(lexicon, Lexicon):
        raise ValueError(f"{what}: lexicon must be a lexicon.Lexicon, got {type(lexicon).__name__}")
    check_built_for(lexicon, "the lexicon", *want, what, need)
    weight, omega, bonus, lm_eos = beam_lm_scalars(lm_weight, length_bonus, lm_eos, what, word_bonus)
    if lm is None:
        if weight != 1.0 or lm_eos is not True:
            raise ValueError(f"{what}: lm_weight and lm_eos need an lm")
    elif not isinstance(lm, NGramLM):
        raise ValueError(f"{what}: lm must be an lm.NGramLM, got {type(lm).__name__}")
    else:
        check_word_lm(lexicon, lm, what)
    return weight, omega, bonus, lm_eos


def beam_lexicon_no_frames(B, nbest, lm, lm_weight, lm_eos, dtype=torch.int64):
    """(hyps, scores) of a search with an LM's </s> term -- a lexicon's word LM (or none), a token LM -- for B utterances
    without a frame, on the host: every rank the empty sequence, the first scored by the LM's </s> alone, the others -inf"""
    hyps, scores = beam_no_frames(B, nbest, dtype)
    # (a rank whose </s> step is -inf is dropped, whatever the weight -- never 0 * -inf or -w * -inf)
    end = 0.0
    if lm is not None and lm_eos:
        step = lm.score([], eos=True)
        end = -math.inf if step == -math.inf else lm_weight * step
    scores[:, 1:] = -math.inf
    scores[:, 0] = end
    return hyps, scores


class AsgLexiconBeamPlan(namedtuple(
        "AsgLexiconBeamPlan", "C beam classes_per_frame nbest garbage lexicon lm lm_weight word_bonus length_bonus lm_eos")):
    """The options of one ASG beam search with a lexicon (wfl_asg_beam_search_lexicon) over C raw
    classes (tokens + replabels + garbage), checked once (`checked`, the one constructor) and handed on whole:
    AsgBeamPlan's four ints, the garbage class (None: the criterion has none), a lexicon.Lexicon over raw class
    sequences (ASG.lexicon builds one), its word LM (an lm.NGramLM by the convention of lexicon.py) or None, and the
    constants of the CTC lexicon search.  Only on_device(), search() and errors need a device."""
    __slots__ = ()

    @classmethod
    def checked(cls, C, beam_size, classes_per_frame, nbest, garbage, lexicon, lm, lm_weight, word_bonus, length_bonus, lm_eos,
                what):
        """The plan of these arguments, within the limits of wfl_asg_beam_search_lexicon, or ValueError (`what`: the call
        they were given to): what AsgBeamPlan.checked refuses; a garbage outside [0, C); a lexicon that is none or was not
        built for (C, garbage) -- with a garbage class -- or (C + 1, C) -- without one: a phantom blank that is never a
        label --; an lm that is no word LM of the lexicon; lm_weight or lm_eos away from their defaults without an lm; a
        number that is not finite.  NotImplementedError for a start-marked lexicon."""
        C, W, K, n = AsgBeamPlan.checked(C, beam_size, classes_per_frame, nbest, what)
        if garbage is not None:
            g = beam_integer(garbage)
            if g is None or not 0 <= g < C:
                raise ValueError(f"{what}: the garbage class {garbage!r} is outside [0, {C})")
            garbage = g
        want = (C, garbage) if garbage is not None else (C + 1, C)
        need = (f"for {C} raw classes " + (f"with the garbage class {garbage}" if garbage is not None else
                                           "without a garbage class") +
                f" it must have {want[0]} with blank {want[1]} (ASG.lexicon builds it)")
        weight, omega, bonus, lm_eos = beam_lexicon_terms(lexicon, want, need, lm, lm_weight, word_bonus, length_bonus, lm_eos, what)
        if lexicon.boundary != "end":
            raise NotImplementedError(
                f"{what}: a start-marked lexicon (boundary='start', DESIGN.md section 26) is for CTC and the Transducer -- "
                f"replabels pack a repeated pair of classes, and how they pack across a word boundary that no separator marks "
                f"is a question of its own; ASG's grapheme lexicons end in a separator (ASG.lexicon(wordsep=))")
        return cls(C, W, K, n, garbage, lexicon, lm, weight, omega, bonus, lm_eos)

    def no_frames(self, B):
        """(hyps, scores) of search() for B utterances without a frame (B == 0 or T == 0), on the host, as
        BeamPlan.no_frames: every rank the empty sequence, the first scored by the LM's </s> alone, the others -inf"""
        return beam_lexicon_no_frames(B, self.nbest, self.lm, self.lm_weight, self.lm_eos)

    def on_device(self, device):
        """The plan as the operators take it (ops.AsgLexiconPlan, csrc/torch_ops.cpp), its lexicon and lm on `device`"""
        return N.ops.AsgLexiconPlan(beam=self.beam, classes_per_frame=self.classes_per_frame, nbest=self.nbest,
                                    garbage=-1 if self.garbage is None else self.garbage,
                                    lexicon=self.lexicon.on_device(device),
                                    lm=None if self.lm is None else self.lm.on_device(device), lm_weight=self.lm_weight,
                                    word_bonus=self.word_bonus, length_bonus=self.length_bonus, score_eos=self.lm_eos)

    def search(self, x, W, normalize=True, drop=None, num_replabels=0):
        """asg_beam_search_lexicon's (hyps, scores) for x: float32 [B,T,C] on a GPU, contiguous, C the plan's; W: float32
        [C + 1, C] on x's device, contiguous"""
        flat, offsets, scores = N.ops.asg_beam_search_lexicon(x, W, beam_logz(x, W, normalize), self.on_device(x.device),
                                                              -1 if drop is None else int(drop), int(num_replabels))
        return beam_rows(flat, offsets, x.shape[0], self.nbest), scores


def asg_beam_search_lexicon(x, Wt, lexicon, garbage=None, beam_size=16, classes_per_frame=None, nbest=1, normalize=True,
                            drop=None, num_replabels=0, lm=None, lm_weight=1.0, word_bonus=0.0, length_bonus=0.0, lm_eos=True):
    """asg_beam_search with a lexicon and an optional word LM (wfl_asg_beam_search_lexicon through csrc/torch_ops.cpp; the
    rules: include/wfl.h).  x, Wt, drop, num_replabels and the result: asg_beam_search's.  lexicon: a
    lexicon.Lexicon over RAW class sequences (replabels packed in, the garbage never spelled; ASG.lexicon builds one) for
    (C, garbage), or for (C + 1, C) where garbage is None; garbage: the class that is transparent to the trie.  Only
    sequences of the lexicon's words are returned, garbage anywhere between their classes; lm (if given) is the word LM
    over its word ids; a class other than the garbage adds length_bonus and a completed word lm_weight * step(s, word) +
    word_bonus on top; lm_eos adds lm_weight * step(s, </s>) after the last frame.  The scores include these terms.  The
    options are one AsgLexiconBeamPlan."""
    what = "asg_beam_search_lexicon"
    plan = AsgLexiconBeamPlan.checked(x.shape[2], beam_size, classes_per_frame, nbest, garbage, lexicon, lm, lm_weight,
                                      word_bonus, length_bonus, lm_eos, what)
    return beam_preamble(plan, x, Wt, what, drop, num_replabels) or plan.search(x, Wt, normalize, drop, num_replabels)


class AsgLmBeamPlan(namedtuple(
        "AsgLmBeamPlan", "C beam classes_per_frame nbest garbage replabels lm lm_weight length_bonus lm_eos")):
    """The options of one ASG beam search with a token-level n-gram LM (wfl_asg_beam_search_lm) over
    C raw classes (replabels + tokens + garbage), checked once (`checked`, the one constructor) and handed on whole:
    AsgBeamPlan's four ints, the raw alphabet the LM reads through -- the garbage class (None: the criterion has none)
    and the number of replabels --, an lm.NGramLM over the N = C - replabels - (garbage is not None) tokens, built for
    (N + 1, N) (ASG.token_lm builds one), and the scalars of the CTC search with an LM.  Only on_device(), search() and
    errors need a device."""
    __slots__ = ()

    @classmethod
    def checked(cls, C, beam_size, classes_per_frame, nbest, garbage, replabels, lm, lm_weight, length_bonus, lm_eos, what):
        """The plan of these arguments, within the limits of wfl_asg_beam_search_lm, or ValueError (`what`: the call they
        were given to): what AsgBeamPlan.checked refuses; a garbage outside [0, C); replabels that are no integer >= 0 or
        leave no token; an lm that is no lm.NGramLM or was not built for (N + 1, N); a number that is not finite; an
        lm_eos that is no bool."""
        C, W, K, n = AsgBeamPlan.checked(C, beam_size, classes_per_frame, nbest, what)
        if garbage is not None:
            g = beam_integer(garbage)
            if g is None or not 0 <= g < C:
                raise ValueError(f"{what}: the garbage class {garbage!r} is outside [0, {C})")
            garbage = g
        R = beam_integer(replabels)
        if R is None or R < 0:
            raise ValueError(f"{what}: replabels must be an integer >= 0, got {replabels!r}")
        tokens = C - R - (garbage is not None)
        if tokens < 1:
            raise ValueError(f"{what}: {R} replabels" + (" and the garbage class" if garbage is not None else "") +
                             f" leave no token among {C} classes")
        if not isinstance(lm, NGramLM):
            raise ValueError(f"{what}: the token LM must be an lm.NGramLM, got {type(lm).__name__}")
        check_built_for(lm, "the token LM", tokens + 1, tokens, what,
                        f"for {C} raw classes with {R} replabels " + ("and a garbage class" if garbage is not None else
                                                                      "and no garbage class") +
                        f" it must have {tokens + 1} with blank {tokens} (ASG.token_lm builds it)")
        weight, _, bonus, lm_eos = beam_lm_scalars(lm_weight, length_bonus, lm_eos, what)
        return cls(C, W, K, n, garbage, R, lm, weight, bonus, lm_eos)

    def no_frames(self, B):
        """(hyps, scores) of search() for B utterances without a frame (B == 0 or T == 0), on the host, as
        BeamPlan.no_frames: every rank the empty sequence, the first scored by the LM's </s> alone, the others -inf"""
        return beam_lexicon_no_frames(B, self.nbest, self.lm, self.lm_weight, self.lm_eos)

    def on_device(self, device):
        """The plan as the operators take it (ops.AsgLmPlan, csrc/torch_ops.cpp), its lm on `device` (the LM's own
        per-device cache: nothing is uploaded twice)"""
        return N.ops.AsgLmPlan(beam=self.beam, classes_per_frame=self.classes_per_frame, nbest=self.nbest,
                               garbage=-1 if self.garbage is None else self.garbage, replabels=self.replabels,
                               lm=self.lm.on_device(device), lm_weight=self.lm_weight, length_bonus=self.length_bonus,
                               score_eos=self.lm_eos)

    def search(self, x, W, normalize=True, drop=None, num_replabels=0):
        """asg_beam_search_lm's (hyps, scores) for x: float32 [B,T,C] on a GPU, contiguous, C the plan's; W: float32
        [C + 1, C] on x's device, contiguous"""
        flat, offsets, scores = N.ops.asg_beam_search_lm(x, W, beam_logz(x, W, normalize), self.on_device(x.device),
                                                         -1 if drop is None else int(drop), int(num_replabels))
        return beam_rows(flat, offsets, x.shape[0], self.nbest), scores


def asg_beam_search_lm(x, Wt, lm, garbage=None, replabels=0, beam_size=16, classes_per_frame=None, nbest=1, normalize=True,
                       drop=None, num_replabels=0, lm_weight=1.0, length_bonus=0.0, lm_eos=True):
    """asg_beam_search with a token-level n-gram LM and a length bonus (wfl_asg_beam_search_lm through csrc/torch_ops.cpp;
    the rules: include/wfl.h).  x, Wt, drop, num_replabels and the result: asg_beam_search's.
    garbage, replabels: the raw alphabet the LM reads through -- replabel k is raw class k, token i is raw class
    i + replabels, `garbage` the garbage class or None; lm: an lm.NGramLM over the N = C - replabels - (garbage is not
    None) tokens, built for (N + 1, N).  The LM reads what the mapping (drop = garbage, num_replabels = replabels) writes:
    a token steps it once, a replabel k right behind a token steps it by that token k + 1 more times, the garbage and any
    other replabel not at all; every step adds lm_weight * step(s, token) + length_bonus, lm_eos adds lm_weight *
    step(s, </s>) after the last frame and ranks again.  The scores include these terms.  The search and the n-best list
    stay over raw sequences; drop and num_replabels map the results on the way out and are independent of the LM's view
    (drop None, num_replabels 0: the raw sequences under the same LM).  The options are one AsgLmBeamPlan."""
    what = "asg_beam_search_lm"
    plan = AsgLmBeamPlan.checked(x.shape[2], beam_size, classes_per_frame, nbest, garbage, replabels, lm, lm_weight, length_bonus,
                                 lm_eos, what)
    return beam_preamble(plan, x, Wt, what, drop, num_replabels) or plan.search(x, Wt, normalize, drop, num_replabels)


class TransducerBeamPlan(namedtuple("TransducerBeamPlan", "C blank forced beam classes_per_frame nbest")):
    """The options of one Transducer beam search over C classes (tokens + the blank), checked once (`checked`, the one
    constructor) and handed on whole, as BeamPlan is for CTC and AsgBeamPlan for ASG: Transducer.beam_search,
    Transducer.errors(beam_size=) and transducer_beam_search build one plan per call.  `forced`: the token graph's
    topology (False: the optional blank without repeats, CTC's; True: the forced blank).  No input lengths, LM or
    lexicon.  Only search() and errors() need a device."""
    __slots__ = ()

    @classmethod
    def checked(cls, C, blank, forced, beam_size, classes_per_frame, nbest, what):
        """The plan of these arguments, within the limits of wfl_transducer_beam_search, or ValueError (`what`: the call
        they were given to): what AsgBeamPlan.checked refuses, a blank outside [0, C), a `forced` that is no bool (or 0 / 1)"""
        C, W, K, n = AsgBeamPlan.checked(C, beam_size, classes_per_frame, nbest, what)
        b = beam_integer(blank)
        if b is None or not 0 <= b < C:
            raise ValueError(f"{what}: blank must be an integer in [0, {C}), got {blank!r}")
        if not isinstance(forced, (bool, np.bool_)) and not (isinstance(forced, (int, np.integer)) and forced in (0, 1)):
            raise ValueError(f"{what}: forced must be a bool, got {forced!r}")
        return cls(C, b, bool(forced), W, K, n)

    def no_frames(self, B, dtype=torch.int64):
        """(hyps, scores) of search() for B utterances without a frame (B == 0 or T == 0), on the host: beam_no_frames's"""
        return beam_no_frames(B, self.nbest, dtype)

    def search(self, x, Wt=None, normalize=True, dtype=torch.int64, spelling=None):
        """transducer_beam_search's (hyps, scores) for x: float32 [B,T,C] on a GPU, contiguous, C the plan's; Wt: float32
        [C + 1, C] on x's device, contiguous, or None; the label tensors in `dtype`; spelling: None, or the Spelling of the
        plan's classes and blank (check_spelling) -- transducer_merged_search's result.  The merged search is the one
        whose kind the plan does not carry: a Spelling belongs to the criterion's tokens, not to the options of a call,
        and `type(plan) is TransducerBeamPlan` holds for both."""
        if spelling is not None:
            return transducer_merged_search(self, x, Wt, spelling, normalize, dtype)
        flat, offsets, scores = N.ops.transducer_beam_search(x, Wt, beam_logz(x, Wt, normalize), self.blank, self.forced, self.beam,
                                                             self.classes_per_frame, self.nbest, bool(normalize))
        return beam_rows(flat, offsets, x.shape[0], self.nbest, dtype), scores


SPELL_MAX = 64  # include/wfl.h: WFL_SPELL_MAX, the graphemes of one class


class Spelling:
    """The spelling table of C classes for the Transducer search that merges by spelling, checked
    once (`checked`, the one constructor: wfl_spelling_check on the host arrays) and uploaded once per device
    (`on_device`, cached as metrics.ErrorCounter.tables is).  ptr: int32 [C + 1], sym: int32 [ptr[C]] -- class c spells
    the graphemes sym[ptr[c]:ptr[c + 1]], the blank nothing, every other class 1 .. SPELL_MAX non-negative integers."""

    def __init__(self, ptr, sym, blank):
        self.ptr, self.sym, self.blank = ptr, sym, blank
        self.num_classes, self.num_symbols = len(ptr) - 1, len(sym)
        self._device = {}

    @classmethod
    def checked(cls, spellings, blank, what="Spelling"):
        """The table of `spellings` -- a sequence over the C classes of grapheme index sequences, the blank's empty or
        None -- or ValueError (`what`: the call they were given to).  Needs no device."""
        C = len(spellings)
        b = beam_integer(blank)
        if b is None or not 0 <= b < C:
            raise ValueError(f"{what}: blank must be an integer in [0, {C}), got {blank!r}")
        rows = []
        for c, s in enumerate(spellings):
            row = [] if s is None else [beam_integer(g) for g in s]
            if any(g is None or not -2 ** 31 <= g < 2 ** 31 for g in row):
                raise ValueError(f"{what}: the spelling of class {c} must be a sequence of integers, got {s!r}")
            if c != b and not 1 <= len(row) <= SPELL_MAX:
                raise ValueError(f"{what}: class {c} spells {len(row)} graphemes, a class that is not the blank spells 1 to "
                                 f"{SPELL_MAX}")
            rows.append(row)
        ptr = np.zeros(C + 1, np.int32)
        np.cumsum([len(r) for r in rows], out=ptr[1:])
        sym = np.ascontiguousarray([g for r in rows for g in r], dtype=np.int32)
        pad = sym if len(sym) else np.zeros(1, np.int32)  # (a valid address for a table without a symbol)
        if N.lib.wfl_spelling_check(ptr.ctypes.data, pad.ctypes.data, C, b) != 0:
            raise ValueError(f"{what}: {N.last_error()}")
        return cls(ptr, sym, b)

    def on_device(self, device):
        """int32 [ptr | sym] on `device`, uploaded once"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        held = self._device.get(device)
        if held is None:
            held = self._device[device] = torch.from_numpy(np.concatenate([self.ptr, self.sym])).to(device)
        return held


def transducer_merged_search(plan, x, Wt, spelling, normalize=True, dtype=torch.int64):
    """TransducerBeamPlan.search for the search that merges by spelling (wfl_transducer_beam_search_merged): `plan` a
    checked TransducerBeamPlan, `spelling` the Spelling of its classes and blank; x, Wt, the result: as search()'s, a
    hypothesis a representative token sequence of its spelling"""
    flat, offsets, scores = N.ops.transducer_beam_search_merged(x, Wt, beam_logz(x, Wt, normalize), spelling.on_device(x.device),
                                                                spelling.num_symbols, plan.blank, plan.forced, plan.beam,
                                                                plan.classes_per_frame, plan.nbest, bool(normalize))
    return beam_rows(flat, offsets, x.shape[0], plan.nbest, dtype), scores


def check_spelling(spelling, plan, what):
    """ValueError unless `spelling` is a Spelling of the plan's classes and blank"""
    if not isinstance(spelling, Spelling):
        raise ValueError(f"{what}: spelling must be an engine.Spelling, got {type(spelling).__name__}")
    check_built_for(spelling, "the spelling table", plan.C, plan.blank, what)


def transducer_beam_search(x, Wt, blank, forced=False, beam_size=16, classes_per_frame=None, nbest=1, normalize=True,
                           spelling=None):
    """Transducer prefix beam search on the device (wfl_transducer_beam_search through csrc/torch_ops.cpp; the rules:
    include/wfl.h).  x: float32 [B,T,C] on a GPU, contiguous; Wt: float32 [C + 1, C] on x's device,
    contiguous, the frame-level transitions over the C classes in the dense engine's layout (row 0: start -> c, row
    1 + i: j -> i), or None: no transition model; blank: the blank's class; forced: the forced-blank token graph instead
    of the optional blank without repeats.  Returns (hyps, scores): hyps[b][r] the int64 CPU label tensor of rank r of
    utterance b (views of one tensor; never the blank), scores float64 CPU [B, nbest] -- the log mass of the sequence's
    alignments that the beam kept, minus the normaliser if `normalize` (with Wt the logz_b of dense_forward(x, Wt),
    without it the sum of the rows' log-sum-exps): then minus the criterion's loss of that sequence where nothing was
    pruned, a lower bound of it otherwise; a rank beyond the result is empty with score -inf.  With Wt None and forced
    False this is ctc_beam_search, bit for bit.  The options are one TransducerBeamPlan.  spelling: a Spelling of the C
    classes -- the search of wfl_transducer_beam_search_merged: hypotheses are identified by the
    graphemes they spell, a result is a representative token sequence of its spelling and its score the kept mass of
    every decomposition of that spelling; no two ranks spell the same.  spelling None: the call it was."""
    plan = TransducerBeamPlan.checked(x.shape[2], blank, forced, beam_size, classes_per_frame, nbest, "transducer_beam_search")
    return (beam_preamble(plan, x, Wt, "transducer_beam_search", spelling=spelling) or
            plan.search(x, Wt, normalize, spelling=spelling))


class TransducerLexiconBeamPlan(namedtuple(
        "TransducerLexiconBeamPlan", "C blank forced beam classes_per_frame nbest lexicon lm lm_weight word_bonus length_bonus lm_eos")):
    """The options of one Transducer beam search with a lexicon (wfl_transducer_beam_search_lexicon)
    over C classes (tokens + the blank), checked once (`checked`, the one constructor) and handed on whole:
    TransducerBeamPlan's six fields, a lexicon.Lexicon over token sequences for (C, blank) (Transducer.word_lexicon
    builds one), its word LM (an lm.NGramLM by the convention of lexicon.py) or None, and the constants of the CTC
    lexicon search.  Only on_device(), search() and errors need a device.  lookahead: as BeamPlan's -- None, or the
    prepared lexicon.LexiconLookahead of a TransducerLexiconBeamPlanLookahead."""
    __slots__ = ()
    lookahead = None

    @classmethod
    def checked(cls, C, blank, forced, beam_size, classes_per_frame, nbest, lexicon, lm, lm_weight, word_bonus, length_bonus,
                lm_eos, what, lookahead=None):
        """The plan of these arguments, within the limits of wfl_transducer_beam_search_lexicon, or ValueError (`what`:
        the call they were given to): what TransducerBeamPlan.checked refuses; a lexicon that is none or was not built
        for (C, blank); an lm that is no word LM of the lexicon; lm_weight or lm_eos away from their defaults without an
        lm; a number that is not finite; a lookahead (None, "unigram" or word scores: lexicon.check_lookahead) without an lm."""
        p = TransducerBeamPlan.checked(C, blank, forced, beam_size, classes_per_frame, nbest, what)
        need = f"the emissions have {p.C} with blank {p.blank} (Transducer.word_lexicon builds it)"
        weight, omega, bonus, lm_eos = beam_lexicon_terms(lexicon, (p.C, p.blank), need, lm, lm_weight, word_bonus, length_bonus,
                                                          lm_eos, what)
        plan = cls(*p, lexicon, lm, weight, omega, bonus, lm_eos)
        look = check_lookahead(lookahead, lexicon, lm, False, what)
        return plan if look is None else TransducerLexiconBeamPlanLookahead(plan, look)

    def no_frames(self, B, dtype=torch.int64):
        """(hyps, scores) of search() for B utterances without a frame (B == 0 or T == 0), on the host, as
        BeamPlan.no_frames: every rank the empty sequence, the first scored by the LM's </s> alone, the others -inf"""
        return beam_lexicon_no_frames(B, self.nbest, self.lm, self.lm_weight, self.lm_eos, dtype)

    def on_device(self, device):
        """The plan as the operators take it (ops.TransducerLexiconPlan, csrc/torch_ops.cpp), its lexicon and lm on `device`"""
        return N.ops.TransducerLexiconPlan(blank=self.blank, forced=self.forced, beam=self.beam,
                                           classes_per_frame=self.classes_per_frame, nbest=self.nbest,
                                           lexicon=self.lexicon.on_device(device),
                                           lm=None if self.lm is None else self.lm.on_device(device), lm_weight=self.lm_weight,
                                           word_bonus=self.word_bonus, length_bonus=self.length_bonus, score_eos=self.lm_eos,
                                           lookahead=None if self.lookahead is None else self.lookahead.on_device(device))

    def search(self, x, Wt=None, normalize=True, dtype=torch.int64):
        """transducer_beam_search_lexicon's (hyps, scores) for x: float32 [B,T,C] on a GPU, contiguous, C the plan's; Wt:
        float32 [C + 1, C] on x's device, contiguous, or None; the label tensors in `dtype`"""
        flat, offsets, scores = N.ops.transducer_beam_search_lexicon(x, Wt, beam_logz(x, Wt, normalize), self.on_device(x.device),
                                                                     bool(normalize))
        return beam_rows(flat, offsets, x.shape[0], self.nbest, dtype), scores


class TransducerLexiconBeamPlanLookahead(_WithLookahead, TransducerLexiconBeamPlan):
    """A TransducerLexiconBeamPlan with look-ahead"""


def transducer_beam_search_lexicon(x, Wt, blank, lexicon, forced=False, beam_size=16, classes_per_frame=None, nbest=1,
                                   normalize=True, lm=None, lm_weight=1.0, word_bonus=0.0, length_bonus=0.0, lm_eos=True):
    """transducer_beam_search with a lexicon and an optional word LM (wfl_transducer_beam_search_lexicon through
    csrc/torch_ops.cpp; the rules: include/wfl.h).  x, Wt, blank, forced and the result:
    transducer_beam_search's.  lexicon: a lexicon.Lexicon over token sequences for (C, blank).  Only sequences of the
    lexicon's words are returned; lm (if given) is the word LM over its word ids; every token adds length_bonus and a
    completed word lm_weight * step(s, word) + word_bonus on top; lm_eos adds lm_weight * step(s, </s>) after the last
    frame.  The scores include these terms.  With Wt None and forced False this is ctc_beam_search(lexicon=) without
    lengths, bit for bit.  A start-marked lexicon runs wfl_transducer_beam_search_lexicon_marked:
    the plan's DeviceLexicon carries the convention.  Look-ahead: `lexicon` may be the prepared
    lexicon.LexiconLookahead of one (Lexicon.lookahead(word scores), Lexicon.unigram_lookahead(lm)) -- the search is then
    wfl_transducer_beam_search_lexicon_lookahead or its start-marked sibling, and an lm is needed.  The options are one
    TransducerLexiconBeamPlan."""
    what = "transducer_beam_search_lexicon"
    lookahead = None
    if isinstance(lexicon, LexiconLookahead):
        lookahead, lexicon = lexicon, lexicon.lexicon
    plan = TransducerLexiconBeamPlan.checked(x.shape[2], blank, forced, beam_size, classes_per_frame, nbest, lexicon, lm,
                                             lm_weight, word_bonus, length_bonus, lm_eos, what, lookahead=lookahead)
    return beam_preamble(plan, x, Wt, what) or plan.search(x, Wt, normalize)


class TransducerLmBeamPlan(namedtuple(
        "TransducerLmBeamPlan", "C blank forced beam classes_per_frame nbest lm lm_weight length_bonus lm_eos")):
    """The options of one Transducer beam search with a token-level n-gram LM (wfl_transducer_beam_search_lm, DESIGN.md
    section 28) over C classes (tokens + the blank), checked once (`checked`, the one constructor) and handed on whole:
    TransducerBeamPlan's six fields, an lm.NGramLM over those classes and that blank (Transducer.token_lm builds one),
    and the scalars of the CTC search with an LM.  Only on_device(), search() and errors need a device."""
    __slots__ = ()

    @classmethod
    def checked(cls, C, blank, forced, beam_size, classes_per_frame, nbest, lm, lm_weight, length_bonus, lm_eos, what):
        """The plan of these arguments, within the limits of wfl_transducer_beam_search_lm, or ValueError (`what`: the
        call they were given to): what TransducerBeamPlan.checked refuses; an lm that is no lm.NGramLM or was not built
        for (C, blank); a number that is not finite; an lm_eos that is no bool."""
        p = TransducerBeamPlan.checked(C, blank, forced, beam_size, classes_per_frame, nbest, what)
        if not isinstance(lm, NGramLM):
            raise ValueError(f"{what}: the token LM must be an lm.NGramLM, got {type(lm).__name__}")
        check_built_for(lm, "the token LM", p.C, p.blank, what)
        weight, _, bonus, lm_eos = beam_lm_scalars(lm_weight, length_bonus, lm_eos, what)
        return cls(*p, lm, weight, bonus, lm_eos)

    def no_frames(self, B, dtype=torch.int64):
        """(hyps, scores) of search() for B utterances without a frame (B == 0 or T == 0), on the host, as
        BeamPlan.no_frames: every rank the empty sequence, the first scored by the LM's </s> alone, the others -inf"""
        return beam_lexicon_no_frames(B, self.nbest, self.lm, self.lm_weight, self.lm_eos, dtype)

    def on_device(self, device):
        """The plan as the operators take it (ops.TransducerLmPlan, csrc/torch_ops.cpp), its lm on `device` (the LM's own
        per-device cache: nothing is uploaded twice)"""
        return N.ops.TransducerLmPlan(blank=self.blank, forced=self.forced, beam=self.beam,
                                      classes_per_frame=self.classes_per_frame, nbest=self.nbest,
                                      lm=self.lm.on_device(device), lm_weight=self.lm_weight,
                                      length_bonus=self.length_bonus, score_eos=self.lm_eos)

    def search(self, x, Wt=None, normalize=True, dtype=torch.int64):
        """transducer_beam_search_lm's (hyps, scores) for x: float32 [B,T,C] on a GPU, contiguous, C the plan's; Wt:
        float32 [C + 1, C] on x's device, contiguous, or None; the label tensors in `dtype`"""
        flat, offsets, scores = N.ops.transducer_beam_search_lm(x, Wt, beam_logz(x, Wt, normalize), self.on_device(x.device),
                                                                bool(normalize))
        return beam_rows(flat, offsets, x.shape[0], self.nbest, dtype), scores


def transducer_beam_search_lm(x, Wt, blank, lm, forced=False, beam_size=16, classes_per_frame=None, nbest=1, normalize=True,
                              lm_weight=1.0, length_bonus=0.0, lm_eos=True):
    """transducer_beam_search with a token-level n-gram LM and a length bonus (wfl_transducer_beam_search_lm through
    csrc/torch_ops.cpp; the rules: include/wfl.h).  x, Wt, blank, forced and the result:
    transducer_beam_search's.  lm: an lm.NGramLM over the C classes with this blank.  An extension by token c from LM
    state s adds lm_weight * step(s, c) + length_bonus; lm_eos adds lm_weight * step(s, </s>) after the last frame, behind
    the topology's score, and ranks again.  The scores include these terms.  With Wt None and forced False this is
    ctc_beam_search(lm=) without lengths, bit for bit.  The options are one TransducerLmBeamPlan."""
    what = "transducer_beam_search_lm"
    plan = TransducerLmBeamPlan.checked(x.shape[2], blank, forced, beam_size, classes_per_frame, nbest, lm, lm_weight,
                                        length_bonus, lm_eos, what)
    return beam_preamble(plan, x, Wt, what) or plan.search(x, Wt, normalize)


_LENGTH_RINGS = threading.local()  # per host thread, like the lattice packers' rings (_lattice_ring)


def input_lengths_on_device(lengths, device):
    """int32 [B] device tensor of a padded batch's input lengths (a sequence of B ints, already checked).  A small
    upload of its own, apart from the targets' stager (whose cache and recognition of a re-used target list it does not
    touch): the lengths of a training step differ from the last step's, so nothing is cached -- they are written into
    the next slot of a ring of eight pinned buffers (allocated once; a slot is reused only after the upload that last
    read it has completed) and a kernel reads them from there (wfl_upload: asynchronous, no synchronisation).  The
    device buffer comes from torch's caching allocator; the upload and the launches that read it share the current
    stream."""
    device = torch.device(device)
    index = torch.cuda.current_device() if device.index is None else device.index
    rings = getattr(_LENGTH_RINGS, "by_device", None)
    if rings is None:
        rings = _LENGTH_RINGS.by_device = {}
    ring = rings.get(index)
    if ring is None:
        ring = rings[index] = _StagingRing(slots=8, nbytes=1 << 12)
    n = len(lengths)
    nbytes = (4 * n + 15) & ~15
    i, pinned, view = ring.next(nbytes, True)
    view[:4 * n].view(np.int32)[:] = lengths
    with torch.cuda.device(index):
        dev = torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", index))
        upload(dev, pinned, nbytes)
        done = ring.events[i]
        if done is None:
            done = ring.events[i] = torch.cuda.Event()
        done.record()
    return dev[:4 * n].view(torch.int32)


def ctc_pad_frames(x, lengths, blank):
    """A copy of x [B,T,C] (float32, contiguous, on the device) whose rows t >= lengths[b] are certain-blank frames --
    0 for the blank, -inf for every other class (wfl_ctc_pad_frames): the identity of the CTC label graph."""
    B, T, C = x.shape
    out = torch.empty_like(x)
    N.check(N.lib.wfl_ctc_pad_frames(ptr(x), ptr(lengths), B, T, C, int(blank), ptr(out), stream_ptr()))
    return out


def zero_pad_rows(dx, lengths):
    """dx[b, t, :] = 0 for t >= lengths[b], in place on the current stream (wfl_zero_pad_rows): behind every CTC
    gradient taken with input lengths, before it is handed out."""
    B, T, C = dx.shape
    N.check(N.lib.wfl_zero_pad_rows(ptr(dx), ptr(lengths), B, T, C, stream_ptr()))
    return dx


def ctc_workspace(x, max_len):
    """Scratch of the pipelined step (checkpoints, flags, certificate words) and the per-utterance nll, one per
    (device, stream, shape), kept by the C++ operator: consecutive steps on a stream are ordered, so they can share it
    -- no allocation per call.  (The returned nll is overwritten by the next step of the same shape on the same stream.)"""
    return N.ops.ctc_workspace(x, max_len)


def ctc_host_state(x, max_len):
    """The CTC step's memory between calls (`wfl_ctc_call.host_state`, include/wfl.h): the address of two int32 of pinned
    host memory per (device, stream, shape) -- the repair launch leaves there how many utterances it recomputed, the
    next call of the shape reads it (no synchronisation) and picks its launch.  One pool, the C++ operator's, for every
    caller: at most 256 shapes (least recently used out, its pair reused), pages never freed (a launch may still write
    them), zeroed by ctc_reset_state(); 0 while the current stream is being captured (no allocation: the captured step
    replays one choice)."""
    return N.ops.ctc_host_state(x, max_len)


def ctc_reset_state():
    """Forget which launch the CTC steps preferred (tests that run unrelated data through one shape)."""
    N.ops.ctc_reset_host_state()


def ctc_forward_backward(x, tg, blank, coef, gout, dx, loss_scale=None, want_loss=False, lse=None, shared_ws=False,
                         xlen=None):
    """Loss and gradient in one pipelined launch (wfl_ctc_forward_backward): returns (ws, nll) or,
    with want_loss, (ws, nll, mean_b(loss_scale[b] * nll[b]) as a 0-dim device tensor).  `coef` / `loss_scale`
    may be tensors or raw device addresses (CtcTargets.addr).  shared_ws: use the per-stream cached workspace.
    xlen (int32 [B] on the device, input_lengths_on_device; targets of up to CTC_LENGTHS_MAX_LEN labels): the launch reads
    the frames t >= xlen[b] as certain-blank frames (wfl_ctc_call.input_lengths); the caller zeroes those rows of dx."""
    B, T, C = x.shape
    if shared_ws:
        ws, nll = ctc_workspace(x, tg.max_len)
    else:
        key = (B, T, C, tg.max_len)
        n_ws = _CTC_WS_SIZES.get(key)
        if n_ws is None:
            n = ctypes.c_int64()
            N.check(N.lib.wfl_ctc_workspace(B, T, C, tg.max_len, ctypes.byref(n)))
            n_ws = _CTC_WS_SIZES[key] = n.value
        ws = torch.empty(n_ws, dtype=_F32, device=x.device)
        nll = torch.empty(B, dtype=_F32, device=x.device)
    loss = torch.empty((), dtype=_F32, device=x.device) if want_loss else None
    tok = _mark("ctc_step")
    call = N.CtcCall(tg.n, ctc_host_state(x, tg.max_len) or None, ptr(xlen))
    N.check(
        N.lib.wfl_ctc_forward_backward_call(ptr(x), B, T, C, ptr(tg.addr("flat")), ptr(tg.addr("offsets")), tg.max_len,
                                            blank, ptr(ws), ptr(nll), ptr(coef), ptr(gout), ptr(dx), ptr(loss_scale),
                                            ptr(loss), ptr(lse), ctypes.byref(call), stream_ptr())
    )
    _done(tok)
    return (ws, nll, loss) if want_loss else (ws, nll)


_CTC_WS_FIELDS = {}


def ctc_workspace_field(ws, B, T, max_len, field):
    """Slice of the CTC workspace that holds a bookkeeping field (include/wfl.h, WFL_CTC_WS_*)."""
    key = (B, T, max_len, field)
    span = _CTC_WS_FIELDS.get(key)
    if span is None:
        off, n = ctypes.c_int64(), ctypes.c_int64()
        N.check(N.lib.wfl_ctc_workspace_field(B, T, max_len, field, ctypes.byref(off), ctypes.byref(n)))
        span = _CTC_WS_FIELDS[key] = (off.value, n.value)
    return ws[span[0]:span[0] + span[1]]


def ctc_pipeline_gave_up(ws, B, T, max_len):
    """True if a gradient wave of the pipelined step stopped waiting for a checkpoint (diagnostics)."""
    return bool(ctc_workspace_field(ws, B, T, max_len, N.CTC_WS_STATUS).view(torch.int32)[0].item())


def ctc_pipeline_repaired(ws, B, T, max_len):
    """Number of utterances of the last pipelined step whose lane-exponent chains failed the certificate
    and were recomputed in the log domain by the repair launch (diagnostics; 0 on the log-domain step)."""
    return int(ctc_workspace_field(ws, B, T, max_len, N.CTC_WS_STATUS).view(torch.int32)[1].item())


def ctc_grad(x, tg, blank, ws, nll, coef, gout, dx):
    B, T, C = x.shape
    N.check(
        N.lib.wfl_ctc_grad(ptr(x), B, T, C, ptr(tg.dev_flat), ptr(tg.dev_offsets), tg.max_len, blank, ptr(ws),
                           ptr(nll), ptr(coef), ptr(gout), ptr(dx), stream_ptr())
    )


def loss_factors(tg, reduction, norm_lens=None):
    """Per-utterance loss scale and gradient coefficients as device tensors (scale, +scale/B, -scale/B).

    scale_b = 1/len_b for "mean" (1 if len_b == 0), 1 for "none" (ctc.py:53-58, asg.py:116-121,
    transducer.py:302-305).  Normalised by the target lengths they are views of the buffer uploaded with the
    targets (no kernel, no copy); `norm_lens` (STC normalises by T) builds them separately, cached on `tg`."""
    if reduction not in ("mean", "none"):
        raise ValueError("invalid value for reduction '" + str(reduction) + "'")
    key = ("factors", reduction, None if norm_lens is None else tuple(norm_lens))
    hit = tg.cache.get(key)
    if hit is None:
        if norm_lens is None:
            hit = (tg.factor("scale_" + reduction), tg.factor("cpos_" + reduction), tg.factor("cneg_" + reduction))
        else:
            sc = [1.0 / n if n > 0 else 1.0 for n in norm_lens] if reduction == "mean" else [1.0] * len(norm_lens)
            scale = torch.tensor(sc, dtype=_F32, device=tg.dev_buf.device)
            hit = (scale, scale / len(sc), -scale / len(sc))
        tg.cache[key] = hit
    return hit


def targets_on_device(targets, device):
    """Stage and upload the targets of a batch (once per distinct content: the stager's cache, CtcTargets).  A CtcTargets
    built earlier is passed through -- ordered, like every hand-out of the cache, behind its upload."""
    if isinstance(targets, CtcTargets):
        targets._st.wait_upload()
        return targets
    return CtcTargets(targets, device)
