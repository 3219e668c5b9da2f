"""The decode behind viterbi() on the device (csrc/decode_kernels.hip: wfl_decode_emissions / wfl_decode_paths) against
the host spellings it replaces in the hot path -- asg.collapse_and_unpack on a numpy array (pinned to the reference's
row-by-row spelling by tests/test_host_library.py), torch.argmax + the row-by-row collapse of ctc.py:130-134,
wfl_row_argmax + the collapse, G.transducer_decode_batch -- and the three modules' viterbi() against their host routes
(a CPU input) and the oracle.  Everything is integer labels: results must match exactly.  Shapes straddle the chunk
length K = wfl_decode_chunk_frames(): the previous label, the last kept value and the output count cross it."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import criteria as OC

pytestmark = pytest.mark.gpu


def _mods():
    from gtn_applications_amd import _native as N
    from gtn_applications_amd import engine as E
    from gtn_applications_amd import graph as G

    return N, E, G


def chunk():
    return _mods()[0].lib.wfl_decode_chunk_frames()


def frame_counts():
    K = chunk()
    return sorted({1, 2, 63, 64, 65, K - 1, K, K + 1, 2 * K + 1} - {0})


def _buffers(B, T, R):
    N, _, _ = _mods()
    cap, ws = ctypes.c_int64(), ctypes.c_int64()
    N.check(N.lib.wfl_decode_workspace(B, T, R, ctypes.byref(cap), ctypes.byref(ws)))
    assert cap.value == B * T * max(1, R)
    out = torch.full((cap.value + 8,), -99, dtype=torch.int32, device="cuda")  # (8 more: nothing may land behind the capacity)
    offs = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(ws.value, dtype=torch.uint8, device="cuda")
    return cap.value, out, offs, scratch


def _lists(B, cap, out, offs):
    torch.cuda.synchronize()
    o, f = offs.cpu().numpy(), out.cpu().numpy()
    assert o[0] == 0 and np.all(np.diff(o) >= 0) and o[B] <= cap
    assert np.all(f[o[B]:] == -99), "stores behind the end of the result"
    return [f[o[b]:o[b + 1]].tolist() for b in range(B)]


def abi_decode_paths(paths, T, drop, R, flags=0):
    """wfl_decode_paths through the C ABI on a numpy [B, stride] int32 array; device output buffers"""
    N, E, _ = _mods()
    B, stride = paths.shape
    d = torch.from_numpy(np.ascontiguousarray(paths, dtype=np.int32)).cuda()
    cap, out, offs, scratch = _buffers(B, T, R)
    N.check(N.lib.wfl_decode_paths(E.ptr(d), stride, B, T, -1 if drop is None else drop, R, flags, E.ptr(scratch), E.ptr(out),
                                   cap, E.ptr(offs), E.stream_ptr()))
    return _lists(B, cap, out, offs)


def abi_decode_emissions(x, bias, drop, R=0, flags=0):
    N, E, _ = _mods()
    B, T, C = x.shape
    cap, out, offs, scratch = _buffers(B, T, R)
    N.check(N.lib.wfl_decode_emissions(E.ptr(x), E.ptr(bias), B, T, C, -1 if drop is None else drop, R, flags, E.ptr(scratch),
                                       E.ptr(out), cap, E.ptr(offs), E.stream_ptr()))
    return _lists(B, cap, out, offs)


def host_paths(paths, drop, R):
    from gtn_applications_amd.criterions import asg

    return [t.tolist() for t in asg.collapse_and_unpack(np.ascontiguousarray(paths), drop, R)]


# ------------------------------------------------------------------------------------------------------------------
# 1. wfl_decode_paths == asg.collapse_and_unpack on the numpy array
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", frame_counts())
def test_paths_decode_equals_the_host_spelling(T):
    rs = np.random.RandomState(100 + T)
    for B in (1, 3, 8):
        for R in (0, 1, 2, 3):
            for with_drop in (False, True):
                C = R + rs.randint(1, 6) + 1
                drop = C - 1 if with_drop else None
                stride = T + (0 if (B + R) % 2 else 5)  # (path_stride > T: the padding is never read as frames)
                paths = np.full((B, stride), C - 1, np.int32)
                paths[:, :T] = np.repeat(rs.randint(0, C, size=(B, (T + 2) // 3)).astype(np.int32), 3, axis=1)[:, :T]  # runs of three
                want = host_paths(paths[:, :T], drop, R)
                assert abi_decode_paths(paths, T, drop, R) == want, (B, T, R, drop)


def test_paths_decode_hand_made_rows():
    K, R, g = chunk(), 2, 9  # labels >= 2, replabels 0 and 1, garbage 9
    T = 2 * K + 7
    rows = [
        [5] * T,                                                   # all frames equal
        [g] * T,                                                   # every frame dropped
        [4] * (K - 3) + [5] * 6 + [6] * (K - 1) + [g] * 5,         # runs that straddle both chunk boundaries
        [5] + [g] * (K + 5) + [1] + [g] * 3 + [0],                 # label, a whole chunk of garbage, replabel: expands
        [g] * (K - 1) + [7] + [g] * K + [0] + [g, 1, 3, 1],        # the same across two boundaries; a replabel behind a replabel behind garbage
        [1, 1, 0, 5, 5, 1],                                        # a replabel as the first kept value of the row
        [g] * K + [0, 6, 1, 0, 1, 6, 0],                           # ... as the first kept value of a chunk, with nothing before it
        [5, 0, 1, 6, 1, 1, 0, 0, 7],                               # a replabel behind a replabel
        [3] * K + [1] * K + [4, 0],                                # a replabel run that opens a chunk right behind a label
        [6] * (K - 1) + [1] + [g] * K + [1],                       # a replabel in a chunk's last lane, then a dropped chunk, then a replabel
    ]
    paths = np.array([r + [g] * (T - len(r)) for r in rows], np.int32)
    for drop in (g, None):
        want = host_paths(paths, drop, R)
        assert abi_decode_paths(paths, T, drop, R) == want, drop
    got = abi_decode_paths(paths, T, g, R)
    assert got[0] == [3] and got[1] == [] and got[3] == [3, 3, 3] and got[5] == [3, 3, 3] and got[7] == [3, 3, 4, 4, 4, 5]
    # every frame dropped in every row: empty rows, constant offsets
    assert abi_decode_paths(np.full((4, T), g, np.int32), T, g, R) == [[], [], [], []]
    # R = 0 on the same rows: a plain collapse + drop
    assert abi_decode_paths(paths, T, g, 0) == host_paths(paths, g, 0)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_paths_decode_at_capacity(R):
    """the largest replabel behind every label: T / 2 labels emit (1 + R) T / 2 outputs -- for R = 1 the whole capacity
    T max(1, R), to the last element of `out`"""
    K = chunk()
    T = 2 * K + 2
    rs = np.random.RandomState(R)
    labs = R + 1 + rs.randint(0, 4, size=(3, T // 2))
    labs[:, 1::2] += 4  # (neighbours differ: nothing collapses)
    paths = np.empty((3, T), np.int32)
    paths[:, 0::2], paths[:, 1::2] = labs, R - 1
    want = host_paths(paths, None, R)
    assert all(len(w) == (1 + R) * T // 2 for w in want)
    assert abi_decode_paths(paths, T, None, R) == want


def test_decode_rejects_bad_arguments():
    N, E, _ = _mods()
    B, T, C = 2, 5, 4
    x = torch.zeros((B, T, C), device="cuda")
    p = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    cap, out, offs, scratch = _buffers(B, T, 0)
    s = E.stream_ptr()

    def em(T=T, C=C, drop=0, R=0, flags=0):
        return N.lib.wfl_decode_emissions(E.ptr(x), None, B, T, C, drop, R, flags, E.ptr(scratch), E.ptr(out), cap, E.ptr(offs), s)

    def pa(stride=T, T=T, drop=0, R=0):
        return N.lib.wfl_decode_paths(E.ptr(p), stride, B, T, drop, R, 0, E.ptr(scratch), E.ptr(out), cap, E.ptr(offs), s)

    assert em() == N.WFL_OK and pa() == N.WFL_OK
    for rc in (em(T=0), em(C=0), em(R=-1), em(drop=-2), em(drop=C), pa(T=0), pa(R=-1), pa(drop=-2), pa(stride=T - 1)):
        assert rc == N.ERR_INVALID
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# 2. wfl_decode_emissions == torch.argmax + ctc.py:130-134  /  wfl_row_argmax + the collapse
# ------------------------------------------------------------------------------------------------------------------
def ctc_spelling(pred_rows, blank):
    """ctc.py:130-134, row by row"""
    res = []
    for pred in pred_rows:
        mask = pred[1:] != pred[:-1]
        pred = torch.cat([pred[0:1], pred[1:][mask]])
        res.append(pred[pred != blank].tolist())
    return res


def host_collapse(frames, drop):
    """engine.collapse_rows (the host spelling of the collapse) as lists"""
    _, E, _ = _mods()
    flat, lens = E.collapse_rows(frames, drop=drop)
    return [r.tolist() for r in np.split(flat, np.cumsum(lens)[:-1])]


def _emission_case(rs, B, T, C, special):
    x = rs.randint(-3, 4, size=(B, T, C)).astype(np.float32)  # integer scores: ties are common
    if special and T >= 2:
        x[0, 0, :] = -np.inf  # a row without a finite score
        x[0, T // 2, rs.randint(0, C)] = np.nan
        if C >= 3:
            x[B - 1, T - 1, [C - 1, C // 2]] = np.nan  # two NaNs: the first wins under torch's rule
            x[B - 1, 0, 0] = np.inf
            x[B - 1, 0, C - 1] = np.inf  # a tie at +inf
    return torch.from_numpy(x).cuda()


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 100, 128, 129, 200, 256, 257, 512, 513, 1001, 1024, 1025, 2049])
def test_emissions_decode_equals_argmax_and_the_row_by_row_collapse(C):
    N, E, _ = _mods()
    rs = np.random.RandomState(C)
    B = 3
    for T in frame_counts():
        for with_bias in (False, True):
            for special in (False, True):
                x = _emission_case(rs, B, T, C, special)
                bias = torch.from_numpy(rs.randint(-2, 3, size=C).astype(np.float32)).cuda() if with_bias else None
                scores = x + bias if with_bias else x
                blank = rs.randint(0, C)
                # torch.argmax's rule
                want = ctc_spelling(torch.argmax(scores, dim=2).cpu(), blank)
                got = abi_decode_emissions(x, bias, blank, flags=N.DECODE_NAN_IS_MAX)
                assert got == want, (C, T, with_bias, special, "nan is max")
                # wfl_row_argmax's rule (NaN = -inf, no finite score: class 0) + the collapse
                frames = E.row_argmax(scores.contiguous()).cpu().numpy()
                assert abi_decode_emissions(x, bias, blank) == host_collapse(frames, blank), (C, T, with_bias, special, "default")
                assert abi_decode_emissions(x, bias, None) == host_collapse(frames, None), (C, T, with_bias, special, "no drop")


def test_emissions_decode_nan_rules_on_hand_made_rows():
    N, _, _ = _mods()
    ninf, nan = -np.inf, np.nan
    x = torch.tensor([[[0.0, 1.0, nan, 5.0, nan],      # two NaNs: torch takes the first (2), the default rule 3
                       [ninf, ninf, ninf, ninf, ninf],  # nothing finite: 0 under both rules
                       [-0.0, 0.0, -1.0, 0.0, ninf],    # -0 == +0: the first
                       [nan, nan, nan, nan, nan],       # all NaN: 0 under both rules
                       [1.0, np.inf, nan, np.inf, 0.0]]], device="cuda")
    assert torch.argmax(x, 2).tolist() == [[2, 0, 0, 0, 2]]
    assert abi_decode_emissions(x, None, None, flags=N.DECODE_NAN_IS_MAX) == ctc_spelling(torch.argmax(x, 2).cpu(), -1) == [[2, 0, 2]]
    assert abi_decode_emissions(x, None, None) == [[3, 0, 1]]
    # replabels from emissions go through the same back end: three frames of label 3 with R = 2 are one token 1
    assert abi_decode_emissions(x[:, :1].repeat(1, 3, 1), None, None, R=2) == [[1]]


# ------------------------------------------------------------------------------------------------------------------
# 3. WFL_DECODE_BLANK_SEPARATED == the blank="forced" token graph
# ------------------------------------------------------------------------------------------------------------------
def test_blank_separated_equals_the_forced_token_graph():
    N, _, G = _mods()
    from gtn_applications_amd.criterions import transducer as TR

    K, ntok = chunk(), 5
    b = ntok
    tokens = TR.make_token_graph([(i,) for i in range(ntok)], blank="forced", allow_repeats=True)
    tokens.arc_sort()
    T = 2 * K + 3
    rs = np.random.RandomState(3)
    accepted = [
        [b] * T,
        [b, 1, 1, b, 2, b] + [b] * (T - 6),
        [b] * (K - 1) + [3] * 2 + [b] * (T - K - 1),                 # a token run across the chunk boundary
        [b] + [4] * (T - 2) + [b],
        [b, 0] * (T // 2) + [b],
    ]
    rejected = [
        [1] + [b] * (T - 1),                                         # does not start with the blank
        [b] * (T - 1) + [2],                                         # does not end with it
        [b, 1, 2, b] + [b] * (T - 4),                                # two different tokens adjacent
        [b] * (K - 1) + [1, 2] + [b] * (T - K - 1),                  # ... on the two sides of a chunk boundary
        [b] * (2 * K) + [0, b, 3],
    ]
    rows = accepted + rejected + [rs.choice([b, b, 1, 2], size=T).tolist() for _ in range(6)]
    labels = np.array(rows, np.int32)
    out, off = G.transducer_decode_batch(tokens, labels.reshape(-1), np.arange(len(rows) + 1, dtype=np.int64) * T)
    want = [out[off[i]:off[i + 1]].tolist() for i in range(len(rows))]
    assert all(len(w) == 0 for w in want[len(accepted):len(accepted) + len(rejected)]) and want[1] == [1, 2] and want[4] == [0] * (T // 2)
    assert abi_decode_paths(labels, T, b, 0, flags=N.DECODE_BLANK_SEPARATED) == want
    # the same labels as emissions (one-hot scores)
    x = torch.nn.functional.one_hot(torch.from_numpy(labels).long(), ntok + 1).float().cuda()
    assert abi_decode_emissions(x, None, b, flags=N.DECODE_BLANK_SEPARATED) == want
    # a single frame: accepted iff it is the blank
    assert abi_decode_paths(np.array([[b], [1]], np.int32), 1, b, 0, flags=N.DECODE_BLANK_SEPARATED) == [[], []]


# ------------------------------------------------------------------------------------------------------------------
# 4. the modules: same lists, dtype and device as before
# ------------------------------------------------------------------------------------------------------------------
def as_lists(tensors, dtype):
    assert isinstance(tensors, list)
    for t in tensors:
        assert t.dtype == dtype and t.device.type == "cpu" and t.dim() == 1
    return [t.tolist() for t in tensors]


def test_ctc_module_viterbi(monkeypatch):
    N, E, _ = _mods()
    from gtn_applications_amd.criterions import ctc

    K = chunk()
    rs = np.random.RandomState(11)
    B, T, C = 5, 2 * K + 9, 7
    x = torch.from_numpy(np.repeat(rs.randint(-3, 4, size=(B, (T + 1) // 2, C)), 2, axis=1)[:, :T].astype(np.float32))
    m = ctc.CTC(blank=C - 1, use_pt=False)
    want = ctc_spelling(torch.argmax(x, dim=2), C - 1)
    calls = []
    real = E.decode_emissions
    monkeypatch.setattr(E, "decode_emissions", lambda *a, **k: calls.append(1) or real(*a, **k))
    assert as_lists(m.viterbi(x.cuda()), torch.int64) == want and len(calls) == 1
    # a permuted (non-contiguous) view
    xt = x.permute(1, 0, 2).contiguous().cuda().permute(1, 0, 2)
    assert not xt.is_contiguous()
    assert as_lists(m.viterbi(xt), torch.int64) == want and len(calls) == 2
    # requires_grad emissions, as train.py hands them over
    assert as_lists(m.viterbi(x.cuda().requires_grad_(True)), torch.int64) == want
    # CPU and non-float32 inputs never touch the new path
    calls.clear()
    assert as_lists(m.viterbi(x), torch.int64) == want
    assert as_lists(m.viterbi(x.cuda().double()), torch.int64) == want
    assert calls == []
    # the result does not alias the operator's buffer: a second call leaves the first one's tensors alone
    first = m.viterbi(x.cuda())
    kept = [t.clone() for t in first]
    m.viterbi(torch.flip(x, dims=[2]).cuda())
    assert all(torch.equal(a, b) for a, b in zip(first, kept))


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("garbage", [False, True])
def test_asg_module_viterbi_equals_the_oracle(R, garbage):
    from gtn_applications_amd.criterions import asg

    rs = np.random.RandomState(10 * R + garbage)
    ncls = 6
    m = asg.ASG(ncls, num_replabels=R, use_garbage=garbage).cuda()
    C = m.N
    assert C <= 12
    B, T = 4, 40
    x = np.repeat(rs.randint(-3, 4, size=(B, T // 2, C)), 2, axis=1).astype(np.float32)
    W = rs.randint(-1, 2, size=(C + 1, C)).astype(np.float32)
    with torch.no_grad():
        m.transitions.copy_(torch.from_numpy(W))
    want = OC.asg_viterbi(x, W, R, m.garbage_idx)
    assert as_lists(m.viterbi(torch.from_numpy(x).cuda()), torch.int32) == want
    assert as_lists(m.viterbi(torch.from_numpy(x)), torch.int32) == want  # (the host route: a CPU input)


TOKEN_MODES = [("none", True), ("optional", True), ("forced", True), ("optional", False)]


def _transducer(blank, repeats, ngram, ntok, seed):
    from gtn_applications_amd.criterions import transducer as TR

    toks = [chr(ord("a") + i) for i in range(ntok)]
    m = TR.Transducer(toks, {t: i for i, t in enumerate(toks)}, ngram=ngram, blank=blank, allow_repeats=repeats).cuda()
    if ngram:
        rs = np.random.RandomState(seed)
        with torch.no_grad():
            m.transition_params.copy_(torch.from_numpy(rs.randint(-2, 3, size=m.transition_params.numel()).astype(np.float32)))
    return m, toks


@pytest.mark.parametrize("blank,repeats", TOKEN_MODES)
@pytest.mark.parametrize("ngram", [0, 1, 2])
def test_transducer_module_viterbi_equals_the_host_route(blank, repeats, ngram, monkeypatch):
    _, E, _ = _mods()
    K, ntok = chunk(), 4
    m, toks = _transducer(blank, repeats, ngram, ntok, 7)
    C = ntok + int(blank != "none")
    rs = np.random.RandomState(ngram * 10 + len(blank))
    B, T = 6, K + 9
    x = np.repeat(rs.randint(-3, 4, size=(B, (T + 2) // 3, C)), 3, axis=1)[:, :T].astype(np.float32)
    if blank == "forced":  # some rows the forced graph accepts under no model: blank first and last, tokens apart
        x[:3, 0, :] = x[:3, -1, :] = 0
        x[:3, 0, C - 1] = x[:3, -1, C - 1] = 50
        x[:3, 1:-1:2, C - 1] = 50
    x = torch.from_numpy(x)
    used = []
    for name in ("decode_emissions", "decode_paths"):
        real = getattr(E, name)
        monkeypatch.setattr(E, name, lambda *a, _n=name, _r=real, **k: used.append(_n) or _r(*a, **k))
    got = as_lists(m.viterbi(x.cuda()), torch.int32)
    assert used == ["decode_paths" if ngram == 2 else "decode_emissions"]
    want = as_lists(m.viterbi(x), torch.int32)  # a CPU input: frame labels to the host, wfl_transducer_decode_batch there
    assert len(used) == 1
    assert got == want
    if blank == "forced" and ngram == 0:
        assert any(want[:3]) and [] in want  # (accepted and rejected rows were among them)


def test_transducer_module_viterbi_equals_the_oracle():
    ntok = 3
    m, toks = _transducer("optional", False, 1, ntok, 5)
    orc = OC.TransducerOracle(toks, {t: i for i, t in enumerate(toks)}, ngram=1, blank="optional", allow_repeats=False)
    orc.transition_params = m.transition_params.detach().cpu().numpy().astype(np.float64)
    rs = np.random.RandomState(2)
    x = np.repeat(rs.randint(-3, 4, size=(3, 12, ntok + 1)), 2, axis=1).astype(np.float32)
    want = [list(p) for p in orc.viterbi(x)]
    assert as_lists(m.viterbi(torch.from_numpy(x).cuda()), torch.int32) == want


def test_transducer_host_route_is_kept_for_other_token_graphs_and_wider_emissions(monkeypatch):
    _, E, _ = _mods()
    m, _ = _transducer("optional", True, 0, 4, 1)
    used = []
    real = E.decode_emissions
    monkeypatch.setattr(E, "decode_emissions", lambda *a, **k: used.append(1) or real(*a, **k))
    x = torch.from_numpy(np.random.RandomState(0).randint(-3, 4, size=(2, 9, 5)).astype(np.float32)).cuda()
    want = as_lists(m.viterbi(x), torch.int32)
    assert used == [1]
    m.tokens.add_arc(0, 0, 1000, 1000, 0.0)  # (one arc more: no longer one of make_token_graph's graphs, same language here)
    assert as_lists(m.viterbi(x), torch.int32) == want and used == [1]


def test_modules_at_the_benchmark_shape():
    """B = 128, T = 1000, C = 100: all three criteria against their host spellings"""
    from gtn_applications_amd.criterions import asg, ctc

    g = torch.Generator().manual_seed(9)
    B, T, C = 128, 1000, 100
    x = torch.randn(B, T // 4, C, generator=g).repeat_interleave(4, dim=1).contiguous()
    xd = x.cuda()
    # CTC: the host route is pure torch
    m = ctc.CTC(blank=C - 1, use_pt=False)
    assert as_lists(m.viterbi(xd), torch.int64) == as_lists(m.viterbi(x), torch.int64)
    # ASG: 98 tokens + 1 replabel + garbage
    a = asg.ASG(98, num_replabels=1, use_garbage=True).cuda()
    with torch.no_grad():
        a.transitions.copy_(torch.randn(C + 1, C, generator=g))
    assert as_lists(a.viterbi(xd), torch.int32) == as_lists(a.viterbi(x), torch.int32)
    # Transducer: 99 tokens + optional blank, no model and the unigram model
    for ngram in (0, 1):
        t, _ = _transducer("optional", False, ngram, 99, 4)
        assert as_lists(t.viterbi(xd), torch.int32) == as_lists(t.viterbi(x), torch.int32)
