"""The device decode (csrc/decode_kernels.hip) past the sizes tests/test_gpu_decode.py runs: utterances of more than 64
chunks of Kd = wfl_decode_chunk_frames() frames -- the scan launch walks the chunk summaries 64 at a time and carries the
last kept value, the running output count and the forced-blank verdict from one trip to the next -- and the emission
front end at the smallest and the largest class count of each of its six instantiations.  The expectations are
test_gpu_decode.py's: asg.collapse_and_unpack on the numpy array, torch.argmax + the row-by-row collapse,
G.transducer_decode_batch; everything is integer labels and compared with ==.  Each case asserts from this side that it
reaches its branch: the chunk count against 64, the class count against the bounds of its instantiation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_decode import (_buffers, _lists, _mods, abi_decode_emissions, abi_decode_paths, chunk, ctc_spelling,  # noqa: E402
                             host_paths)

TRIP = 64  # chunk summaries per trip of the scan


def chunks(T):
    return -(-T // chunk())


def long_frame_counts():
    Kd = chunk()
    return [TRIP * Kd, TRIP * Kd + 1, (TRIP + 1) * Kd + 1, 2 * TRIP * Kd + 1]


def abi_decode_lengths(x, lengths, drop, R=0, flags=0):
    """wfl_decode_emissions_lengths through the C ABI"""
    N, E, _ = _mods()
    B, T, C = x.shape
    cap, out, offs, scratch = _buffers(B, T, R)
    xlen = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    N.check(N.lib.wfl_decode_emissions_lengths(E.ptr(x), None, E.ptr(xlen), B, T, C, -1 if drop is None else drop, R, flags,
                                               E.ptr(scratch), E.ptr(out), cap, E.ptr(offs), E.stream_ptr()))
    return _lists(B, cap, out, offs)


# ------------------------------------------------------------------------------------------------------------------
# 1. the scan across 64 chunks: wfl_decode_paths == asg.collapse_and_unpack
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4))
def test_paths_decode_across_the_scan_trips(which):
    T = long_frame_counts()[which]
    assert chunks(T) == (TRIP, TRIP + 1, TRIP + 2, 2 * TRIP + 1)[which]  # the last chunk count of one trip, then two and three trips
    rs = np.random.RandomState(200 + which)
    for B in (1, 3):
        for R in (0, 1, 2, 3):
            for with_drop in (False, True):
                C = R + rs.randint(1, 6) + 1
                drop = C - 1 if with_drop else None
                stride = T + (0 if (B + R) % 2 else 5)
                paths = np.full((B, stride), C - 1, np.int32)
                paths[:, :T] = np.repeat(rs.randint(0, C, size=(B, (T + 2) // 3)).astype(np.int32), 3, axis=1)[:, :T]  # runs of three
                want = host_paths(paths[:, :T], drop, R)
                assert abi_decode_paths(paths, T, drop, R) == want, (B, T, R, drop)


def test_paths_decode_hand_made_rows_around_the_trips():
    Kd, R, g = chunk(), 2, 9  # labels >= 2, replabels 0 and 1, garbage 9
    T = 2 * TRIP * Kd + 7
    assert chunks(T) == 2 * TRIP + 1
    a, b = TRIP * Kd, 2 * TRIP * Kd  # the first frames of chunks 64 and 128
    rows = [
        [g] * (a - 1) + [5, 1],                                        # a label in chunk 63's last frame, a replabel in chunk 64's first
        [g] * (b - 1) + [6, 0],                                        # the same around chunks 127 / 128
        [g] * (10 * Kd + 3) + [7] + [g] * (60 * Kd + 1) + [1],         # a label in chunk 10, garbage through chunk 70, a replabel: expands
        [g] * (60 * Kd) + [7] + [g] * (b - 60 * Kd - 1) + [0],         # ... from chunk 60 through the whole second trip to chunk 128
        [g] * a + [1, 6],                                              # a replabel opens chunk 64, nothing kept before it: does not expand
        [g] * b + [0, 1, 4],                                           # ... chunk 128
        [4] * (a - 3) + [5] * 6 + [6] * (a - 6) + [7] * 5,             # runs that straddle both trip boundaries
        [3] * (a - 1) + [1] * 2 + [g] * (a - 1) + [1] * 2,             # a replabel run over the boundary behind a label; one behind garbage behind a replabel
        [g] * T,                                                       # every frame dropped
        [5] * a + [0] * a + [5, 1],                                    # a replabel run that fills the whole second trip
    ]
    assert len(rows[2]) == 70 * Kd + 6 and all(len(r) <= T for r in rows)
    paths = np.array([r + [g] * (T - len(r)) for r in rows], np.int32)
    for drop in (g, None):
        want = host_paths(paths, drop, R)
        assert abi_decode_paths(paths, T, drop, R) == want, drop
    got = abi_decode_paths(paths, T, g, R)
    assert got == [[3, 3, 3], [4, 4], [5, 5, 5], [5, 5], [4], [2], [2, 3, 4, 5], [1, 1, 1], [], [3, 3, 3, 3, 3]]
    assert abi_decode_paths(paths, T, g, 0) == host_paths(paths, g, 0)


def test_paths_decode_at_capacity_across_the_trips():
    """test_gpu_decode.py's construction at T = 64 Kd + 2, R = 1: every label is followed by the replabel, T / 2 labels
    emit T outputs -- the whole capacity, to the last element of `out`"""
    Kd, R, B = chunk(), 1, 3
    T = TRIP * Kd + 2
    assert chunks(T) == TRIP + 1
    rs = np.random.RandomState(R)
    labs = R + 1 + rs.randint(0, 4, size=(B, T // 2))
    labs[:, 1::2] += 4  # (neighbours differ: nothing collapses)
    paths = np.empty((B, T), np.int32)
    paths[:, 0::2], paths[:, 1::2] = labs, R - 1
    want = host_paths(paths, None, R)
    assert all(len(w) == T for w in want)  # B T max(1, R) in all: wfl_decode_workspace's out_capacity
    assert abi_decode_paths(paths, T, None, R) == want


# ------------------------------------------------------------------------------------------------------------------
# 2. WFL_DECODE_BLANK_SEPARATED over long rows == the blank="forced" token graph
# ------------------------------------------------------------------------------------------------------------------
def test_blank_separated_across_the_scan_trips():
    N, _, G = _mods()
    from gtn_applications_amd.criterions import transducer as TR

    Kd, ntok = chunk(), 5
    b = ntok
    T = TRIP * Kd + 1
    assert chunks(T) == TRIP + 1 and (T - 1) % 4 == 0
    tokens = TR.make_token_graph([(i,) for i in range(ntok)], blank="forced", allow_repeats=True)
    tokens.arc_sort()
    rs = np.random.RandomState(4)
    valid = [v for tok in rs.randint(0, ntok, size=(T - 1) // 4).tolist() for v in (b, tok, tok, b)] + [b]
    late, early = list(valid), list(valid)
    late[T - 1] = 2                      # chunk 64, the second trip's only chunk: the row does not end with the blank
    early[1], early[2] = 1, 2            # chunk 0: two different tokens adjacent
    assert (T - 1) // Kd == TRIP
    labels = np.array([valid, late, early], np.int32)
    out, off = G.transducer_decode_batch(tokens, labels.reshape(-1), np.arange(4, dtype=np.int64) * T)
    want = [out[off[i]:off[i + 1]].tolist() for i in range(3)]
    assert len(want[0]) == (T - 1) // 4 and want[1] == [] and want[2] == []
    assert abi_decode_paths(labels, T, b, 0, flags=N.DECODE_BLANK_SEPARATED) == want
    x = torch.nn.functional.one_hot(torch.from_numpy(labels).long(), ntok + 1).float().cuda()
    assert abi_decode_emissions(x, None, b, flags=N.DECODE_BLANK_SEPARATED) == want
    # without the flag the three rows decode as they are
    assert [len(r) for r in abi_decode_paths(labels, T, b, 0)] == [(T - 1) // 4, (T - 1) // 4 + 1, (T - 1) // 4 + 1]


# ------------------------------------------------------------------------------------------------------------------
# 3. the emission front end over long rows
# ------------------------------------------------------------------------------------------------------------------
def test_emissions_decode_across_the_scan_trips():
    N, _, _ = _mods()
    Kd, B, C = chunk(), 3, 3
    T = TRIP * Kd + 1
    assert chunks(T) > TRIP
    rs = np.random.RandomState(6)
    x = torch.from_numpy(rs.randint(-3, 4, size=(B, T, C)).astype(np.float32)).cuda()
    for blank in (0, 2, None):
        want = ctc_spelling(torch.argmax(x, dim=2).cpu(), -1 if blank is None else blank)
        assert abi_decode_emissions(x, None, blank, flags=N.DECODE_NAN_IS_MAX) == want
        assert abi_decode_emissions(x, None, blank) == want  # (no NaN, no row without a finite score: both rules agree)
    # replabels from emissions: the scan's carry decides behind the same front end
    frames = torch.argmax(x, dim=2).cpu().numpy().astype(np.int32)
    assert abi_decode_emissions(x, None, None, R=2) == host_paths(frames, None, 2)


def test_emissions_lengths_across_the_scan_trips():
    N, _, _ = _mods()
    Kd, C = chunk(), 3
    T = 2 * TRIP * Kd + 1
    lengths = [0, TRIP * Kd - 1, TRIP * Kd, TRIP * Kd + 1, T]
    assert chunks(T) == 2 * TRIP + 1 and [chunks(n) for n in lengths[1:4]] == [TRIP, TRIP, TRIP + 1]
    rs = np.random.RandomState(7)
    x = torch.from_numpy(rs.randint(-3, 4, size=(len(lengths), T, C)).astype(np.float32)).cuda()
    pred = torch.argmax(x, dim=2).cpu()
    for blank in (1, None):
        want = [ctc_spelling([pred[b, :n]], -1 if blank is None else blank)[0] if n else [] for b, n in enumerate(lengths)]
        assert abi_decode_lengths(x, lengths, blank, flags=N.DECODE_NAN_IS_MAX) == want
    want = [host_paths(pred[b:b + 1, :n].numpy().astype(np.int32), None, 1)[0] if n else [] for b, n in enumerate(lengths)]
    assert abi_decode_lengths(x, lengths, None, R=1) == want


# ------------------------------------------------------------------------------------------------------------------
# 4. every width of the emission front end: rows whose first maximum sits where an instantiation could lose it
# ------------------------------------------------------------------------------------------------------------------
# (smallest C, largest C, registers of 64 classes per lane; 0: the loop over any C) -- wfl_decode_emissions's choice
WIDTHS = [(1, 64, 1), (65, 128, 2), (129, 256, 4), (257, 512, 8), (513, 1024, 16), (1025, None, 0)]


def width_rows(C):
    """[(scores [C], the first maximal class under torch.argmax's rule, ... under the default rule)]"""
    nan = float("nan")
    full, part = C // 64, C % 64
    rows = []

    def row(ones, want, want_default=None, nans=()):
        v = np.zeros(C, np.float32)
        v[list(ones)] = 1.0
        v[list(nans)] = nan
        rows.append((v, want, want if want_default is None else want_default))

    row([C - 1], C - 1)                                        # the only maximum in the last class
    if full and part:
        row([64 * full - 1], 64 * full - 1)                    # ... in the last lane of the last full register
    if part:
        row([64 * full + part // 2], 64 * full + part // 2)    # ... in the last, partial register
    if C > 64:
        c = min(5, C - 65)
        row([c, c + 64], c)                                    # ties: the first wins
        last = 64 * ((C - 1) // 64)                            # (the first class of the last register)
        row([0, last], 0)
        row([last, C - 1], last)
        if C > 69:
            row([20, 69], 20)                                  # the later one in a lower lane
            row([69, C - 1], 69)
    row([1 % C], C - 1, 1 % C, nans=[C - 1])                   # a NaN in the last register: first under torch's rule, -inf under the default
    if C > 64:
        row([], C - 64, 0, nans=[C - 64, C - 1])               # two NaNs, nothing else: the first NaN; the default: all equal, class 0
    row([0], 0)
    return rows


@pytest.mark.parametrize("C", [1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2049])
def test_emission_rows_at_the_edges_of_every_width(C):
    N, _, _ = _mods()
    lo, hi, nv = next(w for w in WIDTHS if w[0] <= C and (w[1] is None or C <= w[1]))
    assert C in (lo, hi) or (hi is None and C > 1024)
    assert nv == 0 or 64 * nv >= C > (64 * nv // 2 if nv > 1 else 0)  # the narrowest instantiation that holds the row
    rows = width_rows(C)
    x = torch.from_numpy(np.stack([r[0] for r in rows])[None]).cuda()
    T = len(rows)
    assert torch.argmax(x, dim=2).cpu().tolist() == [[r[1] for r in rows]]  # (torch's rule is the one restated above)
    for flags, col in ((N.DECODE_NAN_IS_MAX, 1), (0, 2)):
        labels = torch.tensor([[r[col] for r in rows]])
        want = ctc_spelling(labels, -1)
        assert C == 1 or len(want[0]) >= T - 2  # (neighbouring rows differ: the collapse hides next to nothing)
        assert abi_decode_emissions(x, None, None, flags=flags) == want, (C, flags)
        # the lengths entry: the whole row, and a row cut before its last two frames
        x2 = x.repeat(2, 1, 1).contiguous()
        assert abi_decode_lengths(x2, [T, T - 2], None, flags=flags) == [want[0], ctc_spelling(labels[:, :T - 2], -1)[0]], (C, flags)
        # with a dropped class: the last one
        assert abi_decode_emissions(x, None, C - 1, flags=flags) == ctc_spelling(labels, C - 1), (C, flags)
