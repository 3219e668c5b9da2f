"""CPU tests (-m "not gpu") of the device decode's C ABI (csrc/decode_kernels.hip, include/wfl.h): the header declares
the entry points, libwfl.so exports them, the ctypes table resolves them, and wfl_graph_token_kind -- what picks `drop`
and the flags of Transducer.viterbi's decode -- tells make_token_graph's four graphs apart.  No device compute here."""
import ctypes
import os
import re

import numpy as np
import pytest

from gtn_applications_amd import _native as N
from gtn_applications_amd import graph as G
from gtn_applications_amd.criterions import transducer as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wfl_decode_workspace", "wfl_decode_emissions", "wfl_decode_paths", "wfl_decode_chunk_frames",
               "wfl_graph_token_kind")


def _header():
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        return f.read()


def test_header_declares_and_library_exports_the_decode_entry_points():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(wfl_[a-z0-9_]+)\s*\(", code))
    for name in NEW_SYMBOLS:
        assert name in declared, name
    consts = dict(re.findall(r"#define\s+(WFL_DECODE_[A-Z_]+)\s+(\d+)", code))
    assert consts == {"WFL_DECODE_NAN_IS_MAX": str(N.DECODE_NAN_IS_MAX),
                      "WFL_DECODE_BLANK_SEPARATED": str(N.DECODE_BLANK_SEPARATED)}
    assert N.DECODE_NAN_IS_MAX != N.DECODE_BLANK_SEPARATED and N.DECODE_NAN_IS_MAX & N.DECODE_BLANK_SEPARATED == 0
    # every entry cites the reference lines it replaces
    for cite in ("ctc.py:126-135", "asg.py:225-234", "transducer.py:216-232"):
        assert cite in text, cite
    fresh = ctypes.CDLL(N.LIB_PATH)  # (a handle of its own: what the library exports, not what the table declared)
    for name in NEW_SYMBOLS:
        assert hasattr(fresh, name), name


def test_ctypes_table_resolves_the_decode_entry_points():
    for name in NEW_SYMBOLS:
        assert name in N.EXPORTED_SYMBOLS, name
        fn = getattr(N.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, name
    K = N.lib.wfl_decode_chunk_frames()
    assert K >= 1
    from gtn_applications_amd import engine as E

    assert E.decode_chunk_frames() == K
    for fn in ("decode_emissions", "decode_paths"):
        assert hasattr(N.ops, fn), fn


@pytest.mark.parametrize("B,T,R", [(1, 1, 0), (3, 65, 0), (8, 129, 3), (128, 1000, 1)])
def test_workspace_reports_capacity_and_scratch(B, T, R):
    cap, ws = ctypes.c_int64(-1), ctypes.c_int64(-1)
    N.check(N.lib.wfl_decode_workspace(B, T, R, ctypes.byref(cap), ctypes.byref(ws)))
    assert cap.value == B * T * max(1, R)
    K = N.lib.wfl_decode_chunk_frames()
    chunks = B * ((T + K - 1) // K)
    assert ws.value >= chunks * K * 4  # (at least the kept values of every chunk)
    assert ws.value <= 64 * (chunks + B) + chunks * K * 4 + 64  # (and nothing of another order of magnitude)


@pytest.mark.parametrize("B,T,R", [(0, 5, 0), (2, 0, 0), (2, 5, -1), (-1, 5, 0)])
def test_workspace_rejects_bad_shapes(B, T, R):
    cap, ws = ctypes.c_int64(), ctypes.c_int64()
    assert N.lib.wfl_decode_workspace(B, T, R, ctypes.byref(cap), ctypes.byref(ws)) == N.ERR_INVALID


def _kind(graph):
    n = ctypes.c_int(-7)
    return N.lib.wfl_graph_token_kind(graph._h, ctypes.byref(n)), n.value


def test_token_kind_tells_the_four_token_graphs_apart():
    modes = {}
    for ntok in (1, 2, 5):
        toks = [(i,) for i in range(ntok)]
        for blank, repeats in (("none", True), ("optional", True), ("forced", True), ("optional", False)):
            if (blank, repeats) == ("optional", False) and ntok < 2:
                continue  # (without a second token the graph has no token -> token arc that tells it from the one with repeats)
            g = TR.make_token_graph(toks, blank=blank, allow_repeats=repeats)
            g.arc_sort()
            mode, n = _kind(g)
            assert mode >= 0 and n == ntok, (ntok, blank, repeats, mode, n)
            assert modes.setdefault((blank, repeats), mode) == mode  # (the same mode for every N)
    assert modes == {("none", True): N.TOKENS_NONE, ("optional", True): N.TOKENS_OPTIONAL, ("forced", True): N.TOKENS_FORCED,
                     ("optional", False): N.TOKENS_OPTIONAL_NO_REPEATS}
    assert len(set(modes.values())) == 4


@pytest.mark.parametrize("blank,repeats", [("none", True), ("optional", True), ("forced", True), ("optional", False)])
def test_token_kind_rejects_a_graph_with_one_weight_changed(blank, repeats):
    g = TR.make_token_graph([(i,) for i in range(4)], blank=blank, allow_repeats=repeats)
    g.arc_sort()
    assert _kind(g)[0] >= 0
    a = g.arrays()
    w = np.array(a["weight"], np.float32)
    w[len(w) // 2] = 0.5
    other = G.Graph(False)
    other.add_nodes(a["start"], a["accept"])
    other.add_arcs(a["src"], a["dst"], a["ilabel"], a["olabel"], w)
    assert _kind(other) == (-1, 0)
    assert N.lib.wfl_graph_token_kind(None, None) == -1


def test_token_decode_plan_follows_the_kind():
    """(drop, flags) Transducer.viterbi hands to the device decode; None where the host has to decode"""
    toks = [(i,) for i in range(4)]
    plan = lambda blank, repeats, C: TR._token_decode_plan(TR.make_token_graph(toks, blank=blank, allow_repeats=repeats), C)
    assert plan("none", True, 4) == (None, 0)
    assert plan("none", True, 5) is None  # (label 4 is outside the graph's alphabet: the graph algebra decides)
    assert plan("optional", True, 5) == (4, 0)
    assert plan("optional", False, 5) == (4, 0)
    assert plan("optional", True, 4) == (None, 0)  # (no column for the blank: nothing to drop)
    assert plan("optional", True, 6) is None
    assert plan("forced", True, 5) == (4, N.DECODE_BLANK_SEPARATED)
    assert plan("forced", True, 4) is None
    other = TR.make_token_graph(toks, blank="optional", allow_repeats=True)
    other.add_arc(0, 0, 1000, 1000, 0.0)
    assert TR._token_decode_plan(other, 5) is None
