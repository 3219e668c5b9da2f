"""CPU tests (-m "not gpu") of the error counts' C ABI (csrc/error_kernels.hip, include/wfl.h) and of
metrics.ErrorCounter's host side: the header declares the entry points, libwfl.so exports them, the ctypes table
resolves them, wfl_errors_chunk_steps gives the distance launch's steps per LDS fill, wfl_errors_workspace bounds the scratch from capacities and longest expansions alone, the counter builds
the tables tokens_to_text / to_text spell (train.py:80), and the caller errors are ValueErrors before any launch.  No
device compute here."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from gtn_applications_amd import ErrorCounter
from gtn_applications_amd import _native as N
from gtn_applications_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wfl_errors_workspace", "wfl_errors_count", "wfl_errors_chunk_steps")


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "wfl.h")) as f:
        text = f.read()
    # each declaration, with the comment right in front of it: the comment cites the lines it replaces
    for name in NEW_SYMBOLS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + name + r"\s*\(", text, flags=re.S)
        assert m, name
        assert "train.py:74-87" in m.group(1) and "test.py:94-109" in m.group(1), name
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+wfl_errors_workspace\s*\(\s*int B,\s*int64_t hyp_capacity,\s*int64_t ref_labels,\s*int "
                     r"hyp_max_expansion,\s*int ref_max_expansion,\s*int64_t\*\s*ws_bytes\)", code)
    fresh = ctypes.CDLL(N.LIB_PATH)  # (a handle of its own: what the library exports, not what the table declared)
    for name in NEW_SYMBOLS:
        assert hasattr(fresh, name), name


def test_ctypes_table_and_operators_resolve():
    for name in NEW_SYMBOLS:
        assert name in N.EXPORTED_SYMBOLS, name
        fn = getattr(N.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, name
    assert len(N.lib.wfl_errors_count.argtypes) == 17 and len(N.lib.wfl_errors_workspace.argtypes) == 6
    # the distance launch's steps per LDS fill: host code, no device needed; a multiple of the wave the edge tests build on
    from gtn_applications_amd import engine as E

    K = N.lib.wfl_errors_chunk_steps()
    assert len(N.lib.wfl_errors_chunk_steps.argtypes) == 0 and E.errors_chunk_steps() == K and K >= 128 and K % 64 == 0
    for fn in ("errors_count", "decode_emissions_errors", "decode_paths_errors"):
        assert hasattr(N.ops, fn), fn
    from gtn_applications_amd.criterions import asg, ctc, transducer

    for cls in (ctc.CTC, asg.ASG, transducer.Transducer):
        assert callable(getattr(cls, "errors"))


def ws_bytes(B, hyp_cap, ref_n, hm, rm):
    n = ctypes.c_int64(-1)
    rc = N.lib.wfl_errors_workspace(B, hyp_cap, ref_n, hm, rm, ctypes.byref(n))
    return rc, n.value


def test_workspace_grows_with_every_argument_and_rejects_bad_shapes():
    base = (8, 1000, 300, 2, 3)
    rc, w0 = ws_bytes(*base)
    assert rc == N.WFL_OK and w0 > 0 and w0 % 16 == 0
    for i in range(5):
        prev = w0
        for step in (1, 7, 100):
            args = list(base)
            args[i] += step
            rc, w = ws_bytes(*args)
            assert rc == N.WFL_OK and w >= prev, (i, step)
            prev = w
        assert prev > w0, i  # (strictly, over a step that is more than the 16-byte rounding)
    # the smallest shapes are served: nothing to count, tables of empty expansions
    assert ws_bytes(1, 0, 0, 1, 1)[0] == N.WFL_OK and ws_bytes(1, 0, 0, 0, 0)[0] == N.WFL_OK
    # the benchmark shape, with and without the word-piece table: a few MB
    assert ws_bytes(128, 128000, 5632, 1, 1)[1] < 4 << 20
    for bad in ((0, 10, 10, 1, 1), (-1, 10, 10, 1, 1), (2, -1, 10, 1, 1), (2, 10, -1, 1, 1), (2, 10, 10, -1, 1), (2, 10, 10, 1, -1)):
        assert ws_bytes(*bad)[0] == N.ERR_INVALID, bad
    assert N.lib.wfl_errors_workspace(2, 10, 10, 1, 1, None) == N.ERR_INVALID
    assert "errors_workspace" in N.last_error()


def test_count_rejects_bad_arguments_before_any_launch():
    """(every rejected call returns before it touches a pointer: the addresses here are never dereferenced)"""
    p = 4096

    def call(B=2, hyp=p, hoff=p, ref=p, roff=p, hp=None, hs=None, hV=0, rp=None, rs=None, rV=0, hcap=4, rn=4, ws=p, counts=p):
        return N.lib.wfl_errors_count(hyp, hoff, ref, roff, B, hp, hs, hV, rp, rs, rV, -1, hcap, rn, ws, counts, None)

    for kw in (dict(B=0), dict(hyp=None), dict(hoff=None), dict(ref=None), dict(roff=None), dict(ws=None), dict(counts=None),
               dict(hcap=-1), dict(rn=-1), dict(hp=p, hV=3), dict(hs=p, hV=3), dict(rp=p, rV=3), dict(rs=p, rV=3),
               dict(hp=p, hs=p, hV=0), dict(rp=p, rs=p, rV=0)):
        assert call(**kw) == N.ERR_INVALID, kw
        assert "errors_count" in N.last_error()


# ------------------------------------------------------------------------------------------------------------------
# ErrorCounter: the tables
# ------------------------------------------------------------------------------------------------------------------
def spelled(table, ids, label):
    """the symbols label `label` stands for, as the objects the counter numbered"""
    ptr, sym, _ = table
    back = {v: k for k, v in ids.items()}
    return [back[s] for s in sym[ptr[label]:ptr[label + 1]]]


def test_tables_against_hand_written_ones():
    c = ErrorCounter(["ab", "", "b_c", "_"], ["a", "b", "c", "_"], "_")
    assert c.symbol_ids == {"a": 0, "b": 1, "_": 2, "c": 3}  # numbered once, in the order they are met
    assert c.sep == 2
    ptr, sym, longest = c.hyp_table
    assert ptr.dtype == np.int32 and sym.dtype == np.int32
    assert ptr.tolist() == [0, 2, 2, 5, 6] and sym.tolist() == [0, 1, 1, 2, 3, 2] and longest == 3
    ptr, sym, longest = c.ref_table
    assert ptr.tolist() == [0, 1, 2, 3, 4] and sym.tolist() == [0, 1, 3, 2] and longest == 1
    assert (c.hyp_size, c.ref_size) == (4, 4)
    # a separator no table spells still gets a number of its own; None: no separator
    assert ErrorCounter(["a"], ["a"], "|").sep == 1 and ErrorCounter(["a"], ["a"]).sep == -1
    # symbols are any hashables
    c = ErrorCounter([(1, 2), ("x",)], [((1, 2),), ()], "x")
    assert c.hyp_table[1].tolist() == [0, 1, 2] and c.ref_table[1].tolist() == [3] and c.sep == 2
    assert c.ref_table[0].tolist() == [0, 1, 1] and c.ref_table[2] == 1  # (an empty expansion)


def test_identity_sides_take_labels_as_symbols():
    c = ErrorCounter()
    assert c.hyp_table is None and c.ref_table is None and c.sep == -1 and c.hyp_size is None
    assert ErrorCounter(wordsep=7).sep == 7
    # a table on one side only: its symbols and the separator are the other side's labels
    c = ErrorCounter(hyp_symbols=[[3, 0], [3, 1, 2], []], wordsep=3)
    assert c.ref_table is None and c.sep == 3
    assert c.hyp_table[0].tolist() == [0, 2, 5, 5] and c.hyp_table[1].tolist() == [3, 0, 3, 1, 2] and c.hyp_table[2] == 3
    for bad in (dict(hyp_symbols=["ab"], wordsep=0), dict(ref_symbols=[[0]], wordsep="_"), dict(hyp_symbols=[[-1]]),
                dict(wordsep="_"), dict(hyp_symbols=[]), dict(hyp_symbols=[], ref_symbols=["a"])):
        with pytest.raises(ValueError):
            ErrorCounter(**bad)


def test_for_preprocessor_with_and_without_a_lexicon():
    tokens = ["_th", "e", "_", "_a", ""]  # multi-character tokens that contain the separator; an empty token string
    graphemes = ["_", "a", "e", "h", "t"]
    pre = types.SimpleNamespace(tokens=tokens, graphemes=graphemes, lexicon=None, wordsep="_")
    c = ErrorCounter.for_preprocessor(pre)
    for v, t in enumerate(tokens):
        assert "".join(spelled(c.hyp_table, c.symbol_ids, v)) == t
    for v, g in enumerate(graphemes):
        assert "".join(spelled(c.ref_table, c.symbol_ids, v)) == g
    assert c.hyp_table[2] == 3 and c.ref_table[2] == 1 and c.sep == c.symbol_ids["_"]
    assert (c.hyp_size, c.ref_size) == (5, 5)
    # under a lexicon the targets are token indices too (to_text, datasets/*.py)
    pre.lexicon = {"the": ["_th", "e"]}
    c = ErrorCounter.for_preprocessor(pre)
    for v, t in enumerate(tokens):
        assert "".join(spelled(c.ref_table, c.symbol_ids, v)) == t
    assert np.array_equal(c.ref_table[0], c.hyp_table[0]) and np.array_equal(c.ref_table[1], c.hyp_table[1])


# ------------------------------------------------------------------------------------------------------------------
# ErrorCounter: caller errors are ValueErrors, raised where the labels are staged -- before anything is launched (and
# before a missing GPU is reported)
# ------------------------------------------------------------------------------------------------------------------
def test_value_errors():
    c = ErrorCounter(["a", "b", "_"], ["a", "_"], "_")
    with pytest.raises(ValueError, match="2 predictions for 1 targets"):
        c.counts([[0], [1]], [[0]])
    with pytest.raises(ValueError, match="target label 2 is outside the reference table"):
        c.counts([[0], [1]], [[0], [1, 2]])
    with pytest.raises(ValueError, match="target label -1 is outside the reference table"):
        c.counts([[0]], [torch.tensor([-1])])
    with pytest.raises(ValueError, match="predicted label 3 is outside the hypothesis table"):
        c.counts([torch.tensor([0, 3]), [1]], [[0], [1]])
    with pytest.raises(ValueError, match="predicted label -2 is outside the hypothesis table"):
        c([[-2]], [[0]])
    # the criteria: the hypothesis table must cover what the decode can emit
    from gtn_applications_amd.criterions import asg, ctc

    x = torch.zeros(1, 3, 5)
    with pytest.raises(ValueError, match="CTC.errors"):
        ctc.CTC(blank=4, use_pt=False).errors(x, [[0]], c)  # labels 0..3 against three entries
    with pytest.raises(ValueError, match="CTC.errors"):
        ctc.CTC(blank=0, use_pt=False).errors(torch.zeros(1, 3, 4), [[0]], c)  # labels 1..3
    with pytest.raises(ValueError, match="ASG.errors"):
        asg.ASG(4, num_replabels=1, use_garbage=False).errors(x, [[0]], c)
    with pytest.raises(ValueError, match="utterances for 2 targets"):
        M.decode_emissions_errors(c, [[0], [1]], x, 4)
    # an identity table covers every label: nothing to raise for
    ErrorCounter().check_hypothesis_labels(10 ** 6, "any")
