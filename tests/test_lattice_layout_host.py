"""CPU test (-m "not gpu") of the alpha / beta tail layout, csrc/lattice_layout.h: builds csrc/lattice_layout_check.cpp with
the system C++ compiler, runs it and checks, for every descriptor of its grid (B x T x shared x max_states), that the
fields of each buffer ascend and do not overlap, that 8-byte fields are 8-byte aligned, that the fields end inside the
reserved size, and that this size and the place of the sweep formats are what the independent restatement of the sum
(tests/lattice_workspace.py) and the library's own queries say.  Integer equalities throughout.  The program's tests skip
without make or a C++ compiler; the last test needs the built library like every test that imports the package."""
import ctypes
import itertools
import os
import shutil
import subprocess
import types

import pytest

from lattice_workspace import tuned_workspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gtn_applications_amd", "csrc")
GRID = list(itertools.product((1, 2, 7, 8, 255, 256), (0, 1, 15, 16, 31, 32, 33, 320, 1000), (0, 1), (1, 64, 263)))
ALPHA_FIELDS = ["offs", "z", "fmt", "wref", "dump", "prog", "bad", "nx", "next", "list", "busy", "meta", "next_base", "based"]
BETA_FIELDS = ["offs", "z", "verdict", "dump", "prog", "bad"]


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """{(B, T, shared, max_states): namespace(desc, A=[(name, unit, lo, hi)], B=[...], end, total)} as the program prints it"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if not (shutil.which("make") and cxx):
        pytest.skip("needs make and a C++ compiler")
    exe = str(tmp_path_factory.mktemp("layout") / "lattice_layout_check")
    subprocess.run(["make", "-C", CSRC, "layout_check", "LAYOUT_CHECK=" + exe, "CXX=" + cxx], check=True, capture_output=True,
                   timeout=120)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    cases, cur = {}, None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "case":
            B, T, shared, max_states, total_states = map(int, w[1:])
            desc = types.SimpleNamespace(B=B, shared=shared, max_states=max_states, total_states=total_states, max_labels=0)
            cur = cases[(B, T, shared, max_states)] = types.SimpleNamespace(desc=desc, T=T, A=[], B=[])
        elif w[0] in ("A", "B"):
            getattr(cur, w[0]).append((w[1], int(w[2]), int(w[3]), int(w[4])))
        else:
            setattr(cur, w[0], int(w[1]))
    return cases


def test_the_program_prints_the_whole_grid_and_every_field(layouts):
    assert sorted(layouts) == sorted(GRID)
    for key, c in layouts.items():
        assert c.desc.total_states == (c.desc.max_states if c.desc.shared else c.desc.B * c.desc.max_states), key
        assert [f[0] for f in c.A] == ALPHA_FIELDS and [f[0] for f in c.B] == BETA_FIELDS, key


def test_fields_ascend_without_overlap_aligned_and_inside_the_reserved_size(layouts):
    for key, c in layouts.items():
        d = c.desc
        tail = 2 * (d.B * (c.T + 1) * d.max_states if d.shared else (c.T + 1) * d.total_states)  # the score arrays (floats)
        assert c.A[0][2] == c.B[0][2] == 4 * tail, key
        for fields in (c.A, c.B):
            for (name, unit, lo, hi), nxt in zip(fields, fields[1:] + [None]):
                assert lo < hi and (hi - lo) % unit == 0, (key, name)
                assert lo % unit == 0, (key, name)  # (8-byte fields 8-byte aligned from the buffer's start, 4-byte ones 4)
                if nxt is not None:
                    assert hi <= nxt[2], (key, name, nxt[0])
            assert fields[-1][3] <= 4 * c.end, (key, fields[-1][0])
        assert c.A[-1][3] == 4 * c.end, key  # `based` is the last field
        assert c.end <= c.total, key


def test_the_total_is_the_restated_sum(layouts):
    for key, c in layouts.items():
        assert c.total == tuned_workspace(c.desc, c.T)[1], key


def test_the_library_answers_with_the_layouts_total_and_formats_offset(layouts):
    """wfl_lattice_workspace and wfl_lattice_formats_offset, for descriptors of the tuned path (these fit LDS)"""
    from gtn_applications_amd import _native as N

    for key, c in layouts.items():
        d = N.LatticeDesc()
        d.B, d.shared, d.max_states, d.total_states = c.desc.B, c.desc.shared, c.desc.max_states, c.desc.total_states
        n_xg, n_ab, off = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        N.check(N.lib.wfl_lattice_workspace(ctypes.byref(d), c.T, ctypes.byref(n_xg), ctypes.byref(n_ab)))
        N.check(N.lib.wfl_lattice_formats_offset(ctypes.byref(d), c.T, ctypes.byref(off)))
        assert (n_xg.value, n_ab.value) == tuned_workspace(c.desc, c.T), key
        assert n_ab.value == c.total, key
        fmt = dict((f[0], f) for f in c.A)["fmt"]
        assert 4 * off.value == fmt[2], key
