"""The row-wise sort at the drop-in boundary (include/misort.h) on the CPU: the
header declares misort_local_sort_rows and misort_rows_plan, libmisort.so
exports them, a null context is refused before any device work, the Python
mirror carries both signatures, and misort_rows_plan (host only) describes a
plan that, replayed on numpy, sorts every row on its own."""
import ctypes
import os
import re

import numpy as np
import pytest

import misort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misort.h")
SORT, PLAN = "misort_local_sort_rows", "misort_rows_plan"


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def params_of(fn):
    m = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)\s*;", header_text())
    assert m, fn
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_entry_points():
    declared = set(re.findall(r"\b(misort_\w+)\s*\(", header_text()))
    lib = ctypes.CDLL(misort.library_path())  # loads without a GPU
    for fn in (SORT, PLAN):
        assert fn in declared
        assert hasattr(lib, fn)


def test_header_signatures():
    assert params_of(SORT) == ["misort_ctx* ctx", "int dtype", "const void* d_in", "void* d_out", "int64_t rows",
                               "int64_t cols", "void* stream"]
    assert params_of(PLAN) == ["int64_t cols", "int key_bytes", "int* path", "int* tile_log2", "int* block_log2",
                               "int* passes", "int max_passes"]


def test_null_context_is_invalid():
    lib = misort.lib()
    buf = (ctypes.c_uint64 * 4)()  # never dereferenced: the context is checked first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (misort.U32, misort.U64, misort.F64):
        assert lib.misort_local_sort_rows(None, dt, p, p, 2, 2, None) == -1
        assert lib.misort_last_error()


def test_python_mirror_has_signatures_and_methods():
    lib = misort.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    pi = ctypes.POINTER(i32)
    assert lib.misort_local_sort_rows.argtypes == [vp, i32, vp, vp, i64, i64, vp]
    assert lib.misort_local_sort_rows.restype is i32
    assert lib.misort_rows_plan.argtypes == [i64, i32, pi, pi, pi, pi, i32]
    assert lib.misort_rows_plan.restype is i32
    assert callable(misort.Context.sort_rows) and callable(misort.rows_plan)
    assert "rows_plan" in misort.__all__
    assert len(misort.KIND_NAMES) == 12 and misort.KIND_NAMES[4] == "other"  # no new kind


def test_rows_plan_rejects_bad_arguments():
    f = misort.lib().misort_rows_plan
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert f(100, 2, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None, 0) == -1
    assert f(-1, 4, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None, 0) == -1
    assert f(100, 4, None, ctypes.byref(b), ctypes.byref(c), None, 0) == -1
    assert f(100, 4, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None, 3) == -1


def ceil_log2(n):
    return max(0, int(n - 1).bit_length())


def cols_of(key_bytes):
    t = 1 << misort.tile_log2(key_bytes)
    return [1, 2, 31, 32, 33, 1000, t - 1, t, t + 1, 40000, 1 << 17, (1 << 17) + 1, 300001, (1 << 24) + 1]


CASES = [(kb, cols) for kb in (4, 8) for cols in cols_of(kb)]


@pytest.mark.parametrize("key_bytes,cols", CASES)
def test_rows_plan_shape(key_bytes, cols):
    t = 1 << misort.tile_log2(key_bytes)
    p = misort.rows_plan(cols, key_bytes)
    assert set(p) == {"path", "tile_log2", "block_log2", "passes"}
    assert (p["path"] == "tile") == (cols <= t)
    assert p["path"] in ("tile", "blocks")
    if p["path"] == "tile":
        assert len(p["passes"]) == 1 and p["passes"][0][0] == "tile_sort"
        assert (1 << p["block_log2"]) >= cols
        assert p["block_log2"] <= p["tile_log2"] <= misort.tile_log2(key_bytes)
        assert p["passes"][0][1] == p["tile_log2"] - 1
    else:
        assert p["block_log2"] == ceil_log2(cols)
        assert p["passes"] == misort.plan(1 << p["block_log2"], key_bytes)
        assert p["tile_log2"] == p["passes"][0][1] + 1


def replay(x, plan, tile_up):
    """The passes on a numpy model, over the whole buffer: a pass sorts every
    aligned 2^up block (the model of tests/test_plan.py::replay; the SORT pass
    of a row tile stops at the padded row length, tile_up)."""
    for kind, hi, r, _ in plan:
        up = tile_up if kind == "tile_sort" else (hi + r if kind == "run_mergek" else hi + 1)
        x = np.sort(x.reshape(-1, 1 << up), axis=1).reshape(-1)
    return x


@pytest.mark.parametrize("key_bytes,cols", [c for c in CASES if c[1] <= 1 << 20])
def test_rows_plan_replay_sorts_every_row(key_bytes, cols):
    dt = np.uint32 if key_bytes == 4 else np.uint64
    rows = 3
    rng = np.random.default_rng(cols + key_bytes)
    keys = rng.integers(0, np.iinfo(dt).max, size=(rows, cols), dtype=dt, endpoint=True)
    keys[:, ::7] = keys[:, :1]  # duplicates
    keys[1, ::5] = np.iinfo(dt).max  # the padding pattern as a real key
    p = misort.rows_plan(cols, key_bytes)
    b = p["block_log2"]
    x = np.full((rows, 1 << b), np.iinfo(dt).max, dtype=dt)
    x[:, :cols] = keys
    # tile path: the one SORT pass ends at level block_log2; blocks path: whole tiles
    up = b if p["path"] == "tile" else p["tile_log2"]
    got = replay(x.reshape(-1), p["passes"], up).reshape(rows, 1 << b)[:, :cols]
    np.testing.assert_array_equal(got, np.sort(keys, axis=1))
    # every pass stayed inside a block: the last one ends exactly at the block
    kind, hi, r, _ = p["passes"][-1]
    assert (up if kind == "tile_sort" else hi + r if kind == "run_mergek" else hi + 1) == b
