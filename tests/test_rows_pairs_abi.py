"""The row-wise key-value sort at the drop-in boundary (include/misort.h) on the
CPU: the header declares misort_local_sort_rows_pairs with the documented
parameter list, libmisort.so exports it, a null context is refused before any
device work, the Python mirror carries the signature and both methods, no
profile kind was added, and misort_rows_plan(cols, 8) -- the plan of a pairs
row sort -- replayed on numpy over padded rows of RECORDS sorts every row by
(key, value)."""
import ctypes
import os
import re

import numpy as np
import pytest

import misort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misort.h")
FN = "misort_local_sort_rows_pairs"
U64 = np.uint64


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_and_library_exports_the_entry_point():
    declared = set(re.findall(r"\b(misort_\w+)\s*\(", header_text()))
    assert FN in declared
    assert hasattr(ctypes.CDLL(misort.library_path()), FN)  # loads without a GPU


def test_header_signature():
    m = re.search(r"\bint\s+" + FN + r"\s*\(([^)]*)\)\s*;", header_text())
    assert m
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "misort_ctx* ctx", "int key_dtype", "const void* d_keys_in", "const void* d_vals_in", "void* d_keys_out",
        "void* d_vals_out", "int64_t rows", "int64_t cols", "void* stream"]


def test_null_context_is_invalid():
    lib = misort.lib()
    buf = (ctypes.c_uint32 * 8)()  # never dereferenced: the context is checked first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (misort.U32, misort.F32):
        assert lib.misort_local_sort_rows_pairs(None, dt, p, p, p, p, 2, 2, None) == -1
        assert lib.misort_last_error()
        assert lib.misort_local_sort_rows_pairs(None, dt, p, None, None, p, 2, 2, None) == -1


def test_python_mirror_has_signature_and_methods():
    lib = misort.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert lib.misort_local_sort_rows_pairs.argtypes == [vp, i32, vp, vp, vp, vp, i64, i64, vp]
    assert lib.misort_local_sort_rows_pairs.restype is i32
    assert callable(misort.Context.sort_rows_pairs) and callable(misort.Context.argsort_rows)


def test_no_new_profile_kind():
    assert len(misort.KIND_NAMES) == 12


def up_of(kind, hi, r, tile_up):
    return tile_up if kind == "tile_sort" else (hi + r if kind == "run_mergek" else hi + 1)


def replay(x, plan, tile_up):
    """The passes on a numpy model, over the whole buffer: a pass sorts every
    aligned 2^up block (the SORT pass of a row tile stops at the padded row
    length, tile_up)."""
    for kind, hi, r, _ in plan:
        x = np.sort(x.reshape(-1, 1 << up_of(kind, hi, r, tile_up)), axis=1).reshape(-1)
    return x


@pytest.mark.parametrize("cols", [(1 << 13) - 1, 1 << 13, (1 << 13) + 1, 40000])
@pytest.mark.parametrize("argsort", [False, True], ids=["values", "argsort"])
def test_rows_plan_replay_sorts_every_row_of_records(cols, argsort):
    rows = 3
    rng = np.random.default_rng(cols + argsort)
    keys = rng.integers(0, 1 << 32, size=(rows, cols), dtype=np.uint64)
    keys[:, ::7] = keys[:, :1]  # duplicates: the value decides
    keys[1, ::5] = 0xFFFFFFFF
    if argsort:
        vals = np.broadcast_to(np.arange(cols, dtype=np.uint64), (rows, cols)).copy()
    else:
        vals = rng.integers(0, 1 << 32, size=(rows, cols), dtype=np.uint64)
        vals[1, ::10] = 0xFFFFFFFF  # with the key above: the padding record as a real record
    rec = keys << U64(32) | vals
    p = misort.rows_plan(cols, 8)
    assert (p["path"] == "tile") == (cols <= 1 << 13)
    b = p["block_log2"]
    x = np.full((rows, 1 << b), ~U64(0), dtype=np.uint64)
    x[:, :cols] = rec
    # tile path: the one SORT pass ends at level block_log2; blocks path: whole tiles
    up = b if p["path"] == "tile" else p["tile_log2"]
    got = replay(x.reshape(-1), p["passes"], up).reshape(rows, 1 << b)[:, :cols]
    gk, gv = got >> U64(32), got & U64(0xFFFFFFFF)
    order = np.lexsort((vals, keys), axis=1)  # by key, then by value
    np.testing.assert_array_equal(gk, np.take_along_axis(keys, order, axis=1))
    np.testing.assert_array_equal(gv, np.take_along_axis(vals, order, axis=1))
    if argsort:  # the stable argsort: equal keys in column order
        np.testing.assert_array_equal(gv, np.argsort(keys, axis=1, kind="stable").astype(np.uint64))
    # every pass stayed inside a block: the last one ends exactly at the block
    kind, hi, r, _ = p["passes"][-1]
    assert up_of(kind, hi, r, up) == b
