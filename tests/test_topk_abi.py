"""The row-wise top-k at the drop-in boundary (include/misort_topk.h) on the CPU:
the extension header declares misort_local_topk_rows and misort_topk_plan with
the documented parameter lists, libmisort.so exports them, a null context is
refused before any device work, the Python mirror carries the signatures and the
methods, no profile kind was added, include/misort.h holds no new stream
prototype, and misort_topk_plan has the documented shape and, replayed on numpy
over tied keys, equals the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

import misort
import stream_order as SO
import topk_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misort_topk.h")
SIGNATURES = {
    "misort_local_topk_rows": [
        "misort_ctx* ctx", "int key_dtype", "const void* d_keys_in", "void* d_keys_out", "void* d_idx_out",
        "int64_t rows", "int64_t cols", "int64_t k", "int largest", "void* stream"],
    "misort_topk_plan": ["int64_t cols", "int64_t k", "int* passes", "int max_passes"],
}
U32 = np.uint32


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def ceil_log2(n):
    return max(int(n) - 1, 0).bit_length()


def test_header_declares_and_library_exports_the_entry_points():
    declared = set(re.findall(r"\b(misort_\w+)\s*\(", header_text()))
    lib = ctypes.CDLL(misort.library_path())  # loads without a GPU
    for fn in SIGNATURES:
        assert fn in declared
        assert hasattr(lib, fn)
    assert re.search(r'#include\s+"misort\.h"', header_text())


@pytest.mark.parametrize("fn", sorted(SIGNATURES))
def test_header_signature(fn):
    m = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)\s*;", header_text())
    assert m
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == SIGNATURES[fn]


def test_null_context_is_invalid():
    lib = misort.lib()
    buf = (ctypes.c_uint32 * 8)()  # never dereferenced: the context is checked first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (misort.U32, misort.F32):
        for largest in (0, 1):
            assert lib.misort_local_topk_rows(None, dt, p, p, p, 2, 2, 1, largest, None) == -1
            assert lib.misort_last_error()
            assert lib.misort_local_topk_rows(None, dt, p, None, p, 2, 2, 1, largest, None) == -1


def test_python_mirror_has_signatures_and_methods():
    lib = misort.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert lib.misort_local_topk_rows.argtypes == [vp, i32, vp, vp, vp, i64, i64, i64, i32, vp]
    assert lib.misort_local_topk_rows.restype is i32
    assert lib.misort_topk_plan.argtypes == [i64, i64, ctypes.POINTER(i32), i32]
    assert lib.misort_topk_plan.restype is i32
    assert callable(misort.Context.topk_rows) and callable(misort.topk_plan)
    assert "topk_plan" in misort.__all__


def test_no_new_profile_kind():
    assert len(misort.KIND_NAMES) == 12


def test_misort_h_has_no_new_stream_prototype():
    protos = SO.stream_prototypes()
    assert "misort_local_topk_rows" not in protos
    # every one of them is still in the table or has its reason
    covered = {c.entry for c in SO.CASES} | set(SO.NOT_ASYNCHRONOUS)
    assert [p for p in protos if p not in covered] == []
    with open(HEADER) as f:
        assert SO.stream_prototypes(f.read()) == ["misort_local_topk_rows"]


COLS = [1, 32, 33, 8192, 8193, 65536, 65537, 1 << 20, 1 << 31]
KS = [1, 7, 1024]


def legal(cols, k):
    return 1 <= k <= cols <= 1 << 31 and (cols <= 1 << 13 or k <= 1 << 10)


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("k", KS)
def test_plan_properties(cols, k):
    if not legal(cols, k):
        with pytest.raises(misort.MisortError) as e:
            misort.topk_plan(cols, k)
        assert e.value.code == -1
        return
    plan = misort.topk_plan(cols, k)
    assert 1 <= len(plan) <= 7
    assert plan[0][0] == cols
    for i, (m_in, lr, npieces, m_out) in enumerate(plan):
        last = i == len(plan) - 1
        assert 5 <= lr <= 13 and lr >= ceil_log2(k)
        assert npieces == -(-m_in // (1 << lr))      # the blocks cover the row
        assert m_out == npieces * k
        assert (npieces == 1) == last                  # only the last pass has one block per row
        assert (m_in <= 1 << 13) == last
        if last:
            assert lr == max(ceil_log2(m_in), 5) and m_out == k
        else:
            assert lr == 13 and plan[i + 1][0] == m_out  # the passes chain
            assert m_out < m_in


def test_plan_pass_counts():
    assert len(misort.topk_plan(65537, 1024)) == 3
    assert len(misort.topk_plan(65536, 1024)) == 2
    assert len(misort.topk_plan(1 << 20, 1024)) == 4
    assert len(misort.topk_plan(1 << 17, 64)) == 2
    assert misort.topk_plan(1000, 8) == [(1000, 10, 1, 8)]
    assert misort.topk_plan(65537, 1024) == [(65537, 13, 9, 9216), (9216, 13, 2, 2048), (2048, 11, 1, 1024)]


@pytest.mark.parametrize("cols,k", [(0, 0), (0, 1), (5, 0), (5, 6), (-1, 1), (5, -1), (8193, 1025), (1 << 20, 2048),
                                    ((1 << 31) + 1, 1), (1 << 40, 1)])
def test_illegal_shapes_have_no_plan(cols, k):
    lib = misort.lib()
    buf = (ctypes.c_int32 * 64)()
    assert lib.misort_topk_plan(cols, k, buf, 16) < 0
    assert lib.misort_last_error()
    assert lib.misort_topk_plan(cols, k, None, 0) < 0
    assert list(buf) == [0] * 64


def test_plan_writes_no_more_than_asked():
    lib = misort.lib()
    buf = (ctypes.c_int32 * 12)(*([-7] * 12))
    assert lib.misort_topk_plan(65537, 1024, buf, 2) == 3
    assert list(buf) == [65537, 13, 9, 9216, 9216, 13, 2, 2048, -7, -7, -7, -7]
    assert lib.misort_topk_plan(65537, 1024, None, 1) == -1  # passes asked for, nowhere to write them


def tied_keys(cols, rows=3):
    """Four distinct values, so ties span the pieces, and a run of the best value
    in the last columns."""
    rng = np.random.default_rng(cols)
    keys = rng.integers(0, 4, size=(rows, cols), dtype=np.uint64).astype(U32) * U32(0x55555555)
    keys[1, -min(cols, 5):] = 0xFFFFFFFF
    keys[2, -min(cols, 5):] = 0
    return keys


@pytest.mark.parametrize("cols", [33, 8193, 65537])
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
def test_plan_replay_equals_the_oracle_on_ties(cols, largest):
    keys = tied_keys(cols)
    for k in (1, 7, min(cols, 1024)):
        plan = misort.topk_plan(cols, k)
        for f32 in (False, True):
            wk, wi = TO.topk_rows(keys, k, largest, f32)
            gk, gi = TO.replay_plan(keys, k, largest, f32, plan)
            np.testing.assert_array_equal(gi, wi)
            np.testing.assert_array_equal(gk, wk)
            # equal keys in ascending column order, whatever the direction
            same = wk[:, 1:] == wk[:, :-1]
            assert np.all(wi[:, 1:][same] > wi[:, :-1][same])
