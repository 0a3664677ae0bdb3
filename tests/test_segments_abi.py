"""The segmented sort at the drop-in boundary (include/misort.h) on the CPU: the
header declares misort_local_sort_segments and misort_segment_class, libmisort.so
exports them with the documented parameter lists, a null context is refused
before any device work, the Python mirror carries both signatures, and
misort_segment_class (host only; the kernels include the same function) agrees
with misort_rows_plan on the path and the block of every length."""
import ctypes
import os
import re

import pytest

import misort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misort.h")
SORT, CLASS = "misort_local_sort_segments", "misort_segment_class"


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
    for fn in (SORT, CLASS):
        assert fn in declared
        assert hasattr(lib, fn)


def test_header_signatures():
    assert params_of(SORT) == ["misort_ctx* ctx", "int dtype", "const void* d_in", "void* d_out", "int64_t n",
                               "const int64_t* d_offsets", "int64_t nseg", "void* stream"]
    assert params_of(CLASS) == ["int64_t len", "int key_bytes"]


def test_null_context_is_invalid():
    lib = misort.lib()
    buf = (ctypes.c_uint64 * 8)()  # never dereferenced: the context is checked first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (misort.U32, misort.U64, misort.F64, misort.F32):
        assert lib.misort_local_sort_segments(None, dt, p, p, 4, p, 1, None) == -1
        assert lib.misort_last_error()


def test_python_mirror_has_signatures_and_methods():
    lib = misort.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert lib.misort_local_sort_segments.argtypes == [vp, i32, vp, vp, i64, vp, i64, vp]
    assert lib.misort_local_sort_segments.restype is i32
    assert lib.misort_segment_class.argtypes == [i64, i32]
    assert lib.misort_segment_class.restype is i32
    assert callable(misort.Context.sort_segments) and callable(misort.segment_class)
    assert "segment_class" in misort.__all__
    assert len(misort.KIND_NAMES) == 12  # no new kind


def test_segment_class_rejects_bad_arguments():
    f = misort.lib().misort_segment_class
    assert f(100, 2) == -1 and f(-1, 4) == -1
    with pytest.raises(ValueError):
        misort.segment_class(-1, 4)
    with pytest.raises(ValueError):
        misort.segment_class(10, 2)


LENGTHS = sorted({0, 1, 2, 31, 32, 33} | {(1 << j) + d for j in range(5, 21) for d in (-1, 0, 1)})


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_segment_class_agrees_with_rows_plan(key_bytes):
    t = misort.tile_log2(key_bytes)
    assert misort.segment_class(0, key_bytes) == -1
    for n in LENGTHS[1:]:
        c = misort.segment_class(n, key_bytes)
        p = misort.rows_plan(n, key_bytes)
        assert (p["path"] == "tile") == (c <= t) == (n <= 1 << t), (n, c, p)
        assert c == max(p["block_log2"], 5), (n, c, p)
        assert (1 << c) >= n and (c == 5 or (1 << (c - 1)) < n), (n, c)
