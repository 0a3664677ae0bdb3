"""The key-value entry points at the drop-in boundary (include/misort.h) on the
CPU: the header declares them, libmisort.so exports them, MISORT_F32 has its
value, both refuse a null context before any device work, and the Python
mirror carries their signatures and the three Context methods."""
import ctypes
import os
import re

import misort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misort.h")
PAIR_FUNCTIONS = ("misort_local_sort_pairs", "misort_parallel_sort_pairs")


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def declared_functions():
    return sorted(set(re.findall(r"\b(misort_\w+)\s*\(", header_text())))


def test_header_declares_and_library_exports_the_pair_sorts():
    names = declared_functions()
    lib = ctypes.CDLL(misort.library_path())  # loads without a GPU
    for fn in PAIR_FUNCTIONS:
        assert fn in names
        assert hasattr(lib, fn)


def test_f32_dtype_value():
    dtypes = dict(re.findall(r"\b(MISORT_[UF]\d\d)\s*=\s*(\d+)", header_text()))
    assert dtypes == {"MISORT_U32": "0", "MISORT_U64": "1", "MISORT_F64": "2", "MISORT_F32": "3"}
    assert misort.F32 == 3
    assert (misort.U32, misort.U64, misort.F64) == (0, 1, 2)


def test_null_context_is_invalid():
    lib = misort.lib()
    buf = (ctypes.c_uint32 * 4)()  # never dereferenced: the context is checked first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (misort.U32, misort.F32):
        assert lib.misort_local_sort_pairs(None, dt, p, p, p, p, 4, None) == -1
        assert lib.misort_parallel_sort_pairs(None, dt, p, p, p, p, 4, 0, None) == -1
    assert lib.misort_last_error()


def test_python_mirror_has_signatures_and_methods():
    lib = misort.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert lib.misort_local_sort_pairs.argtypes == [vp, i32, vp, vp, vp, vp, i64, vp]
    assert lib.misort_parallel_sort_pairs.argtypes == [vp, i32, vp, vp, vp, vp, i64, i64, vp]
    assert lib.misort_local_sort_pairs.restype is i32
    assert lib.misort_parallel_sort_pairs.restype is i32
    for m in ("sort_pairs", "argsort", "parallel_sort_pairs"):
        assert callable(getattr(misort.Context, m))
    assert len(misort.KIND_NAMES) == 12 and misort.KIND_NAMES[4] == "other"  # no new kind
