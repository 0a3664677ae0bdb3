"""The 64-bit key-value entry point at the drop-in boundary (include/misort.h)
on the CPU: the header declares it, libmisort.so exports it, it refuses a null
context before any device work, and the Python mirror carries its signature
and the two Context methods."""
import ctypes
import os
import re

import misort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misort.h")
FN = "misort_local_sort_pairs64"


def header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_and_library_exports_the_entry_point():
    assert FN in set(re.findall(r"\b(misort_\w+)\s*\(", header_text()))
    lib = ctypes.CDLL(misort.library_path())  # loads without a GPU
    assert hasattr(lib, FN)


def test_header_signature():
    m = re.search(r"\bint\s+" + FN + r"\s*\(([^)]*)\)\s*;", header_text())
    assert m
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["misort_ctx* ctx", "int key_dtype", "const void* d_keys_in", "const void* d_vals_in",
                      "int val_bytes", "void* d_keys_out", "void* d_vals_out", "int64_t n", "void* stream"]


def test_null_context_is_invalid():
    lib = misort.lib()
    buf = (ctypes.c_uint64 * 4)()  # never dereferenced: the context is checked first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (misort.U64, misort.F64):
        assert lib.misort_local_sort_pairs64(None, dt, p, p, 8, p, p, 4, None) == -1
        assert lib.misort_last_error()
        assert lib.misort_local_sort_pairs64(None, dt, p, None, 4, None, p, 4, None) == -1
        assert lib.misort_last_error()


def test_python_mirror_has_signature_and_methods():
    lib = misort.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert lib.misort_local_sort_pairs64.argtypes == [vp, i32, vp, vp, i32, vp, vp, i64, vp]
    assert lib.misort_local_sort_pairs64.restype is i32
    for m in ("sort_pairs64", "argsort64"):
        assert callable(getattr(misort.Context, m))
    assert len(misort.KIND_NAMES) == 12 and misort.KIND_NAMES[4] == "other"  # no new kind
