"""The segmented key-value sort at the drop-in boundary
(include/misort_segments_pairs.h) on the CPU: the extension header declares
misort_local_sort_segments_pairs with the documented parameter list and says
that the call waits, libmisort.so exports it, a null context is refused before
any device work, the Python mirror carries the signature and the methods, no
profile kind was added, include/misort.h holds no new stream prototype, and the
oracle of tests/segments_pairs_oracle.py equals a plain per-segment loop on a
small ragged case with ties."""
import ctypes
import os
import re

import numpy as np
import pytest

import misort
import segments_pairs_oracle as SPO
import stream_order as SO
from segment_layouts import offsets_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misort_segments_pairs.h")
FN = "misort_local_sort_segments_pairs"
SIGNATURE = ["misort_ctx* ctx", "int key_dtype", "const void* d_keys_in", "const void* d_vals_in",
             "void* d_keys_out", "void* d_vals_out", "int64_t n", "const int64_t* d_offsets", "int64_t nseg",
             "void* stream"]
U32 = np.uint32


def header_raw():
    with open(HEADER) as f:
        return f.read()


def header_code():
    return re.sub(r"/\*.*?\*/", "", header_raw(), flags=re.S)


def test_header_declares_and_library_exports_the_entry_point():
    declared = set(re.findall(r"\b(misort_\w+)\s*\(", header_code()))
    assert declared == {FN}
    lib = ctypes.CDLL(misort.library_path())  # loads without a GPU
    assert hasattr(lib, FN)
    assert re.search(r'#include\s+"misort\.h"', header_code())


def test_header_signature():
    m = re.search(r"\bint\s+" + FN + r"\s*\(([^)]*)\)\s*;", header_code())
    assert m
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == SIGNATURE


def test_header_says_that_the_call_waits():
    text = SO.squeeze(header_raw())
    assert re.search(SO.SAYS_IT_WAITS, text)
    assert "ONE HOST WAIT PER CALL" in text and "CANNOT BE CAPTURED IN A GRAPH" in text


def test_null_context_is_invalid():
    lib = misort.lib()
    buf = (ctypes.c_uint64 * 8)()  # never dereferenced: the context is checked first
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = getattr(lib, FN)
    for dt in (misort.U32, misort.F32):
        assert f(None, dt, p, p, p, p, 2, p, 1, None) == -1
        assert lib.misort_last_error()
        assert f(None, dt, p, None, None, p, 2, p, 1, None) == -1


def test_python_mirror_has_signature_and_methods():
    lib = misort.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    f = getattr(lib, FN)
    assert f.argtypes == [vp, i32, vp, vp, vp, vp, i64, vp, i64, vp]
    assert f.restype is i32
    assert callable(misort.Context.sort_segments_pairs) and callable(misort.Context.argsort_segments)
    for method in (misort.Context.sort_segments_pairs, misort.Context.argsort_segments):
        assert "waits once on its stream" in " ".join(method.__doc__.split())


def test_no_new_profile_kind():
    assert len(misort.KIND_NAMES) == 12


def test_misort_h_has_no_new_stream_prototype():
    protos = SO.stream_prototypes()
    assert FN not in protos
    # every one of them is still in the table or has its reason
    covered = {c.entry for c in SO.CASES} | set(SO.NOT_ASYNCHRONOUS)
    assert [p for p in protos if p not in covered] == []
    assert SO.stream_prototypes(header_raw()) == [FN]


# ---- the oracle bites -------------------------------------------------------------------------------

def ragged_case():
    lens = [0, 5, 1, 0, 9, 33, 2, 0]
    offs = offsets_of(lens, first=3)
    n = int(offs[-1]) + 4
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 4, n).astype(U32)  # four distinct keys: the value decides
    keys[rng.random(n) < 0.2] = U32(0xFFFFFFFF)
    vals = rng.integers(0, 3, n).astype(U32)  # tied values too
    vals[rng.random(n) < 0.2] = U32(0xFFFFFFFF)
    return keys, vals, offs


@pytest.mark.parametrize("argsort", [False, True], ids=["pairs", "argsort"])
@pytest.mark.parametrize("f32", [False, True], ids=["u32", "f32"])
def test_oracle_equals_a_plain_loop(f32, argsort):
    keys, vals, offs = ragged_case()
    if f32:
        keys = keys.copy()
        keys[::5] = U32(0x80000000)  # -0.0
        keys[1::7] = U32(0xFFC00000)  # a negative NaN: the smallest
        keys[2::7] = U32(0x7FFFFFFF)  # maps to all-ones
    v = None if argsort else vals
    a, b = int(offs[0]), int(offs[-1])
    fringe = np.full(keys.size, 0xABCD, dtype=U32)
    wk, wv = SPO.want(keys, offs, v, f32, fringe_vals=fringe)
    lk, lv = SPO.loop_want(keys, offs, v, f32)
    assert wk[a:b].tolist() == lk and wv[a:b].tolist() == lv
    # the fringes: the keys are the input's, the values the input's or what was there
    for x, src in ((wk, keys), (wv, fringe if argsort else vals)):
        assert x[:a].tolist() == src[:a].tolist() and x[b:].tolist() == src[b:].tolist()
    # the ties are there, and the order differs from the input's: the comparison says something
    assert wk[a:b].tolist() != keys[a:b].tolist()
    if argsort:
        # the indices gather each sorted segment, and are a permutation of its positions
        for i in range(len(offs) - 1):
            s, e = int(offs[i]), int(offs[i + 1])
            assert keys[s + wv[s:e].astype(np.int64)].tolist() == wk[s:e].tolist()
            assert sorted(wv[s:e].tolist()) == list(range(e - s))


def test_oracle_is_not_a_whole_array_sort():
    keys, vals, offs = ragged_case()
    a, b = int(offs[0]), int(offs[-1])
    wk, _ = SPO.want(keys, offs, vals)
    assert wk[a:b].tolist() != np.sort(keys[a:b]).tolist()
