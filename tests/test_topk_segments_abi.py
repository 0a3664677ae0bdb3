"""The segmented top-k at the drop-in boundary (include/misort_topk_segments.h) on
the CPU: the extension header declares misort_local_topk_segments and
misort_topk_segments_plan with the documented parameter lists, libmisort.so
exports them, a null context is refused before any device work, the Python
mirror carries the signatures and the methods, no profile kind was added,
include/misort.h holds no new stream prototype, misort_topk_segments_plan has
the documented shape and refusals, the numpy oracle equals a plain per-segment
loop on tied keys, and the tied family of the GPU file ties at the cut."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import misort
import stream_order as SO
import topk_segments_cases as C
import topk_segments_oracle as TSO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "misort_topk_segments.h")
SIGNATURES = {
    "misort_local_topk_segments": [
        "misort_ctx* ctx", "int key_dtype", "const void* d_keys_in", "void* d_keys_out", "void* d_idx_out",
        "int64_t n", "const int64_t* d_offsets", "int64_t nseg", "int64_t k", "int largest", "void* stream"],
    "misort_topk_segments_plan": ["int64_t len", "int64_t k", "int* passes", "int max_passes"],
}
U32 = np.uint32


@pytest.fixture(autouse=True, scope="module")
def feature():
    """Every test here is about the feature: without its header or its symbols all of them fail."""
    assert os.path.exists(HEADER)
    lib = ctypes.CDLL(misort.library_path())
    assert all(hasattr(lib, fn) for fn in SIGNATURES)


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


def test_header_states_the_fill_table_and_the_wait():
    with open(HEADER) as f:
        text = " ".join(f.read().split())
    for needle in ("0xFFFFFFFF", "0x7FFFFFFF", "ONE HOST WAIT", "Why a header of its own"):
        assert needle in text
    assert re.search(SO.SAYS_IT_WAITS, text)


def test_null_context_is_invalid():
    lib = misort.lib()
    buf = (ctypes.c_uint64 * 8)()  # never dereferenced: the context is checked first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (misort.U32, misort.F32):
        for largest in (0, 1):
            assert lib.misort_local_topk_segments(None, dt, p, p, p, 4, p, 2, 1, largest, None) == -1
            assert lib.misort_last_error()
            assert lib.misort_local_topk_segments(None, dt, p, None, p, 4, p, 2, 1, largest, None) == -1


def test_python_mirror_has_signatures_and_methods():
    lib = misort.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert lib.misort_local_topk_segments.argtypes == [vp, i32, vp, vp, vp, i64, vp, i64, i64, i32, vp]
    assert lib.misort_local_topk_segments.restype is i32
    assert lib.misort_topk_segments_plan.argtypes == [i64, i64, ctypes.POINTER(i32), i32]
    assert lib.misort_topk_segments_plan.restype is i32
    assert "topk_segments_plan" in misort.__all__ and callable(misort.topk_segments_plan)
    sig = inspect.signature(misort.Context.topk_segments)
    assert list(sig.parameters) == ["self", "keys", "offsets", "k", "largest", "out_values", "out_indices", "stream"]
    assert sig.parameters["largest"].default is True
    assert callable(misort.Context.topk_segments_indices)
    for doc in (misort.Context.topk_segments.__doc__, misort.Context.topk_segments_indices.__doc__):
        assert "0xFFFFFFFF" in doc and "waits once" in doc


def test_no_new_profile_kind():
    assert len(misort.KIND_NAMES) == 12


def test_misort_h_has_no_new_stream_prototype():
    protos = SO.stream_prototypes()
    assert "misort_local_topk_segments" not in protos
    # every one of them is still in the table or has its reason
    covered = {c.entry for c in SO.CASES} | set(SO.NOT_ASYNCHRONOUS)
    assert [p for p in protos if p not in covered] == []
    with open(HEADER) as f:
        assert SO.stream_prototypes(f.read()) == ["misort_local_topk_segments"]


# ---- misort_topk_segments_plan ---------------------------------------------------------------------------

LENS = [0, 1, 32, 33, 8192, 8193, 1 << 14, (1 << 14) + 1, 1 << 17, 1 << 31, (1 << 31) + 1]
KS = [1, 64, 1024, 1025]


def legal(ln, k):
    return 1 <= k <= 1 << 13 and 0 <= ln <= 1 << 31 and (ln <= 1 << 13 or k <= 1 << 10)


@pytest.mark.parametrize("ln", LENS)
@pytest.mark.parametrize("k", KS)
def test_plan(ln, k):
    if not legal(ln, k):
        assert ln == (1 << 31) + 1 or (k == 1025 and ln > 1 << 13)
        with pytest.raises(misort.MisortError) as e:
            misort.topk_segments_plan(ln, k)
        assert e.value.code == -1
        return
    plan = misort.topk_segments_plan(ln, k)
    if ln == 0:
        assert plan == []
    elif ln <= 1 << 13:
        assert plan == [(ln, max(ceil_log2(ln), 5), 1, min(ln, k))]
        assert plan[0][1] == misort.segment_class(ln, 8)
    else:
        c = ceil_log2(ln)
        assert c == misort.segment_class(ln, 8)
        assert plan == misort.topk_plan(1 << c, k)
        assert plan[0] == (1 << c, 13, 1 << (c - 13), k << (c - 13)) and plan[-1][2] == 1 and plan[-1][3] == k


@pytest.mark.parametrize("ln", LENS)
def test_k_above_the_tile_is_always_refused(ln):
    lib = misort.lib()
    buf = (ctypes.c_int32 * 64)()
    for k in (8193, 0, -1, 1 << 40):
        assert lib.misort_topk_segments_plan(ln, k, buf, 16) == -1
        assert lib.misort_last_error()
    assert lib.misort_topk_segments_plan(-1, 1, buf, 16) == -1
    assert list(buf) == [0] * 64
    if ln <= 1 << 13:
        assert len(misort.topk_segments_plan(ln, 8192)) == (1 if ln else 0)


def test_plan_pass_counts_and_partial_writes():
    assert misort.topk_segments_plan(65537, 1024) == [(1 << 17, 13, 16, 1 << 14), (1 << 14, 13, 2, 2048),
                                                      (2048, 11, 1, 1024)]
    assert len(misort.topk_segments_plan(65536, 1024)) == 2
    assert misort.topk_segments_plan(5, 64) == [(5, 5, 1, 5)]
    lib = misort.lib()
    buf = (ctypes.c_int32 * 12)(*([-7] * 12))
    assert lib.misort_topk_segments_plan(65537, 1024, buf, 2) == 3
    assert list(buf) == [1 << 17, 13, 16, 1 << 14, 1 << 14, 13, 2, 2048, -7, -7, -7, -7]
    assert lib.misort_topk_segments_plan(65537, 1024, None, 1) == -1  # passes asked for, nowhere to write them


# ---- the oracle and the tied family ----------------------------------------------------------------------

@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("f32", [False, True], ids=["u32", "f32"])
def test_oracle_equals_a_plain_loop_on_tied_keys(largest, f32):
    lens = [0, 5, 40, 0, 0, 1, 700, 33, 2, 0]
    offs = C.L.offsets_of(lens, first=3)
    rng = np.random.default_rng(5)
    keys = C.fam_tied(rng, C.L.offsets_of([int(offs[-1]) + 4]), largest)
    for k in (1, 3, 40, 64):
        wv, wi = TSO.topk_segments_loop(keys, offs, k, largest, f32)
        gv, gi = TSO.topk_segments(keys, offs, k, largest, f32)
        np.testing.assert_array_equal(gi, wi)
        np.testing.assert_array_equal(gv, wv)
        # the fill: positions past the length, and nowhere else
        short = np.arange(k)[None, :] >= np.asarray(lens)[:, None]
        assert np.array_equal(gi == TSO.FILL_INDEX, short)
        assert np.all(gv[short] == TSO.fill_key(largest, f32))
        # equal keys in ascending position order, whatever the direction
        same = (gv[:, 1:] == gv[:, :-1]) & ~short[:, 1:]
        assert np.all(gi[:, 1:][same] > gi[:, :-1][same])


def test_fill_keys():
    table = {(False, False): 0xFFFFFFFF, (False, True): 0, (True, False): 0x7FFFFFFF, (True, True): 0xFFFFFFFF}
    for (f32, largest), key in table.items():
        assert TSO.fill_key(largest, f32) == key


@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("f32", [False, True], ids=["u32", "f32"])
@pytest.mark.parametrize("layout", sorted(C.LAYOUTS))
def test_the_tied_family_ties_at_the_cut(layout, f32, largest):
    """Otherwise 'of equal keys at the cut, the lowest positions are kept' is not tested."""
    keys, offs = C.keys_of("tied", layout, largest), C.offsets(layout)
    for k in C.KS[layout]:
        assert TSO.ties_at_the_cut(keys, offs, k, largest, f32) >= 1, (layout, k)


def test_layouts_cover_what_the_gpu_file_relies_on():
    classes = {misort.segment_class(x, 8) for x in C.LAYOUTS["short"] if x}
    assert classes == set(range(5, 14))
    lens = C.LAYOUTS["short"]
    assert lens[0] == lens[1] == lens[-1] == lens[-2] == 0 and set(range(71)) <= set(lens)
    assert [misort.segment_class(x, 8) for x in (8193, 16384, 16385, 40001, 65536, 65537)] == [14, 14, 15, 16, 16, 17]
    assert set((8193, 16384, 16385, 40001, 65536, 65537)) <= set(C.LAYOUTS["long"])
    assert len(misort.topk_segments_plan(65537, 1024)) == 3  # a pass from records to records
    assert sorted(C.FAMILIES) == sorted(["tied", "four", "equal", "half_sentinel", "half_sentinel_f32",
                                         "winners_last", "winners_one_piece", "f32"])
