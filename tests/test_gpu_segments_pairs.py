"""Segmented key-value sort and argsort on one GPU
(misort_local_sort_segments_pairs, Context.sort_segments_pairs,
Context.argsort_segments) against the numpy oracle of segments_pairs_oracle.py:
every segment [offsets[i], offsets[i + 1]) sorted on its own by (key, value), u32
keys directly, f32 keys through their order-preserving pattern; for the argsort
the value is the position inside the segment.  Every comparison is on bit
patterns; there is no tolerance.

Two paths (misort.segment_class(len, 8): the records are 8 bytes): segments up
to 2^13 pairs go through the u64 record tile, one launch per class LR = 5..13
with R = 2^(13 - LR) segments per LDS tile; longer ones class by class through
padded blocks of 2^k records.  The shapes are the smallest that cross each
boundary."""
import functools

import numpy as np
import pytest

import segment_layouts as L
import segments_pairs_oracle as SPO
import stream_order as SO
from guard_bands import assert_guards, canary_for, guarded
from sort_oracles import argsort_oracle, pairs_oracle, want_rows_pairs
from stream_order import In, Out

torch = pytest.importorskip("torch")
import misort  # noqa: E402

pytestmark = pytest.mark.gpu

U32 = np.uint32
ONES = U32(0xFFFFFFFF)
KEYS = pytest.mark.parametrize("f32", [False, True], ids=["u32", "f32"])
MODES = ["pairs", "pairs_in_place", "argsort", "argsort_default_out", "argsort_keys_in_place"]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def side(ctx):
    """A stream that is neither torch's default nor the context's own."""
    SO.calibrate()
    return torch.cuda.Stream()


def dev(a, f32=False):
    """u32 bit patterns on the device: int32 storage, or the same bits as float32 keys."""
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    return t.view(torch.float32) if f32 else t


def bits(t):
    torch.cuda.synchronize()
    return t.contiguous().view(torch.int32).reshape(-1).cpu().numpy().view(U32)


def sentinel_key(f32):
    """The key whose mapped pattern is all-ones."""
    return U32(0x7FFFFFFF) if f32 else ONES


# ---- one call in every mode against the oracle ---------------------------------------------------------

FILL = U32(0xC3C3C3C3)  # what an index output holds before an argsort: its fringe stays


def run(ctx, keys, vals, offs, f32, mode, what=""):
    """One call in ``mode`` on host bit patterns against the oracle; inputs that
    are not outputs, and the offsets, are unchanged."""
    what = f"{what} [{mode}, {'f32' if f32 else 'u32'}]"
    a, b = int(offs[0]), int(offs[-1])
    dk, o = dev(keys, f32), torch.from_numpy(offs).cuda()
    if mode.startswith("pairs"):
        dv = dev(vals)
        wk, wv = SPO.want(keys, offs, vals, f32)
        if mode == "pairs":
            ok, ov = ctx.sort_segments_pairs(dk, o, dv)
            assert ok.dtype == dk.dtype and ov.dtype == dv.dtype and ok.shape == dk.shape == ov.shape
            assert ok.data_ptr() != dk.data_ptr() and ov.data_ptr() != dv.data_ptr()
        else:
            ok, ov = ctx.sort_segments_pairs(dk, o, dv, out_keys=dk, out_values=dv)
            assert ok is dk and ov is dv
        np.testing.assert_array_equal(bits(ok), wk, err_msg=what + " keys")
        np.testing.assert_array_equal(bits(ov), wv, err_msg=what + " values")
        if mode == "pairs":
            np.testing.assert_array_equal(bits(dk), keys, err_msg=what + " (keys changed)")
            np.testing.assert_array_equal(bits(dv), vals, err_msg=what + " (values changed)")
    else:
        wk, wv = SPO.want(keys, offs, None, f32, fringe_vals=np.full(keys.size, FILL))
        if mode == "argsort":
            out = dev(np.full(keys.size, FILL))
            assert ctx.argsort_segments(dk, o, out=out) is out
            np.testing.assert_array_equal(bits(out), wv, err_msg=what + " indices")  # the fringe is not written
            np.testing.assert_array_equal(bits(dk), keys, err_msg=what + " (keys changed)")
        elif mode == "argsort_default_out":
            out = ctx.argsort_segments(dk, o)
            assert out.shape == dk.shape and out.dtype == torch.int32
            np.testing.assert_array_equal(bits(out)[a:b], wv[a:b], err_msg=what + " indices")
            np.testing.assert_array_equal(bits(dk), keys, err_msg=what + " (keys changed)")
        else:  # the keys sorted in place, the indices beside them
            out = dev(np.full(keys.size, FILL))
            ok, ov = ctx.sort_segments_pairs(dk, o, None, out_keys=dk, out_values=out)
            assert ok is dk and ov is out
            np.testing.assert_array_equal(bits(dk), wk, err_msg=what + " keys")
            np.testing.assert_array_equal(bits(out), wv, err_msg=what + " indices")
        # the indices gather every sorted segment
        idx = bits(out)[a:b].astype(np.int64)
        starts = np.repeat(offs[:-1], np.diff(offs))
        np.testing.assert_array_equal(keys[starts + idx], wk[a:b], err_msg=what + " gather")
    np.testing.assert_array_equal(o.cpu().numpy(), offs, err_msg=what + " (offsets changed)")


def tied(seed, n, f32=False):
    """n (key, value) bit patterns with ties in both: a third of the keys from 16
    values (f32: the specials among them), values from 8."""
    rng = np.random.default_rng(seed)
    k = SO.f32_keys(seed, n).view(U32).copy() if f32 else SO.tied_u32(seed, n)
    v = rng.integers(0, 8, n).astype(U32)
    v[rng.random(n) < 0.1] = ONES
    return k, v


# ---- lengths: every class, interleaved ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def every_length():
    lens = list(range(71)) + [(1 << j) + d for j in range(7, 14) for d in (-1, 0, 1)]
    lens = np.random.default_rng(11).permutation(lens)
    classes = {misort.segment_class(int(x), 8) for x in lens if x}
    assert classes == set(range(5, 15))  # every tile class and the first long one
    return L.offsets_of(lens)


@KEYS
@pytest.mark.parametrize("mode", MODES)
def test_every_length_in_one_call(ctx, f32, mode):
    offs = every_length()
    k, v = tied(12, int(offs[-1]), f32)
    run(ctx, k, v, offs, f32, mode, "every length")


# ---- counts of one class around the tile's rows ------------------------------------------------------

@pytest.mark.parametrize("lr", [5, 9, 13])
def test_counts_of_one_class(ctx, lr):
    r = 1 << (13 - lr)
    lo = L.class_lo(lr)
    rng = np.random.default_rng(100 * lr)
    for count in sorted({1, r - 1, r, r + 1, 2 * r + r // 2 + 1} - {0}):
        lens = rng.integers(lo + 1, (1 << lr) + 1, size=count)
        lens[rng.integers(0, count)] = 1 << lr  # a full block
        lens[rng.integers(0, count)] = lo + 1  # the shortest of the class
        assert all(misort.segment_class(int(x), 8) == lr for x in lens)
        offs = L.offsets_of(lens)
        k, v = tied(7 * count + lr, int(offs[-1]))
        for mode in ("pairs", "argsort"):
            run(ctx, k, v, offs, False, mode, f"{count} segments of class {lr}")


# ---- long classes ---------------------------------------------------------------------------------------

@KEYS
@pytest.mark.parametrize("mode", ["pairs", "pairs_in_place", "argsort", "argsort_keys_in_place"])
def test_two_long_classes(ctx, f32, mode):
    lens = [0, 5, 16385, 0, 8193, 100, 16384, 33, 20000, 0, 1]
    # the shortest and the padding-free length of k = 14, the shortest of k = 15 and one inside it
    assert [misort.segment_class(x, 8) for x in (8193, 16384, 16385, 20000)] == [14, 14, 15, 15]
    offs = L.offsets_of(lens)
    k, v = tied(51, int(offs[-1]), f32)
    run(ctx, k, v, offs, f32, mode, "two long classes")


# ---- key families built on ties -------------------------------------------------------------------------

FAMILY_LENS = [0, 1, 33, 5, 700, 64, 0, 8192, 31, 129, 2, 4097, 8193, 0, 20000, 3]


def family(name, f32):
    offs = L.offsets_of(FAMILY_LENS, first=2)
    n = int(offs[-1]) + 3
    rng = np.random.default_rng(len(name) + 40)
    ids, pos, ln = L.seg_ids(offs)
    k, v = tied(41, n, f32)
    body = slice(int(offs[0]), int(offs[-1]))
    if name == "four_keys":  # the value, or the position, decides
        pool = np.array([0x80000000, 0x00000000, 0x3F800000, 0xBF800000], dtype=U32)  # -0.0, +0.0, 1.0, -1.0 as f32
        k[body] = pool[rng.integers(0, 4, ids.size)]
    elif name == "all_equal":
        k[body] = U32(0x3F800000)
    elif name == "sentinels":  # a third of each segment is the all-ones record
        kb, vb = k[body], v[body]
        kb[pos % 3 == 0] = sentinel_key(f32)
        vb[pos % 3 == 0] = ONES
    elif name == "opposed":  # every key of segment i above every key of segment i + 1 (positive floats too)
        k[body] = L.fam_opposed(rng, ids, pos, ln, U32) >> U32(1)
    else:
        assert name == "f32_specials" and f32  # NaNs of both signs, +-0, +-inf, denormals: tied() has them
        assert {0x7FC00000, 0xFFC00000, 0, 0x80000000, 0x7F800000, 0xFF800000, 1} <= set(k[body].tolist())
    return k, v, offs


def family_cases():
    for name in ("four_keys", "all_equal", "sentinels", "opposed"):
        for f32 in (False, True):
            yield pytest.param(name, f32, id=f"{name}-{'f32' if f32 else 'u32'}")
    yield pytest.param("f32_specials", True, id="f32_specials")


@pytest.mark.parametrize("name,f32", list(family_cases()))
def test_key_families(ctx, name, f32):
    k, v, offs = family(name, f32)
    for mode in ("pairs", "argsort", "pairs_in_place"):
        run(ctx, k, v, offs, f32, mode, name)


def test_f32_order_is_the_total_order(ctx):
    """Negative NaN < -inf < -0.0 < +0.0 < +inf < positive NaN, bit-exact."""
    pat = np.array([0x7FC00000, 0x7F800000, 0x00000000, 0x80000000, 0xFF800000, 0xFFC00000], dtype=U32)
    offs = L.offsets_of([6, 6])
    k = np.concatenate([pat, pat[::-1]])
    ok, ov = ctx.sort_segments_pairs(dev(k, True), torch.from_numpy(offs).cuda())
    np.testing.assert_array_equal(bits(ok), np.concatenate([pat[::-1], pat[::-1]]))
    np.testing.assert_array_equal(bits(ov), [5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5])


# ---- past one workgroup of offsets -----------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def many_case(name):
    offs, n = L.layout(name, 8)
    assert offs.size - 1 > 2040
    k = L.make("dups", 1000 + len(name), offs, n, U32)  # four keys per segment, no two segments share one
    v = np.random.default_rng(len(name)).integers(0, 8, n).astype(U32)
    return k, v, offs


@pytest.mark.parametrize("mode", ["pairs", "pairs_in_place", "argsort"])
@pytest.mark.parametrize("name", ["mixed", "boundary2047", "boundary2048", "boundary2049"])
def test_many_segments(ctx, name, mode):
    k, v, offs = many_case(name)
    if name == "mixed":
        spans = L.class_spans(np.diff(offs), 8)
        assert any(len(s) > 1 for s in spans.values()) and max(spans) > 13
    run(ctx, k, v, offs, False, mode, name)


# ---- buffers: guard bands, views, fringes -------------------------------------------------------------

def banded(a, lead, canary, f32=False):
    """(device base, device view) of the u32 patterns ``a`` between guard bands."""
    base, _ = guarded(a.size, U32, lead, canary, a)
    dbase = dev(base, f32)
    return dbase, dbase[lead:lead + a.size]


@KEYS
@pytest.mark.parametrize("lead", [1, 4])
def test_outputs_between_guard_bands_and_fringes(ctx, f32, lead):
    lens = [40, 0, 700, 1, 8193 + 9, 64, 8192, 20000]
    offs = L.offsets_of(lens, first=7)
    n = int(offs[-1]) + 9
    k, v = tied(71, n, f32)
    canary = canary_for(k, v)
    prefill = np.full(n, canary + U32(1), dtype=U32)
    o = torch.from_numpy(offs).cuda()
    wk, wv = SPO.want(k, offs, v, f32)
    # out of place: the fringes are the inputs'
    bk_in, dk = banded(k, lead, canary, f32)
    bv_in, dv = banded(v, lead, canary)
    bk_out, ok = banded(prefill, lead, canary, f32)
    bv_out, ov = banded(prefill, lead, canary)
    got = ctx.sort_segments_pairs(dk, o, dv, out_keys=ok, out_values=ov)
    assert got[0] is ok and got[1] is ov
    np.testing.assert_array_equal(bits(ok), wk)
    np.testing.assert_array_equal(bits(ov), wv)
    for base in (bk_out, bv_out, bk_in, bv_in):
        assert_guards(bits(base), n, lead, canary)
    np.testing.assert_array_equal(bits(dk), k)
    np.testing.assert_array_equal(bits(dv), v)
    # argsort: the index fringe is not written, the key fringe is copied
    ak, ai = SPO.want(k, offs, None, f32, fringe_vals=prefill)
    bk_out, ok = banded(prefill, lead, canary, f32)
    bi_out, oi = banded(prefill, lead, canary)
    ctx.sort_segments_pairs(dk, o, None, out_keys=ok, out_values=oi)
    np.testing.assert_array_equal(bits(ok), ak)
    np.testing.assert_array_equal(bits(oi), ai)
    bi2_out, oi2 = banded(prefill, lead, canary)
    ctx.argsort_segments(dk, o, out=oi2)
    np.testing.assert_array_equal(bits(oi2), ai)
    for base in (bk_out, bi_out, bi2_out, bk_in):
        assert_guards(bits(base), n, lead, canary)
    np.testing.assert_array_equal(bits(dk), k)
    # in place: the fringes are untouched (they are the inputs' anyway), the bands too
    ctx.sort_segments_pairs(dk, o, dv, out_keys=dk, out_values=dv)
    np.testing.assert_array_equal(bits(dk), wk)
    np.testing.assert_array_equal(bits(dv), wv)
    for base in (bk_in, bv_in):
        assert_guards(bits(base), n, lead, canary)


def test_values_without_keys_out_at_the_c_boundary(ctx):
    """d_keys_out == NULL with a value array: the values only."""
    lens = [33, 0, 1000, 8193, 5]
    offs = L.offsets_of(lens, first=1)
    n = int(offs[-1]) + 2
    k, v = tied(77, n)
    dk, dv, o = dev(k), dev(v), torch.from_numpy(offs).cuda()
    out = dev(np.full(n, FILL))
    f = misort.lib().misort_local_sort_segments_pairs
    torch.cuda.synchronize()
    assert f(ctx._h, misort.U32, dk.data_ptr(), dv.data_ptr(), None, out.data_ptr(), n, o.data_ptr(), len(lens),
             ctx.native_stream) == 0
    ctx.synchronize()
    np.testing.assert_array_equal(bits(out), SPO.want(k, offs, v)[1])
    np.testing.assert_array_equal(bits(dk), k)
    np.testing.assert_array_equal(bits(dv), v)


def test_nothing_to_sort(ctx):
    k, v = tied(91, 100)
    dk, dv = dev(k), dev(v)
    for offs in ([0], [5], [3, 3, 3, 3], [0, 0], [100, 100]):
        o = torch.tensor(offs, dtype=torch.int64, device="cuda")
        ok, ov = ctx.sort_segments_pairs(dk, o, dv)  # the fringe copies alone
        np.testing.assert_array_equal(bits(ok), k, err_msg=str(offs))
        np.testing.assert_array_equal(bits(ov), v, err_msg=str(offs))
        out = dev(np.full(100, FILL))
        ctx.argsort_segments(dk, o, out=out)
        np.testing.assert_array_equal(bits(out), np.full(100, FILL), err_msg=str(offs))
        ctx.sort_segments_pairs(dk, o, dv, out_keys=dk, out_values=dv)
        np.testing.assert_array_equal(bits(dk), k, err_msg=str(offs))
    e = torch.empty(0, dtype=torch.int32, device="cuda")
    for offs in ([0], [0, 0, 0]):
        o = torch.tensor(offs, dtype=torch.int64, device="cuda")
        assert ctx.argsort_segments(e, o).numel() == 0
        assert ctx.sort_segments_pairs(e, o, e)[1].numel() == 0
    f = misort.lib().misort_local_sort_segments_pairs
    assert f(ctx._h, misort.U32, None, None, None, None, 0, None, 3, ctx.native_stream) == 0  # n == 0: no pointer


# ---- refusals, outputs unchanged -------------------------------------------------------------------------

@pytest.mark.parametrize("argsort", [False, True], ids=["pairs", "argsort"])
@pytest.mark.parametrize("case", ["decreasing", "negative_first", "last_past_n"])
def test_malformed_offsets_are_refused_before_anything_is_written(ctx, case, argsort):
    lens = [40, 10, 700, 1, 20000, 64, 9]
    offs = L.offsets_of(lens, first=2)
    n = int(offs[-1]) + 3  # fringes on both sides: they are not copied either
    k, v = tied(101, n)
    if case == "decreasing":
        offs[3], offs[4], bad = offs[4], offs[3], 3
    elif case == "negative_first":
        offs[0], bad = -2, 0
    else:
        offs[-1], bad = n + 3, len(lens) - 1
    canary = canary_for(k, v)
    prefill = np.full(n, canary + U32(1), dtype=U32)
    bk, ok = banded(prefill, 4, canary)
    bv, ov = banded(prefill, 4, canary)
    dk, dv = dev(k), dev(v)
    with pytest.raises(misort.MisortError) as ei:
        if argsort:
            ctx.sort_segments_pairs(dk, torch.from_numpy(offs).cuda(), None, out_keys=ok, out_values=ov)
        else:
            ctx.sort_segments_pairs(dk, torch.from_numpy(offs).cuda(), dv, out_keys=ok, out_values=ov)
    msg = str(ei.value)
    assert ei.value.code == -1 and f"index {bad} " in msg and "malformed offsets: 1 of 7 segments" in msg
    np.testing.assert_array_equal(bits(ok), prefill)
    np.testing.assert_array_equal(bits(ov), prefill)
    assert_guards(bits(bk), n, 4, canary)
    assert_guards(bits(bv), n, 4, canary)
    np.testing.assert_array_equal(bits(dk), k)
    np.testing.assert_array_equal(bits(dv), v)


def test_refused_overlaps(ctx):
    n = 4096
    base = torch.zeros(2 * n + 16, dtype=torch.int64, device="cuda")
    b32 = base.view(torch.int32)  # 4 n + 32 elements
    o = torch.tensor([0, 100, n], dtype=torch.int64, device="cuda")
    A, A_SHIFT = b32[:n], b32[4:n + 4]
    free = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    X, Y, Z = free
    # (keys, values, out_keys, out_values)
    refused = [
        (A, X, A_SHIFT, Y),        # out_keys overlaps keys, not exactly
        (X, A, Y, A_SHIFT),        # out_values overlaps values, not exactly
        (X, Y, A, A_SHIFT),        # the outputs overlap each other
        (X, Y, A, A),              # ... exactly
        (X, A, A_SHIFT, Y),        # out_keys overlaps values
        (X, A, A, Y),              # ... exactly
        (A, X, Y, A_SHIFT),        # out_values overlaps keys
        (A, X, Y, A),              # ... exactly
        (A, A_SHIFT, X, Y),        # keys overlap values
        (A, None, X, A_SHIFT),     # argsort: the indices overlap the keys
        (A, None, A_SHIFT, X),     # argsort: out_keys overlaps keys, not exactly
    ]
    for i, (k, v, ok, ov) in enumerate(refused):
        with pytest.raises(misort.MisortError) as ei:
            ctx.sort_segments_pairs(k, o, v, out_keys=ok, out_values=ov)
        assert ei.value.code == -1 and "overlap" in str(ei.value), i
    with pytest.raises(misort.MisortError) as ei:
        ctx.argsort_segments(A, o, out=A_SHIFT)
    assert ei.value.code == -1 and "overlap" in str(ei.value)
    # an output and the offsets: the offsets' first word lies in the output
    offs_in_a = base[n // 2 - 2:n // 2 + 1]
    assert A.data_ptr() <= offs_in_a.data_ptr() < A.data_ptr() + 4 * n
    for k, v, ok, ov in ((X, Y, A, Z), (X, Y, Z, A), (X, None, None, A)):
        with pytest.raises(misort.MisortError) as ei:
            if ok is None:
                ctx.argsort_segments(k, offs_in_a, out=ov)
            else:
                ctx.sort_segments_pairs(k, offs_in_a, v, out_keys=ok, out_values=ov)
        assert ei.value.code == -1 and "d_offsets" in str(ei.value)
    torch.cuda.synchronize()
    assert int(base.abs().sum()) == 0 and all(int(t.abs().sum()) == 0 for t in free)


def test_entry_point_refusals(ctx):
    f = misort.lib().misort_local_sort_segments_pairs
    t = [torch.full((64,), 7, dtype=torch.int32, device="cuda") for _ in range(4)]
    o = torch.tensor([0, 4, 4], dtype=torch.int64, device="cuda")
    (p, q, r, w), s = [x.data_ptr() for x in t], ctx.native_stream
    torch.cuda.synchronize()
    for dt in (misort.U64, misort.F64, 4, -1):  # a wrong key dtype
        assert f(ctx._h, dt, p, q, r, w, 4, o.data_ptr(), 1, s) == -1
    assert b"MISORT_U32 or MISORT_F32" in misort.lib().misort_last_error()
    assert f(ctx._h, misort.U32, p, q, r, w, -1, o.data_ptr(), 1, s) == -1
    assert f(ctx._h, misort.U32, p, q, r, w, 4, o.data_ptr(), -1, s) == -1
    assert f(ctx._h, misort.U32, p, q, r, w, 4, o.data_ptr(), 1 << 31, s) == -1
    assert f(ctx._h, misort.U32, p, q, r, w, 4, o.data_ptr() + 4, 1, s) == -1  # offsets need 8-byte alignment
    assert b"8-byte aligned" in misort.lib().misort_last_error()
    assert f(ctx._h, misort.U32, p, q, r, w, 4, None, 1, s) == -1
    assert f(ctx._h, misort.U32, None, q, r, w, 4, o.data_ptr(), 1, s) == -1  # no keys
    assert f(ctx._h, misort.U32, p, q, r, None, 4, o.data_ptr(), 1, s) == -1  # d_vals_out is required
    assert f(ctx._h, misort.U32, p + 2, q, r, w, 4, o.data_ptr(), 1, s) == -1  # 4-byte alignment
    ctx.synchronize()
    for x in t:
        assert bits(x).tolist() == [7] * 64
    assert f(ctx._h, misort.U32, p + 4, q + 4, r + 4, w + 4, 4, o.data_ptr(), 1, s) == 0  # 4-byte alignment is enough
    ctx.synchronize()


def test_python_argument_checks(ctx):
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    o = torch.tensor([0, 10, 64], dtype=torch.int64, device="cuda")
    for call in (lambda k, off, **kw: ctx.sort_segments_pairs(k, off, d, **kw),
                 lambda k, off, **kw: ctx.argsort_segments(k, off, **kw)):
        with pytest.raises(TypeError):
            call(d, o.to(torch.int32))
        with pytest.raises(TypeError):
            call(d.to(torch.int64), o)  # a wrong key dtype
        with pytest.raises(TypeError):
            call(d.to(torch.float64), o)
        with pytest.raises(ValueError):
            call(d, o.cpu())
        with pytest.raises(ValueError):
            call(d, o.view(1, 3))
        with pytest.raises(ValueError):
            call(d, o[:0])
        with pytest.raises(ValueError):
            call(d.view(8, 8), o)
    with pytest.raises(ValueError):
        ctx.argsort_segments(torch.zeros(128, dtype=torch.int32, device="cuda")[::2], o)
    with pytest.raises(TypeError):
        ctx.sort_segments_pairs(d, o, d.to(torch.float32))
    with pytest.raises(ValueError):
        ctx.sort_segments_pairs(d, o, torch.zeros(32, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        ctx.sort_segments_pairs(d, o, d, out_keys=torch.zeros(64, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        ctx.argsort_segments(d, o, out=torch.zeros(64, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ctx.argsort_segments(d, o, out=torch.zeros(63, dtype=torch.int32, device="cuda"))


# ---- agreement with the existing entry points -----------------------------------------------------------

@KEYS
@pytest.mark.parametrize("rows,cols", [(64, 1000), (3, 9000)])
def test_uniform_offsets_equal_the_row_calls(ctx, f32, rows, cols):
    k, v = tied(cols, rows * cols, f32)
    dk, dv = dev(k, f32), dev(v)
    o = torch.arange(0, rows * cols + 1, cols, dtype=torch.int64, device="cuda")
    ok, ov = ctx.sort_segments_pairs(dk, o, dv)
    rk, rv = ctx.sort_rows_pairs(dk.view(rows, cols), dv.view(rows, cols))
    np.testing.assert_array_equal(bits(ok), bits(rk))
    np.testing.assert_array_equal(bits(ov), bits(rv))
    np.testing.assert_array_equal(bits(ctx.argsort_segments(dk, o)), bits(ctx.argsort_rows(dk.view(rows, cols))))
    wk, wv = want_rows_pairs(k.reshape(rows, cols), v.reshape(rows, cols), f32)
    np.testing.assert_array_equal(bits(ok), wk.reshape(-1))
    np.testing.assert_array_equal(bits(ov), wv.reshape(-1))


@KEYS
def test_one_segment_equals_sort_pairs(ctx, f32):
    n = 20000
    k, v = tied(n, n, f32)
    dk, dv = dev(k, f32), dev(v)
    o = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    ok, ov = ctx.sort_segments_pairs(dk, o, dv)
    rk, rv = ctx.sort_pairs(dk, dv)
    np.testing.assert_array_equal(bits(ok), bits(rk))
    np.testing.assert_array_equal(bits(ov), bits(rv))
    np.testing.assert_array_equal(bits(ctx.argsort_segments(dk, o)), bits(ctx.argsort(dk)))
    hk = k.view(np.float32) if f32 else k
    np.testing.assert_array_equal(bits(ok), pairs_oracle(hk, v)[0])
    np.testing.assert_array_equal(bits(ctx.argsort_segments(dk, o)), argsort_oracle(hk))


# ---- launch accounting under the profiler ---------------------------------------------------------------

def profiled(ctx, call):
    ctx.profile(True)
    try:
        ctx.profile_reset()
        call()
        torch.cuda.synchronize()
        return ctx.profile_read(), ctx.profile_trace()
    finally:
        ctx.profile(False)


@pytest.mark.parametrize("mode,arrays", [("pairs", 4), ("argsort", 2), ("argsort_keys", 3)])
def test_profile_tile_classes(ctx, mode, arrays):
    lens = [40, 0, 700, 1, 3000, 64, 9, 650, 8192, 33]  # tile classes only
    classes = {misort.segment_class(x, 8) for x in lens if x}
    assert max(classes) == 13
    offs = L.offsets_of(lens)
    k, v = tied(121, int(offs[-1]))
    dk, dv, o = dev(k), dev(v), torch.from_numpy(offs).cuda()
    out = torch.empty_like(dv)
    call = {"pairs": lambda: ctx.sort_segments_pairs(dk, o, dv),
            "argsort": lambda: ctx.argsort_segments(dk, o, out=out),
            "argsort_keys": lambda: ctx.sort_segments_pairs(dk, o, None, out_values=out)}[mode]
    rec, trace = profiled(ctx, call)
    launches, ms, nbytes = rec["tile_sort"]
    assert launches == len(classes) and ms > 0.0 and nbytes == arrays * 4 * sum(lens)
    per_class = sorted(b for kind, _, b in trace if kind == "tile_sort")
    want = sorted(arrays * 4 * sum(x for x in lens if x and misort.segment_class(x, 8) == c) for c in classes)
    assert per_class == want
    assert rec["other"][0] == 2  # count and scatter
    assert all(rec[kind][0] == 0 for kind in rec if kind not in ("tile_sort", "other"))


def test_profile_long_class_pad_and_unpad(ctx):
    lens = [8193, 40, 10000, 0]  # one long class, k = 14, and one tile class
    assert [misort.segment_class(x, 8) for x in lens] == [14, 6, 14, -1]
    offs = L.offsets_of(lens)
    k, v = tied(131, int(offs[-1]))
    dk, dv, o = dev(k), dev(v), torch.from_numpy(offs).cuda()
    long_keys, blocks = 8193 + 10000, 2 << 14
    for with_vals, with_keys in ((True, True), (False, False)):
        out = torch.empty_like(dv)
        call = ((lambda: ctx.sort_segments_pairs(dk, o, dv)) if with_vals
                else (lambda: ctx.argsort_segments(dk, o, out=out)))
        rec, trace = profiled(ctx, call)
        others = [b for kind, _, b in trace if kind == "other"]
        assert rec["other"][0] == len(others) == 4  # count, scatter, pad, unpad
        pad = (8 if with_vals else 4) * long_keys + 8 * blocks
        unpad = (16 if with_keys else 12) * long_keys
        assert sorted(others[2:]) == sorted([pad, unpad])
        tiles = [b for kind, _, b in trace if kind == "tile_sort"]
        arrays = 2 + with_vals + with_keys
        assert arrays * 4 * 40 in tiles and 2 * 8 * blocks in tiles  # class 6; the blocks' own SORT pass


# ---- stream order ---------------------------------------------------------------------------------------

STREAM_LENS = [40, 0, 700, 1, 20000, 64, 9, 8193, 8192, 0, 33]


@functools.lru_cache(maxsize=None)
def stream_case(argsort, in_place=False, salt=0):
    offs = L.offsets_of(STREAM_LENS, first=3)
    n = int(offs[-1]) + 5
    k, v = tied(900 + salt, n)
    k |= U32(1)  # never the poison
    if argsort:
        wk, wi = SPO.want(k, offs, None, fringe_vals=SO.out_fill(n, U32))
        return ({"keys": In(k, lead=1), "offs": In(offs), "idx": Out(n, U32, lead=1)},
                {"keys": k, "offs": offs, "idx": wi})
    wk, wv = SPO.want(k, offs, v)
    if in_place:
        return ({"keys": In(k, lead=1), "vals": In(v, lead=1), "offs": In(offs)},
                {"keys": wk, "vals": wv, "offs": offs})
    return ({"keys": In(k, lead=1), "vals": In(v, lead=1), "offs": In(offs), "ok": Out(n, U32, lead=1),
             "ov": Out(n, U32, lead=1)},
            {"keys": k, "vals": v, "offs": offs, "ok": wk, "ov": wv})


def issue(c, t, handle):
    if "idx" in t:
        c.argsort_segments(t["keys"], t["offs"], out=t["idx"], stream=handle)
    elif "ok" in t:
        c.sort_segments_pairs(t["keys"], t["offs"], t["vals"], out_keys=t["ok"], out_values=t["ov"], stream=handle)
    else:
        c.sort_segments_pairs(t["keys"], t["offs"], t["vals"], out_keys=t["keys"], out_values=t["vals"],
                              stream=handle)


def run_stream(c, stream, kind, mode, salt=0, pending=True):
    """The call behind a producer pending on ``stream``.  The call waits on its
    own stream by contract: the result alone is compared."""
    stage, expect = stream_case(kind == "argsort", kind == "in_place", salt)
    handle = None if mode == "current" else stream.cuda_stream
    res = SO.behind_pending_work(stream, stage, lambda t: issue(c, t, handle),
                                 ms=SO.PRODUCER_MS if pending else 0.01,
                                 current="stream" if mode == "current" else "elsewhere")
    SO.compare(res, expect, f"segments pairs {kind} ({mode})")
    return res


@pytest.mark.parametrize("mode", ["explicit", "current"])
@pytest.mark.parametrize("kind", ["pairs", "in_place", "argsort"])
def test_behind_pending_work_on_a_warm_context(ctx, side, kind, mode):
    run_stream(ctx, side, kind, mode, salt=SO.WARM_SALT, pending=False)  # other data: grows the scratch
    run_stream(ctx, side, kind, mode)


@pytest.mark.parametrize("mode", ["explicit", "current"])
@pytest.mark.parametrize("kind", ["pairs", "argsort"])
def test_behind_pending_work_on_a_fresh_context(side, kind, mode):
    c = misort.Context(0)
    try:
        run_stream(c, side, kind, mode)
    finally:
        c.close()


def test_two_calls_back_to_back_on_one_stream(ctx, side):
    """The second call reads other inputs and reuses the header, the lists and
    the padded blocks while the first's kernels may still be running: both exact."""
    cases = [stream_case(False, False, 77), stream_case(True, False, 78)]
    stage = {f"{name}{i}": b for i, (st, _) in enumerate(cases) for name, b in st.items()}
    expect = {f"{name}{i}": w for i, (_, ex) in enumerate(cases) for name, w in ex.items()}

    def call(t):
        for i in range(2):
            issue(ctx, {name[:-1]: x for name, x in t.items() if name.endswith(str(i))}, side.cuda_stream)
    SO.compare(SO.behind_pending_work(side, stage, call), expect, "back to back")


# ---- repeatability ----------------------------------------------------------------------------------------

def test_repeatability(ctx):
    """The order of a class's list is whatever the atomics gave: it must not show."""
    k, v, offs = many_case("mixed")
    dk, dv, o = dev(k), dev(v), torch.from_numpy(offs).cuda()
    first = [bits(t) for t in ctx.sort_segments_pairs(dk, o, dv)]
    again = [bits(t) for t in ctx.sort_segments_pairs(dk, o, dv)]
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(bits(ctx.argsort_segments(dk, o)), bits(ctx.argsort_segments(dk, o)))
