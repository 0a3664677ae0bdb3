"""The buffer contract of the keys-only hot path (include/misort.h): what
misort_local_sort, misort_parallel_bitonic_sort(_oop), misort_merge_split,
misort_merge_split_tail, the codec's decode and misort_check_sort do to memory.

* Every output lies between two bands of a canary key that does not occur in
  the data (guard_bands.py); after the call both bands are compared bit for
  bit, so one padding key (all-ones) stored at index n or -1 fails the test.
* The inputs are compared with what was uploaded.
* Views start 1, 2 or 3 elements into their storage: the entry points need
  element alignment only, while the SORT tile and the merge passes take
  16-byte vector accesses (the runtime routes such arrays through an aligned
  buffer).  Every base tensor is 256-byte aligned, so a lead says exactly how
  a view is aligned.
* Partly overlapping input and output are refused with code -1; wrong dtypes,
  short outputs and strided tensors raise in Python; nothing is written then.
* check_sort counts a descent at a lane, wave, workgroup or grid-stride
  boundary exactly once.

Keys are tile_battery.sentinels_random (all-ones and zero keys among uniform
ones: all-ones is the kernels' padding value); f64 keys of the local sort are
test_gpu_rows.f64_mix (NaNs of both signs, +-0, denormals) against
kunmap(np.sort(kmap(x))).  Every comparison is on bit patterns."""
import functools

import numpy as np
import pytest

import guard_bands as G
import oracle_lib as O
import tile_battery as B

torch = pytest.importorskip("torch")
import misort  # noqa: E402
from test_gpu_rows import f64_mix  # noqa: E402
from test_gpu_runs import expect, expectk  # noqa: E402

pytestmark = pytest.mark.gpu

U32_T = torch.uint32 if hasattr(torch, "uint32") else torch.int32
U64_T = torch.uint64 if hasattr(torch, "uint64") else torch.int64
KINDS = ["u32", "u64", "f64"]
BITS = {"u32": np.uint32, "u64": np.uint64, "f64": np.uint64}
ALIGNED = {"u32": 64, "u64": 32, "f64": 32}  # keys in 256 bytes: a view at this lead is as aligned as its base
LEADS = {"u32": (64, 1, 2, 3), "u64": (32, 1), "f64": (32, 1)}
U32_N = [1, 5, 16383, 16385, (1 << 16) + 3, (1 << 17) + 9, (1 << 18) + 3, (1 << 21) + 5]
U64_N = [5, 8191, 8193, (1 << 17) + 3, (1 << 21) - 3]
SORT_CASES = [("u32", n) for n in U32_N] + [(k, n) for k in ("u64", "f64") for n in U64_N]
SORT_OUT_CASES = [(k, n, lead) for k, n in SORT_CASES for lead in LEADS[k]]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


def to_dev(bits, kind):
    """Bit patterns (u32 / u64) as a device tensor of the kind's key type."""
    bits = np.array(bits)  # a private, writable copy (the cached cases are read-only)
    if kind == "u32":
        return torch.from_numpy(bits.view(np.int32)).cuda().view(U32_T)
    if kind == "u64":
        return torch.from_numpy(bits.view(np.int64)).cuda().view(U64_T)
    return torch.from_numpy(bits.view(np.float64)).cuda()


def to_host(t):
    """The bit patterns of a device tensor."""
    torch.cuda.synchronize()
    if t.element_size() == 8:
        return t.view(torch.int64).cpu().numpy().view(np.uint64)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


class Band:
    """n keys of `kind` on the device, `lead` elements into a 256-byte-aligned
    base tensor, canaries on both sides (guard_bands.guarded)."""

    def __init__(self, kind, n, lead, canary, body=None):
        self.n, self.lead, self.canary = n, lead, canary
        self.h, _ = G.guarded(n, BITS[kind], lead, canary, body)
        self.base = to_dev(self.h, kind)
        assert self.base.data_ptr() % 256 == 0
        self.view = self.base[lead:lead + n]
        if n:
            assert self.view.data_ptr() == self.base.data_ptr() + lead * self.base.element_size()

    def block(self):
        return to_host(self.base)[self.lead:self.lead + self.n]

    def assert_guards(self):
        G.assert_guards(to_host(self.base), self.n, self.lead, self.canary)

    def assert_unchanged(self, what):
        got = to_host(self.base)
        if not np.array_equal(got, self.h):
            i = int(np.flatnonzero(got != self.h)[0])
            raise AssertionError(f"{what} changed: key {i - self.lead} of {self.n} (lead {self.lead}) is "
                                 f"{int(got[i]):#x}, was {int(self.h[i]):#x}")


def assert_block(got, want, what):
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at key {i} of {want.size}: got {int(got[i]):#x}, "
                             f"want {int(want[i]):#x}; {int(np.count_nonzero(got != want))} keys differ")


@functools.lru_cache(maxsize=None)
def sort_case(kind, n):
    """(key bits, their sorted bits, a canary): computed once per (kind, n); read-only."""
    if kind == "f64":
        x = f64_mix(np.random.default_rng(9100 + n), 1, n).reshape(-1)
        bits = np.ascontiguousarray(x.view(np.uint64))
        want = G.kunmap(np.sort(G.kmap(x)))
    else:
        bits = B.sentinels_random(n, BITS[kind], 9100, n % 97)
        want = np.sort(bits)
    for a in (bits, want):
        a.setflags(write=False)
    return bits, want, G.canary_for(bits)


def f64_finite(n, seed):
    """Finite doubles of both signs, +0.0 and both infinities as bit patterns:
    keys on which the reference's double compare is a total order (the oracle
    of the multi-rank sort and of compare_split is the reference's code)."""
    x = O.generate_f64(n + seed % 7)[-n:].copy()
    x[x == 0] = 1.0
    x[::3] *= -0.5
    x[5::13] = 0.0
    if n > 8:
        x[7], x[8] = np.inf, -np.inf
    return x


# ---------------------------------------------------------------- merge passes

MERGE_PASSES = [("run_merge", np.uint32, 13, 0), ("run_merge", np.uint64, 13, 0)] + \
    [("run_mergek", dt, hi, lk) for lk in (1, 2, 3, 4) for dt, hi in ((np.uint32, 14), (np.uint64, 13))]


def pass_sizes(hi, lk):
    K = 1 << max(lk, 1)  # a 2-way level merges pairs of runs
    return [5000, (1 << hi) + 1, (K << hi) - 4097, (K << hi) + ((K - 1) << hi) + 1000]


@pytest.mark.parametrize("which", range(4), ids=["5000", "run+1", "group-4097", "group+ragged"])
@pytest.mark.parametrize("kind,dt,hi,lk", MERGE_PASSES,
                         ids=[f"{k}-{np.dtype(d).name}-hi{h}-lk{lk}" for k, d, h, lk in MERGE_PASSES])
def test_merge_pass_between_guards(ctx, kind, dt, hi, lk, which):
    """One merge pass (k_runs_merge; mergek_chunk's shifted LDS copy with scalar
    head and tail stores) on ragged inputs: the output equals numpy's, nothing
    is written outside its n keys, the input is left unchanged."""
    n = pass_sizes(hi, lk)[which]
    tk = "u32" if dt == np.uint32 else "u64"
    x = B.sentinels_random(n, dt, 9200 + hi + lk, which)
    w = 1 << hi
    for s in range(0, n, w):
        x[s:s + w].sort()
    want = expect(x, hi) if kind == "run_merge" else expectk(x, hi, lk)
    c = G.canary_for(x)
    src = Band(tk, n, ALIGNED[tk], c, x)
    dst = Band(tk, n, ALIGNED[tk], c)
    torch.cuda.synchronize()  # the probe runs on the context's own stream
    ctx.pass_probe(src.view, dst.view, kind, hi, lk, False, reps=1, n=n)
    ctx.synchronize()
    assert_block(dst.block(), want, f"{kind} hi={hi} lk={lk} n={n}")
    dst.assert_guards()
    src.assert_unchanged("the pass's input")


# ------------------------------------------------------------------ local sort

def test_sort_sizes_reach_every_pass_shape():
    """The sizes below run a tile-only plan, a 2-way pass and multi-way passes
    of 2, 3 and 4 levels (read from the plan the library reports)."""
    shapes = set()
    for kb, sizes in ((4, U32_N), (8, U64_N)):
        for n in sizes:
            plan = misort.plan(n, kb)
            assert plan[0][0] == "tile_sort"
            if len(plan) == 1:
                shapes.add(("tile_only", 0))
            shapes.update((kind, r) for kind, _, r, _ in plan[1:])
    assert {("tile_only", 0), ("run_merge", 0), ("run_mergek", 2), ("run_mergek", 3), ("run_mergek", 4)} <= shapes


@pytest.mark.parametrize("kind,n,lead_out", SORT_OUT_CASES, ids=[f"{k}-{n}-out{ld}" for k, n, ld in SORT_OUT_CASES])
def test_local_sort_out_of_place_between_guards(ctx, kind, n, lead_out):
    """Input and output guarded with independent leads: every pair of the
    kind's leads (aligned and not)."""
    bits, want, c = sort_case(kind, n)
    for lead_in in LEADS[kind]:
        src = Band(kind, n, lead_in, c, bits)
        dst = Band(kind, n, lead_out, c)
        res = ctx.local_sort(src.view, dst.view)
        assert res is dst.view
        what = f"local_sort {kind} n={n} lead in={lead_in} out={lead_out}"
        assert_block(dst.block(), want, what)
        dst.assert_guards()
        src.assert_unchanged(what + ": the input")


@pytest.mark.parametrize("kind,n", SORT_CASES, ids=[f"{k}-{n}" for k, n in SORT_CASES])
def test_local_sort_in_place_between_guards(ctx, kind, n):
    bits, want, c = sort_case(kind, n)
    for lead in LEADS[kind]:
        blk = Band(kind, n, lead, c, bits)
        ctx.local_sort(blk.view)
        assert_block(blk.block(), want, f"local_sort in place {kind} n={n} lead={lead}")
        blk.assert_guards()


def test_local_sort_of_the_first_n_keys_only(ctx):
    """n smaller than the tensors: out[n:] and inp stay as they were."""
    n, cap = 40001, 40100
    bits, _, _ = sort_case("u32", cap)
    c = G.canary_for(bits)
    for lead in LEADS["u32"]:
        src = Band("u32", cap, lead, c, bits)
        dst = Band("u32", cap, 4 - lead if lead < 4 else lead, c)
        ctx.local_sort(src.view, dst.view, n=n)
        got = dst.block()
        assert_block(got[:n], np.sort(bits[:n]), f"local_sort n={n} of {cap}, lead {lead}")
        assert (got[n:] == c).all()
        dst.assert_guards()
        src.assert_unchanged("the input")


# ------------------------------------------------------- parallel_bitonic_sort

def filler(n, bits_dt, salt):
    """Keys for [loc, capacity): descending, so a sort that touched them shows."""
    return (np.arange(n, 0, -1).astype(np.uint64) * np.uint64(2654435761) + np.uint64(salt)).astype(bits_dt)


def parallel_keys(kind, n, seed):
    """(bit patterns, the same as the oracle's dtype)."""
    if kind == "f64":
        x = f64_finite(n, seed)
        return np.ascontiguousarray(x.view(np.uint64)), x
    x = B.sentinels_random(n, BITS[kind], seed)
    return x, x


@pytest.mark.parametrize("oop", [False, True], ids=["in_place", "out"])
@pytest.mark.parametrize("lead", ["aligned", 1])
@pytest.mark.parametrize("kind", KINDS)
def test_single_rank_block_in_a_larger_buffer(ctx, kind, lead, oop):
    """P = 1, loc_size < capacity: [loc, capacity) and the guards stay; with
    out= the input stays too."""
    loc, cap = (1 << 18) + 3, (1 << 18) + 3 + 1000
    lead = ALIGNED[kind] if lead == "aligned" else lead
    bits, x = parallel_keys(kind, loc, 9300)
    want = O.parallel_bitonic_sort(x, 1).view(BITS[kind])
    rest, rest_out = filler(cap - loc, BITS[kind], 1), filler(cap - loc, BITS[kind], 2)
    c = G.canary_for(bits, rest, rest_out)
    buf = Band(kind, cap, lead, c, np.concatenate([bits, rest]))
    out = Band(kind, cap, lead, c, np.concatenate([filler(loc, BITS[kind], 3) | BITS[kind](1), rest_out])) if oop else None
    res = ctx.parallel_bitonic_sort(buf.view, loc, loc, out=out.view if oop else None)
    assert res is (out.view if oop else buf.view)
    dst = out if oop else buf
    got = dst.block()
    assert_block(got[:loc], want, f"parallel_bitonic_sort P=1 {kind} lead={lead}")
    assert_block(got[loc:], rest_out if oop else rest, "[loc_size, capacity)")
    dst.assert_guards()
    if oop:
        buf.assert_unchanged("the input")
    assert ctx.check_sort(dst.view, loc) == O.check_sort(want.view(x.dtype), 1)


@pytest.mark.parametrize("oop", [False, True], ids=["in_place", "out"])
@pytest.mark.parametrize("lead", ["aligned", 1])
@pytest.mark.parametrize("kind", ["u32", "f64"])
@pytest.mark.parametrize("p", [2, 4])
def test_rank_group_blocks_between_guards(p, kind, lead, oop):
    """P = 2 and 4 (in-process group): every rank's buffer holds max_size + 64
    keys between guards; the blocks equal the oracle's, [loc, capacity) and
    the guards are intact, with out= the inputs are unchanged."""
    n = (1 << 18) + 3
    lead = ALIGNED[kind] if lead == "aligned" else lead
    bits, x = parallel_keys(kind, n, 9400 + p)
    want = O.parallel_bitonic_sort(x, p).view(BITS[kind])
    sizes = misort.block_sizes(n, p)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    max_size = n // p + 1
    cap = max_size + 64
    rests = [filler(cap - sizes[r], BITS[kind], 10 + r) for r in range(p)]
    c = G.canary_for(bits, *rests)

    def rank_fn(r, rctx):
        buf = Band(kind, cap, lead, c, np.concatenate([bits[offs[r]:offs[r + 1]], rests[r]]))
        out = Band(kind, cap, lead, c, np.concatenate([np.zeros(sizes[r], BITS[kind]), rests[r]])) if oop else None
        torch.cuda.synchronize()  # the sort runs on the context's own stream
        rctx.parallel_bitonic_sort(buf.view, sizes[r], max_size, out=out.view if oop else None,
                                   stream=rctx.native_stream)
        rctx.synchronize()
        return buf, out

    g = misort.Group(p)
    try:
        res = g.run(rank_fn)
    finally:
        g.close()
    for r, (buf, out) in enumerate(res):
        dst = out if oop else buf
        got = dst.block()
        assert_block(got[:sizes[r]], want[offs[r]:offs[r + 1]], f"rank {r} of {p}, {kind}, lead {lead}")
        assert_block(got[sizes[r]:], rests[r], f"rank {r}: [loc_size, capacity)")
        dst.assert_guards()
        if oop:
            buf.assert_unchanged(f"rank {r}: the input")


# --------------------------------------------------------------- compare_split

def split_keys(kind, n, seed):
    """A sorted block: (bit patterns, the oracle's array)."""
    if n == 0:
        return np.empty(0, BITS[kind]), np.empty(0, np.float64 if kind == "f64" else BITS[kind])
    if kind == "f64":
        x = O.local_sort(f64_finite(n, seed))
        return np.ascontiguousarray(x.view(np.uint64)), x
    x = np.sort(B.sentinels_random(n, BITS[kind], seed))
    return x, x


@pytest.mark.parametrize("lead_out", ["aligned", 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("keep_max", [0, 1])
@pytest.mark.parametrize("na,nb", [(1, 1), (5, 0), (2047, 2049), (2048, 2048), (2049, 1), (100000, 99999)])
def test_compare_split_between_guards(ctx, na, nb, keep_max, kind, lead_out):
    lead_out = ALIGNED[kind] if lead_out == "aligned" else lead_out
    abits, a = split_keys(kind, na, 9500 + na)
    bbits, b = split_keys(kind, nb, 9600 + nb)
    want = O.compare_split(a, b, keep_max).view(BITS[kind])
    c = G.canary_for(abits, bbits)
    for lead_in in (ALIGNED[kind], 1):
        da, db = Band(kind, na, lead_in, c, abits), Band(kind, nb, lead_in, c, bbits)
        out = Band(kind, na, lead_out, c)
        res = ctx.compare_split(da.view, db.view, keep_max, out=out.view)
        assert res is out.view
        what = f"compare_split {kind} ({na}, {nb}) keep_max={keep_max} lead in={lead_in} out={lead_out}"
        assert_block(out.block(), want, what)
        out.assert_guards()
        da.assert_unchanged(what + ": local")
        db.assert_unchanged(what + ": recv")


def tail_case(case, na, nb, keep_max, kd):
    """The keys of test_gpu_parity.test_merge_split_tail's cases `tail` (the
    partner's keys at the block's far end) and `wide` (they straddle all of it)."""
    big = 1 << 30 if kd == np.uint32 else 1 << 60
    a = O.local_sort((O.splitmix(na * 5 + 2, na, np.uint64) % big).astype(kd))
    r = O.splitmix(nb * 3 + 9, nb, np.uint64)
    if case == "tail":
        lo = int(a[max(0, na - 3 * nb)]) if not keep_max else 0
        hi = int(a[-1]) + 1000 if not keep_max else int(a[min(na - 1, 3 * nb)])
    else:
        lo, hi = 0, big
    return a, O.local_sort((lo + r % max(1, hi - lo)).astype(kd))


@pytest.mark.parametrize("lead", ["aligned", 1])
@pytest.mark.parametrize("kind", ["u32", "f64"])
@pytest.mark.parametrize("keep_max", [0, 1])
@pytest.mark.parametrize("na,nb", [(4097, 3), (100000, 4096)])
@pytest.mark.parametrize("case", ["tail", "wide"])
def test_merge_split_tail_between_guards(ctx, case, na, nb, keep_max, kind, lead):
    """The in-place compare-split on the guarded block itself: whatever window
    it rewrites, it stays inside the block, and recv is only read."""
    lead = ALIGNED[kind] if lead == "aligned" else lead
    a, b = tail_case(case, na, nb, keep_max, np.uint32 if kind == "u32" else np.float64)
    want = O.compare_split(a, b, keep_max).view(BITS[kind])
    abits, bbits = a.view(BITS[kind]), b.view(BITS[kind])
    c = G.canary_for(abits, bbits)
    blk, recv = Band(kind, na, lead, c, abits), Band(kind, nb, 1, c, bbits)
    res = ctx.compare_split(blk.view, recv.view, keep_max, out=blk.view, in_place_tail=True)
    assert res is blk.view
    assert_block(blk.block(), want, f"merge_split_tail {case} {kind} ({na}, {nb}) keep_max={keep_max} lead={lead}")
    blk.assert_guards()
    recv.assert_unchanged("recv")


# ---------------------------------------------------------------- codec decode

@pytest.mark.parametrize("lead", ["aligned", 1])
@pytest.mark.parametrize("kind", ["u32", "u64"])
@pytest.mark.parametrize("n", [1, 1023, 1025, 3 * 1024 + 17])
def test_codec_decode_between_guards(ctx, n, kind, lead):
    """k_codec_unpack stores 16-byte vectors where the destination is 16-byte
    aligned and single keys elsewhere (a view one key in; a block's ragged
    end): both sides of that branch, nothing past the n keys."""
    lead = ALIGNED[kind] if lead == "aligned" else lead
    x = np.sort(B.sentinels_random(n, BITS[kind], 9700 + n))
    c = G.canary_for(x)
    run = Band(kind, n, lead, c, x)
    dec = Band(kind, n, lead, c)
    torch.cuda.synchronize()  # the probe runs on the context's own stream
    ctx.codec_probe(run.view, dec.view, reps=1)
    assert_block(dec.block(), x, f"codec roundtrip {kind} n={n} lead={lead}")
    dec.assert_guards()
    run.assert_unchanged("the coded run")


# --------------------------------------------------------------------- overlap

@pytest.mark.parametrize("kind,n", [("u32", 40000), ("u64", 10000)])
def test_local_sort_refuses_partial_overlap(ctx, kind, n):
    bits, _, _ = sort_case(kind, 2 * n)
    for k in (1, n // 2, n - 1):
        d = to_dev(bits, kind)
        with pytest.raises(misort.MisortError) as e:
            ctx.local_sort(d[:n], d[k:k + n])
        assert e.value.code == -1
        assert_block(to_host(d), bits, f"k={k}: a refused call wrote")
    d = to_dev(bits, kind)
    ctx.local_sort(d[:n], d[0:n])  # k = 0: in place
    got = to_host(d)
    assert_block(got[:n], np.sort(bits[:n]), "in place")
    assert_block(got[n:], bits[n:], "past the block")


@pytest.mark.parametrize("kind", KINDS)
def test_compare_split_refuses_an_output_inside_its_inputs(ctx, kind):
    na, nb = 5000, 6000
    abits, _ = split_keys(kind, na + 8, 9800)
    bbits, _ = split_keys(kind, nb, 9801)
    for pick in ("local", "local+1", "recv", "recv+7"):
        da, db = to_dev(abits, kind), to_dev(bbits, kind)
        local, recv = da[:na], db
        out = {"local": local, "local+1": da[1:na + 1], "recv": db[:na], "recv+7": db[7:7 + na]}[pick]
        with pytest.raises(misort.MisortError) as e:
            ctx.compare_split(local, recv, 0, out=out)
        assert e.value.code == -1, pick
        assert_block(to_host(da), abits, f"{pick}: local")
        assert_block(to_host(db), bbits, f"{pick}: recv")


# --------------------------------------------------------------- Python checks

def test_wrapper_checks_raise_and_write_nothing(ctx):
    """The checks of sort_rows on every keys-only entry point: TypeError for a
    tensor of another dtype, ValueError for a strided or short one."""
    n = 1000
    bits, _, _ = sort_case("u32", n)
    sbits = np.sort(bits)
    held = []

    def dev(b, kind="u32"):
        t = to_dev(b, kind)
        held.append((t, np.ascontiguousarray(b)))
        return t

    x, srt, srt2 = dev(bits), dev(sbits), dev(sbits)
    wide = dev(np.concatenate([bits, bits]))
    out, short = dev(np.zeros(n, np.uint32)), dev(np.zeros(n - 1, np.uint32))
    out64 = dev(np.zeros(n, np.uint64), "u64")
    outf = dev(np.zeros(n, np.uint64), "f64")
    strided, strided_out = wide[::2], dev(np.zeros(2 * n, np.uint32))[::2]
    assert strided.numel() == n and not strided.is_contiguous()
    cases = [
        (TypeError, lambda: ctx.local_sort(x, out64)),
        (TypeError, lambda: ctx.local_sort(out64, outf)),
        (ValueError, lambda: ctx.local_sort(x, short)),
        (ValueError, lambda: ctx.local_sort(x, strided_out)),
        (ValueError, lambda: ctx.local_sort(strided, out)),
        (ValueError, lambda: ctx.local_sort(strided)),
        (ValueError, lambda: ctx.local_sort(x, out, n=n + 1)),
        (TypeError, lambda: ctx.parallel_bitonic_sort(x, n, n, out=out64)),
        (ValueError, lambda: ctx.parallel_bitonic_sort(x, n, n, out=short)),
        (ValueError, lambda: ctx.parallel_bitonic_sort(x, n, n, out=strided_out)),
        (ValueError, lambda: ctx.parallel_bitonic_sort(strided, n, n)),
        (ValueError, lambda: ctx.parallel_bitonic_sort(x, n + 1, n + 1)),
        (TypeError, lambda: ctx.compare_split(srt, out64, 0)),
        (TypeError, lambda: ctx.compare_split(srt, srt2, 0, out=out64)),
        (ValueError, lambda: ctx.compare_split(srt, srt2, 0, out=short)),
        (ValueError, lambda: ctx.compare_split(srt, srt2, 0, out=strided_out)),
        (ValueError, lambda: ctx.compare_split(strided, srt2, 0)),
        (ValueError, lambda: ctx.compare_split(srt, strided, 0)),
        (ValueError, lambda: ctx.compare_split(srt, srt2, 1, out=short, in_place_tail=True)),
        (ValueError, lambda: ctx.check_sort(strided)),
        (ValueError, lambda: ctx.check_sort(x, n + 1)),
        (TypeError, lambda: ctx.parallel_quick_sort(x, out=out64)),
        (ValueError, lambda: ctx.parallel_quick_sort(x, out=strided_out)),
        (ValueError, lambda: ctx.parallel_quick_sort(strided)),
        (ValueError, lambda: ctx.parallel_quick_sort(x, n + 1)),
        (TypeError, lambda: ctx.parallel_sample_sort(x, n, n, out=out64)),
        (ValueError, lambda: ctx.parallel_sample_sort(x, n, n, out=short)),
        (ValueError, lambda: ctx.parallel_sample_sort(x, n, n, out=strided_out)),
        (ValueError, lambda: ctx.parallel_sample_sort(strided, n, n)),
    ]
    for i, (exc, call) in enumerate(cases):
        with pytest.raises(exc):
            call()
        for t, was in held:
            assert_block(to_host(t), was, f"case {i}: a refused call wrote a tensor")


# ------------------------------------------------- other callers' arrays, misaligned

def test_quick_and_sample_sort_take_a_view_one_key_in(ctx):
    """Their local sort reads the caller's block too (SORT tile, vector loads)."""
    n = (1 << 16) + 3
    bits, want, c = sort_case("u32", n)
    src = Band("u32", n, 1, c, bits)
    out, cnt = ctx.parallel_quick_sort(src.view)
    assert cnt == n
    assert_block(to_host(out)[:n], want, "parallel_quick_sort, P = 1")
    src.assert_unchanged("the input")

    p = 2
    sizes = misort.block_sizes(n, p)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)

    def rank_fn(r, rctx):
        blk = Band("u32", int(sizes[r]), 1, c, bits[offs[r]:offs[r + 1]])
        dst = Band("u32", int(sizes[r]), 64, c)
        torch.cuda.synchronize()
        rctx.parallel_sample_sort(blk.view, sizes[r], n // p + 1, out=dst.view, stream=rctx.native_stream)
        rctx.synchronize()
        return blk, dst

    g = misort.Group(p)
    try:
        res = g.run(rank_fn)
    finally:
        g.close()
    assert_block(np.concatenate([dst.block() for _, dst in res]), want, "parallel_sample_sort, P = 2")
    for blk, dst in res:
        dst.assert_guards()
        blk.assert_unchanged("the input")


# ------------------------------------------------------------------ check_sort

CHECK_N = (1 << 20) + 3  # more than the counting kernel's 2048 x 256 grid stride
DESCENTS = (0, 62, 63, 64, 255, 256, 524287, 524288, CHECK_N - 2)  # lane, wave, workgroup, grid stride, end


def with_descents(n, positions, dt):
    """arange(n) with a[i] > a[i+1] exactly at `positions`: every maximal
    stretch of consecutive positions i..j has keys i..j+1 reversed."""
    a = np.arange(n, dtype=np.int64)
    pos = sorted(positions)
    k = 0
    while k < len(pos):
        j = k
        while j + 1 < len(pos) and pos[j + 1] == pos[j] + 1:
            j += 1
        a[pos[k]:pos[j] + 2] = a[pos[k]:pos[j] + 2][::-1].copy()
        k = j + 1
    assert np.flatnonzero(a[:-1] > a[1:]).tolist() == pos
    return a.astype(dt)


@pytest.mark.parametrize("kind", KINDS)
def test_check_sort_counts_each_descent_once(ctx, kind):
    dt = {"u32": np.uint32, "u64": np.uint64, "f64": np.float64}[kind]
    n = CHECK_N
    assert n > 2048 * 256

    def count(a, lead=0):
        want = int(np.count_nonzero(a[:-1] > a[1:]))
        bits = np.ascontiguousarray(a).view(BITS[kind])
        d = to_dev(np.concatenate([np.zeros(lead, BITS[kind]), bits]), kind)[lead:]
        return ctx.check_sort(d), want

    got, want = count(np.arange(n).astype(dt))
    assert (got, want) == (0, 0)
    for i in DESCENTS:
        got, want = count(with_descents(n, [i], dt))
        assert want == 1 and got == 1, f"one descent at {i}: counted {got}"
    for lead in (0, 1):  # lead 1: a view that is not 16-byte aligned
        got, want = count(with_descents(n, DESCENTS, dt), lead)
        assert want == len(DESCENTS) and got == want, f"descents at {DESCENTS}: counted {got}"
    got, want = count(np.arange(n)[::-1].astype(dt))
    assert want == n - 1 and got == want
    if kind == "f64":
        # a NaN is greater than nothing and nothing is greater than it
        a = with_descents(n, DESCENTS, dt)
        a[100] = np.nan        # between ascending keys: no descent
        a[524289] = np.nan     # the smaller side of the descent at 524288: it no longer counts
        a[256] = -np.nan       # the greater side of the descent at 256 (and the smaller of 255)
        got, want = count(a)
        assert want == len(DESCENTS) - 3 and got == want


@pytest.mark.parametrize("kind", KINDS)
def test_check_sort_of_tiny_blocks(ctx, kind):
    dt = {"u32": np.uint32, "u64": np.uint64, "f64": np.float64}[kind]
    for keys, want in (([], 0), ([7], 0), ([1, 2], 0), ([2, 2], 0), ([2, 1], 1)):
        d = to_dev(np.array(keys, dtype=dt).view(BITS[kind]), kind)
        assert ctx.check_sort(d) == want, keys
