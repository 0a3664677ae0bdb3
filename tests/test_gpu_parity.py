"""GPU parity: the HIP path (libmisort.so through its C-ABI) against the CPU
oracle (oracle/oracle.c, itself pinned to the reference by golden fixtures).

Bar: bit-exact for every key type.  Sizes the oracle finishes in seconds are
compared element for element; here the BASELINE-sized runs (2^28, 2^30 u32) of
misort_local_sort are also checked through size-independent properties
(sorted, same multiset by sum / sum-of-squares modulo 2^64 and an exact
2^16-bucket histogram of the top bits); their bit-exact SHA-256 checks are in
test_gpu_baseline_configs.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")
import misort  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD_DIR, "golden.json")) as f:
    GOLD = json.load(f)["cases"]

U32_T = torch.uint32 if hasattr(torch, "uint32") else torch.int32
U64_T = torch.uint64 if hasattr(torch, "uint64") else torch.int64


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = misort.Context(0)
    yield c
    c.close()


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda().view(U32_T)
    if a.dtype == np.uint64:
        return torch.from_numpy(a.view(np.int64)).cuda().view(U64_T)
    return torch.from_numpy(a).cuda()


def to_host(t, dtype):
    torch.cuda.synchronize()
    if dtype == np.uint32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    if dtype == np.uint64:
        return t.view(torch.int64).cpu().numpy().view(np.uint64)
    return t.cpu().numpy()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def mixed_u64(n, seed):
    """Duplicate-heavy / skewed / sentinel-colliding u64 mix (BASELINE config 5)."""
    rng = np.random.default_rng(seed)
    parts = [rng.integers(0, 2**63, size=1024, dtype=np.uint64)[rng.integers(0, 1024, int(n * .4))],
             O.generate_f64(max(int(n * .3), 1)).view(np.uint64)[: int(n * .3)],
             rng.integers(0, 2**64 - 1, size=int(n * .2), dtype=np.uint64),
             np.zeros(int(n * .05), dtype=np.uint64)]
    parts.append(np.full(n - sum(p.size for p in parts), 2**64 - 1, dtype=np.uint64))
    k = np.concatenate(parts)
    rng.shuffle(k)
    return k


U32_SIZES = [1, 2, 3, 31, 32, 33, 127, 1000, 4095, 16383, 16384, 16385, 65537, 131072,
             1 << 20, (1 << 20) + 12345, 3 * (1 << 21) + 7, 1 << 24]


@pytest.mark.parametrize("n", U32_SIZES)
def test_local_sort_u32(ctx, n):
    x = O.splitmix(0x5EED0001 + n, n, np.uint32)
    d_in = to_dev(x)
    d_out = torch.empty_like(d_in)
    ctx.local_sort(d_in, d_out)
    got = to_host(d_out, np.uint32)
    np.testing.assert_array_equal(got, O.local_sort(x))
    np.testing.assert_array_equal(to_host(d_in, np.uint32), x)  # input untouched


@pytest.mark.parametrize("n", [1, 5, 8191, 8192, 8193, 40000, 1 << 18, (1 << 20) + 3, 5 << 20])
def test_local_sort_u64_mixed(ctx, n):
    x = mixed_u64(n, n)
    d = to_dev(x)
    ctx.local_sort(d)  # in place
    np.testing.assert_array_equal(to_host(d, np.uint64), O.local_sort(x))


@pytest.mark.parametrize("n", [13, 1031, 65537, 1000003])
def test_local_sort_f64(ctx, n):
    x = O.generate_f64(n)  # psort.cc generator: non-negative doubles
    rng = np.random.default_rng(n)
    y = np.concatenate([x, -x[: n // 3] * rng.random(n // 3), [np.inf, -np.inf, 1e308, -1e-308]])
    d = to_dev(y)
    out = torch.empty_like(d)
    ctx.local_sort(d, out)
    np.testing.assert_array_equal(to_host(out, np.float64).view(np.uint64),
                                  O.local_sort(y).view(np.uint64))


def test_local_sort_all_equal_and_presorted(ctx):
    for x in [np.full(100003, 7, np.uint32), np.arange(1 << 20, dtype=np.uint32),
              np.arange(1 << 20, dtype=np.uint32)[::-1].copy(),
              np.full(70001, 0xFFFFFFFF, np.uint32)]:
        d = to_dev(x)
        ctx.local_sort(d)
        np.testing.assert_array_equal(to_host(d, np.uint32), np.sort(x))


@pytest.mark.parametrize("na,nb", [(1, 1), (5, 0), (0, 5), (1000, 1001), (4096, 4095),
                                   (100000, 99999), (65536, 65536), (123457, 3)])
@pytest.mark.parametrize("keep_max", [0, 1])
def test_merge_split(ctx, na, nb, keep_max):
    a = O.local_sort(O.splitmix(na * 7 + 1, na, np.uint32) % 5000)  # duplicates
    b = O.local_sort(O.splitmix(nb * 11 + 3, nb, np.uint32) % 5000)
    want = O.compare_split(a, b, keep_max)
    out = ctx.compare_split(to_dev(a), to_dev(b), keep_max)
    np.testing.assert_array_equal(to_host(out, np.uint32), want)


@pytest.mark.parametrize("case", ["tail", "head", "overlap", "dups", "wide"])
@pytest.mark.parametrize("na,nb", [(1, 1), (4097, 3), (100000, 4096), (1 << 20, 777)])
@pytest.mark.parametrize("keep_max", [0, 1])
@pytest.mark.parametrize("kd", [np.uint32, np.uint64, np.float64])
def test_merge_split_tail(ctx, case, na, nb, keep_max, kd):
    """The in-place compare-split of a small bracket (merge_split_tail: only
    the end of the block the partner's keys reach is rewritten) against the
    oracle's keep-n merge (psort.cc:116-164).  The partner's keys sit at the
    block's far end (tail: the usual small-bracket stage), straddle all of it
    (wide: the window is the whole block), duplicate its boundary keys, or
    overlap its middle."""
    big = 1 << 30 if kd == np.uint32 else 1 << 60
    a = O.local_sort((O.splitmix(na * 5 + 2, na, np.uint64) % big).astype(kd))
    r = O.splitmix(nb * 3 + 9, nb, np.uint64)
    if case == "tail":  # keep-min receives keys above most of a; keep-max, below most of it
        lo = int(a[max(0, na - 3 * nb)]) if not keep_max else 0
        hi = int(a[-1]) + 1000 if not keep_max else int(a[min(na - 1, 3 * nb)])
    elif case == "head":  # the other end: the window is (nearly) the whole block
        lo, hi = (0, int(a[min(na - 1, 2)]) + 1) if not keep_max else (int(a[max(0, na - 3)]), big)
    elif case == "wide":
        lo, hi = 0, big
    elif case == "overlap":
        lo, hi = int(a[na // 3]), int(a[(2 * na) // 3]) + 1
    else:  # dups: b repeats a's keys at the boundary
        idx = (r % max(1, min(na, 8))).astype(np.int64)
        b = O.local_sort(a[(na - 1 - idx) if not keep_max else idx].astype(kd))
        lo = hi = None
    if lo is not None:
        b = O.local_sort((lo + r % max(1, hi - lo)).astype(kd))
    want = O.compare_split(a, b, keep_max)
    out = ctx.compare_split(to_dev(a), to_dev(b), keep_max, in_place_tail=True)
    np.testing.assert_array_equal(to_host(out, kd).view(np.uint64 if kd == np.float64 else kd),
                                  want.view(np.uint64 if kd == np.float64 else kd))


@pytest.mark.parametrize("keep_max", [0, 1])
@pytest.mark.parametrize("kd", [np.uint32, np.float64])
def test_merge_split_tail_on_another_stream(ctx, kd, keep_max):
    """compare_split(in_place_tail=True, stream=s): the copy of `local` into
    `out` and the merge are ordered, whatever torch's current stream is doing
    (the copy once ran there and the merge on s, unordered; both now run on
    s: tests/test_gpu_stream_order.py has the case with work pending on s).
    The current stream is kept busy (a 2^26-key sort queued just
    before the call), so a merge that does not wait for a copy behind that sort
    reads `out` before the copy lands.  `out` starts as zeros -- a sorted block,
    so the kernels' preconditions hold whatever they read -- and the late copy
    then overwrites the merge's result: the output differs from the oracle's."""
    na, nb = 100000, 4096
    a = O.local_sort((1 + O.splitmix(na * 5 + 2, na, np.uint64) % (1 << 30)).astype(kd))
    b = O.local_sort((1 + O.splitmix(nb * 3 + 9, nb, np.uint64) % (1 << 30)).astype(kd))
    want = O.compare_split(a, b, keep_max)
    assert not np.array_equal(want, a)  # the merge changes the block
    iv = np.uint64 if kd == np.float64 else kd
    d_a, d_b = to_dev(a), to_dev(b)
    # the context's scratch buffers grow on first use, and growing them waits
    # for the device: one call on the current stream first
    warm = ctx.compare_split(d_a, d_b, keep_max, in_place_tail=True)
    np.testing.assert_array_equal(to_host(warm, kd).view(iv), want.view(iv))
    out = to_dev(np.zeros_like(a))
    busy = torch.randint(0, 1 << 30, (1 << 26,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    busy.sort()
    ctx.compare_split(d_a, d_b, keep_max, out=out, stream=ctx.native_stream, in_place_tail=True)
    ctx.synchronize()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(to_host(out, kd).view(iv), want.view(iv))
    np.testing.assert_array_equal(to_host(d_a, kd).view(iv), a.view(iv))


@pytest.mark.parametrize("keep_max", [0, 1])
def test_merge_split_f64(ctx, keep_max):
    a = O.local_sort(O.generate_f64(5001))
    b = O.local_sort(O.generate_f64(4999) * 0.5)
    want = O.compare_split(a, b, keep_max)
    out = ctx.compare_split(to_dev(a), to_dev(b), keep_max)
    np.testing.assert_array_equal(to_host(out, np.float64).view(np.uint64), want.view(np.uint64))


def virtual_ranks(ctx, x, p):
    """psort.cc:167-201 with P virtual ranks on one GPU: the device local sort
    and device merge-split of the multi-GPU path, the exchange replaced by
    indexing (the RCCL leg is exercised by bench/psort at N>1)."""
    sizes = misort.block_sizes(x.size, p)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    blocks = [to_dev(x[offs[r]:offs[r + 1]]) for r in range(p)]
    for b in blocks:
        ctx.local_sort(b)
    sched = [misort.schedule(p, r) for r in range(p)]
    for st in range(len(sched[0])):
        blocks = [ctx.compare_split(blocks[r], blocks[sched[r][st][0]], sched[r][st][1])
                  for r in range(p)]
    return np.concatenate([to_host(b, x.dtype) for b in blocks])


PSORT = [c for c in GOLD if c["mode"] == "psort" and c.get("algo", "bitonic") == "bitonic"]
KEYS = [c for c in GOLD if c["mode"] == "keys" and c.get("algo", "bitonic") == "bitonic"]


@pytest.mark.parametrize("case", PSORT, ids=lambda c: f"N{c['n']}_P{c['p']}")
def test_golden_psort(ctx, case):
    x = O.generate_f64(case["n"])
    y = virtual_ranks(ctx, x, case["p"])
    assert sha(y) == case["out_sha256"]
    assert O.check_sort(y, case["p"]) == case["errors"]


@pytest.mark.parametrize("case", KEYS, ids=lambda c: f"{c['name']}_P{c['p']}")
def test_golden_keys(ctx, case):
    if case["dtype"] == "u32":
        x = O.splitmix(0x5EED0001, case["n"], np.uint32)
    else:
        x = np.fromfile(os.path.join(GOLD_DIR, f"keys_{case['name']}.in"), dtype=np.uint64)
    y = virtual_ranks(ctx, x, case["p"])
    assert sha(y) == case["out_sha256"]


@pytest.mark.parametrize("p", [2, 4, 8])
def test_uneven_u64_sentinel_collisions(ctx, p):
    # BASELINE config 5 shape at test scale: N % P != 0, all-ones keys present.
    n = (1 << 18) - 3
    x = mixed_u64(n, 5)
    np.testing.assert_array_equal(virtual_ranks(ctx, x, p), O.parallel_bitonic_sort(x, p))


def test_parallel_sort_single_rank_and_check(ctx):
    x = O.generate_f64(1031)
    d = to_dev(x)
    ctx.parallel_bitonic_sort(d, 1031, 1031)
    y = to_host(d, np.float64)
    np.testing.assert_array_equal(y.view(np.uint64), O.parallel_bitonic_sort(x, 1).view(np.uint64))
    assert ctx.check_sort(d) == 0
    assert ctx.check_sort(to_dev(x)) == O.check_sort(x, 1)


def test_sort_host_pinned(ctx):
    x = O.splitmix(99, 3000017, np.uint32)
    np.testing.assert_array_equal(ctx.sort_host(x), np.sort(x))


def test_fill_splitmix_matches_oracle(ctx):
    d = torch.empty(100003, dtype=U32_T, device="cuda")
    ctx.fill_splitmix(d, 0x5EED0003, g0=12345)
    np.testing.assert_array_equal(to_host(d, np.uint32), O.splitmix(0x5EED0003, 100003, np.uint32, 12345))


def _multiset_props(t):
    """Order-independent fingerprint of a u32 tensor (exact, int64 arithmetic)."""
    v = t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    hist = torch.bincount((v >> 16).to(torch.int64), minlength=65536)
    return int(v.sum()), int((v * v).sum()), hist.cpu()  # (v*v).sum() wraps mod 2^64


@pytest.mark.parametrize("logn", [28, 30])
def test_baseline_size_u32(ctx, logn):
    n = 1 << logn
    d_in = torch.empty(n, dtype=U32_T, device="cuda")
    ctx.fill_splitmix(d_in, 0x5EED0002 if logn == 28 else 0x5EED0003)
    d_out = torch.empty_like(d_in)
    ctx.local_sort(d_in, d_out)
    torch.cuda.synchronize()
    assert ctx.check_sort(d_out) == 0
    s_in, q_in, h_in = _multiset_props(d_in)
    s_out, q_out, h_out = _multiset_props(d_out)
    assert (s_in, q_in) == (s_out, q_out)
    assert torch.equal(h_in, h_out)
    # the bit-exact (SHA-256) checks of these sizes against the reference-pinned
    # fixtures are in test_gpu_baseline_configs.py


def _multiset_props64(t):
    """Order-independent fingerprint of a u64 tensor: sum, sum of squares (both
    mod 2^64), xor of all keys, 2^16-bucket histogram of the top bits."""
    v = t.view(torch.int64)
    x = v.clone()
    while x.numel() > 1:  # xor-reduce by halves (no torch xor reduction)
        h = x.numel() // 2
        y = x[:h] ^ x[h:2 * h]
        x = torch.cat([y, x[2 * h:]]) if x.numel() % 2 else y
    hist = torch.bincount(((v >> 48) & 0xFFFF).to(torch.int64), minlength=65536)
    return int(v.sum()), int((v * v).sum()), int(x[0]), hist.cpu()


def test_past_the_multiway_limit_u32(ctx):
    """2^31 - 3 u32 keys: four multi-way passes end at runs of 2^30 (32-bit row
    offsets), one 2-way pass merges the last level; ragged tail."""
    n = (1 << 31) - 3
    plan = misort.plan(n, 4)
    assert [p[0] for p in plan][-2:] == ["run_mergek", "run_merge"]
    d_in = torch.empty(n, dtype=U32_T, device="cuda")
    ctx.fill_splitmix(d_in, 0x5EED0031)
    d_out = torch.empty_like(d_in)
    ctx.local_sort(d_in, d_out)
    torch.cuda.synchronize()
    assert ctx.check_sort(d_out) == 0
    a, b = _multiset_props(d_in), _multiset_props(d_out)
    assert a[:2] == b[:2] and torch.equal(a[2], b[2])


def test_past_the_multiway_limit_u64(ctx):
    """2^30 + 5 u64 keys: four 16-way passes end at runs of 2^29, two 2-way
    passes follow; ragged tail."""
    n = (1 << 30) + 5
    plan = misort.plan(n, 8)
    assert [p[0] for p in plan][-3:] == ["run_mergek", "run_merge", "run_merge"]
    d_in = torch.empty(n, dtype=U64_T, device="cuda")
    ctx.fill_splitmix(d_in, 0x5EED0064)
    d_out = torch.empty_like(d_in)
    ctx.local_sort(d_in, d_out)
    torch.cuda.synchronize()
    assert ctx.check_sort(d_out) == 0
    a, b = _multiset_props64(d_in), _multiset_props64(d_out)
    assert a[:3] == b[:3] and torch.equal(a[3], b[3])


F64Z = json.load(open(os.path.join(GOLD_DIR, "f64zero.json")))["cases"]


@pytest.mark.parametrize("case", F64Z, ids=lambda c: f"P{c['p']}")
def test_f64_signed_zeros_vs_reference(ctx, case):
    """-0.0 / +0.0 mixtures against the compiled reference's own output
    (tests/golden/make_golden_f64zero.py: parallel_bitonic_sort, psort.cc:167-201,
    at P = 1, 2, 4, 8 on the same 4002 doubles).  The reference writes its 1000
    zeros in an implementation-defined sign order (std::sort and the strict
    '<'/'>' merges, psort.cc:128-137,153-162: 487-515 sign changes across P);
    this build sorts by the order-preserving u64 map (-0.0 before +0.0 within a
    rank's block, include/misort.h).  Pinned against the reference: every
    position equal as a double, every non-zero position bit-exact, the same
    per-rank sizes and check_sort count, and the output a permutation of the
    input's bit patterns.  The measured deviation (zero positions whose sign
    differs) is reported, not asserted to be zero."""
    x = np.fromfile(os.path.join(GOLD_DIR, "f64zero.in"))
    ref = np.fromfile(os.path.join(GOLD_DIR, f"f64zero_P{case['p']}.out"))
    assert sha(ref) == case["out_sha256"]
    y = virtual_ranks(ctx, x, case["p"])
    assert np.array_equal(y, ref)  # as doubles: -0.0 == +0.0
    nz = ref != 0
    np.testing.assert_array_equal(y.view(np.uint64)[nz], ref.view(np.uint64)[nz])
    np.testing.assert_array_equal(np.sort(y.view(np.uint64)), np.sort(x.view(np.uint64)))
    assert O.check_sort(y, case["p"]) == case["errors"]
    sizes = misort.block_sizes(x.size, case["p"])
    assert list(sizes) == case["sizes"]
    # within each rank's block this build's zeros are -0.0 first
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for r in range(case["p"]):
        z = np.signbit(y[offs[r]:offs[r + 1]][y[offs[r]:offs[r + 1]] == 0])
        assert np.all(z[:z.sum()]) and not np.any(z[z.sum():])
    differ = int(np.count_nonzero(y.view(np.uint64) != ref.view(np.uint64)))
    print(f"P={case['p']}: {differ} of {case['zeros']} zero positions differ in sign from the reference")
