"""The numpy model of the K-way merge pass's chunking (runsk.hip) and the key
families that drive it to its edges.  A helper, not a test module:
test_runsk_model.py, test_merge_battery.py (CPU) and test_gpu_merge_battery.py
import it.

The kernels' constants and the pass plan come from the library's own host code
(csrc/mergek_plan.h), printed by lib/mergek_plan_dump (built by the default
make target): nothing here is a literal copy.  The rules modelled: fences every
FG keys of each run, ordered by the total order (key, run, position / FG) --
for u32 and u64 keys alike, as three arrays sorted by np.lexsort, not as a
packed word -- the group's fences merged; every fm-th one starts a chunk whose
start in each run is that run's count of keys before the fence (found as
k_bounds finds it: the run's fences before it, then window_bound's guess,
gallop and binary search between two of them); chunks are then merged
independently.  With the capacity split a chunk over CAP is cut at its middle
merged fence.  FG = 2^fgl is the build's fence stride (7, or 6 for
runsk_fg6.hip); K = 2^lk, lk = 1..4.

The families (FAMILIES, battery): every function takes (dtype, lw, lk, n, fm,
FG) and returns {variant: keys}, every run of 2^lw keys ascending.  For u64
each pattern comes three ways: in the high word over a constant low word, in
the low word under a constant high word, and spread over both words."""
import functools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, "parallel-computing-mpi_amd", "lib", "mergek_plan_dump")
ASAN_DUMP = os.path.join(ROOT, "build", "asan", "mergek_plan_dump")


def run_dump(args, knobs=None, exe=DUMP):
    """The dump program's JSON lines for `args`; knobs = the MISORT_* settings it
    sees (this process's own are not passed on; the rest of the environment is)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MISORT_")}
    env.update(knobs or {})
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (args, knobs, r.returncode, r.stderr[-2000:])
    return [json.loads(line) for line in r.stdout.splitlines()]


@functools.lru_cache(maxsize=None)
def shape(lk, key_bytes=4, fgl=7):
    """Shape<KEY, lk> and KTr<KEY> of the build with 2^fgl-key fences."""
    return run_dump([key_bytes, lk, fgl])[0]


def plans(ns, lw, lk, key_bytes=4, fgl=7, depth=0, knobs=None, exe=DUMP):
    """plan_pass<KEY, lk>(n, lw, depth) for every n of ns."""
    out = run_dump([",".join(map(str, ns)), lw, lk, key_bytes, fgl, depth], knobs, exe)
    assert len(out) == len(ns) and all(p["ok"] for p in out)
    return out


FG_LOG2 = shape(1)["FG_LOG2"]  # the default build
FG = 1 << FG_LOG2


def fences(x, lw, lk, n, fgl=FG_LOG2):
    """Every 2^fgl-th key with its run in the group and its position / FG: the
    three fields of the total order, as (key, run, j) arrays."""
    p = np.arange(0, n, 1 << fgl, dtype=np.int64)
    r = (p >> lw) & ((1 << lk) - 1)
    j = (p & ((1 << lw) - 1)) >> fgl
    return x[p].astype(np.uint64), r, j


def chunk_bounds(x, lw, lk, g, F, fm, fgl=FG_LOG2):
    """Start of every chunk of group g in each run (+ the end slot), as k_bounds;
    bound_at(i, log): the same for the group's i-th merged fence (k_split_desc),
    its window searches appended to log; and the searches of every chunk start."""
    K = 1 << lk
    n, W = x.size, 1 << lw
    base = g << (lw + lk)
    lens = [max(0, min(W, n - base - r * W)) for r in range(K)]
    f0, f1 = base >> fgl, (min(n, base + K * W) + (1 << fgl) - 1) >> fgl
    Fk, Fr, Fj = (a[f0:f1] for a in F)
    order = np.lexsort((Fj, Fr, Fk))  # (key, run, position): the merged fences
    Mk, Mr, Mj = Fk[order], Fr[order], Fj[order]
    runs = [x[base + r * W: base + r * W + lens[r]] for r in range(K)]
    # run r's own fence keys, in position order
    frs = [F[0][(base + r * W) >> fgl: ((base + r * W) >> fgl) + ((lens[r] + (1 << fgl) - 1) >> fgl)] for r in range(K)]

    def bound_at(i, log=None):
        v, r0, j0 = int(Mk[i]), int(Mr[i]), int(Mj[i])
        st = []
        for r in range(K):
            if r == r0:
                st.append(j0 << fgl)
                continue
            side = "right" if r < r0 else "left"  # ties go to the lower run
            want = int(np.searchsorted(runs[r], x.dtype.type(v), side=side))
            st.append(want)
            if lens[r] == 0:
                continue
            # k_bounds' two-stage search: fences of run r before f, then the
            # FG positions between two of them
            lo = int(np.searchsorted(frs[r], np.uint64(v), side=side))
            got = 0 if lo == 0 else refine(runs[r], frs[r], lo, lens[r], v, r < r0, fgl, log)
            assert got == want
        return st

    logs = []
    out = []
    for t in range(0, (f1 - f0 + fm - 1) // fm):
        logs.append([])
        out.append(bound_at(t * fm, logs[-1]))
    out.append(lens)
    return out, lens, bound_at, f1 - f0, logs


def interp(run, v, ka, kb, a, b):
    """window_bound's guess: integer for u32 keys, in doubles for u64."""
    if run.dtype.itemsize == 4:
        return a + ((v - ka) * (b - a)) // (kb - ka)
    return a + int(float(v - ka) / float(kb - ka) * float(b - a))


def refine(run, fr, lo, ln, v, le, fgl=FG_LOG2, log=None):
    """k_bounds' window search: the first position in [a, b] whose key is not
    before the fence (key > v if le, key >= v otherwise), guessed by
    interpolating v between the window's fence keys, bracketed by galloping
    from the guess, then binary-searched.  fr: the run's fence keys.  log gets
    one record per search: the branch taken and the gallop's probes."""
    vk = run.dtype.type(v)  # compared as a key; v itself stays a Python int for the guess

    def before(q):
        return run[q] <= vk if le else run[q] < vk
    a, b = ((lo - 1) << fgl) + 1, min(lo << fgl, ln)
    ka = int(fr[lo - 1])
    p = a + ((b - a) >> 1)
    rec = {"last": not (lo << fgl) < ln, "eq": False, "inner": False, "fwd": 0, "bwd": 0}
    if (lo << fgl) < ln:
        kb = int(fr[lo])
        rec["eq"], rec["inner"] = kb == ka, ka < v < kb
        if kb > ka:
            p = interp(run, v, ka, kb, a, b)
    p = min(max(p, a), b)
    if p < b and before(p):
        lo_b, hi_b, step = p + 1, b, 4
        while lo_b + step - 1 < hi_b:
            x = lo_b + step - 1
            rec["fwd"] += 1
            if before(x):
                lo_b, step = x + 1, step * 2
            else:
                hi_b = x
                break
    else:
        lo_b, hi_b, step = a, p, 4
        while hi_b - step >= lo_b:
            x = hi_b - step
            rec["bwd"] += 1
            if not before(x):
                hi_b, step = x, step * 2
            else:
                lo_b = x + 1
                break
    while lo_b < hi_b:
        mid = (lo_b + hi_b) >> 1
        if before(mid):
            lo_b = mid + 1
        else:
            hi_b = mid
    rec["at_a"], rec["at_b"] = lo_b == a, lo_b == b
    if log is not None:
        log.append(rec)
    return lo_b


def group_pieces(x, lw, lk, fm, g, F, split, fgl=FG_LOG2):
    """Group g's chunks as k_mergek runs them: (t, half, a, b, searches) with a, b
    the bounds in each run, half = None (a whole chunk) or 0 / 1 (a cut chunk's
    halves) and searches the window searches of the piece's start fence.  Also
    the bounds, the run lengths and the group's fence count."""
    S = shape(lk, x.dtype.itemsize, fgl)
    bounds, lens, bound_at, nfg, logs = chunk_bounds(x, lw, lk, g, F, fm, fgl)
    pieces = []
    for t, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        size = sum(b[r] - a[r] for r in range(S["K"]))
        if split and size > S["CAP"]:
            mid = min(fm, nfg - t * fm) // 2
            assert mid > 0
            mlog = []
            m = bound_at(t * fm + mid, mlog)
            pieces += [(t, 0, a, m, logs[t]), (t, 1, m, b, mlog)]
        else:
            pieces.append((t, None, a, b, logs[t]))
    return pieces, bounds, lens, nfg


def check_groups(x, lw, lk, fm, groups, split, fgl=FG_LOG2):
    """The chunking invariants on the given groups of x, cut every fm merged
    fences; split: a chunk over CAP is cut at its middle merged fence into two
    (k_chunk_desc lists it, k_split_desc cuts it) and each half must fit.
    Returns the number of chunks cut."""
    S = shape(lk, x.dtype.itemsize, fgl)
    K, CAP, RW, NROWS = S["K"], S["CAP"], S["RW"], S["NROWS"]
    n, W = x.size, 1 << lw
    F = fences(x, lw, lk, n, fgl)
    kf = ((K * W >> fgl) + fm - 1) // fm
    ncut = 0
    for g in groups:
        pieces, bounds, lens, nfg = group_pieces(x, lw, lk, fm, g, F, split, fgl)
        if (g + 1) * K * W <= n:
            assert len(bounds) - 1 == kf
        base = g << (lw + lk)
        merged = []
        prev_max = None
        assert bounds[0] == [0] * K
        ncut += sum(1 for p in pieces if p[1] == 0)
        for _, _, a, b, _ in pieces:
            seg = [x[base + r * W + a[r]: base + r * W + b[r]] for r in range(K)]
            size = sum(s.size for s in seg)
            assert all(0 <= a[r] <= b[r] <= lens[r] for r in range(K)) and size <= CAP
            # load rows: each row of RW keys inside one segment, NROWS per chunk
            assert sum(-(-s.size // RW) for s in seg) <= NROWS
            chunk = np.sort(np.concatenate(seg))
            if chunk.size and prev_max is not None:
                assert chunk[0] >= prev_max
            if chunk.size:
                prev_max = chunk[-1]
            merged.append(chunk)
        want = np.sort(x[base: base + sum(lens)])
        np.testing.assert_array_equal(np.concatenate(merged), want)
    return ncut


def chunk_stats(x, lw, lk, fm, split, fgl=FG_LOG2):
    """One record per chunk, or per half of a cut chunk, of every group of x:
    group, t, half (None / 0 / 1), size (keys), seg (the K segment lengths),
    rows (load rows used), cut and halves (both halves' sizes, on each half of a
    cut chunk), and searches: refine's record of every window search of the
    piece's start fence -- eq (ka == kb), last (the run's last window: no kb),
    at_a / at_b (the answer at the window's first / last position) and fwd /
    bwd (the probes of the forward / backward gallop)."""
    S = shape(lk, x.dtype.itemsize, fgl)
    K, RW = S["K"], S["RW"]
    n = x.size
    F = fences(x, lw, lk, n, fgl)
    out = []
    for g in range((n + (K << lw) - 1) // (K << lw)):
        pieces = group_pieces(x, lw, lk, fm, g, F, split, fgl)[0]
        for i, (t, half, a, b, log) in enumerate(pieces):
            seg = [b[r] - a[r] for r in range(K)]
            rec = {"group": g, "t": t, "half": half, "size": sum(seg), "seg": seg,
                   "rows": sum(-(-s // RW) for s in seg), "cut": half is not None, "halves": None, "searches": log}
            if half is not None:
                o = pieces[i + 1 - 2 * half]
                other = sum(o[3][r] - o[2][r] for r in range(K))
                rec["halves"] = (rec["size"], other) if half == 0 else (other, rec["size"])
            out.append(rec)
    return out


# ---------------------------------------------------------------- the families

def make_keys(kind, n, lw, lk, seed, fm=0, dtype=np.uint32, fg=FG):
    """The families the GPU suite had before the battery (uniform, dup, equal,
    interleaved) and "clumped", as one array each."""
    K, W = 1 << lk, 1 << lw
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    if kind == "uniform":
        x = rng.integers(0, top, n, dtype=np.uint64, endpoint=True).astype(dtype)
    elif kind == "dup":
        x = rng.integers(0, 7, n).astype(dtype)
    elif kind == "equal":
        x = np.full(n, top, dtype)
    elif kind == "interleaved":
        x = (np.arange(n) % K * 1000 + np.arange(n) // K).astype(dtype)
    else:
        # "clumped" (for chunks cut every fm fences): after a prefix of zeros, every
        # run repeats a period of c + 1 fences, c = ceil(fm / K) -- one key 2m + 1,
        # then (c + 1) FG - 1 keys 2m + 2 holding c fences.  The prefixes hold
        # fm - K fences in all, so the group's chunk 1 starts at run 0's first
        # fence of the first clump and takes nearly that whole clump from every
        # run: its window offsets add up instead of cancelling, and it exceeds CAP.
        c, i = -(-fm // K), np.arange(n)
        r, pos = (i >> lw) & (K - 1), i & (W - 1)
        q = pos - ((fm - K) // K + (r < (fm - K) % K)) * fg
        per = (c + 1) * fg
        x = np.where(q < 0, 0, 1 + 2 * (q // per) + (q % per != 0)).astype(dtype)
    for s in range(0, n, W):
        x[s:s + W].sort()
    return x


OLD_KINDS = ("uniform", "dup", "equal", "interleaved")
TOP32 = 0xFFFFFFFF


def place(n, lw, lk):
    """Every key's group, run in the group and position in the run."""
    i = np.arange(n, dtype=np.int64)
    return i >> (lw + lk), (i >> lw) & ((1 << lk) - 1), i & ((1 << lw) - 1)


def lifts(p, dtype, ext=False):
    """A pattern of 32-bit values as keys of dtype: itself for u32; for u64 in
    the high word over a constant low word, in the low word under a constant
    high word, and in both words (p * (2^32 + 1): 0 stays 0 and 2^32 - 1 becomes
    all-ones).  ext: the constant words are the extremes (all-ones below the
    pattern, zero above it), so that the pattern's 0 / all-ones keep their
    meaning for the kernels (ZW / the padding value) in one variant each."""
    p = np.asarray(p)
    assert p.min() >= 0 and p.max() <= TOP32
    if np.dtype(dtype).itemsize == 4:
        return {"": p.astype(np.uint32)}
    p = p.astype(np.uint64)
    s = np.uint64(32)
    return {"/hi": (p << s) | np.uint64(TOP32 if ext else 5),
            "/lo": (np.uint64(0 if ext else 7) << s) | p,
            "/both": (p << s) | p}


def named(base, variants, dtype, ext=False):
    return {base + ("/" + v if v else "") + suffix: x
            for v, p in variants.items() for suffix, x in lifts(p, dtype, ext).items()}


def fam_clumped(dtype, lw, lk, n, fm, fg):
    """Chunks whose window offsets add up.  mid: make_keys' clumps, c =
    ceil(fm / K) fences a clump in every run, so chunk 1 ends inside the clump of
    run fm // c.  full: run r's clumps hold c_r fences, sum c_r = fm: chunk 1
    takes the whole first clump of every run, c_0 FG keys of run 0 (the chunk
    starts at its fence) and (c_r + 1) FG - 1 of every other -- fm FG + (K - 1)
    (FG - 1) keys, the most a chunk of fm fences can hold.  (A run shorter than
    the prefix and a clump gives valid keys with smaller chunks.)"""
    K, W = 1 << lk, 1 << lw
    out = {"mid": make_keys("clumped", n, lw, lk, 0, fm, np.int64, fg)}
    _, r, pos = place(n, lw, lk)
    c = np.array([fm // K + (q < fm % K) for q in range(K)])[r]
    q = pos - ((fm - K) // K + (r < (fm - K) % K)) * fg
    per = (c + 1) * fg
    out["full"] = np.where(q < 0, 0, 1 + 2 * (q // per) + (q % per != 0))
    # lopsided (for the capacity split): chunk 1's first mid = fm // 2 fences
    # are clumps of 2s in the first nA runs, as in "full"; the other fm - mid
    # are 4s in the other nB runs, each after FG - 1 keys of 2 and followed at
    # once by 6s.  The middle fence is the first 4: half 0 takes every window
    # around the 2s, mid FG + (K - 1)(FG - 1) keys, half 1 the bare fences,
    # (fm - mid) FG - nB (FG - 1).  nA: the fewest runs that put the chunk over CAP.
    S = shape(lk, np.dtype(dtype).itemsize, fg.bit_length() - 1)
    mid, pre, nfr = fm // 2, (fm - K) // K + 1, W // fg
    for nA in range(1, K):
        nB = K - nA
        if fm * fg + (nA - 1) * (fg - 1) <= S["CAP"] or fm - mid < nB:
            continue
        if pre + -(-mid // nA) + 2 > nfr or pre + -(-(fm - mid) // nB) + 2 > nfr:
            continue
        cA = np.array([mid // nA + (a < mid % nA) for a in range(nA)] + [0] * nB)[r]
        cB = np.array([0] * nA + [(fm - mid) // nB + (b < (fm - mid) % nB) for b in range(nB)])[r]
        A = np.where(q < (cA + 1) * fg, 2, 5)
        Bv = np.where(q < fg, 2, np.where(q <= cB * fg, 4, 6))
        out["lopsided"] = np.where(q < 0, 0, np.where(q == 0, 1, np.where(r < nA, A, Bv)))
        break
    return named("clumped", out, dtype)


def fam_one_run(dtype, lw, lk, n, fm, fg):
    """The runs' value ranges disjoint, so the merged fences come run after run
    and a chunk's keys come from one run (two where it straddles): K - 1 empty
    segments, LA == 0 or LB == 0 at every in-LDS level.  The ranges in
    ascending, descending and rotated run order, and flat (constant) runs."""
    K = 1 << lk
    g, r, pos = place(n, lw, lk)
    orders = {"asc": r, "desc": K - 1 - r, "rot": (r + K // 2 + 1) % K}
    out = {k: (o << lw) + pos for k, o in orders.items()}
    out["flat"] = ((K - 1 - r + g) % K) * 3
    return named("one_run", out, dtype)


def fam_two_valued(dtype, lw, lk, n, fm, fg):
    """Run r = z_r zeros, then all-ones (the kernels' padding value; zero is the
    word below every A sequence), z_r from the edges of a fence, a load row and
    the run.  All runs equal, a staircase, one-hot and seeded random draws."""
    K, W = 1 << lk, 1 << lw
    RW = shape(lk, np.dtype(dtype).itemsize, fg.bit_length() - 1)["RW"]
    Z = [0, 1, fg - 1, fg, fg + 1, RW - 1, RW + 1, W // 2, W - 1, W]
    g, r, pos = place(n, lw, lk)
    run = (g << lk) + r  # the run's index in the input
    zs = {}
    for i in range(4):  # all equal within a group: every z in some group of 3
        zs["equal%d" % i] = np.array(Z)[(3 * i + g) % len(Z)]
    zs["stairs"] = np.array(sorted(Z))[((r + g) * len(Z) // K) % len(Z)]
    zs["onehot"] = np.where(r == g % K, W, 0)
    zs["onecold"] = np.where(r == (g + 1) % K, 0, W - 1)
    for seed in (0, 1):
        draw = np.random.default_rng(seed).integers(0, len(Z), int(run.max()) + 1)
        zs["rand%d" % seed] = np.array(Z)[draw[run]]
    return named("two_valued", {k: np.where(pos < z, 0, TOP32) for k, z in zs.items()}, dtype, ext=True)


def fam_fence_plateaus(dtype, lw, lk, n, fm, fg):
    """Distinct keys (2 pos + 1) broken by plateaus that begin and end at
    j FG + {-1, 0, +1}: every 4 fences one of 1 or 2 fences' length, the nine
    offset pairs by (plateau + run), so the same plateau value lies in several
    runs.  The last run of each group ends in a plateau that the next group's
    first run begins with (that run lies above it)."""
    K, W = 1 << lk, 1 << lw
    g, r, pos = place(n, lw, lk)
    p = 2 * pos + 1
    j = pos // fg
    m = j // 4  # the plateau of this stretch of 4 fences: begins at fence 4m + 1
    combo = (m + r) % 9
    begin = (4 * m + 1) * fg + combo // 3 - 1
    end = (4 * m + 2 + (m + r) % 2) * fg + combo % 3 - 1
    p = np.where((pos >= begin) & (pos < end), 2 * begin, p)
    top = 2 * W + 2
    p = np.where((r == K - 1) & (pos >= W - fg - 1), top, p)  # ends a group ...
    p = np.where((r == 0) & (g > 0), np.where(pos < fg - 1, top, top + p), p)  # ... and begins the next
    return named("fence_plateaus", {"": p}, dtype)


def fam_clustered(dtype, lw, lk, n, fm, fg):
    """Inside every FG window the keys sit at one end of [ka, kb]: run r's
    fence j is j D + r D / (K + 1), so another run's fence falls a fraction
    (r0 - r) / (K + 1) into the window and the interpolated guess lands there.
    low: the window repeats ka and jumps at the next fence -- the answer is the
    window's end, a forward gallop; high: it jumps after ka and crowds up to kb
    -- the answer is the window's start, a backward gallop."""
    K = 1 << lk
    D = 1 << 16
    assert ((1 << lw) // fg) * D <= 1 << 31 and fg < D // (K + 1)
    _, r, pos = place(n, lw, lk)
    j, i = pos // fg, pos % fg
    ka = j * D + r * (D // (K + 1))
    return named("clustered", {"low": ka, "high": np.where(i == 0, ka, ka + D - fg + i)}, dtype)


def fam_ragged_tail(dtype, lw, lk, n, fm, fg):
    """One full group, then a last group of 1 to K runs whose last run holds 1,
    FG - 1, FG, FG + 1 or RW + 1 keys; spread keys, every other run ending in
    all-ones keys (1 to FG + 1 of them)."""
    K, W = 1 << lk, 1 << lw
    RW = shape(lk, np.dtype(dtype).itemsize, fg.bit_length() - 1)["RW"]
    out = {}
    for i, last in enumerate([1, fg - 1, fg, fg + 1, RW + 1]):
        m = [1, K, max(1, K - 1), 2, K][i]
        nn = (K + m - 1) * W + last
        rng = np.random.default_rng(nn)
        p = rng.integers(0, 1 << 31, nn)
        _, r, pos = place(nn, lw, lk)
        ends = [1, fg + 1, fg - 1, RW, 2][i]
        p = np.where((r % 2 == 0) & (pos >= W - ends), TOP32, p)
        p[-1] = TOP32 if i % 2 else p[-1]
        for s in range(0, nn, W):
            p[s:s + W].sort()
        out["m%d_l%d" % (m, last)] = p
    return named("ragged_tail", out, dtype, ext=True)


FAMILIES = {"clumped": fam_clumped, "one_run": fam_one_run, "two_valued": fam_two_valued,
            "fence_plateaus": fam_fence_plateaus, "clustered": fam_clustered, "ragged_tail": fam_ragged_tail}


def battery_n(lw, lk, nfull=2):
    """Two full groups (or nfull), a tail group of K - 1 runs and a short run."""
    K, W = 1 << lk, 1 << lw
    return nfull * K * W + (K - 1) * W + 777


def battery(dtype, lw, lk, n, fm, fg=FG, families=None):
    """[(name, keys)] of the named families (default: all), every run of 2^lw
    keys ascending (checked here)."""
    out = []
    W = 1 << lw
    for fam in families or FAMILIES:
        for name, x in FAMILIES[fam](dtype, lw, lk, n, fm, fg).items():
            assert x.dtype == np.dtype(dtype) and 0 < x.size <= n
            d = x[1:] < x[:-1]
            d[W - 1::W] = False  # a descent may only sit between two runs
            assert not d.any(), name
            out.append((name, x))
    return out


# The knob sets the battery runs under besides the defaults (the GPU runs read
# them once per process; the model takes fm and split from the plan the dump
# program prints under the same settings).  The dump program takes the fence
# stride as an argument: fgl_of gives the one a knob set selects.
KNOB_SETS = {
    # k_fence_lds / k_fence_merge, k_fence_counts, k_bounds, k_chunk_desc; the split at its shipped add (u32 lk 3, 4)
    "unfused": {"MISORT_PLAN_FUSE": "0"},
    # the split at every lk and for u64, after the plan's own clamp
    "unfused_add40": {"MISORT_PLAN_FUSE": "0", "MISORT_MK_FM_ADD": "40"},
    # fused planning without k_fence_rank
    "norank": {"MISORT_FENCE_RANK_MAX": "0"},
    # the 64-key fence build (from 2^10 keys: every size here), fused and with the split
    "fg6": {"MISORT_FENCE_FG6_MIN": "10", "MISORT_FENCE_FG6_MIN_U64": "10"},
    "fg6_unfused_add40": {"MISORT_FENCE_FG6_MIN": "10", "MISORT_FENCE_FG6_MIN_U64": "10", "MISORT_PLAN_FUSE": "0",
                          "MISORT_MK_FM_ADD": "40"},
}


def fgl_of(knobs):
    return 6 if knobs and "MISORT_FENCE_FG6_MIN" in knobs else FG_LOG2


def battery_plan(dtype, lw, lk, knobs=None, nfull=2):
    """(n, fm, split, fgl) of the battery's shape under a knob set."""
    fgl = fgl_of(knobs)
    n = battery_n(lw, lk, nfull)
    p = plans([n], lw, lk, np.dtype(dtype).itemsize, fgl, 0, knobs)[0]
    return n, p["fm"], bool(p["split"]), fgl
