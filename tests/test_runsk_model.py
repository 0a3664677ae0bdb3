"""numpy model of the K-way merge pass's chunking (runsk.hip), CPU only.

The kernels' constants and the pass plan come from the library's own host code
(csrc/mergek_plan.h), printed by lib/mergek_plan_dump (built by the default
make target): nothing here is a literal copy.  The model itself (fences,
chunk_bounds, refine, check_groups, make_keys and the dump's readers) lives in
merge_battery.py, shared with the merge battery.  The rules modelled: fences every
FG keys of each run in the total order (key, run, position/FG);
the group's fences merged; every fm-th one starts a chunk whose
start in each run is that run's count of keys before the fence; chunks are
then merged independently.  Checks the properties the kernels rely on: chunks
tile each group exactly, no chunk exceeds CAP keys nor the load rows (RW keys
of one segment, NROWS per chunk), every chunk's keys precede the next chunk's,
and the chunk/slot indexing (chunks per full group = ceil(fences / fm)) matches
the bounds layout -- with the worst-case fm, and with the raised fm of the
capacity split, where a chunk over CAP is cut at its middle fence.  The plan's
workspace layout and knob rules are checked from the dump alone
(test_pass_layout).  K = 2^lk, lk = 1..4."""
import os

import numpy as np
import pytest

from merge_battery import (ASAN_DUMP, FG, FG_LOG2, check_groups, chunk_bounds, fences, make_keys, plans,  # noqa: F401
                           refine, run_dump, shape)


@pytest.mark.parametrize("lk", [1, 2, 3, 4])
@pytest.mark.parametrize("lw", [15, 16])
@pytest.mark.parametrize("n_groups,tail", [(2, 0), (1, 3 * (1 << 15) + 5), (1, 777), (0, (1 << 15) * 2 + 1)])
@pytest.mark.parametrize("kind", ["uniform", "dup", "equal", "interleaved"])
def test_chunks_tile_and_bound(lk, lw, n_groups, tail, kind):
    """The worst-case fm, (fm + K) * FG <= CAP: no chunk can exceed CAP.  It is
    what the plan cuts these sizes at (fused passes have no capacity split)."""
    S = shape(lk)
    K, FM, W = S["K"], S["FM"], 1 << lw
    assert (FM + K) * FG <= S["CAP"] < (FM + K + 1) * FG and S["NROWS"] == S["LS"] * S["NR"]
    assert S["NT"] % S["RW"] == 0 and S["NR"] == S["NT"] // S["RW"] and S["CAP"] <= S["NT"] * S["IT"]
    n = n_groups * K * W + tail
    x = make_keys(kind, n, lw, lk, lw + n)
    ngroups = (n + K * W - 1) // (K * W)
    assert check_groups(x, lw, lk, FM, range(ngroups), split=False) == 0
    p = plans([n], lw, lk)[0]
    kf = ((K * W >> FG_LOG2) + FM - 1) // FM
    assert (p["fuse"], p["split"], p["fm"], p["kf"], p["nfull"]) == (1, 0, FM, kf, n >> (lw + lk))


@pytest.mark.parametrize("lk", [3, 4])
@pytest.mark.parametrize("kind", ["uniform", "dup", "equal", "interleaved", "clumped"])
def test_chunks_tile_and_bound_split(lk, kind):
    """The shipped shape of a large pass: the smallest u32 size (runs of 2^14)
    whose plan is unfused -- 4096 chunks at the worst-case fm -- cuts at the
    plan's raised fm and splits the chunks that then exceed CAP.  The plan's
    counts are checked on the whole size from the dump; the group invariants on
    keys of 4 full groups plus the tail group (a group's chunking depends on fm
    and the group alone)."""
    lw = 14
    S = shape(lk)
    K, FM, W = S["K"], S["FM"], 1 << lw
    gf = K * W >> FG_LOG2  # fences of a full group
    tail = 3 * W + 5
    nfull = -(-4096 // (-(-gf // FM)))
    n = nfull * K * W + tail
    small, p = plans([n - K * W, n], lw, lk)
    assert small["fuse"] == 1 and (p["fuse"], p["split"], p["rank"]) == (0, 1, 0)
    fm = p["fm"]
    # above the worst case, halves still fit, 8-bit fence counts
    assert FM < fm <= 255 and ((fm + 1) // 2 + K) * FG <= S["CAP"]
    kf, tail_chunks = -(-gf // fm), -(-((tail + FG - 1) >> FG_LOG2) // fm)
    assert (p["kf"], p["nfull"], p["tail"]) == (kf, nfull, 1)
    assert p["nchunks"] == nfull * kf + tail_chunks
    assert nfull * -(-gf // FM) + -(-((tail + FG - 1) >> FG_LOG2) // FM) >= 4096  # unfused: by the worst-case count
    assert p["nslots"] == p["nchunks"] + nfull + 1
    x = make_keys(kind, 4 * K * W + tail, lw, lk, lk, fm)
    ncut = check_groups(x, lw, lk, fm, range(5), split=True)
    if kind == "clumped":
        assert ncut >= 4  # the split is exercised, not only allowed: chunk 1 of every full group


PASS_NS = [lambda lw: (1 << lw) + 1, lambda lw: (1 << 20) + 77, lambda lw: (1 << 24) + 999,
           lambda lw: (1 << 26) + 12345, lambda lw: 1 << 30]


def layout_grid(key_bytes, fgl):
    """(lk, lw, depth, ns) over lk = 1..4, the shortest, a middle and the longest
    runs a pass takes, both depths and the five sizes."""
    for lk in (1, 2, 3, 4):
        S = shape(lk, key_bytes, fgl)
        for lw in sorted({S["LW_MIN"], 18, S["LWK_MAX"] - lk}):
            for depth in (0, 1):
                yield lk, lw, depth, [f(lw) for f in PASS_NS]


def check_layout(p, S, depth):
    K, parts = S["K"], {q["name"]: q for q in p["parts"]}
    assert [q["name"] for q in p["parts"]] == ["M", "T", "bounds", "cnt", "bsum", "desc", "ovf"]
    end = 0
    for q in p["parts"]:  # aligned, disjoint, in order
        assert q["off"] % 256 == 0 and q["bytes"] % 256 == 0 and q["off"] >= end
        end = q["off"] + q["bytes"]
    assert end <= p["plan_bytes"]
    need = {"M": p["nf"] * S["fence_bytes"], "T": p["nf"] * S["fence_bytes"], "bounds": p["nslots"] * K * 8,
            "cnt": p["nbk"] * p["cpb"] * K * 4, "bsum": p["nbk"] * K * 4,
            "desc": p["nchunks"] * S["desc_bytes"] * (3 if p["split"] else 1),
            "ovf": (p["nchunks"] + 1) * 4 if p["split"] else 0}
    for name, b in need.items():
        assert parts[name]["bytes"] >= b, name
    assert p["fb"] == p["fence_buffer_fb"] and p["fb"] % 256 == 0 and p["fb"] >= need["M"]
    assert p["fence_bytes"] == 2 * p["fb"] and (p["fence_set"], p["plan_set"]) == (2 * depth, 2 * depth + 1)
    # the counts the sizes stand on
    ngroups = -(-p["n"] >> (p["lw"] + p["lk"]))
    assert p["nf"] == -(-p["n"] >> S["FG_LOG2"]) and p["nslots"] == p["nchunks"] + ngroups
    assert p["nbk"] * p["cpb"] >= p["nchunks"] > (p["nbk"] - 1) * p["cpb"] and p["cpb"] in (32, 64, 128, 256)
    assert p["dc"] in (4, 16) and S["desc_bytes"] % 128 == 0
    assert p["fm_worst"] == S["FM"] and (p["fm"] > S["FM"] if p["split"] else p["fm"] == S["FM"])
    assert not (p["fuse"] and p["split"]) and not (p["rank"] and not p["fuse"]) and not (p["nest"] and p["rank"])
    assert p["nest_lk"] == (p["left"] if p["nest"] else 0) and (not p["nest"] or p["nest_lk"] in (3, 4))


@pytest.mark.parametrize("fgl", [7, 6])
@pytest.mark.parametrize("key_bytes", [4, 8])
def test_pass_layout(key_bytes, fgl):
    """plan_pass's workspace parts are 256-byte aligned, disjoint, in order
    inside the reported total and large enough for what the plan's counts say is
    written there; the fence buffer is the one MergekBuild::fence_buffer sizes; and
    the knob rules the GPU variants (test_gpu_runs.py) rely on hold."""
    seen = set()
    for lk, lw, depth, ns in layout_grid(key_bytes, fgl):
        S = shape(lk, key_bytes, fgl)
        for p in plans(ns, lw, lk, key_bytes, fgl, depth):
            check_layout(p, S, depth)
            assert not (p["nest"] and (depth == 1 or key_bytes == 8))
            seen |= {k for k in ("fuse", "split", "rank", "nest", "line", "slices", "fmerge", "nbs") if p[k]}
            seen |= {"unfused"} if not p["fuse"] else set()
        if depth == 1:
            continue
        for knobs, rule in [({"MISORT_PLAN_FUSE": "0"}, lambda p: not p["fuse"] and not p["rank"]),
                            ({"MISORT_PLAN_FUSE": "2"}, lambda p: p["fuse"] and not p["split"]),
                            ({"MISORT_MK_FM_ADD": "0"}, lambda p: not p["split"] and p["fm"] == p["fm_worst"]),
                            ({"MISORT_FENCE_NEST_MIN": "0"}, lambda p: not p["nest"]),
                            ({"MISORT_FENCE_RANK_MAX": "0"}, lambda p: not p["rank"])]:
            for p in plans(ns, lw, lk, key_bytes, fgl, depth, knobs):
                check_layout(p, S, depth)
                assert rule(p), (knobs, p)
    # the grid reaches every shape the defaults have for this key type
    want = {"fuse", "unfused", "rank", "line", "slices", "fmerge", "nbs"} | ({"split", "nest"} if key_bytes == 4 else set())
    assert want <= seen, want - seen


def test_plan_dump_clean_under_asan_ubsan():
    """The same grid through the dump program built with ASan + UBSan (a
    stand-alone executable, nothing preloaded for it): exit status 0, no report."""
    assert os.path.exists(ASAN_DUMP), "sanitized dump missing: make -C parallel-computing-mpi_amd/csrc asan"
    for key_bytes in (4, 8):
        for fgl in (7, 6):
            for lk, lw, depth, ns in layout_grid(key_bytes, fgl):
                assert run_dump([key_bytes, lk, fgl], exe=ASAN_DUMP)[0] == shape(lk, key_bytes, fgl)
                assert plans(ns, lw, lk, key_bytes, fgl, depth, exe=ASAN_DUMP) == plans(ns, lw, lk, key_bytes, fgl, depth)


def fence_rank_model(F, nf, wf_log2, lk, fm, nt=256):
    """k_fence_rank (runsk.hip) on a flat fence array: blocks of nt threads own
    nt - 1 fences each (thread 0 ranks the fence before them); returns the
    merged fences M and the per-(chunk, run) counts P exactly as the kernel
    writes them (-1 = never written)."""
    K, wf, gl = 1 << lk, 1 << wf_log2, wf_log2 + lk
    ngroups = (nf + (1 << gl) - 1) >> gl
    fences_per_group = 1 << gl
    kf = (fences_per_group + fm - 1) // fm
    nch_of = [kf if (g + 1) << gl <= nf else (min(nf - (g << gl), fences_per_group) + fm - 1) // fm
              for g in range(ngroups)]
    M = np.zeros(nf, np.uint64)
    P = np.full((ngroups * kf + 1) * K, -1, np.int64)
    nblocks = (nf + nt - 2) // (nt - 1)
    for b in range(nblocks):
        sp = [-1] * nt
        info = [None] * nt
        for tid in range(nt):
            e = b * (nt - 1) - 1 + tid
            if e < 0 or e >= nf:
                continue
            g = e >> gl
            gbase = g << gl
            nfg = min(nf - gbase, 1 << gl)
            gi = e - gbase
            q, i = gi >> wf_log2, gi & (wf - 1)
            v = F[e]
            p = i
            for r in range(K):
                ln = 0 if r == q else max(0, min(nfg - r * wf, wf))
                pos, st = 0, wf
                while st > 0:  # the kernel's power-of-two lower bound
                    if pos + st <= ln and F[gbase + r * wf + pos + st - 1] < v:
                        pos += st
                    st >>= 1
                p += pos
            M[gbase + p] = v
            sp[tid] = p
            info[tid] = (g, gbase, nfg, gi, q, i, p)
        for tid in range(1, nt):
            if info[tid] is None:
                continue
            g, gbase, nfg, gi, q, i, p = info[tid]
            c0, nch = g * kf, nch_of[g]
            lq = min(nfg - q * wf, wf)
            t0 = 0 if i == 0 else sp[tid - 1] // fm + 1
            t1 = p // fm
            for t in range(t0, t1 + 1):
                P[(c0 + t) * K + q] = i
            if i == lq - 1:
                for t in range(t1 + 1, nch):
                    P[(c0 + t) * K + q] = i + 1
            nruns = (nfg + wf - 1) >> wf_log2
            if gi < nch:
                for r in range(nruns, K):
                    P[(c0 + gi) * K + r] = 0
    return M, P, nch_of, kf


@pytest.mark.parametrize("lk,wf_log2,nf,fm", [(3, 5, 3 * 256 + 40, 7), (3, 5, 256 * 2, 60), (2, 6, 256 + 64 * 2 + 3, 9),
                                              (4, 3, 16 * 8 * 3 + 17, 5), (1, 7, 700, 13), (3, 8, 2048 + 1, 66)])
@pytest.mark.parametrize("kind", ["uniform", "dup", "interleaved"])
def test_fence_rank_counts(lk, wf_log2, nf, fm, kind):
    """k_fence_rank's merged order and counts equal the sorted group fences and
    the direct per-(chunk, run) counts, tail groups with short and missing runs
    included."""
    K, wf, gl = 1 << lk, 1 << wf_log2, wf_log2 + lk
    rng = np.random.default_rng(nf + fm)
    if kind == "uniform":
        keys = rng.integers(0, 2**20, nf)
    elif kind == "dup":
        keys = rng.integers(0, 3, nf)
    else:
        keys = np.arange(nf) % wf * K + (np.arange(nf) // wf) % K
    F = np.zeros(nf, np.uint64)
    for s in range(0, nf, wf):  # per run: sorted keys packed with (run, position) as the fences are
        e = np.arange(s, min(s + wf, nf))
        run = (e >> wf_log2) & (K - 1)
        F[s:s + e.size] = ((np.sort(keys[s:s + e.size]).astype(np.uint64) << np.uint64(32))
                           | (run.astype(np.uint64) << np.uint64(32 - lk)) | (e & (wf - 1)).astype(np.uint64))
    M, P, nch_of, kf = fence_rank_model(F, nf, wf_log2, lk, fm)
    for g in range(len(nch_of)):
        gbase = g << gl
        nfg = min(nf - gbase, 1 << gl)
        want = np.sort(F[gbase:gbase + nfg])
        np.testing.assert_array_equal(M[gbase:gbase + nfg], want)
        for t in range(nch_of[g]):
            start = int(want[t * fm])
            for r in range(K):
                run = F[gbase + r * wf: gbase + min(nfg, (r + 1) * wf)] if r * wf < nfg else F[:0]
                assert P[(g * kf + t) * K + r] == int(np.sum(run < start)), (g, t, r)
