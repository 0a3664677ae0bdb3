#!/usr/bin/env python3
"""Segmented key-value sort and argsort against their yardsticks (u32 keys,
random bit patterns, one GPU).  None of the yardsticks is the code under test.

Uniform offsets: 2^27 pairs as segments of 64, 1000, 2^13, 2^16 + 1 and 2^20:
(a) Context.argsort_rows and Context.sort_rows_pairs on the same data as a view
    one element into its storage (element accesses, as the segment tile takes:
    the fair bar), and on the aligned tensors for reference;
(b) Context.sort_segments on u64 keys of the same count and offsets: the same
    classes and the same block passes, without the split arrays.
The ragged case of tools/segments_probe.py (lengths drawn log-uniformly from
1 .. 2^18) at 2^25 pairs: (b), and
(c) what a caller runs today: the keys scattered into a (segments x longest)
    array filled with all-ones, then Context.argsort_rows (the scatter is timed
    with it and alone).

Everything runs on the context's own stream.  The candidates of a shape
ALTERNATE in one process: after one warm-up run of each, --reps rounds, every
round running each candidate once between two HIP events.  Each figure is the
median over the rounds with minimum and maximum, as device time and as wall
time up to the end of the device work (the segmented calls wait once on the
host).  The segmented calls' profiler records are split into count, scatter,
tile classes, pad, block passes and unpad.  Writes one JSON line to --out
(default profiles/segments_pairs/segments_pairs_probe.json) and prints it."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-computing-mpi_amd"))
import torch  # noqa: E402
import misort  # noqa: E402

LENGTHS = [64, 1000, 1 << 13, (1 << 16) + 1, 1 << 20]


def stats(xs, prefix=""):
    return {prefix + "ms": statistics.median(xs), prefix + "min_ms": min(xs), prefix + "max_ms": max(xs)}


def alternate(cands, reps):
    """{name: {ms, min_ms, max_ms, wall_ms, ...}} of the candidates (name -> fn),
    one warm-up each, then ``reps`` rounds over all of them in turn."""
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    dev = {k: [] for k in cands}
    wall = {k: [] for k in cands}
    for _ in range(reps):
        for name, fn in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            dev[name].append(a.elapsed_time(b))
    return {k: dict(stats(dev[k]), **stats(wall[k], "wall_")) for k in cands}


def parts(ctx, fn, reps, long_classes):
    """Median ms of the parts of one segmented call, from the profiler's trace."""
    fn()
    per = []
    ctx.profile(True)
    try:
        for _ in range(reps):
            ctx.profile_reset()
            fn()
            torch.cuda.synchronize()
            tr = ctx.profile_trace()
            other = [ms for kind, ms, _ in tr if kind == "other"]
            assert len(other) == 2 + 2 * long_classes, (len(other), long_classes)
            # per long class: pad, the block passes (their first is a tile_sort record), unpad
            tiles = [ms for kind, ms, _ in tr if kind == "tile_sort"]
            merges = sum(ms for kind, ms, _ in tr if kind in ("run_merge", "run_mergek"))
            block_tiles = sum(tiles[len(tiles) - long_classes:]) if long_classes else 0.0
            per.append({"count_ms": other[0], "scatter_ms": other[1],
                        "tile_classes_ms": sum(tiles) - block_tiles,
                        "pad_ms": sum(other[2::2]), "unpad_ms": sum(other[3::2]),
                        "block_passes_ms": block_tiles + merges})
    finally:
        ctx.profile(False)
    return {k: statistics.median(p[k] for p in per) for k in per[0]}


def classes_of(lens):
    count = {}
    for x in lens:
        c = misort.segment_class(int(x), 8)
        if c >= 0:
            count[c] = count.get(c, 0) + 1
    return count


def unsigned_order(k32):
    """The stable argsort of int32 storage compared unsigned (torch, the check's own yardstick)."""
    return torch.sort((k32.to(torch.int64) & 0xFFFFFFFF), stable=True).indices


def ratios(res, mine, bars):
    for m in mine:
        for b in bars:
            if m in res and b in res:
                res[f"{m}_over_{b}_time"] = res[m]["ms"] / res[b]["ms"]


def uniform(ctx, cols, rows, reps):
    n = rows * cols
    kstore = torch.empty(n + 4, dtype=torch.int32, device="cuda")
    vstore = torch.empty(n + 4, dtype=torch.int32, device="cuda")
    ctx.fill_splitmix(kstore, 0x5E690000 + cols)
    ctx.fill_splitmix(vstore, 0x5E6A0000 + cols)
    keys, vals, kodd, vodd = kstore[:n], vstore[:n], kstore[1:n + 1], vstore[1:n + 1]
    okstore, ovstore = torch.empty_like(kstore), torch.empty_like(vstore)
    ok, ov, okodd, ovodd = okstore[:n], ovstore[:n], okstore[1:n + 1], ovstore[1:n + 1]
    k64 = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.fill_splitmix(k64, 0x5E6B0000 + cols)
    o64 = torch.empty_like(k64)
    offs = torch.arange(0, n + 1, cols, dtype=torch.int64, device="cuda")
    count = classes_of([cols])
    long_classes = sum(1 for c in count if c > 13)
    res = {"len": cols, "segments": rows, "pairs": n, "class": next(iter(count)),
           "path": "blocks" if long_classes else "tile"}
    shape = (rows, cols)
    cands = {
        "argsort_segments": lambda: ctx.argsort_segments(keys, offs, out=ov),
        "sort_segments_pairs": lambda: ctx.sort_segments_pairs(keys, offs, vals, out_keys=ok, out_values=ov),
        "argsort_rows_unaligned": lambda: ctx.argsort_rows(kodd.view(shape), out=ovodd.view(shape)),
        "sort_rows_pairs_unaligned": lambda: ctx.sort_rows_pairs(kodd.view(shape), vodd.view(shape),
                                                                 out_keys=okodd.view(shape),
                                                                 out_values=ovodd.view(shape)),
        "argsort_rows_aligned": lambda: ctx.argsort_rows(keys.view(shape), out=ov.view(shape)),
        "sort_rows_pairs_aligned": lambda: ctx.sort_rows_pairs(keys.view(shape), vals.view(shape),
                                                               out_keys=ok.view(shape), out_values=ov.view(shape)),
        "sort_segments_u64": lambda: ctx.sort_segments(k64, offs, out=o64),
    }
    res.update(alternate(cands, reps))
    # what was timed is a segmented argsort
    ctx.argsort_segments(keys, offs, out=ov)
    torch.cuda.synchronize()
    for r in (0, rows // 2, rows - 1):
        seg = keys[r * cols:(r + 1) * cols]
        assert torch.equal(ov[r * cols:(r + 1) * cols].to(torch.int64) & 0xFFFFFFFF, unsigned_order(seg))
    res["argsort_segments_parts"] = parts(ctx, cands["argsort_segments"], reps, long_classes)
    res["sort_segments_pairs_parts"] = parts(ctx, cands["sort_segments_pairs"], reps, long_classes)
    res["sort_segments_u64_parts"] = parts(ctx, cands["sort_segments_u64"], reps, long_classes)
    ratios(res, ["argsort_segments"], ["argsort_rows_unaligned", "argsort_rows_aligned", "sort_segments_u64"])
    ratios(res, ["sort_segments_pairs"], ["sort_rows_pairs_unaligned", "sort_rows_pairs_aligned", "sort_segments_u64"])
    return res


def ragged(ctx, log2_pairs, reps):
    g = torch.Generator().manual_seed(0x5E67)
    lens = []
    total = 0
    while total < (1 << log2_pairs):
        x = int(math.floor(2.0 ** (18.0 * torch.rand(1, generator=g).item())))
        lens.append(max(1, min(x, 1 << 18)))
        total += lens[-1]
    n = total
    lens_t = torch.tensor(lens, dtype=torch.int64)
    offs_h = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens_t, 0)])
    offs, lens_dev = offs_h.cuda(), lens_t.cuda()
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    vals = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.fill_splitmix(keys, 0x5E670000)
    ctx.fill_splitmix(vals, 0x5E680000)
    ok, ov = torch.empty_like(keys), torch.empty_like(vals)
    k64 = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.fill_splitmix(k64, 0x5E6C0000)
    o64 = torch.empty_like(k64)
    count = classes_of(lens)
    long_classes = sum(1 for c in count if c > 13)
    longest = max(lens)
    res = {"pairs": n, "segments": len(lens), "longest": longest,
           "segments_per_class": {str(c): count[c] for c in sorted(count)},
           "tile_launches": sum(1 for c in count if c <= 13), "long_classes": long_classes,
           "padded_elements": len(lens) * longest}
    # (c) pad to the longest segment, then argsort_rows
    row = torch.repeat_interleave(torch.arange(len(lens), device="cuda"), lens_dev)
    col = torch.arange(n, device="cuda") - torch.repeat_interleave(offs[:-1], lens_dev)
    padded = torch.empty((len(lens), longest), dtype=torch.int32, device="cuda")
    pidx = torch.empty_like(padded)

    def scatter():
        padded.fill_(-1)  # all-ones: sorts last
        padded[row, col] = keys

    def pad_argsort():
        scatter()
        ctx.argsort_rows(padded, out=pidx)

    cands = {
        "argsort_segments": lambda: ctx.argsort_segments(keys, offs, out=ov),
        "sort_segments_pairs": lambda: ctx.sort_segments_pairs(keys, offs, vals, out_keys=ok, out_values=ov),
        "sort_segments_u64": lambda: ctx.sort_segments(k64, offs, out=o64),
        "pad_to_longest_argsort_rows": pad_argsort,
        "pad_to_longest_scatter_alone": scatter,
    }
    res.update(alternate(cands, reps))
    ctx.argsort_segments(keys, offs, out=ov)
    torch.cuda.synchronize()
    bounds = list(zip(offs_h[:-1].tolist(), offs_h[1:].tolist()))
    for a, b in bounds[:: max(1, len(bounds) // 16)]:
        assert torch.equal(ov[a:b].to(torch.int64) & 0xFFFFFFFF, unsigned_order(keys[a:b]))
    res["argsort_segments_parts"] = parts(ctx, cands["argsort_segments"], reps, long_classes)
    res["sort_segments_pairs_parts"] = parts(ctx, cands["sort_segments_pairs"], reps, long_classes)
    res["sort_segments_u64_parts"] = parts(ctx, cands["sort_segments_u64"], reps, long_classes)
    ratios(res, ["argsort_segments", "sort_segments_pairs"], ["sort_segments_u64", "pad_to_longest_argsort_rows"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shift", type=int, default=0, help="halve the pair counts this many times (a quick run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_pairs", "segments_pairs_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segments_pairs_probe needs a GPU")
    ctx = misort.Context(0)
    uni = []
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.native_stream)):
        for cols in LENGTHS:
            uni.append(uniform(ctx, cols, max(1, (1 << (27 - a.shift)) // cols), a.reps))
            print(json.dumps(uni[-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        rag = ragged(ctx, 25 - a.shift, a.reps)
        print(json.dumps(rag), file=sys.stderr, flush=True)
        torch.cuda.synchronize()
    ctx.close()
    line = json.dumps({"probe": "segments_pairs", "reps": a.reps, "device": torch.cuda.get_device_name(0),
                       "uniform": uni, "ragged": rag})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
