#!/usr/bin/env python3
"""Segmented sort against its yardsticks (random bit patterns, one GPU).

(a) uniform offsets: 2^28 u32 and 2^27 u64 keys as segments of 64, 1000, 2^14
    (u32), 2^16 + 1 and 2^20 keys: Context.sort_segments against
    Context.sort_rows on the same data, once on an aligned tensor and once on a
    view one element into its storage (element accesses, as the segment tile
    takes: the fair bar), with the segmented call's profiler records split into
    count, scatter, tile classes, pad, block passes and unpad;
(b) for the two longest shapes, a host loop of local_sort, one call per segment;
(c) u32: the record composition: repeat_interleave segment ids, (seg << 32) |
    key, one u64 local_sort, split;
(d) a ragged case: lengths drawn log-uniformly from 1 .. 2^18, against (b) and
    (c), with the launches per class and the scratch the context holds.

Everything runs on the context's own stream.  Each figure is the median of
--reps runs after a warm-up, with minimum and maximum, as device time (HIP
events around the call) and as wall time of the whole call up to the end of its
device work (the segmented call waits once on the host).  Writes one JSON line
to --out (default profiles/segments/segments_probe.json) and prints it."""
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

LENGTHS = [64, 1000, 1 << 14, (1 << 16) + 1, 1 << 20]
LOOP_LENGTHS = ((1 << 16) + 1, 1 << 20)


def timed(fn, reps):
    """{ms, min_ms, max_ms, wall_ms, wall_min_ms, wall_max_ms} of fn() over reps runs, after one warm-up."""
    fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return {"ms": statistics.median(dev), "min_ms": min(dev), "max_ms": max(dev),
            "wall_ms": statistics.median(wall), "wall_min_ms": min(wall), "wall_max_ms": max(wall)}


def parts(ctx, fn, reps, long_classes):
    """Median ms of the parts of one segmented call, from the profiler's trace."""
    fn()
    per = []
    ctx.profile(True)
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
    ctx.profile(False)
    return {k: statistics.median(p[k] for p in per) for k in per[0]}


def tile_record(ctx, fn, reps):
    """Median ms of the one tile_sort record of fn() under the profiler."""
    fn()
    ms = []
    ctx.profile(True)
    for _ in range(reps):
        ctx.profile_reset()
        fn()
        torch.cuda.synchronize()
        rec = [m for kind, m, _ in ctx.profile_trace() if kind == "tile_sort"]
        assert len(rec) == 1, len(rec)
        ms.append(rec[0])
    ctx.profile(False)
    return statistics.median(ms)


def classes_of(lens, size):
    """{class: segments} and the scratch bytes the context holds for these lengths."""
    t = misort.tile_log2(size)
    count = {}
    for x in lens:
        c = misort.segment_class(int(x), size)
        if c >= 0:
            count[c] = count.get(c, 0) + 1
    blocks = max([n << c for c, n in count.items() if c > t] + [0])
    return count, 2048 + 4 * len(lens) + 2 * blocks * size


def host_loop(ctx, keys, out, bounds):
    for a, b in bounds:
        ctx.local_sort(keys[a:b], out[a:b])


def composition(ctx, keys, lens_dev, out):
    """u32 keys: (segment << 32) | key records through one u64 local_sort."""
    seg = torch.repeat_interleave(torch.arange(lens_dev.numel(), device="cuda"), lens_dev)
    rec = (seg << 32) | (keys.to(torch.int64) & 0xFFFFFFFF)
    ctx.local_sort(rec)
    out.copy_((rec & 0xFFFFFFFF).to(torch.int32))  # (the low words wrap back to the u32 storage)


def unsigned_sorted(x):
    lo = torch.iinfo(x.dtype).min
    return torch.sort(x ^ lo).values ^ lo


def uniform(ctx, dtype, cols, rows, reps):
    size = torch.empty(0, dtype=dtype).element_size()
    n = rows * cols
    store = torch.empty(n + 4, dtype=dtype, device="cuda")
    ctx.fill_splitmix(store, 0x5E650000 + cols)
    keys, odd = store[:n], store[1:n + 1]
    out_store = torch.empty_like(store)
    out, out_odd = out_store[:n], out_store[1:n + 1]
    offs = torch.arange(0, n + 1, cols, dtype=torch.int64, device="cuda")
    count, scratch = classes_of([cols], size)
    long_classes = sum(1 for c in count if c > misort.tile_log2(size))
    res = {"key_bytes": size, "len": cols, "segments": rows, "keys": n, "class": next(iter(count)),
           "path": "blocks" if long_classes else "tile"}
    res["sort_segments"] = timed(lambda: ctx.sort_segments(keys, offs, out=out), reps)
    for r in (0, rows // 2, rows - 1):  # what was timed is a segmented sort
        assert torch.equal(out[r * cols:(r + 1) * cols], unsigned_sorted(keys[r * cols:(r + 1) * cols]))
    res["sort_segments_parts"] = parts(ctx, lambda: ctx.sort_segments(keys, offs, out=out), reps, long_classes)
    res["sort_rows_aligned"] = timed(lambda: ctx.sort_rows(keys.view(rows, cols), out=out.view(rows, cols)), reps)
    res["sort_rows_unaligned"] = timed(lambda: ctx.sort_rows(odd.view(rows, cols), out=out_odd.view(rows, cols)), reps)
    if not long_classes:
        # the row tile's record under the profiler, on the view: what tile_classes_ms compares with
        res["sort_rows_unaligned_tile_record_ms"] = tile_record(
            ctx, lambda: ctx.sort_rows(odd.view(rows, cols), out=out_odd.view(rows, cols)), reps)
        res["tile_classes_over_rows_unaligned_record_time"] = (res["sort_segments_parts"]["tile_classes_ms"]
                                                               / res["sort_rows_unaligned_tile_record_ms"])
    a, u, s = res["sort_rows_aligned"], res["sort_rows_unaligned"], res["sort_segments"]
    res["segments_over_rows_aligned_time"] = s["ms"] / a["ms"]
    res["segments_over_rows_unaligned_time"] = s["ms"] / u["ms"]
    key_part = res["sort_segments_parts"]
    key_ms = sum(key_part[k] for k in ("tile_classes_ms", "pad_ms", "unpad_ms", "block_passes_ms"))
    res["key_kernels_over_rows_unaligned_time"] = key_ms / u["ms"]
    res["host_wait_ms"] = s["wall_ms"] - sum(key_part.values())
    if cols in LOOP_LENGTHS:
        bounds = [(r * cols, (r + 1) * cols) for r in range(rows)]
        res["host_loop"] = timed(lambda: host_loop(ctx, keys, out, bounds), min(reps, 3))
        res["segments_over_host_loop_time"] = s["wall_ms"] / res["host_loop"]["wall_ms"]
    if size == 4:
        lens_dev = torch.full((rows,), cols, dtype=torch.int64, device="cuda")
        res["composition"] = timed(lambda: composition(ctx, keys, lens_dev, out), min(reps, 3))
        assert torch.equal(out[:cols], unsigned_sorted(keys[:cols]))
        res["segments_over_composition_time"] = s["wall_ms"] / res["composition"]["wall_ms"]
    return res


def ragged(ctx, dtype, log2_keys, reps):
    size = torch.empty(0, dtype=dtype).element_size()
    g = torch.Generator().manual_seed(0x5E67)
    lens = []
    total = 0
    while total < (1 << log2_keys):
        x = int(math.floor(2.0 ** (18.0 * torch.rand(1, generator=g).item())))
        lens.append(max(1, min(x, 1 << 18)))
        total += lens[-1]
    n = total
    lens_t = torch.tensor(lens, dtype=torch.int64)
    offs_h = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens_t, 0)])
    offs, lens_dev = offs_h.cuda(), lens_t.cuda()
    keys = torch.empty(n, dtype=dtype, device="cuda")
    ctx.fill_splitmix(keys, 0x5E670000)
    out = torch.empty_like(keys)
    count, scratch = classes_of(lens, size)
    t = misort.tile_log2(size)
    long_classes = sum(1 for c in count if c > t)
    res = {"key_bytes": size, "keys": n, "segments": len(lens), "segments_per_class": {str(c): count[c] for c in sorted(count)},
           "tile_launches": sum(1 for c in count if c <= t), "long_classes": long_classes, "scratch_bytes": scratch}
    res["sort_segments"] = timed(lambda: ctx.sort_segments(keys, offs, out=out), reps)
    bounds = list(zip(offs_h[:-1].tolist(), offs_h[1:].tolist()))
    for a, b in bounds[:: max(1, len(bounds) // 16)]:
        assert torch.equal(out[a:b], unsigned_sorted(keys[a:b]))
    res["sort_segments_parts"] = parts(ctx, lambda: ctx.sort_segments(keys, offs, out=out), reps, long_classes)
    res["host_loop"] = timed(lambda: host_loop(ctx, keys, out, bounds), min(reps, 3))
    res["segments_over_host_loop_time"] = res["sort_segments"]["wall_ms"] / res["host_loop"]["wall_ms"]
    if size == 4:
        res["composition"] = timed(lambda: composition(ctx, keys, lens_dev, out), min(reps, 3))
        res["segments_over_composition_time"] = res["sort_segments"]["wall_ms"] / res["composition"]["wall_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shift", type=int, default=0, help="halve the key counts this many times (a quick run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments", "segments_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segments_probe needs a GPU")
    ctx = misort.Context(0)
    uni, rag = [], []
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.native_stream)):
        for dtype, log2_keys in ((torch.int32, 28 - a.shift), (torch.int64, 27 - a.shift)):
            for cols in LENGTHS:
                if cols == 1 << 14 and dtype != torch.int32:
                    continue
                uni.append(uniform(ctx, dtype, cols, max(1, (1 << log2_keys) // cols), a.reps))
                print(json.dumps(uni[-1]), file=sys.stderr, flush=True)
            rag.append(ragged(ctx, dtype, log2_keys - 2, a.reps))
            print(json.dumps(rag[-1]), file=sys.stderr, flush=True)
        torch.cuda.synchronize()
    ctx.close()
    line = json.dumps({"probe": "segments", "reps": a.reps, "device": torch.cuda.get_device_name(0),
                       "uniform": uni, "ragged": rag})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
