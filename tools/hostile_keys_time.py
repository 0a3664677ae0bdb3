#!/usr/bin/env python3
"""Time ctx.local_sort on keys that defeat the seeded co-rank search (ascending,
descending, constant) and on iid keys -- measurement only; run it once per
library (MISORT_LIBRARY) in one session and compare.
  python3 tools/hostile_keys_time.py --logn 28 --reps 10"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-computing-mpi_amd"))
import torch  # noqa: E402

import misort  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--logn", type=int, default=28)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()
n = 1 << a.logn
U32 = torch.uint32 if hasattr(torch, "uint32") else torch.int32
ctx = misort.Context(0)
out = torch.empty(n, dtype=U32, device="cuda")
res = {}
for name in ("iid", "ascending", "descending", "constant"):
    if name == "iid":
        d = torch.empty(n, dtype=U32, device="cuda")
        ctx.fill_splitmix(d, 0x5EED0003)
    else:
        i = torch.arange(n, dtype=torch.int64, device="cuda") * ((1 << 32) // n)
        if name == "descending":
            i = i.flip(0)
        if name == "constant":
            i = torch.full_like(i, 0x5A5A5A5A)
        # the low 32 bits as they are (int32 wraps, the bit pattern is the u32 key)
        d = (i & 0xFFFFFFFF).to(torch.int64).contiguous().view(torch.int32)[::2].contiguous().view(U32)
        del i
    torch.cuda.synchronize()
    ms = []
    for r in range(a.reps + 2):
        torch.cuda.synchronize()
        ctx.synchronize()
        t0 = time.perf_counter()  # the sort runs on the context's own stream: host clock around its sync
        ctx.local_sort(d, out)
        ctx.synchronize()
        t1 = time.perf_counter()
        if r >= 2:  # two warm-up sorts
            ms.append((t1 - t0) * 1e3)
    chk = out.view(torch.int32)[:: max(1, n >> 16)].to(torch.int64) & 0xFFFFFFFF
    assert bool((chk[1:] >= chk[:-1]).all()), name
    ms.sort()
    res[name] = {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}
    del d
print(json.dumps({"logn": a.logn, "reps": a.reps, "library": os.path.basename(misort.library_path()), "local_sort": res}))
ctx.close()
