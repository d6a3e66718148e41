#!/usr/bin/env python3
"""Filtered exact-kNN timing at the OpenImages DB size (20,927,907 x 512 fp16, the size of tools/knn_bench.py): ms per call of
  * the unfiltered search (rdm_knn),
  * the filtered search (rdm_knn_filtered) with ONE mask at densities 1, 1/2 and 1/1000,
  * the filtered search with 64 DIFFERENT masks at density 1/1000 (query j names mask j % 64),
for B = 64 (the dim-512 online scan) and B = 512 (the bulk scan).  What the filter costs is the difference to the unfiltered line of the
same run; the alternative it replaces is another rdm_db_load of the 21 GB database per subset.  Also prints what a live-tile list would
walk: the share of 256-row tiles that hold at least one allowed row, per mask.  Prints the box's calibration probe first.

usage: knn_filter_bench.py [N [k [reps]]]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rdm_amd  # noqa: F401
from rdm_amd import _lib

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20_927_907
k = int(sys.argv[2]) if len(sys.argv) > 2 else 4
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
ctx = _lib.Context(0)
d = ctx.device
tf, gb = ctx.calib_probe()
print(f"calibration: mfma probe {tf:.1f} TFLOP/s, hbm stream {gb:.1f} GB/s", flush=True)
g = torch.Generator(device=d).manual_seed(7)
db = torch.empty((N, 512), device=d, dtype=torch.float16)
for r0 in range(0, N, 1 << 20):
    r1 = min(N, r0 + (1 << 20))
    db[r0:r1] = (torch.randn((r1 - r0, 512), device=d, generator=g) * 0.45).half()
ctx.db_load(db)
del db
torch.cuda.empty_cache()


def mask(density):
    if density >= 1.0:
        return torch.full((_lib.knn_mask_words(N),), -1, dtype=torch.int64, device=d)
    return ctx.row_mask(torch.rand(N, device=d, generator=g) < density)


def live_tiles(bits):
    """share of the 256-row tiles with at least one allowed row (bits beyond N belong to the last tile, which holds rows anyway)"""
    return float((bits.reshape(-1, 4) != 0).any(dim=1).float().mean())


masks = {"1": mask(1.0), "1/2": mask(0.5), "1/1000": mask(1e-3)}
many = torch.stack([mask(1e-3) for _ in range(64)])
counts = ctx.row_mask_count(torch.stack(list(masks.values())))
print("allowed rows: " + ", ".join(f"density {n}: {c}" for n, c in zip(masks, counts)) + f"; 64 masks at 1/1000: {ctx.row_mask_count(many).mean():.0f} on average")
print("tiles with an allowed row: " + ", ".join(f"density {n}: {live_tiles(m):.4f}" for n, m in masks.items()))


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


out = {"n": N, "k": k, "reps": reps, "calibration": {"mfma_probe_tflops": round(tf, 1), "hbm_stream_gbps": round(gb, 1)}, "ms": {}}
for B in (64, 512):
    q = torch.randn((B, 512), device=d, generator=g) * 0.45
    ids = (torch.arange(B) % 64).numpy()
    path = _lib.knn_select(N, 512, B, k)["path"]
    cases = [("unfiltered", lambda: ctx.knn(q, k))]
    cases += [(f"one mask, density {n}", lambda m=m: ctx.knn(q, k, allow=m)) for n, m in masks.items()]
    cases += [("64 masks, density 1/1000", lambda: ctx.knn(q, k, allow=many, mask_of_query=ids)),
              ("unfiltered again", lambda: ctx.knn(q, k))]
    for name, fn in cases:
        ms = timed(fn)
        out["ms"][f"B{B} {name}"] = round(ms, 3)
        print(f"B={B} ({path}) k={k} {name}: {ms:.3f} ms per call (fallback {ctx.knn_last_fallback()})", flush=True)
print(json.dumps(out))
