#!/usr/bin/env python3
"""The metric kernels (csrc/metrics.hip) against their torch restatement on the same card, at n = m = 50 000 rows of d = 512:

  radius + hits   Context.op_knn_radius + Context.op_manifold_hits           vs   torch.cdist in row blocks + kthvalue / any
  moments         Context.op_moments_f64                                     vs   fp64 matmul in row blocks (x.double().T @ x.double())

Both sides produce the same three results (k-NN radii of the reference set, hit flags of the probe set, fp64 moments); the comparison is
kernel against torch chain, never kernel against kernel.  Prints the box's calibration probe and one line per side on stderr (ms per call
and the peak of torch.cuda.max_memory_allocated() over the timed calls; the library's own scratch, 4 bytes per row, is not torch's),
one JSON line on stdout.  There is no threshold: the acceptance bar of these kernels is correctness (tests/test_gpu_metrics.py).

    python tools/metrics_bench.py [--n 50000] [--m 50000] [--d 512] [--k 3] [--reps 3] [--block 2048]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=50000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=2048, help="rows per torch.cdist / matmul block")
    a = ap.parse_args()

    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib

    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.randn(a.n, a.d, device=dev, generator=g) * 0.45
    probe = torch.randn(a.m, a.d, device=dev, generator=g) * 0.45 * 0.98

    def kernel_pr():
        r2 = ctx.op_knn_radius(ref, a.k)
        return r2, ctx.op_manifold_hits(probe, ref, r2)

    def torch_pr():
        r2 = torch.empty(a.n, device=dev)
        for lo in range(0, a.n, a.block):
            dist = torch.cdist(ref[lo:lo + a.block], ref)
            rows = torch.arange(dist.shape[0], device=dev)
            dist[rows, rows + lo] = float("inf")                        # self, by index
            r2[lo:lo + a.block] = dist.kthvalue(a.k, dim=1).values ** 2
        hit = torch.empty(a.m, device=dev, dtype=torch.uint8)
        for lo in range(0, a.m, a.block):
            hit[lo:lo + a.block] = (torch.cdist(probe[lo:lo + a.block], ref) ** 2 <= r2[None, :]).any(dim=1)
        return r2, hit

    def kernel_moments():
        s = torch.zeros(a.d, device=dev, dtype=torch.float64); o = torch.zeros(a.d, a.d, device=dev, dtype=torch.float64)
        ctx.op_moments_f64(ref, s, o)
        return s, o

    def torch_moments():
        s = torch.zeros(a.d, device=dev, dtype=torch.float64); o = torch.zeros(a.d, a.d, device=dev, dtype=torch.float64)
        for lo in range(0, a.n, a.block):
            xb = ref[lo:lo + a.block].double()
            s += xb.sum(0); o += xb.T @ xb
        return s, o

    def timed(fn):
        out = fn()                                                      # warm-up: scratch, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.reps * 1e3
        return out, round(ms, 2), round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    tf, gb = ctx.calib_probe()
    print(f"calibration: mfma probe {tf:.1f} TFLOP/s, hbm stream {gb:.1f} GB/s", file=sys.stderr, flush=True)
    print(f"n = {a.n}, m = {a.m}, d = {a.d}, k = {a.k}, {a.reps} timed calls after one warm-up, torch blocks of {a.block} rows", file=sys.stderr, flush=True)
    out = {"n": a.n, "m": a.m, "d": a.d, "k": a.k, "reps": a.reps, "block": a.block,
           "calibration": {"mfma_probe_tflops": round(tf, 1), "hbm_stream_gbps": round(gb, 1)}, "ms": {}, "peak_torch_mib_over_inputs": {}}
    res = {}
    for name, fn in (("kernel radius+hits", kernel_pr), ("torch radius+hits", torch_pr), ("kernel moments", kernel_moments), ("torch moments", torch_moments)):
        res[name], out["ms"][name], out["peak_torch_mib_over_inputs"][name] = timed(fn)
        print(f"{name}: {out['ms'][name]:.2f} ms per call, peak torch memory over the inputs {out['peak_torch_mib_over_inputs'][name]:.1f} MiB", file=sys.stderr, flush=True)
    (kr, kh), (tr, th) = res["kernel radius+hits"], res["torch radius+hits"]
    (ks, ko), (ts, to) = res["kernel moments"], res["torch moments"]
    flop = 2.0 * a.d * (float(a.n) * a.n + float(a.m) * a.n)
    out["kernel_radius_hits_tflops"] = round(flop / out["ms"]["kernel radius+hits"] / 1e9, 1)
    out["kernel_moments_tflops"] = round(2.0 * a.n * a.d * a.d / out["ms"]["kernel moments"] / 1e9, 2)
    out["speedup_radius_hits"] = round(out["ms"]["torch radius+hits"] / out["ms"]["kernel radius+hits"], 2)
    out["speedup_moments"] = round(out["ms"]["torch moments"] / out["ms"]["kernel moments"], 2)
    # agreement of the two sides (not a test: cdist's own arithmetic differs): radii relative, hit flags, moments relative
    out["agreement"] = {"radius2_max_rel": float(((kr - tr).abs() / tr).max()), "hit_rate_kernel": float(kh.float().mean()), "hit_rate_torch": float(th.float().mean()),
                        "hits_differ": int((kh != th).sum()), "outer_max_rel": float(((ko - to).abs().max() / to.abs().max())), "sum_max_rel": float(((ks - ts).abs().max() / ts.abs().max()))}
    print(f"agreement: {out['agreement']}", file=sys.stderr, flush=True)
    print(f"radius + hits: kernel {out['speedup_radius_hits']}x the torch chain ({out['kernel_radius_hits_tflops']} TFLOP/s fp32); moments: kernel "
          f"{out['speedup_moments']}x the torch chain ({out['kernel_moments_tflops']} TFLOP/s fp64)", file=sys.stderr, flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
