#!/usr/bin/env python3
"""The metric kernels (csrc/metrics.hip) against their torch restatement on the same card, at n = m = 50 000 rows of d = 512:

  radius + hits   Context.op_knn_radius + Context.op_manifold_hits           vs   torch.cdist in row blocks + kthvalue / any
  moments         Context.op_moments_f64                                     vs   fp64 matmul in row blocks (x.double().T @ x.double())
  hits / counts / nearest   Context.op_manifold_hits / op_manifold_counts / op_nearest_d2 on given radii (the three share one loop)
                                                                             vs   torch.cdist in row blocks + any / sum / min
  KID             rdm_amd.metrics.kernel_distance (Context.op_poly3_rowsums) at `--kid_subsets` x `--kid_subset_size` rows, and at subsets = 0
                  on the whole sets                                          vs   fp32 matmul in row blocks, then the same fp64 pointwise
                                                                                  arithmetic and reduction, on the same subset draw

Both sides produce the same results (k-NN radii of the reference set, hit flags / counts / nearest distances of the probe set, fp64
moments, KID mean and std); the comparison is kernel against torch chain, never kernel against kernel.  Prints the box's calibration probe and one line per side on stderr (ms per call
and the peak of torch.cuda.max_memory_allocated() over the timed calls; the library's own scratch, 4 bytes per row, is not torch's),
one JSON line on stdout.  There is no threshold: the acceptance bar of these kernels is correctness (tests/test_gpu_metrics.py).

    python tools/metrics_bench.py [--n 50000] [--m 50000] [--d 512] [--k 3] [--reps 3] [--block 2048] [--kid_subsets 100] [--kid_subset_size 1000]
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
    ap.add_argument("--kid_subsets", type=int, default=100)
    ap.add_argument("--kid_subset_size", type=int, default=1000)
    a = ap.parse_args()

    import numpy as np
    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, metrics

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

    # hits, counts and nearest alone, on the radii of one op_knn_radius call scaled so that a probe lies in a few balls
    radii = ctx.op_knn_radius(ref, a.k) * 1.02

    def kernel_hits():
        return ctx.op_manifold_hits(probe, ref, radii)

    def kernel_counts():
        return ctx.op_manifold_counts(probe, ref, radii)

    def kernel_nearest():
        return ctx.op_nearest_d2(probe, ref)

    def torch_counts():
        cnt = torch.empty(a.m, device=dev, dtype=torch.int32)
        for lo in range(0, a.m, a.block):
            cnt[lo:lo + a.block] = (torch.cdist(probe[lo:lo + a.block], ref) ** 2 <= radii[None, :]).sum(dim=1)
        return cnt

    def torch_nearest():
        best = torch.empty(a.m, device=dev)
        for lo in range(0, a.m, a.block):
            best[lo:lo + a.block] = (torch.cdist(probe[lo:lo + a.block], ref) ** 2).min(dim=1).values
        return best

    # KID: the kernel path is rdm_amd.metrics.kernel_distance as shipped; the torch side restates it on the same subset draw
    gamma, coef0 = 1.0 / a.d, 1.0

    def torch_poly_sum(x, y, excl):
        """SUM_ij (gamma x_i . y_j + coef0)^3 in fp64 from fp32 matmuls in row blocks, without i == j when excl"""
        tot = torch.zeros((), device=dev, dtype=torch.float64)
        for lo in range(0, x.shape[0], a.block):
            kv = (x[lo:lo + a.block] @ y.T).double() * gamma + coef0
            kv = kv * kv * kv
            if excl:
                rows = torch.arange(kv.shape[0], device=dev)
                keep = rows + lo < y.shape[0]
                kv[rows[keep], rows[keep] + lo] = 0.0
            tot += kv.sum()
        return tot

    def torch_kid_one(x, y):
        m_, n_ = x.shape[0], y.shape[0]
        return torch_poly_sum(x, x, True) / (m_ * (m_ - 1.0)) + torch_poly_sum(y, y, True) / (n_ * (n_ - 1.0)) - 2.0 * torch_poly_sum(x, y, False) / (float(m_) * n_)

    def kernel_kid_subsets():
        return metrics.kernel_distance(ctx, ref, probe, subsets=a.kid_subsets, subset_size=a.kid_subset_size, seed=0)

    def torch_kid_subsets():
        s_ = min(a.kid_subset_size, a.n, a.m)
        rng = np.random.default_rng(0)
        vals = []
        for _ in range(a.kid_subsets):
            ix = torch.from_numpy(rng.choice(a.n, s_, replace=False)).to(dev); iy = torch.from_numpy(rng.choice(a.m, s_, replace=False)).to(dev)
            vals.append(torch_kid_one(ref[ix], probe[iy]))
        vals = torch.stack(vals).cpu().numpy()
        return float(vals.mean()), float(vals.std())

    def kernel_kid_whole():
        return metrics.kernel_distance(ctx, ref, probe, subsets=0)

    def torch_kid_whole():
        return float(torch_kid_one(ref, probe)), 0.0

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
    kid_sub = f"KID {a.kid_subsets}x{a.kid_subset_size}"
    for name, fn in (("kernel radius+hits", kernel_pr), ("torch radius+hits", torch_pr), ("kernel moments", kernel_moments), ("torch moments", torch_moments),
                     ("kernel hits", kernel_hits), ("kernel counts", kernel_counts), ("torch counts", torch_counts), ("kernel nearest", kernel_nearest),
                     ("torch nearest", torch_nearest), ("kernel hits (again)", kernel_hits), (f"kernel {kid_sub}", kernel_kid_subsets),
                     (f"torch {kid_sub}", torch_kid_subsets), ("kernel KID whole sets", kernel_kid_whole), ("torch KID whole sets", torch_kid_whole)):
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
    kc, tc, kn, tn = res["kernel counts"], res["torch counts"], res["kernel nearest"], res["torch nearest"]
    (kks, kkstd), (tks, tkstd), (kkw, _), (tkw, _) = res[f"kernel {kid_sub}"], res[f"torch {kid_sub}"], res["kernel KID whole sets"], res["torch KID whole sets"]
    out["agreement"].update({"mean_count_kernel": float(kc.float().mean()), "mean_count_torch": float(tc.float().mean()), "counts_differ": int((kc != tc).sum()),
                             "counts_positive_equal_hits": bool(torch.equal(kc > 0, res["kernel hits"] > 0)),
                             "nearest_max_rel": float(((kn - tn).abs() / tn).max()), "kid_subsets_kernel": [kks, kkstd], "kid_subsets_torch": [tks, tkstd],
                             "kid_whole_kernel": kkw, "kid_whole_torch": tkw})
    for what in ("counts", "nearest", kid_sub, "KID whole sets"):
        out[f"speedup_{what}"] = round(out["ms"][f"torch {what}"] / out["ms"][f"kernel {what}"], 2)
    out["hits_run_to_run_spread_ms"] = round(abs(out["ms"]["kernel hits"] - out["ms"]["kernel hits (again)"]), 2)
    print(f"agreement: {out['agreement']}", file=sys.stderr, flush=True)
    print(f"hits {out['ms']['kernel hits']:.2f} ms (again: {out['ms']['kernel hits (again)']:.2f}), counts {out['ms']['kernel counts']:.2f} ms, nearest "
          f"{out['ms']['kernel nearest']:.2f} ms: one loop, three epilogues; counts {out['speedup_counts']}x, nearest {out['speedup_nearest']}x, {kid_sub} "
          f"{out['speedup_' + kid_sub]}x, KID whole sets {out['speedup_KID whole sets']}x the torch chain", file=sys.stderr, flush=True)
    print(f"radius + hits: kernel {out['speedup_radius_hits']}x the torch chain ({out['kernel_radius_hits_tflops']} TFLOP/s fp32); moments: kernel "
          f"{out['speedup_moments']}x the torch chain ({out['kernel_moments_tflops']} TFLOP/s fp64)", file=sys.stderr, flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
