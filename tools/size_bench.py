#!/usr/bin/env python3
"""Sampling at other image sizes (sample_log(custom_shape=)): ms per image of guided DDIM-50 (scale 2.0, k = 4) + VQ-f4 decode at B = 8 on the
shipped synthetic models for 256 x 256 (the training size), 256 x 512, 512 x 256 and 512 x 512 images, and beside each size the rdm_prof
per-class table of a traced 2-step run + decode -- conv3x3 / linear / attention / GroupNorm / LayerNorm / Upsample convs with their share and
achieved rate, and the conv3x3 launches by GEMM shape (the strip form of conv_halo4 and the generic implicit GEMM show in the TFLOP/s).
Prints the tables on stderr and one JSON line (with the box's calibration probe) on stdout.

    python tools/size_bench.py [--batch 8] [--steps 50] [--reps 1] [256x256 256x512 ...]        (HEIGHTxWIDTH in pixels)
"""
import argparse
import collections
import csv
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KIND = {0: "conv3x3", 1: "linear", 2: "knn", 3: "attention", 4: "groupnorm", 5: "layernorm", 6: "upsconv"}
FLOP_KINDS = (0, 1, 3, 6)                       # work in FLOPs (the norms: bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", default=["256x256", "256x512", "512x256", "512x512"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=1, help="timed calls per size (after one warm-up call)")
    a = ap.parse_args()

    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, synthetic
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion

    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    d = ctx.device
    model = MinimalRETRODiffusion(unet_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, k_nn=4, ctx=ctx)
    model.load_unet_state_dict(synthetic.unet_state_dict(model.unet_cfg))
    model.load_first_stage_state_dict(synthetic.vq_state_dict(model.vq_cfg))
    f = 1 << (model.vq_cfg.n_ch_mult - 1)
    B = a.batch
    g = torch.Generator(device=d).manual_seed(0)
    cond = torch.randn(B, 4, 512, device=d, generator=g) * 0.45
    uncond = torch.zeros_like(cond)
    tf, gb = ctx.calib_probe()
    out = {"batch": B, "ddim_steps": a.steps, "scale": 2.0, "k": 4, "reps": a.reps, "ms_per_image": {}, "classes": {},
           "calibration": {"mfma_probe_tflops": round(tf, 1), "hbm_stream_gbps": round(gb, 1)}}

    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        shape = model._latent_shape((model.channels, H // f, W // f))
        x_T = torch.randn((B,) + shape, device=d, generator=g)

        def sample(S):
            z, _, _ = ctx.ddim_sample(S, x_T, cond, uncond, model.alphas_cumprod, eta=0.0, scale=2.0)
            return ctx.vq_decode(z)

        sample(2)                                # warm-up: arena, derived weights, K/V cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            img = sample(a.steps)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.reps
        assert tuple(img.shape[2:]) == (H, W) and bool(torch.isfinite(img).all())
        out["ms_per_image"][size] = round(dt * 1e3 / B, 2)
        # traced: 2 DDIM steps + the decode
        ctx.prof_reset()
        ctx.prof_enable(tuple(range(7)))
        sample(2)
        torch.cuda.synchronize()
        ctx.prof_enable(())
        with tempfile.TemporaryDirectory() as td:
            raw = os.path.join(td, "prof.csv")
            ctx.prof_dump(raw)
            rows = list(csv.DictReader(open(raw)))
        ctx.prof_reset()
        per_kind = collections.OrderedDict()
        convs = collections.OrderedDict()
        for r in rows:
            k = int(r["kind"])
            e = per_kind.setdefault(k, [0, 0.0, 0.0]); e[0] += 1; e[1] += float(r["ms"]); e[2] += float(r["work"])
            if k in (0, 6):
                c = convs.setdefault((KIND[k], int(r["d0"]), int(r["d1"]), int(r["d2"])), [0, 0.0, 0.0]); c[0] += 1; c[1] += float(r["ms"]); c[2] += float(r["work"])
        tot = sum(e[1] for e in per_kind.values())
        print(f"\n== {size}: {dt * 1e3:.1f} ms per call, {dt * 1e3 / B:.2f} ms per image (DDIM-{a.steps} + decode, B = {B}); traced 2 steps + decode: {tot:.2f} ms in bracketed launches",
              file=sys.stderr)
        print(f"{'class':10s} {'launches':>8s} {'ms':>9s} {'share':>6s} {'TF|TB/s':>8s}", file=sys.stderr)
        cls = {}
        for k, (n, ms, work) in sorted(per_kind.items(), key=lambda kv: -kv[1][1]):
            rate = work / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            print(f"{KIND.get(k, str(k)):10s} {n:8d} {ms:9.3f} {ms / tot:6.3f} {rate:8.2f}", file=sys.stderr)
            cls[KIND.get(k, str(k))] = {"launches": n, "ms": round(ms, 3), "share": round(ms / tot, 3), ("tflops" if k in FLOP_KINDS else "tbps"): round(rate, 2)}
        print(f"{'conv':8s} {'M x N x K':>26s} {'launches':>8s} {'ms':>9s} {'TFLOP/s':>8s}", file=sys.stderr)
        conv_rows = []
        for (kind, M, N, K), (n, ms, work) in sorted(convs.items(), key=lambda kv: -kv[1][1]):
            rate = work / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            print(f"{kind:8s} {f'{M} x {N} x {K}':>26s} {n:8d} {ms:9.3f} {rate:8.1f}", file=sys.stderr)
            conv_rows.append({"kind": kind, "M": M, "N": N, "K": K, "launches": n, "ms": round(ms, 3), "tflops": round(rate, 1)})
        out["classes"][size] = {"per_class": cls, "convs": conv_rows}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
