#!/usr/bin/env python3
"""DDIM against PLMS and DPM-Solver++, native loops on the shipped synthetic UNet + VQ-f4 decoder at B = 64 (CFG 2.0, k = 4
neighbours; the UNet batch is the guided B' = 128): ms per image, VQ decode included, for each `name:S` given (default ddim:50 plms:50
plms:25).  PLMS with S timesteps runs S + 1 forwards; dpmpp:S is DPM-Solver++(2M) on the logSNR grid of S targets, whose real step
count (reported under "forwards") can come out below S; unipc:S is UniPC (order 2, bh2, with the corrector) on the same grid, one
forward per step like dpmpp.  Prints the box's calibration probe and one line per run on stderr, one JSON line on stdout.

    python tools/sampler_bench.py [--reps N] [--batch B] [ddim:50 plms:50 plms:25 dpmpp:20 ...]
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
    ap.add_argument("runs", nargs="*", default=["ddim:50", "plms:50", "plms:25"])
    ap.add_argument("--reps", type=int, default=2, help="timed calls per run (after one warm-up call)")
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()

    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, packing, synthetic
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion

    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    d = ctx.device
    model = MinimalRETRODiffusion(unet_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, k_nn=4, ctx=ctx)
    model.load_unet_state_dict(synthetic.unet_state_dict(model.unet_cfg))
    model.load_first_stage_state_dict(synthetic.vq_state_dict(model.vq_cfg))
    B = a.batch
    g = torch.Generator(device=d).manual_seed(0)
    x_T = torch.randn(B, 3, 64, 64, device=d, generator=g)
    cond = torch.randn(B, 4, 512, device=d, generator=g) * 0.45
    uncond = torch.zeros_like(cond)

    def sample(name, S):
        if name == "ddim":
            z, _, _ = ctx.ddim_sample(S, x_T, cond, uncond, model.alphas_cumprod, eta=0.0, scale=2.0)
        elif name == "plms":
            z, _, _ = ctx.plms_sample(S, x_T, cond, uncond, model.alphas_cumprod, scale=2.0)
        elif name == "dpmpp":
            z, _, _ = ctx.dpmpp_sample(ctx.dpmpp_timesteps(S, model.alphas_cumprod), x_T, cond, uncond, model.alphas_cumprod, scale=2.0)
        elif name == "unipc":
            z, _, _ = ctx.unipc_sample(ctx.dpmpp_timesteps(S, model.alphas_cumprod), x_T, cond, uncond, model.alphas_cumprod, scale=2.0)
        else:
            raise SystemExit(f"unknown sampler {name!r} (ddim | plms | dpmpp | unipc)")
        return ctx.vq_decode(z)

    def forwards(name, S):
        if name in ("dpmpp", "unipc"):
            return len(ctx.dpmpp_timesteps(S, model.alphas_cumprod)) - 1
        return S + (1 if name == "plms" else 0)

    tf, gb = ctx.calib_probe()
    print(f"calibration: mfma probe {tf:.1f} TFLOP/s, hbm stream {gb:.1f} GB/s", file=sys.stderr, flush=True)
    out = {"batch": B, "scale": 2.0, "k": 4, "reps": a.reps, "calibration": {"mfma_probe_tflops": round(tf, 1), "hbm_stream_gbps": round(gb, 1)},
           "ms_per_image": {}, "forwards": {}}
    for run in a.runs:
        name, S = run.split(":")
        S = int(S)
        sample(name, S)                      # warm-up: scratch, tables, K/V cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            img = sample(name, S)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.reps
        assert torch.isfinite(img).all()
        out["ms_per_image"][run] = round(dt * 1e3 / B, 3)
        out["forwards"][run] = forwards(name, S)
        print(f"{run}: {dt * 1e3:.1f} ms per call, {dt * 1e3 / B:.3f} ms per image", file=sys.stderr, flush=True)
    ms = out["ms_per_image"]
    if "ddim:50" in ms and "plms:25" in ms:
        out["speedup_plms25_over_ddim50"] = round(ms["ddim:50"] / ms["plms:25"], 3)
    if "ddim:50" in ms and "dpmpp:20" in ms:
        out["speedup_dpmpp20_over_ddim50"] = round(ms["ddim:50"] / ms["dpmpp:20"], 3)
    if "dpmpp:20" in ms and "unipc:10" in ms:
        out["speedup_unipc10_over_dpmpp20"] = round(ms["dpmpp:20"] / ms["unipc:10"], 3)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
