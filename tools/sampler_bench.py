#!/usr/bin/env python3
"""DDIM against PLMS and DPM-Solver++, native loops on the shipped synthetic UNet + VQ-f4 decoder at B = 64 (CFG 2.0, k = 4
neighbours; the UNet batch is the guided B' = 128): ms per image, VQ decode included, for each `name:S` given (default ddim:50 plms:50
plms:25).  PLMS with S timesteps runs S + 1 forwards; dpmpp:S is DPM-Solver++(2M) on the logSNR grid of S targets, whose real step
count (reported under "forwards") can come out below S; unipc:S is UniPC (order 2, bh2, with the corrector) on the same grid, one
forward per step like dpmpp.  The stochastic loops come in two forms: ddimeta:S (DDIM, eta = 1) and ddpm:S (ancestral DDPM, unguided)
draw the starting latents and the [S, B, 3, 64, 64] noise stack per call the way MinimalRETRODiffusion._sample_shard does (one torch
generator per sample row, then the transposed copy) and time that with the loop; ddimeta_rng:S and ddpm_rng:S are the seeded entries,
whose step kernels generate the noise (no x_T, no stack); dpmpp_sde:S is SDE-DPM-Solver++(2M) on dpmpp's grid through its seeded entry
(fresh noise every step, generated in the step kernel; no x_T, no stack).  Every line also carries the peak of torch.cuda.max_memory_allocated() over the
timed calls.  Image-to-image: img2img:S:STRENGTH encodes a [B, 3, 256, 256] image batch with the first-stage encoder, noises the latent to
n = min(total, max(1, int(STRENGTH * total))) steps up the S-step schedule with the seeded forward process (no noise tensor) and runs
the native decode from there -- n forwards; invert:S:STRENGTH takes the latent there by n steps of native DDIM inversion (unguided)
instead -- 2 n forwards; inpaint:S:STRENGTH is img2img with a centred square mask (the middle quarter of the latent is repainted, the
rest kept): the native inpainting loop through its seeded entry -- n forwards and n blend passes whose known-region noise is generated
in the blend kernel, then the keep-known blend; inpaint_stack:S:STRENGTH is the same loop fed with an [n, B, 3, 64, 64] torch.randn
stack for that noise, drawn per call as DDIMSampler.decode draws it without a seed.  The encoder's own ms per image is reported under "vq_encode_ms_per_image".  A spec given twice is timed twice (the second under `name:S#2`): the box's own A/A spread.  Prints the box's calibration
probe and one line per run on stderr, one JSON line on stdout.

    python tools/sampler_bench.py [--reps N] [--batch B] [ddim:50 plms:50 plms:25 dpmpp:20 ddpm:250 ddpm:250 ddpm_rng:250 ...]
    python tools/sampler_bench.py ddim:50 ddim:50 img2img:50:0.6 invert:50:0.6
    python tools/sampler_bench.py ddim:50 img2img:50:0.6 img2img:50:0.6 inpaint:50:0.6 inpaint_stack:50:0.6
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
    from rdm_amd import _lib, packing, parallel, synthetic
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion

    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    d = ctx.device
    model = MinimalRETRODiffusion(unet_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, k_nn=4, ctx=ctx)
    model.load_unet_state_dict(synthetic.unet_state_dict(model.unet_cfg))
    fsd = synthetic.vq_state_dict(model.vq_cfg)
    FROM_IMAGE = ("img2img", "invert", "inpaint", "inpaint_stack")
    from_image = any(run.split(":")[0] in FROM_IMAGE for run in a.runs)
    if from_image:
        fsd.update(synthetic.vq_encoder_state_dict(model.vq_cfg))
    model.load_first_stage_state_dict(fsd)
    B = a.batch
    g = torch.Generator(device=d).manual_seed(0)
    x_T = torch.randn(B, 3, 64, 64, device=d, generator=g)
    cond = torch.randn(B, 4, 512, device=d, generator=g) * 0.45
    uncond = torch.zeros_like(cond)
    image = torch.rand(B, 3, 256, 256, device=d, generator=g) * 2 - 1 if from_image else None
    keep = torch.ones(B, 1, 64, 64, device=d)               # 1 = keep the init latent; the centred 32 x 32 square is repainted
    keep[:, :, 16:48, 16:48] = 0.0

    def steps_of(S, strength):
        total = len(range(0, model.num_timesteps, model.num_timesteps // S))
        return min(total, max(1, int(strength * total))), total

    sched_ddpm = {n: getattr(model, n).numpy() for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                                          "posterior_mean_coef2", "posterior_log_variance_clipped")}
    calls = [0]

    def stack(steps):
        """The starting latents and the noise stack of one call, as _sample_shard draws them."""
        calls[0] += 1
        x = parallel.per_sample_noise(1000 + calls[0], range(B), (3, 64, 64), device=d)
        nz = parallel.per_sample_noise(1001 + calls[0], range(B), (steps, 3, 64, 64), device=d)
        return x, nz.transpose(0, 1).contiguous()

    def sample(name, S, strength=None):
        if name in FROM_IMAGE:
            import numpy as np
            calls[0] += 1
            n, total = steps_of(S, strength)
            lat = ctx.vq_encode(image)
            if name == "invert":
                start, _ = ctx.ddim_encode(S, n, lat, cond, None, model.alphas_cumprod)
            else:
                a_n = float(model.alphas_cumprod[range(0, model.num_timesteps, model.num_timesteps // S)[n - 1] + 1])
                start = ctx.op_q_sample_seeded(lat, np.sqrt(a_n), np.sqrt(1.0 - a_n), 1000 + calls[0], out=None if "inpaint" in name else lat)
            if name == "inpaint":
                z, _, _ = ctx.ddim_inpaint(S, n, start, lat, keep, cond, uncond, model.alphas_cumprod, eta=0.0, scale=2.0, seed=1000 + calls[0])
            elif name == "inpaint_stack":
                z, _, _ = ctx.ddim_inpaint(S, n, start, lat, keep, cond, uncond, model.alphas_cumprod, eta=0.0, scale=2.0,
                                           q_noise=torch.randn((n,) + tuple(lat.shape), device=d))
            else:
                z, _, _ = ctx.ddim_decode(S, n, start, cond, uncond, model.alphas_cumprod, eta=0.0, scale=2.0)
            if "inpaint" in name:
                ctx.op_masked_blend(z, lat, keep, None, 1.0, 0.0, out=z)
        elif name == "ddimeta":
            x, nz = stack(S)
            z, _, _ = ctx.ddim_sample(S, x, cond, uncond, model.alphas_cumprod, eta=1.0, scale=2.0, noise=nz)
        elif name == "ddimeta_rng":
            calls[0] += 1
            z, _, _ = ctx.ddim_sample(S, None, cond, uncond, model.alphas_cumprod, eta=1.0, scale=2.0, seed=1000 + calls[0], shape=(3, 64, 64))
        elif name == "ddpm":
            x, nz = stack(S)
            z = ctx.ddpm_sample(S, x, cond, nz, sched_ddpm, clip_denoised=True)
        elif name == "ddpm_rng":
            calls[0] += 1
            z = ctx.ddpm_sample(S, None, cond, None, sched_ddpm, clip_denoised=True, seed=1000 + calls[0], shape=(3, 64, 64))
        elif name == "ddim":
            z, _, _ = ctx.ddim_sample(S, x_T, cond, uncond, model.alphas_cumprod, eta=0.0, scale=2.0)
        elif name == "plms":
            z, _, _ = ctx.plms_sample(S, x_T, cond, uncond, model.alphas_cumprod, scale=2.0)
        elif name == "dpmpp":
            z, _, _ = ctx.dpmpp_sample(ctx.dpmpp_timesteps(S, model.alphas_cumprod), x_T, cond, uncond, model.alphas_cumprod, scale=2.0)
        elif name == "dpmpp_sde":
            calls[0] += 1
            z, _, _ = ctx.dpmpp_sde_sample(ctx.dpmpp_timesteps(S, model.alphas_cumprod), None, cond, uncond, model.alphas_cumprod, scale=2.0,
                                           seed=1000 + calls[0], shape=(3, 64, 64))
        elif name == "unipc":
            z, _, _ = ctx.unipc_sample(ctx.dpmpp_timesteps(S, model.alphas_cumprod), x_T, cond, uncond, model.alphas_cumprod, scale=2.0)
        else:
            raise SystemExit(f"unknown sampler {name!r} (ddim | plms | dpmpp | dpmpp_sde | unipc | ddimeta | ddimeta_rng | ddpm | ddpm_rng | "
                             "img2img:S:STRENGTH | invert:S:STRENGTH | inpaint:S:STRENGTH | inpaint_stack:S:STRENGTH)")
        return ctx.vq_decode(z)

    def forwards(name, S, strength=None):
        if name in FROM_IMAGE:
            return steps_of(S, strength)[0] * (2 if name == "invert" else 1)
        if name in ("dpmpp", "dpmpp_sde", "unipc"):
            return len(ctx.dpmpp_timesteps(S, model.alphas_cumprod)) - 1
        return S + (1 if name == "plms" else 0)

    tf, gb = ctx.calib_probe()
    print(f"calibration: mfma probe {tf:.1f} TFLOP/s, hbm stream {gb:.1f} GB/s", file=sys.stderr, flush=True)
    out = {"batch": B, "scale": 2.0, "k": 4, "reps": a.reps, "calibration": {"mfma_probe_tflops": round(tf, 1), "hbm_stream_gbps": round(gb, 1)},
           "ms_per_image": {}, "forwards": {}, "peak_torch_mib": {}}
    for n_run, run in enumerate(a.runs):
        name, S, *rest = run.split(":")
        S = int(S)
        if (name in FROM_IMAGE) != (len(rest) == 1):
            raise SystemExit(f"{run!r}: img2img, invert, inpaint and inpaint_stack take name:S:STRENGTH, the other samplers name:S")
        strength = float(rest[0]) if rest else None
        if strength is not None and not 0.0 < strength <= 1.0:
            raise SystemExit(f"{run!r}: STRENGTH must lie in (0, 1]")
        if run in a.runs[:n_run]:
            run = f"{run}#{a.runs[:n_run].count(run) + 1}"
        sample(name, S, strength)            # warm-up: scratch, tables, K/V cache
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            img = sample(name, S, strength)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.reps
        assert torch.isfinite(img).all()
        out["ms_per_image"][run] = round(dt * 1e3 / B, 3)
        out["forwards"][run] = forwards(name, S, strength)
        peak = torch.cuda.max_memory_allocated() / 2 ** 20
        out["peak_torch_mib"][run] = round(peak, 1)
        del img
        print(f"{run}: {dt * 1e3:.1f} ms per call, {dt * 1e3 / B:.3f} ms per image, peak torch memory {peak:.1f} MiB", file=sys.stderr, flush=True)
    if from_image:                           # the first-stage encoder alone: what an image-to-image call adds to its n forwards
        ctx.vq_encode(image)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            ctx.vq_encode(image)
        torch.cuda.synchronize()
        out["vq_encode_ms_per_image"] = round((time.perf_counter() - t0) / a.reps * 1e3 / B, 3)
        print(f"vq_encode: {out['vq_encode_ms_per_image']:.3f} ms per image", file=sys.stderr, flush=True)
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
