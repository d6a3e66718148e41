#!/usr/bin/env python3
"""Distances between the samplers of ONE model, in CLIP-feature FID, KID, precision / recall and density / coverage (rdm_amd.metrics): the shipped synthetic UNet
+ VQ-f4 decoder at B = 64 (CFG 2.0, k = 4 neighbours) draws the same seeds -- starting latents and conditioning from the library's
counter-based generator, rows 0 .. seeds - 1 of `--noise_seed` -- with DDIM-200 as the converged stand-in, then again with each `name:S`
given (default ddim:50 plms:25 dpmpp:20 unipc:10 unipc:8; dpmpp_sde:S is SDE-DPM-Solver++(2M), whose per-step noise is the generator's
stream 1 under `noise_seed` for the same rows, and ddimeta:S is DDIM with eta = 1 on the same noise: the two stochastic samplers, whose images are
not paired with the reference's seed by seed), and every set is compared with the DDIM-200 set on the features of the
synthetic CLIP ViT-B/32 image tower.  At the default 2048 rows of 512 features a covariance has four rows per dimension and the Frechet
distance is biased; KID (mean +- std over `--kid_subsets` subsets of `--kid_subset_size` rows) is not.  Precision and recall OR over the
reference balls and saturate; density counts the balls and coverage uses the reference set's balls alone (k = `--dc_k`).

With random weights these numbers are NOT image quality: they say how far a sampler's output distribution lies from the converged
sampler's of the same model, in the units a trained checkpoint would be reported in.  Prints the box's calibration probe and one line
per sampler on stderr, one JSON line on stdout.

    python tools/sampler_quality.py [--seeds 2048] [--batch 64] [--reference ddim:200] [--kid_subsets 100] [--kid_subset_size 1000] [--dc_k 5]
                                    [ddim:50 plms:25 ...]
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
    ap.add_argument("runs", nargs="*", default=["ddim:50", "plms:25", "dpmpp:20", "unipc:10", "unipc:8"])
    ap.add_argument("--reference", default="ddim:200")
    ap.add_argument("--seeds", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--noise_seed", type=int, default=2024)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--kid_subsets", type=int, default=100)
    ap.add_argument("--kid_subset_size", type=int, default=1000)
    ap.add_argument("--kid_seed", type=int, default=0)
    ap.add_argument("--dc_k", type=int, default=5)
    a = ap.parse_args()
    if a.seeds % a.batch:
        raise SystemExit("--seeds must be a multiple of --batch")

    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, metrics, synthetic
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    from rdm_amd.modules.retrievers import ClipImageRetriever

    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    model = MinimalRETRODiffusion(unet_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, k_nn=4, ctx=ctx)
    model.load_unet_state_dict(synthetic.unet_state_dict(model.unet_cfg))
    model.load_first_stage_state_dict(synthetic.vq_state_dict(model.vq_cfg))
    clip = ClipImageRetriever(state_dict=synthetic.clip_state_dict(_lib.make_clip_cfg()), ctx=ctx)
    B, acp = a.batch, model.alphas_cumprod

    def sample(name, S, row0):
        """Rows row0 .. row0 + B - 1: the start is stream 0 of the generator under `noise_seed` (what the seeded DDIM entry draws), the
        conditioning the same rows under `noise_seed + 1`."""
        x_T = ctx.op_randn(a.noise_seed, B, 3 * 64 * 64, row0=row0).view(B, 3, 64, 64)
        cond = ctx.op_randn(a.noise_seed + 1, B, 4 * 512, row0=row0).view(B, 4, 512) * 0.45
        uncond = torch.zeros_like(cond)
        if name == "ddim":
            z, _, _ = ctx.ddim_sample(S, x_T, cond, uncond, acp, eta=0.0, scale=2.0)
        elif name == "plms":
            z, _, _ = ctx.plms_sample(S, x_T, cond, uncond, acp, scale=2.0)
        elif name == "dpmpp":
            z, _, _ = ctx.dpmpp_sample(ctx.dpmpp_timesteps(S, acp), x_T, cond, uncond, acp, scale=2.0)
        elif name == "dpmpp_sde":
            z, _, _ = ctx.dpmpp_sde_sample(ctx.dpmpp_timesteps(S, acp), x_T, cond, uncond, acp, scale=2.0, seed=a.noise_seed, row0=row0)
        elif name == "ddimeta":
            z, _, _ = ctx.ddim_sample(S, x_T, cond, uncond, acp, eta=1.0, scale=2.0, seed=a.noise_seed, row0=row0)
        elif name == "unipc":
            z, _, _ = ctx.unipc_sample(ctx.dpmpp_timesteps(S, acp), x_T, cond, uncond, acp, scale=2.0)
        else:
            raise SystemExit(f"unknown sampler {name!r} (ddim | ddimeta | plms | dpmpp | dpmpp_sde | unipc)")
        return ctx.vq_decode(z).clamp_(-1.0, 1.0)

    def features(run):
        name, S = run.split(":")
        t0 = time.perf_counter()
        stats, feats = metrics.FeatureStats(clip.model.cfg.embed_dim), []
        for row0 in range(0, a.seeds, B):
            f = metrics.clip_features(clip, sample(name, int(S), row0), batch=B)
            stats.update(ctx, f)
            feats.append(f)
            if (row0 // B) % 8 == 7:
                torch.cuda.synchronize()
                print(f"  {run}: {row0 + B} of {a.seeds} images, {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
        f = torch.cat(feats)
        assert bool(torch.isfinite(f).all())
        return stats, f

    tf, gb = ctx.calib_probe()
    print(f"calibration: mfma probe {tf:.1f} TFLOP/s, hbm stream {gb:.1f} GB/s", file=sys.stderr, flush=True)
    print(f"{a.seeds} seeds (noise_seed {a.noise_seed}, rows 0..{a.seeds - 1}), B = {B}, CFG 2.0, synthetic UNet / VQ-f4 / CLIP ViT-B/32 weights: "
          f"distances between samplers of one model, not image quality", file=sys.stderr, flush=True)
    ref_stats, ref_f = features(a.reference)
    out = {"seeds": a.seeds, "batch": B, "noise_seed": a.noise_seed, "k": a.k, "reference": a.reference, "features": "clip-vit-b32-synthetic, un-normalised",
           "calibration": {"mfma_probe_tflops": round(tf, 1), "hbm_stream_gbps": round(gb, 1)},
           "kid_subsets": a.kid_subsets, "kid_subset_size": a.kid_subset_size, "kid_seed": a.kid_seed, "dc_k": a.dc_k,
           "trace_cov_reference": round(float(ref_stats.cov().trace()), 4), "fid": {}, "kid": {}, "kid_std": {}, "precision": {}, "recall": {},
           "density": {}, "coverage": {}}
    for run in a.runs:
        stats, f = features(run)
        fid = metrics.frechet_distance(ref_stats, stats)
        p, r = metrics.precision_recall(ctx, ref_f, f, k=a.k)
        kid, kid_std = metrics.kernel_distance(ctx, ref_f, f, subsets=a.kid_subsets, subset_size=a.kid_subset_size, seed=a.kid_seed)
        dens, cov = metrics.density_coverage(ctx, ref_f, f, k=a.dc_k)
        out["fid"][run], out["precision"][run], out["recall"][run] = round(fid, 5), round(p, 4), round(r, 4)
        out["kid"][run], out["kid_std"][run], out["density"][run], out["coverage"][run] = float(f"{kid:.5e}"), float(f"{kid_std:.3e}"), round(dens, 4), round(cov, 4)
        print(f"{run} against {a.reference}: FID {fid:.5f} (Tr Sigma of the reference {out['trace_cov_reference']}), KID {kid:.5e} +- {kid_std:.2e}, "
              f"precision {p:.4f}, recall {r:.4f}, density {dens:.4f}, coverage {cov:.4f}", file=sys.stderr, flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
