#!/usr/bin/env python3
"""How far DDIM inversion and DDIM decoding carry a difference in eps, on the tiny synthetic UNet of the tests (S = 5, B = 2, 16 x 16
latents, k = 4): relative L2 after 1 .. 5 steps of

  * the native loops against the restated loops over the CPU oracle UNet (fp32): the bf16 forward's error, as each loop carries it;
  * the native inversion against the same loop restated on the GPU with the UNet through (a) rdm_unet_forward_guided, the loops' own
    forward, which DDIMSampler.encode's per-step path takes, and (b) rdm_unet_forward on the doubled batch [x | x], [cond | uncond]: the
    same function through other kernel configurations (every sample's own prefix, no zero-context shortcut, per-row time embedding);
  * the native decode against DDIMSampler.decode's per-step path (rdm_unet_forward on the doubled batch),

guided (CFG 2.0) and unguided, in the default and in the deterministic mode, for three input seeds.  A step up the schedule carries an eps
difference on undamped (the weight of eps in x_next grows while x's shrinks); a step down contracts it.

    python tools/img2img_drift_probe.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    from oracle import diffusion as odiff, unet as ounet
    import _img2img_ref as ref
    from _util import rel_l2

    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    spec = ounet.tiny_spec()
    up = dict(in_channels=spec.in_channels, out_channels=spec.out_channels, model_channels=spec.model_channels,
              num_res_blocks=spec.num_res_blocks, attention_resolutions=spec.attention_resolutions, channel_mult=spec.channel_mult,
              num_head_channels=spec.num_head_channels, context_dim=spec.context_dim)
    m = MinimalRETRODiffusion(unet_config={"params": up}, first_stage_config=None, k_nn=4, image_size=16, ctx=ctx)
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234)
    m.load_unet_state_dict(sd)
    acp = odiff.Schedule().alphas_cumprod
    B, S = 2, 5
    sched = ref.schedule(acp, S)
    tf, gb = ctx.calib_probe()
    print(f"calibration: mfma probe {tf:.1f} TFLOP/s, hbm stream {gb:.1f} GB/s", flush=True)
    row = lambda vals: "  ".join(f"{v:.2e}" for v in vals)
    for seed in (10, 11, 12):
        rng = np.random.default_rng(seed)
        x0 = torch.from_numpy((rng.standard_normal((B, 3, 16, 16)) * 0.5).astype(np.float32)).to(m.device)
        x_l = torch.from_numpy(rng.standard_normal((B, 3, 16, 16)).astype(np.float32)).to(m.device)
        cond = torch.from_numpy((rng.standard_normal((B, 4, 512)) * 0.45).astype(np.float32)).to(m.device)
        uc = torch.zeros_like(cond)
        c_cpu, u_cpu = cond.cpu(), uc.cpu()

        def oracle(x, t, scale):
            if scale == 1.0:
                return ounet.unet_forward(sd, spec, x, torch.full((B,), t, dtype=torch.long), c_cpu)
            out = ounet.unet_forward(sd, spec, torch.cat([x, x]), torch.full((2 * B,), t, dtype=torch.long), torch.cat([c_cpu, u_cpu]))
            return out[B:] + scale * (out[:B] - out[B:])

        def gpu(x, t, which):
            tt = torch.full((2 * B,), t, dtype=torch.long, device=x.device)
            out = ctx.unet_forward_guided(x, t, cond, uc) if which == "guided" else ctx.unet_forward(torch.cat([x, x]), tt, torch.cat([cond, uc]))
            return out[B:] + 2.0 * (out[:B] - out[B:])

        for det in (False, True):
            ctx.set_deterministic(det)
            sm = DDIMSampler(m)
            sm.make_schedule(S, verbose=False)
            kw = dict(unconditional_guidance_scale=2.0, unconditional_conditioning=uc)
            mode = "deterministic" if det else "default"
            enc = {n: sm.encode(x0, cond, n, **kw)[0] for n in range(1, 6)}
            enc1 = {n: sm.encode(x0, cond, n)[0] for n in range(1, 6)}
            dec = {n: sm.decode(x_l, cond, n, **kw) for n in range(1, 6)}
            print(f"seed {seed} {mode} mode, after 1 .. 5 steps")
            print("  encode CFG 2.0  native vs oracle loop          ", row(rel_l2(enc[n], ref.encode(lambda x, t: oracle(x, t, 2.0), x0.cpu(), sched, n)[0]) for n in enc))
            print("  encode unguided native vs oracle loop          ", row(rel_l2(enc1[n], ref.encode(lambda x, t: oracle(x, t, 1.0), x0.cpu(), sched, n)[0]) for n in enc1))
            print("  encode CFG 2.0  native vs loop on forward (a)  ", row(rel_l2(enc[n], ref.encode(lambda x, t: gpu(x, t, "guided"), x0, sched, n)[0]) for n in enc))
            print("  encode CFG 2.0  native vs loop on forward (b)  ", row(rel_l2(enc[n], ref.encode(lambda x, t: gpu(x, t, "plain"), x0, sched, n)[0]) for n in enc))
            print("  encode CFG 2.0  native vs the per-step path    ", row(rel_l2(enc[n], sm.encode(x0, cond, n, callback=lambda i: None, **kw)[0]) for n in enc))
            print("  decode CFG 2.0  native vs oracle loop          ", row(rel_l2(dec[n], ref.decode(lambda x, t: oracle(x, t, 2.0), x_l.cpu(), sched, n)[0]) for n in dec))
            print("  decode CFG 2.0  native vs the per-step path    ", row(rel_l2(dec[n], sm.decode(x_l, cond, n, callback=lambda i: None, **kw)) for n in dec), flush=True)
        ctx.set_deterministic(False)
    ctx.close()


if __name__ == "__main__":
    main()
