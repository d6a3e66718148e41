"""The native PLMS loop (rdm_plms_sample, fused update kernel) on the GPU: step by step against a torch restatement in deterministic mode,
PLMSSampler against a PLMS loop over the CPU oracle UNet, batch independence in deterministic mode, errors, and the end-to-end entry."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff
from oracle import unet as ounet
from oracle import vqdecoder as ovq

from _util import rel_l2, spec_to_unet_cfg, within

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

LATENT_TOL = 2.5e-2          # as test_gpu_surface.py's DDIM latent bound
UPDATE_TOL = 1e-5            # as the DDIM update in test_gpu_emul.py


_within = functools.partial(within, "plms")


@pytest.fixture(scope="module")
def tiny(ctx):
    from rdm_amd import packing
    spec = ounet.tiny_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234)
    cfg = spec_to_unet_cfg(spec)
    ctx.load_unet(cfg, packing.pack("unet", cfg, sd))
    return ctx, spec, sd


def _schedule(S):
    sched = odiff.Schedule()
    ts, a_t, a_prev, _, s1m = odiff.ddim_schedule(sched, S, 0.0)
    return sched, ts, a_t, a_prev, s1m


def _update(x, e, a_t, a_prev, s1m):
    """ldm get_x_prev_and_pred_x0 with sigma_t = 0, its scalars materialised as torch.full((b, 1, 1, 1), ...) on x's device."""
    full = lambda v: torch.full((x.shape[0], 1, 1, 1), float(v), device=x.device)
    a_t, a_prev, s1m = full(a_t), full(a_prev), full(s1m)
    x0 = (x - s1m * e) / a_t.sqrt()
    return a_prev.sqrt() * x0 + (1. - a_prev).sqrt() * e, x0


def _combine(e_t, old):
    if len(old) == 1:
        return (3 * e_t - old[-1]) / 2
    if len(old) == 2:
        return (23 * e_t - 16 * old[-1] + 5 * old[-2]) / 12
    return (55 * e_t - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24


def _plms_loop(eps, S, x_T, sched_parts):
    """ldm PLMS (eta = 0) over a guided-eps callable eps(x, t_int) -> e."""
    _, ts, a_t, a_prev, s1m = sched_parts
    total, time_range = len(ts), np.flip(ts)
    x, old = x_T, []
    for i, step in enumerate(time_range):
        index = total - i - 1
        e_t = eps(x, int(step))
        if not old:
            x_tmp, _ = _update(x, e_t, a_t[index], a_prev[index], s1m[index])
            e_p = (e_t + eps(x_tmp, int(time_range[min(i + 1, total - 1)]))) / 2
        else:
            e_p = _combine(e_t, old)
        x, _ = _update(x, e_p, a_t[index], a_prev[index], s1m[index])
        old = (old + [e_t])[-3:]
    return x


@pytest.mark.parametrize("hw", [16, 64])
def test_plms_steps_teacher_forced_deterministic(tiny, hw):
    """Every step of the native loop (S = 6: seven timesteps, all four branches; CFG 2.0; B = 3) rebuilt from the logged x_inter with
    ctx.unet_forward on [x | x] and [cond | uncond]: the step's x_inter and pred_x0 against the torch restatement of the update.  The
    restatement runs on the GPU: x_tmp feeds the t_next forward, and this synthetic UNet turns the ulp-level differences between the
    CPU's and the GPU's fp32 arithmetic in it (measured: rel 9e-8) into a percent-level change of e_next (measured: 9e-3)."""
    ctx, spec, _ = tiny
    g = torch.Generator().manual_seed(11 + hw)
    B, S, scale = 3, 6, 2.0
    x_T = torch.randn(B, 3, hw, hw, generator=g).to(ctx.device)
    cond = (torch.randn(B, 4, 512, generator=g) * 0.45).to(ctx.device)
    uncond = torch.zeros_like(cond)
    parts = _schedule(S)
    sched, ts, a_t, a_prev, s1m = parts
    ctx.set_deterministic(True)
    try:
        z, xi, pi = ctx.plms_sample(S, x_T, cond, uncond, sched.alphas_cumprod, scale=scale, log_every_t=1, want_intermediates=True)

        def eps(x, t):
            out = ctx.unet_forward(torch.cat([x, x]), torch.full((2 * B,), t, dtype=torch.long, device=x.device), torch.cat([cond, uncond]))
            return out[B:] + scale * (out[:B] - out[B:])

        total, time_range = len(ts), np.flip(ts)
        assert xi.shape[0] == pi.shape[0] == total == 7
        assert torch.equal(z, xi[-1])
        old = []
        worst = [0.0, 0.0]
        for i, step in enumerate(time_range):
            index = total - i - 1
            x = x_T if i == 0 else xi[i - 1]
            e_t = eps(x, int(step))
            if not old:
                x_tmp, _ = _update(x, e_t, a_t[index], a_prev[index], s1m[index])
                e_p = (e_t + eps(x_tmp, int(time_range[min(i + 1, total - 1)]))) / 2
            else:
                e_p = _combine(e_t, old)
            want_x, want_x0 = _update(x, e_p, a_t[index], a_prev[index], s1m[index])
            ex, e0 = rel_l2(xi[i], want_x), rel_l2(pi[i], want_x0)
            worst = [max(worst[0], ex), max(worst[1], e0)]
            assert ex <= UPDATE_TOL and e0 <= UPDATE_TOL, f"step {i} (history {len(old)}): x {ex:.3e}, pred_x0 {e0:.3e}"
            old = (old + [e_t])[-3:]
        print(f"[plms] {hw}x{hw} teacher-forced steps: worst x_inter {worst[0]:.3e}, pred_x0 {worst[1]:.3e} (bound {UPDATE_TOL:.0e})")
    finally:
        ctx.set_deterministic(False)


@pytest.fixture(scope="module")
def model(ctx):
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    spec, vspec = ounet.tiny_spec(), ovq.tiny_vq_spec()
    fs = {"params": {"embed_dim": 3, "n_embed": vspec.n_embed, "ddconfig": {"z_channels": 3, "ch": vspec.ch, "ch_mult": vspec.ch_mult,
                                                                          "num_res_blocks": vspec.num_res_blocks, "resolution": vspec.resolution}}}
    up = dict(in_channels=spec.in_channels, out_channels=spec.out_channels, model_channels=spec.model_channels,
              num_res_blocks=spec.num_res_blocks, attention_resolutions=spec.attention_resolutions, channel_mult=spec.channel_mult,
              num_head_channels=spec.num_head_channels, context_dim=spec.context_dim)
    m = MinimalRETRODiffusion(unet_config={"params": up}, first_stage_config=fs, k_nn=4, image_size=16, ctx=ctx)
    m.sd_unet = ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234)
    m.load_unet_state_dict(m.sd_unet)
    m.load_first_stage_state_dict(ounet.synth_state_dict(ovq.vq_param_shapes(vspec), seed=5))
    m.spec = spec
    return m


def test_plms_sampler_against_oracle_and_per_step_path(model):
    from rdm_amd.models.diffusion.plms import PLMSSampler
    rng = np.random.default_rng(8)
    B, S, scale = 2, 5, 2.0
    x_T = torch.from_numpy(rng.standard_normal((B, 3, 16, 16)).astype(np.float32)).to(model.device)
    cond = torch.from_numpy((rng.standard_normal((B, 4, 512)) * 0.45).astype(np.float32)).to(model.device)
    uc = torch.zeros_like(cond)
    sampler = PLMSSampler(model)
    z, inter = sampler.sample(S, B, (3, 16, 16), conditioning=cond, x_T=x_T, log_every_t=2, verbose=False,
                              unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    n_log = 1 + sum(1 for i in range(S) if (S - 1 - i) % 2 == 0 or i == 0)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == n_log and torch.equal(inter["x_inter"][0].cpu(), x_T.cpu())
    c_cpu, u_cpu = cond.cpu(), uc.cpu()

    def eps(x, t):
        out = ounet.unet_forward(model.sd_unet, model.spec, torch.cat([x, x]), torch.full((2 * B,), t, dtype=torch.long), torch.cat([c_cpu, u_cpu]))
        return out[B:] + scale * (out[:B] - out[B:])

    z_ref = _plms_loop(eps, S, x_T.cpu(), _schedule(S))
    _within("PLMSSampler.sample latent vs the oracle PLMS loop (5 steps, CFG 2.0)", rel_l2(z, z_ref), LATENT_TOL)
    seen = []
    z2, _ = sampler.sample(S, B, (3, 16, 16), conditioning=cond, x_T=x_T, verbose=False, unconditional_guidance_scale=scale,
                           unconditional_conditioning=uc, callback=seen.append)
    assert seen == list(range(S))
    _within("PLMSSampler per-step path vs the native loop", rel_l2(z2, z), 2e-2)


def test_plms_deterministic_rows_do_not_depend_on_the_batch(tiny):
    ctx, _, _ = tiny
    d = ctx.device
    g = torch.Generator(device=d).manual_seed(5)
    x = torch.randn(6, 3, 16, 16, device=d, generator=g)
    c = torch.randn(6, 4, 512, device=d, generator=g) * 0.45
    ac = odiff.Schedule().alphas_cumprod
    ctx.set_deterministic(True)
    try:
        z6 = ctx.plms_sample(5, x, c, torch.zeros_like(c), ac, scale=2.0)[0]
        for r in (0, 4):
            z1 = ctx.plms_sample(5, x[r:r + 1], c[r:r + 1], torch.zeros_like(c[r:r + 1]), ac, scale=2.0)[0]
            assert torch.equal(z1, z6[r:r + 1]), f"row {r}: batch 1 and batch 6 differ"
    finally:
        ctx.set_deterministic(False)


def test_plms_errors_leave_the_context_usable(tiny, model):
    from rdm_amd import _lib
    from rdm_amd._lib import RdmError
    from rdm_amd.models.diffusion.plms import PLMSSampler
    ctx, _, _ = tiny
    d = ctx.device
    x = torch.randn(2, 3, 16, 16, device=d)
    c = torch.randn(2, 4, 512, device=d) * 0.45
    ac = odiff.Schedule().alphas_cumprod
    # eta != 0 at the C ABI and at the sampler surface
    a = _lib.DdimArgs(S=4, batch=2, k=4, channels=3, height=16, width=16, eta=0.5, temperature=1.0, unconditional_guidance_scale=1.0,
                      log_every_t=100, T=1000, alphas_cumprod=np.ascontiguousarray(ac, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float)))
    z = torch.empty_like(x)
    with pytest.raises(RdmError, match="eta"):
        ctx._check(_lib.lib.rdm_plms_sample(ctx._h, C.byref(a), _lib._ptr(x), _lib._ptr(c), None, _lib._ptr(z), None, None))
    with pytest.raises(ValueError):
        PLMSSampler(model).sample(4, 2, (3, 16, 16), conditioning=c, x_T=x, eta=0.3, verbose=False)
    with pytest.raises(RdmError):
        ctx.plms_sample(4, x, c, None, ac, scale=2.0)                          # guidance without unconditional conditioning
    with pytest.raises(RdmError):
        ctx.plms_sample(4, x, c[:, :, :256].contiguous(), None, ac)           # wrong context width
    with pytest.raises(RdmError):
        ctx.plms_sample(4, x, c[:1], None, ac)                                # batch mismatch
    with pytest.raises(RdmError):
        ctx.plms_sample(4, x, c, torch.zeros(2, 3, 512, device=d), ac, scale=2.0)   # uncond shape
    with pytest.raises(RdmError):
        ctx.plms_sample(4, x[:, :2].contiguous(), c, None, ac)                # latent channels
    zz, _, _ = ctx.plms_sample(4, x, c, torch.zeros_like(c), ac, scale=2.0)
    torch.cuda.synchronize()
    assert zz.shape == x.shape and torch.isfinite(zz).all()


def test_sample_with_query_plms_end_to_end(model):
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    rng = np.random.default_rng(31)
    N = 2000
    pool = {"embedding": (rng.standard_normal((N, 512)) * 0.45).astype(np.float16), "img_id": np.arange(N),
            "patch_coords": rng.integers(0, 1200, (N, 4))}
    db = DatasetBuilder(data_pool=pool, k=20, ctx=model.ctx)
    db.train_searcher()
    model.retriever = db
    q = torch.from_numpy((rng.standard_normal((3, 512)) * 0.45).astype(np.float32))
    out = model.sample_with_query(query=q, query_embedded=True, k_nn=4, ddim=True, ddim_steps=4, plms=True,
                                  unconditional_guidance_scale=2.0, unconditional_retro_guidance_label=0., visualize_nns=False)
    img = out["query_samples"]
    assert img.shape == (3, 3, 64, 64) and torch.isfinite(img).all()
