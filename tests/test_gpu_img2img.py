"""Native DDIM image-to-image on the GPU (rdm_ddim_decode, stack and seeded, / rdm_ddim_encode, the inversion step kernel, the
seeded forward process): the two kernels per element against float64, decode against the DDIM loop bit for bit, the tail property,
every inversion step rebuilt on the GPU, DDIMSampler.encode / decode against the per-step path and the CPU oracle UNet, the end-to-end
entry, errors, and one script run.  tests/_img2img_ref.py is the restatement."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import clip as oclip
from oracle import diffusion as odiff
from oracle import unet as ounet
from oracle import vqdecoder as ovq

import _img2img_ref as ref
from _util import rel_l2, spec_to_clip_cfg, within
from test_gpu_plms import model, tiny  # noqa: F401  (fixtures: the tiny UNet on the session context, the tiny model)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATENT_TOL = 2.5e-2          # as test_gpu_surface.py's DDIM latent bound
UPDATE_TOL = 1e-5            # as the DDIM update in test_gpu_emul.py and the PLMS update in test_gpu_plms.py
ACP = odiff.Schedule().alphas_cumprod
U = 2.0 ** -24

_within = functools.partial(within, "img2img")


def _inputs(ctx, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, 16, 16, generator=g).to(ctx.device)
    cond = (torch.randn(B, 4, 512, generator=g) * 0.45).to(ctx.device)
    return x, cond, torch.zeros_like(cond)


# ---- 1. the inversion step kernel alone
@pytest.mark.parametrize("config", ["guided_all_outputs", "unguided_bare", "guided_in_place"])
@pytest.mark.parametrize("n,offset", [(1027, 0), (4096, 0), (2 * 1024 * 1024 + 4, 0), (2304, 1)],
                         ids=["n1027_scalar_tail", "n4096_vector", "n2Mplus4_second_stride", "n2304_misaligned_scalar"])
def test_inverse_step_kernel_per_element_against_fp64(ctx, n, offset, config):
    """|got - ref| <= 16 * 2^-24 * A per element, A = (sa_n / sa_c) (|x| + s1m_c EA) + s1m_n EA with EA = |e_u| + s (|e_c| + |e_u|) or
    |e_c|: the float64 sum of the absolute values of every term entering the element; 16 is test_gpu_dpmpp.py's factor (fewer roundings
    occur here).  The scalars are step 5 of the S = 10 schedule.  n = 2 * 1024 * 1024 + 4 is one float4 group past 2048 blocks x 256
    threads; offset 1 puts an n % 4 == 0 call on the scalar path."""
    d = ctx.device
    g = torch.Generator(device=d).manual_seed(n + offset)
    cfg = config != "unguided_bare"
    scale = 2.0 if cfg else 1.0
    _, a_t, a_prev = ref.schedule(ACP, 10)
    f32 = lambda v: float(np.float32(v))
    sa_c, s1m_c, sa_n, s1m_n = f32(np.sqrt(a_prev[5])), f32(np.sqrt(1 - a_prev[5])), f32(np.sqrt(a_t[5])), f32(np.sqrt(1 - a_t[5]))
    rnd = lambda m: torch.randn(m, device=d, generator=g)
    x = rnd(n + offset)[offset:]
    assert x.data_ptr() % 16 == 4 * offset and x.is_contiguous()
    eps = rnd(2 * n if cfg else n)
    X = x.double()
    nan = lambda: torch.full((n,), float("nan"), device=d)
    x_out = x if config == "guided_in_place" else nan()
    x_dup, pred_x0 = (nan(), nan()) if config == "guided_all_outputs" else (None, None)
    ctx.op_ddim_inverse_step(x, eps, cfg, scale, sa_c, s1m_c, sa_n, s1m_n, x_out, x_dup=x_dup, pred_x0=pred_x0)
    torch.cuda.synchronize()

    e_c = eps[:n].double()
    if cfg:
        e_u = eps[n:].double()
        E, EA = e_u + scale * (e_c - e_u), e_u.abs() + scale * (e_c.abs() + e_u.abs())
    else:
        E, EA = e_c, e_c.abs()
    P = (X - s1m_c * E) / sa_c
    want = sa_n * P + s1m_n * E
    A_p = (X.abs() + s1m_c * EA) / sa_c
    A = sa_n * A_p + s1m_n * EA
    worst = float(((x_out.double() - want).abs() / A).max())
    print(f"[img2img] inverse step n={n} offset={offset} {config}: worst |got - ref| / A = {worst / U:.2f} * 2^-24 (bound 16)")
    assert torch.isfinite(x_out).all()
    assert ((x_out.double() - want).abs() <= 16.0 * U * A).all()
    if x_dup is not None:
        assert torch.isfinite(pred_x0).all()
        assert torch.equal(x_dup, x_out)
        assert ((pred_x0.double() - P).abs() <= 16.0 * U * A_p).all()


# ---- 2. the seeded forward process
def test_q_sample_seeded_against_op_randn(ctx):
    """B = 3, per_row = 768, row0 = 5: |got - (sa x0 + s1m z)| <= 4 * 2^-24 (|sa x0| + |s1m z|) with z = op_randn(seed, stream 0) -- two
    products and a sum, one rounding each; rows drawn in two calls are the rows of one call; a per_row that is no multiple of 4 and a
    misaligned out are refused and leave the context usable."""
    from rdm_amd._lib import RdmError
    d = ctx.device
    seed, B, per_row, row0 = 0x1234_5678_9ABC, 3, 768, 5
    x0 = torch.randn(B, 3, 16, 16, device=d, generator=torch.Generator(device=d).manual_seed(1))
    sa, s1m = float(np.float32(np.sqrt(float(ACP[601])))), float(np.float32(np.sqrt(1.0 - float(ACP[601]))))
    got = ctx.op_q_sample_seeded(x0, sa, s1m, seed, row0=row0)
    z = ctx.op_randn(seed, B, per_row, row0=row0, step=0, stream=0).reshape(x0.shape)
    a, b = sa * x0.double(), s1m * z.double()
    worst = float(((got.double() - (a + b)).abs() / (a.abs() + b.abs())).max())
    print(f"[img2img] q_sample_seeded: worst |got - ref| / (|sa x0| + |s1m z|) = {worst / U:.2f} * 2^-24 (bound 4)")
    assert got.shape == x0.shape and torch.isfinite(got).all()
    assert ((got.double() - (a + b)).abs() <= 4.0 * U * (a.abs() + b.abs())).all()
    two = torch.cat([ctx.op_q_sample_seeded(x0[:2].contiguous(), sa, s1m, seed, row0=row0),
                     ctx.op_q_sample_seeded(x0[2:].contiguous(), sa, s1m, seed, row0=row0 + 2)])
    assert torch.equal(two, got)
    assert not torch.equal(ctx.op_q_sample_seeded(x0, sa, s1m, seed, row0=row0 + 1), got)
    with pytest.raises(RdmError, match="multiple of 4"):
        ctx.op_q_sample_seeded(torch.zeros(3, 770, device=d), sa, s1m, seed)
    buf = torch.zeros(B * per_row + 4, device=d)
    with pytest.raises(RdmError, match="aligned"):
        ctx.op_q_sample_seeded(x0, sa, s1m, seed, row0=row0, out=buf[1:1 + B * per_row])
    assert torch.equal(ctx.op_q_sample_seeded(x0, sa, s1m, seed, row0=row0, out=buf[4:]).reshape(x0.shape), got)


# ---- 3. decode is the DDIM loop
S6_TOTAL = 7            # S = 6 on T = 1000: seven timesteps


@pytest.fixture(scope="module")
def full_runs(tiny):
    """The whole-schedule runs the decode tests compare with, computed once in deterministic mode: S = 6, B = 3, CFG 2.0,
    log_every_t = 1, at eta = 0 and at eta = 0.7 on a stack."""
    ctx, _, _ = tiny
    x_T, cond, uncond = _inputs(ctx, 3, 41)
    noise = torch.randn(S6_TOTAL, 3, 3, 16, 16, generator=torch.Generator().manual_seed(42)).to(ctx.device)
    ctx.set_deterministic(True)
    try:
        runs = {eta: ctx.ddim_sample(6, x_T, cond, uncond, ACP, eta=eta, scale=2.0, noise=noise if eta else None, log_every_t=1,
                                     want_intermediates=True) for eta in (0.0, 0.7)}
    finally:
        ctx.set_deterministic(False)
    assert runs[0.0][1].shape[0] == S6_TOTAL
    return x_T, cond, uncond, noise, runs


@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_decode_of_the_whole_schedule_is_ddim_sample_bitwise(tiny, full_runs, eta):
    ctx, _, _ = tiny
    x_T, cond, uncond, noise, runs = full_runs
    ctx.set_deterministic(True)
    try:
        z, xi, pi = ctx.ddim_decode(6, S6_TOTAL, x_T, cond, uncond, ACP, eta=eta, scale=2.0, noise=noise if eta else None, log_every_t=1,
                                    want_intermediates=True)
        z3, xi3, pi3 = ctx.ddim_decode(6, S6_TOTAL, x_T, cond, uncond, ACP, eta=eta, scale=2.0, noise=noise if eta else None, log_every_t=3,
                                       want_intermediates=True)
        w3 = ctx.ddim_sample(6, x_T, cond, uncond, ACP, eta=eta, scale=2.0, noise=noise if eta else None, log_every_t=3, want_intermediates=True)
    finally:
        ctx.set_deterministic(False)
    for got, want in zip((z, xi, pi, z3, xi3, pi3), runs[eta] + w3):
        assert got.shape == want.shape and torch.equal(got, want)
    assert not torch.equal(runs[0.0][0], runs[0.7][0])


def test_seeded_decode_of_the_whole_schedule_is_ddim_sample_seeded_bitwise(tiny, full_runs):
    ctx, _, _ = tiny
    x_T, cond, uncond, _, runs = full_runs
    ctx.set_deterministic(True)
    try:
        want = ctx.ddim_sample(6, x_T, cond, uncond, ACP, eta=0.7, scale=2.0, log_every_t=1, want_intermediates=True, seed=99, row0=3)
        got = ctx.ddim_decode(6, S6_TOTAL, x_T, cond, uncond, ACP, eta=0.7, scale=2.0, log_every_t=1, want_intermediates=True, seed=99, row0=3)
        # a seeded partial decode counts its own steps from 0: the stack of op_randn(step = i) fed to the stack entry
        stack = torch.stack([ctx.op_randn(99, 3, 768, row0=3, step=i, stream=1).reshape(3, 3, 16, 16) for i in range(4)])
        part_seeded = ctx.ddim_decode(6, 4, x_T, cond, uncond, ACP, eta=0.7, scale=2.0, seed=99, row0=3)[0]
        part_stack = ctx.ddim_decode(6, 4, x_T, cond, uncond, ACP, eta=0.7, scale=2.0, noise=stack)[0]
    finally:
        ctx.set_deterministic(False)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(want[0], runs[0.7][0])
    assert torch.equal(part_seeded, part_stack)


# ---- 4. the tail property
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_decode_from_a_logged_iterate_finishes_the_full_run(tiny, full_runs, eta):
    """xi[j] of the full run is at level index total - 2 - j: decode(t_start = total - 1 - j) from it, fed the stack's tail, returns the
    full run's z bit for bit."""
    ctx, _, _ = tiny
    _, cond, uncond, noise, runs = full_runs
    z, xi, pi = runs[eta]
    ctx.set_deterministic(True)
    try:
        for j in (0, 2, 4):
            n = S6_TOTAL - 1 - j
            got, gx, gp = ctx.ddim_decode(6, n, xi[j], cond, uncond, ACP, eta=eta, scale=2.0, noise=noise[j + 1:] if eta else None,
                                          log_every_t=1, want_intermediates=True)
            assert torch.equal(got, z), f"j = {j}"
            assert gx.shape[0] == n and torch.equal(gx, xi[j + 1:]) and torch.equal(gp, pi[j + 1:])
    finally:
        ctx.set_deterministic(False)


# ---- 5. the inversion loop, step by step
def _encode_teacher_forced(ctx, S, x0, cond, uncond, scale):
    """Every step rebuilt ON THE GPU from the logged iterate with ctx.unet_forward at ts[i] and the torch restatement (a CPU
    restatement would feed ulp-level differences into the next forward of this synthetic UNet: see test_gpu_plms.py).  -> the worst
    rel-L2 per timestep choice."""
    B = x0.shape[0]
    sched = ref.schedule(ACP, S)
    ts, a_t, a_prev = sched
    total = len(ts)
    z, xi = ctx.ddim_encode(S, total, x0, cond, uncond, ACP, scale=scale, log_every_t=1, want_intermediates=True)
    assert xi.shape[0] == total and torch.equal(z, xi[-1])

    def eps(x, t):
        tt = torch.full(((2 if uncond is not None else 1) * B,), t, dtype=torch.long, device=x.device)
        if uncond is None:
            return ctx.unet_forward(x, tt, cond)
        out = ctx.unet_forward(torch.cat([x, x]), tt, torch.cat([cond, uncond]))
        return out[B:] + scale * (out[:B] - out[B:])

    worst = {"target": 0.0, "current": 0.0, "index": 0.0}
    for i in range(total):
        x = x0 if i == 0 else xi[i - 1]
        for which in worst:
            want, _ = ref.inverse_step(x, eps(x, ref.encode_timestep(ts, i, which)), float(a_prev[i]), float(a_t[i]))
            e = rel_l2(xi[i], want)
            worst[which] = max(worst[which], e)
            if which == "target":
                assert e <= UPDATE_TOL, f"step {i}: {e:.3e}"
    return worst


@pytest.mark.parametrize("guided", [True, False])
def test_encode_steps_teacher_forced_deterministic(tiny, guided):
    """Guided B = 3 and unguided B = 1 at S = 6 (seven steps).  The same rebuild with the forward taken at the current level's timestep,
    or at ldm's t = i, misses the bound at some step: the loop runs the UNet at the TARGET timestep."""
    ctx, _, _ = tiny
    x0, cond, uncond = _inputs(ctx, 3 if guided else 1, 51 + guided)
    ctx.set_deterministic(True)
    try:
        worst = _encode_teacher_forced(ctx, 6, x0 * 0.5, cond, uncond if guided else None, 2.0 if guided else 1.0)
    finally:
        ctx.set_deterministic(False)
    print(f"[img2img] encode teacher-forced (guided {guided}): worst target {worst['target']:.3e} (bound {UPDATE_TOL:.0e}); "
          f"current-level timestep {worst['current']:.3e}, t = i {worst['index']:.3e}")
    assert worst["current"] > UPDATE_TOL and worst["index"] > UPDATE_TOL


def test_encode_intermediates_follow_the_ascending_rule(tiny):
    ctx, _, _ = tiny
    x0, cond, _ = _inputs(ctx, 1, 53)
    ctx.set_deterministic(True)
    try:
        z, every = ctx.ddim_encode(6, 5, x0, cond, None, ACP, log_every_t=1, want_intermediates=True)
        z2, some = ctx.ddim_encode(6, 5, x0, cond, None, ACP, log_every_t=3, want_intermediates=True)
        z3, none = ctx.ddim_encode(6, 5, x0, cond, None, ACP)
    finally:
        ctx.set_deterministic(False)
    assert every.shape[0] == 5 and none is None and torch.equal(z, z2) and torch.equal(z, z3)
    assert some.shape[0] == 3 and torch.equal(some, every[[0, 3, 4]])          # i % 3 == 0 or i == t_enc - 1


# ---- 6. the sampler surface
@pytest.fixture(scope="module")
def surface(model):
    """S = 5, B = 2, CFG 2.0: the sampler with its schedule, the inputs, and the guided / unguided eps of the CPU oracle UNet."""
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    rng = np.random.default_rng(10)
    B = 2
    x0 = torch.from_numpy((rng.standard_normal((B, 3, 16, 16)) * 0.5).astype(np.float32)).to(model.device)
    x_l = torch.from_numpy(rng.standard_normal((B, 3, 16, 16)).astype(np.float32)).to(model.device)
    cond = torch.from_numpy((rng.standard_normal((B, 4, 512)) * 0.45).astype(np.float32)).to(model.device)
    uc = torch.zeros_like(cond)
    sm = DDIMSampler(model)
    sm.make_schedule(5, verbose=False)
    assert sm.ddim_timesteps.shape[0] == 5
    c_cpu, u_cpu = cond.cpu(), uc.cpu()

    def eps(x, t, scale=2.0):
        if scale == 1.0:
            return ounet.unet_forward(model.sd_unet, model.spec, x, torch.full((B,), t, dtype=torch.long), c_cpu)
        out = ounet.unet_forward(model.sd_unet, model.spec, torch.cat([x, x]), torch.full((2 * B,), t, dtype=torch.long), torch.cat([c_cpu, u_cpu]))
        return out[B:] + scale * (out[:B] - out[B:])

    return sm, x0, x_l, cond, uc, eps, ref.schedule(ACP, 5)


def test_sampler_encode_against_the_per_step_path_and_the_oracle(model, surface):
    """DDIMSampler.encode in the default mode, CFG 2.0, t_enc = 3 (the latent decode(t_start = 3) below expects: n of strength 0.6 at
    S = 5), against the per-step path (2e-2) and against the restated loop over the CPU oracle UNet (LATENT_TOL); the same two at the
    inversion's default scale 1.0.  The per-step path's guided forward is the native loops' (apply_model_guided): through
    unet_forward on the doubled batch it ended 2.5e-2 from the native loop here, because a step up the schedule carries an eps
    difference on undamped (tools/img2img_drift_probe.py, profiles/img2img_drift_probe.log)."""
    sm, x0, _, cond, uc, eps, sched = surface
    kw = dict(unconditional_guidance_scale=2.0, unconditional_conditioning=uc)
    z, out = sm.encode(x0, cond, 3, return_intermediates=2, **kw)
    assert out["intermediate_steps"] == [0, 1, 2] and len(out["intermediates"]) == 3 and torch.equal(out["intermediates"][-1], z)
    z4, out4 = sm.encode(x0, cond, 4, return_intermediates=2, **kw)
    assert out4["intermediate_steps"] == [0, 2, 3] and len(out4["intermediates"]) == 3
    seen = []
    z_ps, out_ps = sm.encode(x0, cond, 3, return_intermediates=2, callback=seen.append, **kw)
    assert seen == list(range(3)) and len(out_ps["intermediates"]) == 3
    _within("DDIMSampler.encode native loop vs the per-step path (t_enc 3, CFG 2.0)", rel_l2(z, z_ps), 2e-2)
    z_ref, _ = ref.encode(eps, x0.cpu(), sched, 3)
    _within("DDIMSampler.encode latent vs the restated loop over the oracle UNet (t_enc 3, CFG 2.0)", rel_l2(z, z_ref), LATENT_TOL)
    z1, _ = sm.encode(x0, cond, 3)
    z1_ps, _ = sm.encode(x0, cond, 3, callback=lambda i: None)
    _within("DDIMSampler.encode native loop vs the per-step path (t_enc 3, unguided)", rel_l2(z1, z1_ps), 2e-2)
    z1_ref, _ = ref.encode(lambda x, t: eps(x, t, 1.0), x0.cpu(), sched, 3)
    _within("DDIMSampler.encode latent vs the restated loop over the oracle UNet (t_enc 3, unguided)", rel_l2(z1, z1_ref), LATENT_TOL)


def test_unet_forward_guided_is_the_loops_forward(model, surface):
    """rdm_unet_forward_guided against the oracle UNet on the doubled batch (2.5e-2, the UNet forward's bound in test_gpu_models.py); one
    DDIM step rebuilt from it equals the native loop's first logged step to UPDATE_TOL in the default mode -- rebuilt from unet_forward
    it need not; in deterministic mode it is unet_forward on [x | x], [cond | uncond] bit for bit; bad arguments leave the context usable."""
    from rdm_amd._lib import RdmError
    sm, _, x_l, cond, uc, _, sched = surface
    ctx, B = model.ctx, x_l.shape[0]
    ts, a_t, a_prev = sched
    t = int(ts[-1])
    tt = torch.full((2 * B,), t, dtype=torch.long, device=x_l.device)
    out = ctx.unet_forward_guided(x_l, t, cond, uc)
    want = ounet.unet_forward(model.sd_unet, model.spec, torch.cat([x_l, x_l]).cpu(), tt.cpu(), torch.cat([cond, uc]).cpu())
    assert out.shape == want.shape
    _within("unet_forward_guided vs the oracle UNet on the doubled batch", rel_l2(out, want), 2.5e-2)
    _, xi, _ = ctx.ddim_sample(5, x_l, cond, uc, ACP, scale=2.0, log_every_t=1, want_intermediates=True)
    step = lambda o: ref.ddim_step(x_l, o[B:] + 2.0 * (o[:B] - o[B:]), float(a_t[-1]), float(a_prev[-1]))[0]
    plain = ctx.unet_forward(torch.cat([x_l, x_l]), tt, torch.cat([cond, uc]))
    print(f"[img2img] first DDIM step rebuilt from unet_forward on the doubled batch: {rel_l2(xi[0], step(plain)):.3e}")
    _within("first DDIM step of the native loop rebuilt from unet_forward_guided", rel_l2(xi[0], step(out)), UPDATE_TOL)
    ctx.set_deterministic(True)
    try:
        assert torch.equal(ctx.unet_forward_guided(x_l, t, cond, uc), ctx.unet_forward(torch.cat([x_l, x_l]), tt, torch.cat([cond, uc])))
    finally:
        ctx.set_deterministic(False)
    for bad in (lambda: ctx.unet_forward_guided(x_l, -1, cond, uc), lambda: ctx.unet_forward_guided(x_l, t, cond, uc[:1]),
                lambda: ctx.unet_forward_guided(x_l, t, cond[:, :, :256].contiguous(), uc[:, :, :256].contiguous())):
        with pytest.raises(RdmError):
            bad()
        assert torch.equal(ctx.unet_forward_guided(x_l, t, cond, uc), out)


def test_sampler_decode_against_the_per_step_path_and_the_oracle(model, surface):
    sm, _, x_l, cond, uc, eps, sched = surface
    kw = dict(unconditional_guidance_scale=2.0, unconditional_conditioning=uc)
    d, inter = sm.decode(x_l, cond, 3, log_every_t=2, return_intermediates=True, **kw)
    n_log = 1 + sum(1 for index in range(3) if index % 2 == 0 or index == 2)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == n_log == 3 and torch.equal(inter["x_inter"][0], x_l)
    assert torch.equal(sm.decode(x_l, cond, 3, **kw), d)
    seen = []
    d_ps = sm.decode(x_l, cond, 3, callback=seen.append, **kw)
    assert seen == list(range(3))
    _within("DDIMSampler.decode native loop vs the per-step path (t_start 3, CFG 2.0)", rel_l2(d, d_ps), 2e-2)
    d_ref, _, _ = ref.decode(eps, x_l.cpu(), sched, 3)
    _within("DDIMSampler.decode latent vs the restated loop over the oracle UNet", rel_l2(d, d_ref), LATENT_TOL)


# ---- 7. end to end
@pytest.fixture(scope="module")
def i2i_model(model, ctx):
    """The tiny model with the first-stage encoder loaded beside the decoder (as tests/test_gpu_training.py loads both halves), a
    one-layer CLIP for the caption and a 2000-row database."""
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    from rdm_amd.modules.retrievers import ClipImageRetriever
    vspec = ovq.tiny_vq_spec()
    model.load_first_stage_state_dict({**ounet.synth_state_dict(ovq.vq_param_shapes(vspec), seed=5),
                                       **ounet.synth_state_dict(ovq.vq_encoder_param_shapes(vspec), seed=17)})
    spec = oclip.ClipSpec(embed_dim=512, image_resolution=64, vision_layers=1, vision_width=128, vision_patch_size=32,
                          context_length=77, vocab_size=49408, transformer_width=128, transformer_heads=2, transformer_layers=1)
    sd = ounet.synth_state_dict(oclip.clip_param_shapes(spec), seed=3)
    sd["positional_embedding"] = sd["positional_embedding"] * 0.1
    rng = np.random.default_rng(33)
    pool = {"embedding": (rng.standard_normal((2000, 512)) * 0.45).astype(np.float16), "img_id": np.arange(2000),
            "patch_coords": np.zeros((2000, 4), np.int64)}
    db = DatasetBuilder(data_pool=pool, k=20, retriever=ClipImageRetriever(state_dict=sd, ctx=ctx, clip_cfg=spec_to_clip_cfg(spec)), ctx=ctx)
    db.train_searcher()
    model.retriever = db
    f = vspec.resolution // 16
    image = torch.from_numpy(rng.uniform(-1, 1, (2, 16 * f, 16 * f, 3)).astype(np.float32))
    return model, db, image


def test_sample_with_query_image_to_image_end_to_end(i2i_model):
    from rdm_amd import parallel
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    m, db, image = i2i_model
    kw = dict(query="a caption", bs=2, k_nn=4, ddim=True, ddim_steps=6, unconditional_guidance_scale=2.0,
              unconditional_retro_guidance_label=0., device_noise=True)
    torch.manual_seed(7)
    a = m.sample_with_query(init_image=image, strength=0.5, **kw)["query_samples"]
    torch.manual_seed(7)
    b = m.sample_with_query(init_image=image, strength=0.5, **kw)["query_samples"]
    assert a.shape == (2, 3) + tuple(image.shape[1:3]) and torch.isfinite(a).all() and torch.equal(a, b)
    # the hand composition: encode_first_stage -> stochastic_encode(seeded) -> decode -> decode_first_stage
    torch.manual_seed(7)
    seed = parallel.shared_seed(m.device)
    nn = db.search_k_nearest(["a caption"] * 2, k=4, is_caption=True)
    q_emb, r_emb = torch.as_tensor(nn["q_embeddings"]).float(), torch.as_tensor(nn["embeddings"]).float()
    c = torch.cat([q_emb[:, None], r_emb[:, :3]], dim=1).to(m.device).contiguous()
    uc = m.get_unconditional_conditioning(c.shape, unconditional_guidance_label=0., k_nn=4).to(m.device).float().contiguous()
    lat = m.get_first_stage_encoding(m.encode_first_stage(image.permute(0, 3, 1, 2).to(m.device).contiguous()))
    assert lat.shape == (2, 3, 16, 16)
    sm = DDIMSampler(m)
    sm.make_schedule(6, verbose=False)
    n = sm.img2img_steps(0.5, sm.ddim_timesteps.shape[0])
    assert n == 3
    start = sm.stochastic_encode(lat, n - 1, noise_seed=seed)
    z = sm.decode(start, c, n, unconditional_guidance_scale=2.0, unconditional_conditioning=uc, noise_seed=seed)
    assert torch.equal(m.decode_first_stage(z), a)
    # one image is repeated; a latent is taken as it is; the start of row r depends on (seed, r) only
    torch.manual_seed(7)
    one = m.sample_with_query(init_image=image[0], strength=0.5, **kw)["query_samples"]
    assert torch.equal(one[0], a[0]) and not torch.equal(one[1], a[1])
    torch.manual_seed(7)
    assert torch.equal(m.sample_with_query(init_latent=lat, strength=0.5, **kw)["query_samples"], a)
    assert torch.equal(sm.stochastic_encode(lat[1:], n - 1, noise_seed=seed, noise_row0=1), start[1:])
    # inversion, and strength 1.0: the whole schedule (the published script's off-by-one case)
    torch.manual_seed(7)
    inv = m.sample_with_query(init_image=image, strength=0.5, invert=True, **kw)["query_samples"]
    assert inv.shape == a.shape and torch.isfinite(inv).all() and not torch.equal(inv, a)
    torch.manual_seed(7)
    full = m.sample_with_query(init_image=image, strength=1.0, **kw)["query_samples"]
    assert full.shape == a.shape and torch.isfinite(full).all() and not torch.equal(full, a)
    # without device_noise: torch's generator
    kw.pop("device_noise")
    torch.manual_seed(8)
    t1 = m.sample_with_query(init_image=image, strength=0.5, **kw)["query_samples"]
    torch.manual_seed(8)
    t2 = m.sample_with_query(init_image=image, strength=0.5, eta=0.5, **kw)["query_samples"]
    assert torch.isfinite(t1).all() and torch.isfinite(t2).all() and not torch.equal(t1, t2) and not torch.equal(t1, a)


# ---- 8. errors
def test_errors_leave_the_context_usable(tiny):
    from rdm_amd import _lib
    from rdm_amd._lib import RdmError
    ctx, _, _ = tiny
    x, c, uc = _inputs(ctx, 2, 61)
    noise = torch.zeros(3, 2, 3, 16, 16, device=ctx.device)
    ctx.set_deterministic(True)
    try:
        _errors_leave_the_context_usable(ctx, x, c, uc, noise)
    finally:
        ctx.set_deterministic(False)


def _errors_leave_the_context_usable(ctx, x, c, uc, noise):
    from rdm_amd import _lib
    from rdm_amd._lib import RdmError
    before = ctx.ddim_sample(4, x, c, uc, ACP, scale=2.0)[0].clone()
    total = 4
    acp = np.ascontiguousarray(ACP, dtype=np.float32)

    def raw(fn, *args, eta=0.0, scale=1.0):
        """The C ABI itself (the binding refuses some of these before the call)."""
        a = _lib.DdimArgs(S=4, batch=2, k=4, channels=3, height=16, width=16, eta=eta, temperature=1.0, unconditional_guidance_scale=scale,
                          log_every_t=100, T=1000, alphas_cumprod=acp.ctypes.data_as(C.POINTER(C.c_float)))
        z = torch.empty_like(x)
        ctx._check(fn(ctx._h, C.byref(a), *args, _lib._ptr(z), None, *([None] if fn is not _lib.lib.rdm_ddim_encode else [])))

    P = _lib._ptr
    seeded = lambda seed, row0: C.byref(_lib.Noise(seeded=1, seed=seed, row0=row0))       # a filled rdm_noise
    bad_calls = {
        "t_start = 0": lambda: ctx.ddim_decode(4, 0, x, c, None, ACP),
        "t_start = total + 1": lambda: ctx.ddim_decode(4, total + 1, x, c, None, ACP),
        "t_start = 0 at the C ABI": lambda: raw(_lib.lib.rdm_ddim_decode, 0, P(x), P(c), None, None),
        "t_start = total + 1 at the C ABI": lambda: raw(_lib.lib.rdm_ddim_decode, total + 1, P(x), P(c), None, None),
        "seeded t_start = total + 1 at the C ABI": lambda: raw(_lib.lib.rdm_ddim_decode, total + 1, P(x), P(c), None, seeded(5, 0)),
        "t_enc = 0": lambda: ctx.ddim_encode(4, 0, x, c, None, ACP),
        "t_enc = total + 1": lambda: ctx.ddim_encode(4, total + 1, x, c, None, ACP),
        "t_enc = total + 1 at the C ABI": lambda: raw(_lib.lib.rdm_ddim_encode, total + 1, P(x), P(c), None),
        "eta on encode": lambda: ctx.ddim_encode(4, 2, x, c, None, ACP, eta=0.5),
        "eta on encode at the C ABI": lambda: raw(_lib.lib.rdm_ddim_encode, 2, P(x), P(c), None, eta=0.5),
        "decode at scale 2 without uncond": lambda: ctx.ddim_decode(4, 2, x, c, None, ACP, scale=2.0),
        "encode at scale 2 without uncond": lambda: ctx.ddim_encode(4, 2, x, c, None, ACP, scale=2.0),
        "scale 2 without uncond at the C ABI": lambda: raw(_lib.lib.rdm_ddim_encode, 2, P(x), P(c), None, scale=2.0),
        "a null latent at the C ABI": lambda: raw(_lib.lib.rdm_ddim_decode, 2, None, P(c), None, None),
        "noise together with seed": lambda: ctx.ddim_decode(4, 3, x, c, None, ACP, eta=0.5, noise=noise, seed=3),
        "a noise stack of the wrong length": lambda: ctx.ddim_decode(4, 2, x, c, None, ACP, eta=0.5, noise=noise),
        "eta without noise": lambda: ctx.ddim_decode(4, 2, x, c, None, ACP, eta=0.5),
    }
    for what, call in bad_calls.items():
        with pytest.raises(RdmError):
            call()
            pytest.fail(f"{what} was accepted")
        after = ctx.ddim_sample(4, x, c, uc, ACP, scale=2.0)[0]
        torch.cuda.synchronize()
        assert torch.equal(after, before), f"after {what}"


# ---- 9. the script
def test_rdm_sample_script_init_img(tmp_path):
    """scripts/rdm_sample.py --synthetic --init_img PNG --strength 0.5 --steps 6 -bs 2 -n 1 as a child process: two 256 x 256 PNGs."""
    from PIL import Image
    png = tmp_path / "init.png"
    Image.fromarray((np.random.default_rng(0).random((80, 120, 3)) * 255).astype(np.uint8)).save(png)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "rdm_sample.py"), "--synthetic", "--synthetic_db_rows", "2000", "--gpu", "0",
           "--init_img", str(png), "--strength", "0.5", "--steps", "6", "-bs", "2", "-n", "1", "--seed", "3", "-s", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = sorted(p for p in out.iterdir() if p.suffix == ".png")
    assert len(files) == 2, [f.name for f in files]
    px = [np.asarray(Image.open(f)) for f in files]
    assert all(v.shape == (256, 256, 3) for v in px) and len(np.unique(px[0])) > 16 and not np.array_equal(px[0], px[1])
