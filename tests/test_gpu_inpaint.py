"""Native DDIM inpainting on the GPU (masked_blend_kernel / masked_blend_seeded_kernel, rdm_ddim_inpaint with stacks and seeded,
DDIMSampler.decode(mask=), sample_log(inpaint_mask=), rdm_sample.py --mask): the blend per element against float64 and bit for bit
against its six fp32 operations, the seeded blend against the stack blend, the loop against the same loop rebuilt from op entries, the
identities (an all-zero mask is decode; the oracle's loop; the per-step path), the seeded loop against the stack loop and its
sharding, the public surface, the errors.  tests/_inpaint_ref.py is the restatement."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff
from oracle import unet as ounet

import _inpaint_ref as ref
from _step_ref import ddim_scalars
from _util import rel_l2, within
from test_gpu_plms import model, tiny  # noqa: F401  (fixtures: the tiny UNet on the session context, the tiny model)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATENT_TOL = 2.5e-2          # test_gpu_surface.py's bound of the per-step inpainting latent against the oracle's loop
PER_STEP_TOL = 2e-2          # test_gpu_img2img.py's bound of decode's native loop against its per-step path
ACP = odiff.Schedule().alphas_cumprod
SA, S1M = ref.level_scalars(float(ACP[601]))
SEED = 0x51A7_0000_BEEF

_within = functools.partial(within, "inpaint")


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev(ctx, a, offset=0):
    """numpy fp32 -> a contiguous device tensor `offset` floats past a 16-byte aligned address"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + 4, device=ctx.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * offset and v.is_contiguous()
    return v


class _deterministic:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_deterministic(True)

    def __exit__(self, *exc):
        self.ctx.set_deterministic(False)


# ---- 1. the blend kernel per element
@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
@pytest.mark.parametrize("full_mask", [False, True], ids=["mc1", "mcC"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1_scalar"])
@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_blend_per_element_against_fp64_and_the_six_fp32_operations(ctx, shape, offset, full_mask, soft):
    """|got - ref| <= K(4) 2^-24 A per element, zero elements off the numpy fp32 evaluation of the six operations, and the FMA-contracted
    near miss off it (_inpaint_ref.py has the derivation); x_dup receives out's bits; with a binary mask out is x where m = 0 and
    fp32(sa x0 + s1m z) where m = 1, bit for bit.  offset 1 puts every operand one float past alignment: the scalar form."""
    B, Cc, H, W = ref.SHAPES[shape]
    x, x0, z, m = ref.inputs((B, Cc, H, W), Cc if full_mask else 1, soft, seed=7 + 2 * offset + full_mask)
    dx, dx0, dz, dm = (_dev(ctx, a, offset) for a in (x, x0, z, m))
    out, dup = (_dev(ctx, np.full_like(x, np.nan), offset) for _ in range(2))
    got = ctx.op_masked_blend(dx, dx0, dm, dz, SA, S1M, out=out, x_dup=dup)
    torch.cuda.synchronize()
    assert got is out and _bits(dup, out) and torch.equal(dx.cpu(), torch.from_numpy(x))
    g = out.cpu().numpy()
    print(f"[inpaint] blend {shape} offset {offset} mask_channels {Cc if full_mask else 1} {'soft' if soft else 'binary'}: "
          + ref.check(g, x, x0, z, m, SA, S1M))
    if not soft:
        mb = np.broadcast_to(m, x.shape)
        q = np.float32(SA) * x0 + np.float32(S1M) * z
        assert np.array_equal(g[mb == 0], x[mb == 0]) and np.array_equal(g[mb == 1], q[mb == 1])
        assert (mb == 0).any() and (mb == 1).any()
    ctx.op_masked_blend(dx, dx0, dm, dz, SA, S1M, out=dx)                      # in place
    torch.cuda.synchronize()
    assert _bits(dx, out)
    if not soft:
        bare = ctx.op_masked_blend(out, dx0, dm, None, 1.0, 0.0)               # no z: zeros -- the blend a keep-known call ends with
        mb = torch.from_numpy(np.broadcast_to(m, x.shape).copy()).to(ctx.device)
        assert _bits(bare[mb == 1], dx0[mb == 1]) and _bits(bare[mb == 0], out[mb == 0])


def test_blend_second_grid_stride_trip(ctx):
    """(2, 3, 592, 592): 2 102 784 elements, just above 2048 blocks x 256 threads x 4 -- the float4 form's loop takes a second trip; a soft
    one-channel mask; the seeded form on the same shape equals the stack form fed with op_randn's output."""
    shape = ref.SECOND_TRIP
    x, x0, z, m = ref.inputs(shape, 1, True, seed=23)
    dx, dx0, dz, dm = (_dev(ctx, a) for a in (x, x0, z, m))
    out = ctx.op_masked_blend(dx, dx0, dm, dz, SA, S1M)
    torch.cuda.synchronize()
    print("[inpaint] blend second trip: " + ref.check(out.cpu().numpy(), x, x0, z, m, SA, S1M))
    B, per_row = shape[0], int(np.prod(shape[1:]))
    zs = ctx.op_randn(SEED, B, per_row, row0=3, step=2, stream=0).reshape(shape)
    assert _bits(ctx.op_masked_blend(dx, dx0, dm, None, SA, S1M, seed=SEED, row0=3, step=2), ctx.op_masked_blend(dx, dx0, dm, zs, SA, S1M))


# ---- 2. the seeded blend is the stack blend on op_randn's output
@pytest.mark.parametrize("full_mask", [False, True], ids=["mc1", "mcC"])
@pytest.mark.parametrize("shape", [(4, 3, 8, 8), (4, 4, 3, 3), (4, 3, 2, 6)], ids=["b4c3_8x8", "b4c4_3x3_block_straddles_channels", "b4c3_2x6"])
def test_seeded_blend_equals_the_stack_blend_bitwise(ctx, shape, full_mask):
    """Loop step i = 1: the stack blend fed with op_randn(seed, step = i + 1, stream = 0) and the seeded blend at step = i + 1 agree bit for
    bit; rows 0 .. 3 in one call are rows 0 .. 1 plus rows 2 .. 3 with row0 = 2; per_row = 36 with H W = 9 indexes the mask per element.
    The (2, 4, 3, 3) seeded case of the per-element test rides along: rows 0 .. 1 against float64."""
    B, Cc, H, W = shape
    per_row = Cc * H * W
    i = 1
    x, x0, _, m = ref.inputs(shape, Cc if full_mask else 1, True, seed=31)
    dx, dx0, dm = (_dev(ctx, a) for a in (x, x0, m))
    z = ctx.op_randn(SEED, B, per_row, row0=0, step=i + 1, stream=0).reshape(shape)
    stack = ctx.op_masked_blend(dx, dx0, dm, z, SA, S1M)
    dup = torch.full_like(dx, float("nan"))
    seeded = ctx.op_masked_blend(dx, dx0, dm, None, SA, S1M, x_dup=dup, seed=SEED, step=i + 1)
    halves = torch.cat([ctx.op_masked_blend(dx[lo:lo + 2].contiguous(), dx0[lo:lo + 2].contiguous(), dm[lo:lo + 2].contiguous(), None, SA, S1M,
                                            seed=SEED, row0=lo, step=i + 1) for lo in (0, 2)])
    torch.cuda.synchronize()
    assert _bits(seeded, stack) and _bits(dup, stack) and _bits(halves, stack)
    other = ctx.op_masked_blend(dx, dx0, dm, None, SA, S1M, seed=SEED, step=i + 2)
    start = ctx.op_masked_blend(dx, dx0, dm, ctx.op_randn(SEED, B, per_row, step=0, stream=0).reshape(shape), SA, S1M)
    assert not _bits(other, stack) and not _bits(start, stack)                 # another step: other noise; and not the starting latent's
    print(f"[inpaint] seeded blend {shape}: " + ref.check(seeded.cpu().numpy()[:2], x[:2], x0[:2], z.cpu().numpy()[:2], m[:2], SA, S1M))


# ---- 3. the native loop is blend, forward, step
S5, T_START, B2 = 5, 3, 2


def _loop_inputs(ctx, B, seed, hw=16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x_l, x0 = r(B, 3, hw, hw).to(ctx.device), (r(B, 3, hw, hw) * 0.5).to(ctx.device)
    cond = (r(B, 4, 512) * 0.45).to(ctx.device)
    mask = (torch.rand(B, 1, hw, hw, generator=g) > 0.5).float().to(ctx.device)
    return x_l, x0, mask, cond, torch.zeros_like(cond), g


def _rebuilt(ctx, S, t_start, x_l, x0, mask, cond, uncond, scale, eta, noise, q_noise):
    """rdm_ddim_inpaint's loop from the op entries -> (z, x_inter, pred_x0) with every step logged"""
    B = x_l.shape[0]
    x = x_l.clone()
    xs, ps = [], []
    _, a_t = ref.schedule(ACP, S)
    for i in range(t_start):
        index = t_start - 1 - i
        t, at, ap, sigma, s1m = ddim_scalars(S, index, eta)
        sa, s1 = ref.level_scalars(a_t[index])
        ctx.op_masked_blend(x, x0, mask, q_noise[i].contiguous(), sa, s1, out=x)
        if uncond is not None:
            eps = ctx.unet_forward_guided(x, t, cond, uncond)
        else:
            eps = ctx.unet_forward(x, torch.full((B,), t, dtype=torch.long, device=x.device), cond)
        nxt, pred = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        ctx.op_ddim_step(x, eps, noise[i].contiguous() if eta else None, uncond is not None, scale, at, ap, sigma, s1m, 1.0, nxt, pred_x0=pred)
        x = nxt
        xs.append(x.clone()); ps.append(pred)
    return x, torch.stack(xs), torch.stack(ps)


@pytest.mark.parametrize("eta", [0.0, 1.0], ids=["eta0", "eta1_stacks"])
@pytest.mark.parametrize("scale", [2.0, 1.0], ids=["cfg2", "unguided"])
def test_inpaint_loop_equals_the_loop_rebuilt_from_op_entries_bitwise(tiny, scale, eta):
    """S = 5, t_start = 3, B = 2 in deterministic mode: loop step i blends at level index t_start - 1 - i with the float64 square roots of
    the fp32 alpha, runs the forward, then the DDIM step -- z and both intermediates stacks bit for bit."""
    ctx, _, _ = tiny
    x_l, x0, mask, cond, uncond, g = _loop_inputs(ctx, B2, 71)
    uc = uncond if scale > 1 else None
    noise = torch.randn(T_START, *x_l.shape, generator=g).to(ctx.device)
    q_noise = torch.randn(T_START, *x_l.shape, generator=g).to(ctx.device)
    with _deterministic(ctx):
        z, xi, pi = ctx.ddim_inpaint(S5, T_START, x_l, x0, mask, cond, uc, ACP, eta=eta, scale=scale, noise=noise if eta else None,
                                     q_noise=q_noise, log_every_t=1, want_intermediates=True)
        zr, xr, pr = _rebuilt(ctx, S5, T_START, x_l, x0, mask, cond, uc, scale, eta, noise, q_noise)
        plain = ctx.ddim_decode(S5, T_START, x_l, cond, uc, ACP, eta=eta, scale=scale, noise=noise if eta else None)[0]
        torch.cuda.synchronize()
    assert xi.shape[0] == pi.shape[0] == T_START and torch.isfinite(z).all()
    assert _bits(z, zr), f"z differs: rel L2 {rel_l2(z, zr):.3e}"
    assert _bits(xi, xr) and _bits(pi, pr)
    assert not torch.equal(z, plain), "the mask has no effect: the comparison would show nothing"


# ---- 4. identities
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_an_all_zero_mask_is_decode_bitwise(tiny, eta):
    ctx, _, _ = tiny
    x_l, x0, mask, cond, uncond, g = _loop_inputs(ctx, B2, 72)
    noise = torch.randn(T_START, *x_l.shape, generator=g).to(ctx.device)
    q_noise = torch.randn(T_START, *x_l.shape, generator=g).to(ctx.device)
    kw = dict(eta=eta, scale=2.0, noise=noise if eta else None, log_every_t=1, want_intermediates=True)
    with _deterministic(ctx):
        want = ctx.ddim_decode(S5, T_START, x_l, cond, uncond, ACP, **kw)
        got = ctx.ddim_inpaint(S5, T_START, x_l, x0, torch.zeros_like(mask), cond, uncond, ACP, q_noise=q_noise, **kw)
        got_s = ctx.ddim_inpaint(S5, T_START, x_l, x0, torch.zeros_like(mask), cond, uncond, ACP, eta=0.0, scale=2.0, seed=5)[0]
        want_s = ctx.ddim_decode(S5, T_START, x_l, cond, uncond, ACP, eta=0.0, scale=2.0)[0]
    for a, b in zip(got, want):
        assert _bits(a, b)
    assert _bits(got_s, want_s)


@pytest.fixture(scope="module")
def surface(model):
    """S = 5, B = 2, CFG 2.0 on the tiny model: the sampler with its schedule and the inputs"""
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    x_l, x0, mask, cond, uc, g = _loop_inputs(model.ctx, B2, 73)
    sm = DDIMSampler(model)
    sm.make_schedule(S5, verbose=False)
    assert sm.ddim_timesteps.shape[0] == 5
    q_noise = torch.randn(5, *x_l.shape, generator=g).to(model.device)
    return sm, x_l, x0, mask, cond, uc, q_noise


def test_whole_schedule_against_the_oracles_inpainting_loop(model, surface):
    """t_start = total: oracle.diffusion.ddim_sample(mask=, x0=, q_noise=) on the CPU oracle UNet, CFG 2.0, at the bound
    test_gpu_surface.py holds the per-step inpainting path to."""
    sm, x_l, x0, mask, cond, uc, q_noise = surface
    z = sm.decode(x_l, cond, 5, unconditional_guidance_scale=2.0, unconditional_conditioning=uc, mask=mask, x0=x0, q_noise=q_noise)
    apply = lambda x, t, c: ounet.unet_forward(model.sd_unet, model.spec, x, t, c)
    zr, _ = odiff.ddim_sample(apply, odiff.Schedule(), S5, x_l.cpu(), cond.cpu(), scale=2.0, uncond=uc.cpu(), mask=mask.cpu(), x0=x0.cpu(),
                              q_noise=q_noise.cpu())
    _within("native inpainting latent vs the oracle's loop on the oracle UNet (5 steps, CFG 2.0)", rel_l2(z, zr), LATENT_TOL)
    plain = sm.decode(x_l, cond, 5, unconditional_guidance_scale=2.0, unconditional_conditioning=uc)
    assert rel_l2(plain, zr) > LATENT_TOL, "the mask has no effect: the comparison would show nothing"


def test_decode_with_a_mask_native_against_its_per_step_path(model, surface):
    sm, x_l, x0, mask, cond, uc, q_noise = surface
    kw = dict(unconditional_guidance_scale=2.0, unconditional_conditioning=uc, mask=mask, x0=x0)
    d, inter = sm.decode(x_l, cond, 3, q_noise=q_noise[:3], log_every_t=2, return_intermediates=True, **kw)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 3 and torch.equal(inter["x_inter"][0], x_l)
    seen = []
    d_ps = sm.decode(x_l, cond, 3, q_noise=q_noise[:3], callback=seen.append, **kw)
    assert seen == list(range(3))
    _within("decode(mask=) native loop vs the per-step path (t_start 3, CFG 2.0)", rel_l2(d, d_ps), PER_STEP_TOL)
    # under a seed the per-step path applies the library's stream 0 / step i + 1 to the known region, as the native loop
    s = sm.decode(x_l, cond, 3, noise_seed=17, noise_row0=2, **kw)
    s_ps = sm.decode(x_l, cond, 3, noise_seed=17, noise_row0=2, img_callback=lambda p, i: None, **kw)
    _within("decode(mask=, noise_seed=) native loop vs the per-step path", rel_l2(s, s_ps), PER_STEP_TOL)
    assert not torch.equal(s, d)
    # a [1, 1, H, W] mask is every row's
    one = sm.decode(x_l, cond, 3, q_noise=q_noise[:3], unconditional_guidance_scale=2.0, unconditional_conditioning=uc, mask=mask[:1], x0=x0)
    both = sm.decode(x_l, cond, 3, q_noise=q_noise[:3], unconditional_guidance_scale=2.0, unconditional_conditioning=uc,
                     mask=mask[:1].expand(2, -1, -1, -1), x0=x0)
    assert torch.equal(one, both)


# ---- 5. the seeded loop is the stack loop
def _stacks(ctx, seed, B, steps, per_row, shape, row0=0):
    noise = torch.stack([ctx.op_randn(seed, B, per_row, row0=row0, step=i, stream=1).reshape(shape) for i in range(steps)])
    q_noise = torch.stack([ctx.op_randn(seed, B, per_row, row0=row0, step=i + 1, stream=0).reshape(shape) for i in range(steps)])
    return noise, q_noise


@pytest.mark.parametrize("scale", [2.0, 1.0], ids=["cfg2", "unguided"])
def test_seeded_inpaint_loop_equals_the_stack_loop_and_does_not_depend_on_the_sharding(tiny, scale):
    """eta 1, deterministic mode (batch-invariant, as test_gpu_device_noise.py compares shards): the seeded rdm_ddim_inpaint against the stack
    loop fed with op_randn's outputs -- stream 1 / step i for the update, stream 0 / step i + 1 for the known region; B = 4 in one call
    against two shards of 2 with row0."""
    ctx, _, _ = tiny
    B = 4
    x_l, x0, mask, cond, uncond, _ = _loop_inputs(ctx, B, 74)
    uc = uncond if scale > 1 else None
    kw = dict(eta=1.0, scale=scale, temperature=0.7, log_every_t=1, want_intermediates=True)
    with _deterministic(ctx):
        noise, q_noise = _stacks(ctx, 91, B, T_START, 768, x_l.shape)
        stack = ctx.ddim_inpaint(S5, T_START, x_l, x0, mask, cond, uc, ACP, noise=noise, q_noise=q_noise, **kw)
        seeded = ctx.ddim_inpaint(S5, T_START, x_l, x0, mask, cond, uc, ACP, seed=91, **kw)
        quiet = ctx.ddim_inpaint(S5, T_START, x_l, x0, mask, cond, uc, ACP, noise=noise, q_noise=torch.zeros_like(q_noise), **kw)[0]
        halves = [ctx.ddim_inpaint(S5, T_START, x_l[lo:lo + 2], x0[lo:lo + 2].contiguous(), mask[lo:lo + 2].contiguous(), cond[lo:lo + 2],
                                   None if uc is None else uc[lo:lo + 2], ACP, seed=91, row0=lo, **kw)[0] for lo in (0, 2)]
    for a, b in zip(seeded, stack):
        assert _bits(a, b)
    assert not torch.equal(stack[0], quiet), "the known region's noise has no effect: the comparison would show nothing"
    assert _bits(torch.cat(halves), seeded[0]) and not torch.equal(halves[0], halves[1])


# ---- 6. the public surface
def test_sample_log_inpainting_is_the_manual_sequence_and_keeps_the_known_region(model):
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    ctx = model.ctx
    _, lat, mask, cond, uc, g = _loop_inputs(ctx, B2, 75)
    mask[:, :, :4] = 1.0
    mask[:, :, -4:] = 0.0
    kw = dict(cond=cond, batch_size=2, ddim=True, ddim_steps=S5, unconditional_guidance_scale=2.0, unconditional_conditioning=uc, noise_seed=33,
              noise_row0=1, eta=0.5)
    with _deterministic(ctx):
        z, inter = model.sample_log(init_latent=lat, inpaint_mask=mask, strength=0.6, **kw)
        raw, _ = model.sample_log(init_latent=lat, inpaint_mask=mask, strength=0.6, keep_known=False, **kw)
        i2i, _ = model.sample_log(init_latent=lat, strength=0.6, **kw)
        sm = DDIMSampler(model)
        sm.make_schedule(S5, ddim_eta=0.5, verbose=False)
        n = sm.img2img_steps(0.6, sm.ddim_timesteps.shape[0])
        assert n == 3
        start = sm.stochastic_encode(lat, n - 1, noise_seed=33, noise_row0=1)
        d = sm.decode(start, cond, n, unconditional_guidance_scale=2.0, unconditional_conditioning=uc, eta=0.5, noise_seed=33, noise_row0=1,
                      mask=mask, x0=lat)
        kept = ctx.op_masked_blend(d, lat, mask, None, 1.0, 0.0)
        # the mask at image resolution: every latent pixel's f x f block averaged on the host
        f = 1 << (model.vq_cfg.n_ch_mult - 1)
        big = (torch.rand(2, 16 * f, 16 * f, generator=g) > 0.4).float()
        small = torch.from_numpy(ref.area_average(big.numpy(), f)).float()
        z_big, _ = model.sample_log(init_latent=lat, inpaint_mask=big, strength=0.6, **kw)
        z_small, _ = model.sample_log(init_latent=lat, inpaint_mask=small, strength=0.6, **kw)
        z_2d, _ = model.sample_log(init_latent=lat, inpaint_mask=mask[0, 0], strength=0.6, **kw)
        z_one, _ = model.sample_log(init_latent=lat, inpaint_mask=mask[:1], strength=0.6, **kw)
    assert torch.isfinite(z).all() and "x_inter" in inter
    assert _bits(raw, d) and _bits(z, kept)
    mb = mask.expand_as(z) == 1
    assert _bits(z[mb], lat[mb]) and not torch.equal(raw[mb], lat[mb])            # the known region is the init latent itself
    assert _bits(z[mask.expand_as(z) == 0], raw[mask.expand_as(z) == 0])
    assert not torch.equal(z, i2i)
    assert f > 1 and len(torch.unique(small)) > 2 and _bits(z_big, z_small)
    assert _bits(z_2d, z_one)


def test_rdm_sample_script_mask(tmp_path):
    """scripts/rdm_sample.py --synthetic --init_img PNG --mask PNG --strength 0.5 --steps 6 -bs 2 -n 1 as a child process: two PNGs."""
    from PIL import Image
    rng = np.random.default_rng(0)
    png, mpng = tmp_path / "init.png", tmp_path / "mask.png"
    Image.fromarray((rng.random((80, 120, 3)) * 255).astype(np.uint8)).save(png)
    grey = np.zeros((80, 120), np.uint8)
    grey[20:60, 30:90] = 255
    Image.fromarray(grey).save(mpng)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "rdm_sample.py"), "--synthetic", "--synthetic_db_rows", "2000", "--gpu", "0",
           "--init_img", str(png), "--mask", str(mpng), "--strength", "0.5", "--steps", "6", "-bs", "2", "-n", "1", "--seed", "3", "-s", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = sorted(p for p in out.iterdir() if p.suffix == ".png")
    assert len(files) == 2, [f.name for f in files]
    px = [np.asarray(Image.open(f)) for f in files]
    assert all(v.shape == (256, 256, 3) for v in px) and len(np.unique(px[0])) > 16 and not np.array_equal(px[0], px[1])


# ---- 7. errors
def test_errors_leave_the_context_usable(tiny, model):
    from rdm_amd import _lib
    from rdm_amd._lib import RdmError
    ctx, _, _ = tiny
    x, x0, mask, c, uc, _ = _loop_inputs(ctx, 2, 76)
    qn = torch.zeros(2, 2, 3, 16, 16, device=ctx.device)
    acp = np.ascontiguousarray(ACP, dtype=np.float32)
    P = _lib._ptr
    total = 4

    def raw(fn, *args):
        """The C ABI itself (the binding refuses some of these before the call)."""
        a = _lib.DdimArgs(S=4, batch=2, k=4, channels=3, height=16, width=16, eta=0.0, temperature=1.0, unconditional_guidance_scale=1.0,
                          log_every_t=100, T=1000, alphas_cumprod=acp.ctypes.data_as(C.POINTER(C.c_float)))
        z = torch.empty_like(x)
        ctx._check(fn(ctx._h, C.byref(a), *args, P(z), None, None))

    inp, blend = _lib.lib.rdm_ddim_inpaint, _lib.lib.rdm_op_masked_blend
    seeded = lambda seed, row0, stack=None, step=0: C.byref(_lib.Noise(stack=P(stack), seeded=1, seed=seed, row0=row0, step=step))     # a filled rdm_noise
    o = torch.empty_like(x)
    odd = torch.zeros(2, 3, 5, 7, device=ctx.device)
    buf = torch.zeros(x.numel() + 4, device=ctx.device)
    off = buf[1:1 + x.numel()].view(x.shape)
    bad_calls = {
        "a null x0 at the C ABI": lambda: raw(inp, 2, P(x), None, P(mask), 1, P(c), None, None, P(qn)),
        "a null mask at the C ABI": lambda: raw(inp, 2, P(x), P(x0), None, 1, P(c), None, None, P(qn)),
        "a null q_noise at the C ABI": lambda: raw(inp, 2, P(x), P(x0), P(mask), 1, P(c), None, None, None),
        "a null x0 at the seeded C ABI": lambda: raw(inp, 2, P(x), None, P(mask), 1, P(c), None, seeded(5, 0), None),
        "mask_channels = 2 at the C ABI": lambda: raw(inp, 2, P(x), P(x0), P(mask), 2, P(c), None, None, P(qn)),
        "mask_channels = 0 at the seeded C ABI": lambda: raw(inp, 2, P(x), P(x0), P(mask), 0, P(c), None, seeded(5, 0), None),
        "t_start = 0 at the C ABI": lambda: raw(inp, 0, P(x), P(x0), P(mask), 1, P(c), None, None, P(qn)),
        "t_start = total + 1 at the C ABI": lambda: raw(inp, total + 1, P(x), P(x0), P(mask), 1, P(c), None, None, P(qn)),
        "seeded t_start = total + 1 at the C ABI": lambda: raw(inp, total + 1, P(x), P(x0), P(mask), 1, P(c), None, seeded(5, 0), None),
        "a misaligned x0 in the seeded loop": lambda: raw(inp, 2, P(x), P(off), P(mask), 1, P(c), None, seeded(5, 0), None),
        "row0 beyond 32 bits in the seeded loop": lambda: raw(inp, 2, P(x), P(x0), P(mask), 1, P(c), None, seeded(5, 2 ** 32 - 1), None),
        "a seed with a noise stack at the C ABI": lambda: raw(inp, 2, P(x), P(x0), P(mask), 1, P(c), None, seeded(5, 0, stack=qn), None),
        "a seed with a q_noise stack at the C ABI": lambda: raw(inp, 2, P(x), P(x0), P(mask), 1, P(c), None, seeded(5, 0), P(qn)),
        "t_start = 0": lambda: ctx.ddim_inpaint(4, 0, x, x0, mask, c, None, ACP, q_noise=qn),
        "t_start = total + 1": lambda: ctx.ddim_inpaint(4, total + 1, x, x0, mask, c, None, ACP, q_noise=qn),
        "no q_noise and no seed": lambda: ctx.ddim_inpaint(4, 2, x, x0, mask, c, None, ACP),
        "q_noise together with a seed": lambda: ctx.ddim_inpaint(4, 2, x, x0, mask, c, None, ACP, q_noise=qn, seed=3),
        "a q_noise stack of the wrong length": lambda: ctx.ddim_inpaint(4, 3, x, x0, mask, c, None, ACP, q_noise=qn),
        "a two-channel mask": lambda: ctx.ddim_inpaint(4, 2, x, x0, mask.expand(-1, 2, -1, -1).contiguous(), c, None, ACP, q_noise=qn),
        "an x0 of another shape": lambda: ctx.ddim_inpaint(4, 2, x, x0[:1], mask, c, None, ACP, q_noise=qn),
        "scale 2 without uncond": lambda: ctx.ddim_inpaint(4, 2, x, x0, mask, c, None, ACP, scale=2.0, q_noise=qn),
        "eta without noise": lambda: ctx.ddim_inpaint(4, 2, x, x0, mask, c, None, ACP, eta=0.5, q_noise=qn),
        "blend: a null x0 at the C ABI": lambda: ctx._check(blend(ctx._h, P(x), None, P(mask), None, 2, 3, 16, 16, 1, 1.0, 0.0, P(o), None)),
        "blend: mask_channels = 2 at the C ABI": lambda: ctx._check(blend(ctx._h, P(x), P(x0), P(mask), None, 2, 3, 16, 16, 2, 1.0, 0.0, P(o), None)),
        "blend: B = 0 at the C ABI": lambda: ctx._check(blend(ctx._h, P(x), P(x0), P(mask), None, 0, 3, 16, 16, 1, 1.0, 0.0, P(o), None)),
        "seeded blend: per_row % 4": lambda: ctx.op_masked_blend(odd, odd, odd[:, :1].contiguous(), None, SA, S1M, seed=1),
        "seeded blend: a misaligned out": lambda: ctx.op_masked_blend(x, x0, mask, None, SA, S1M, out=off, seed=1),
        "seeded blend: row0 beyond 32 bits at the C ABI": lambda: ctx._check(blend(ctx._h, P(x), P(x0), P(mask), seeded(1, 2 ** 32 - 1, step=1),
                                                                                 2, 3, 16, 16, 1, 1.0, 0.0, P(o), None)),
        "seeded blend with a z operand": lambda: ctx.op_masked_blend(x, x0, mask, x0, SA, S1M, seed=1),
        "blend: a mask of another plane": lambda: ctx.op_masked_blend(x, x0, mask[:, :, :8].contiguous(), None, SA, S1M),
    }
    with _deterministic(ctx):
        before = ctx.ddim_inpaint(4, 2, x, x0, mask, c, uc, ACP, scale=2.0, seed=9)[0].clone()
        for what, call in bad_calls.items():
            with pytest.raises(RdmError):
                call()
                pytest.fail(f"{what} was accepted")
            after = ctx.ddim_inpaint(4, 2, x, x0, mask, c, uc, ACP, scale=2.0, seed=9)[0]
            torch.cuda.synchronize()
            assert torch.equal(after, before), f"after {what}"
    # the generator's stream 2 stays reserved: the known region's noise lives on stream 0
    for fn in (ctx.op_randn, ctx.op_rng_words):
        with pytest.raises(RdmError, match="reserved"):
            fn(1, 2, 4, stream=2)
    assert _lib.lib.rdm_op_randn is not None and torch.isfinite(ctx.op_randn(1, 2, 4, step=3, stream=0)).all()
    # the refusals of the public surface, each a ValueError before any GPU work
    lat = x0
    run = lambda **kw: model.sample_log(cond=c, batch_size=2, ddim=kw.pop("ddim", True), ddim_steps=4, **kw)
    refusals = {
        "invert with a mask": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask, invert=True),
        "a mask without an init image": lambda: run(inpaint_mask=mask),
        "a mask with PLMS": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask, plms=True),
        "a mask with DPM-Solver++": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask, dpm_solver=True),
        "a mask with UniPC": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask, uni_pc=True),
        "a mask with SDE-DPM-Solver++": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask, dpm_solver_sde=True),
        "a mask with DDPM": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask, ddim=False),
        "values above 1": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask * 1.5),
        "values below 0": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask - 0.5),
        "a mask of another plane": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=mask[:, :, :8]),
        "a mask of three rows": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=torch.ones(3, 1, 16, 16)),
        "an image-resolution mask of another size": lambda: run(init_latent=lat, strength=0.5, inpaint_mask=torch.ones(2, 40, 40)),
        "mask= together with init_latent": lambda: run(init_latent=lat, strength=0.5, mask=mask),
    }
    for what, call in refusals.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{what} was accepted")
    with pytest.raises(ValueError, match="does not take"):
        run(init_latent=lat, strength=0.5, mask=mask)
    with _deterministic(ctx):
        assert torch.equal(ctx.ddim_inpaint(4, 2, x, x0, mask, c, uc, ACP, scale=2.0, seed=9)[0], before)
