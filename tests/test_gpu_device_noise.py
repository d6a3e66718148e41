"""The device noise on the GPU: rdm_op_rng_words bit for bit against the numpy Philox (tests/_rng_ref.py) over partial blocks, the stride
loop's second pass and the unaligned scalar path; rdm_op_randn per element against the float64 Box-Muller; invariance to the split of a
batch; the seeded DDIM / DDPM loops bit for bit against the stack loops fed with rdm_op_randn's output, in deterministic mode; sharding
through noise_row0; the per-step path; the memory a sampling call no longer allocates; errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff

import _rng_ref as ref
from _util import rel_l2
from test_gpu_plms import UPDATE_TOL, model, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = [(3, per_row, row0) for per_row in (1, 3, 4, 5, 7, 768, 1027) for row0 in (0, 5)]
SECOND_PASS = 2048 * 256 * 4 + 4          # one row of 2048 * 256 + 1 blocks: the last one belongs to the stride loop's second pass
SENTINEL = 0x5A5A5A5A
SEED = 0x9E3779B97F4A7C15                 # above 2^63: both key words in use
K_NORMAL = 7                              # see test_randn_per_element


def _words_into(ctx, fn, dtype, n_front, seed, B, per_row, row0, step, stream):
    """fn into a sentinel-filled buffer that starts n_front elements before the output and ends one element after it -> (out, the
    elements around it).  n_front = 0: the 16-byte aligned path when per_row % 4 == 0; n_front = 1: never aligned."""
    n = B * per_row
    buf = torch.full((n_front + n + 1,), SENTINEL, dtype=torch.int32, device=ctx.device).view(dtype)
    out = fn(seed, B, per_row, row0=row0, step=step, stream=stream, out=buf[n_front:n_front + n])
    torch.cuda.synchronize()
    around = torch.cat([buf[:n_front], buf[n_front + n:]]).view(torch.int32).cpu().numpy()
    return out.reshape(B, per_row), around


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("B,per_row,row0", SHAPES)
def test_rng_words_bit_for_bit(ctx, B, per_row, row0):
    for step, stream in ((0, 0), (3, 1)):
        got, around = _words_into(ctx, ctx.op_rng_words, torch.int32, 0, SEED, B, per_row, row0, step, stream)
        assert np.array_equal(_u32(got), ref.words(SEED, row0, B, per_row, step, stream))
        assert (around == SENTINEL).all(), "written past B * per_row"


def test_rng_words_second_pass_and_unaligned(ctx):
    got, around = _words_into(ctx, ctx.op_rng_words, torch.int32, 0, SEED, 1, SECOND_PASS, 7, 2, 1)
    assert np.array_equal(_u32(got), ref.words(SEED, 7, 1, SECOND_PASS, 2, 1)) and (around == SENTINEL).all()
    for per_row in (768, 1027):           # one element into the buffer: scalar stores whatever per_row is
        got, around = _words_into(ctx, ctx.op_rng_words, torch.int32, 1, SEED, 3, per_row, 5, 1, 1)
        assert got.data_ptr() % 16 == 4
        assert np.array_equal(_u32(got), ref.words(SEED, 5, 3, per_row, 1, 1)) and (around == SENTINEL).all()


def _check_normals(got, seed, row0, B, per_row, step, stream, worst):
    """|got - ref| <= K 2^-24 r per element, and the two near misses fall outside that bound."""
    got = got.cpu().numpy().astype(np.float64)
    z, r = ref.normals(seed, row0, B, per_row, step, stream)
    bound = K_NORMAL * 2.0 ** -24 * r
    err = np.abs(got - z)
    worst[0] = max(worst[0], float((err / (2.0 ** -24 * r)).max()))
    assert np.isfinite(got).all() and np.abs(got).max() <= 5.78
    assert (err <= bound).all(), f"worst {worst[0]:.3f} x 2^-24 r (bound {K_NORMAL})"
    z_swapped, _ = ref.normals(seed, row0, B, per_row, step, stream, swap=True)
    z_next, _ = ref.normals(seed, row0, B, per_row, step + 1, stream)
    assert not (np.abs(got - z_swapped) <= bound).all(), "sin and cos exchanged passes the same bound"
    assert not (np.abs(got - z_next) <= bound).all(), "the next step's normals pass the same bound"


def test_randn_per_element(ctx):
    """rdm_op_randn against the float64 Box-Muller of the same exact uniforms: |got - ref| <= K 2^-24 r, r = sqrt(-2 ln u1) in float64
    (relative to r, not to |z| = r |cos|, which can be near 0).  K by counting, in units of 2^-24 r (half an fp32 ulp of a value of r's
    size), with the bounds ROCm's HIP math table documents -- logf 1 ulp, sqrtf 1 ulp, sincospif 1 ulp:
      * logf(u1), 1 ulp = 2 units relative; the square root halves a relative error: 1 unit;
      * -2 * logf and 2 * u2 are exact (powers of two), as are the uniforms themselves;
      * sqrtf, 1 ulp: 2 units;
      * sincospif on the exact argument, 1 ulp of a value of magnitude <= 1: at most 2 units of r after the multiplication;
      * the rounding of the product r * c (or r * s): half an ulp of |z| <= r, 1 unit.
    6 units to first order; K = 7 leaves one unit for the second-order terms and for the float64 reference's own rounding (both below
    2^-20 units).  The measured worst case is printed (DESIGN.md section 3 quotes it)."""
    worst = [0.0]
    for B, per_row, row0 in SHAPES:
        got, around = _words_into(ctx, ctx.op_randn, torch.float32, 0, SEED, B, per_row, row0, 2, 1)
        assert (around == SENTINEL).all(), "written past B * per_row"
        _check_normals(got, SEED, row0, B, per_row, 2, 1, worst)
    got, around = _words_into(ctx, ctx.op_randn, torch.float32, 0, SEED, 1, SECOND_PASS, 7, 0, 0)
    assert (around == SENTINEL).all()
    _check_normals(got, SEED, 7, 1, SECOND_PASS, 0, 0, worst)
    got, around = _words_into(ctx, ctx.op_randn, torch.float32, 1, SEED, 3, 1027, 5, 1, 1)
    assert (around == SENTINEL).all()
    _check_normals(got, SEED, 5, 3, 1027, 1, 1, worst)
    print(f"[device noise] rdm_op_randn worst |got - ref| = {worst[0]:.3f} x 2^-24 r (bound {K_NORMAL})")


def test_randn_does_not_depend_on_the_split(ctx):
    whole = ctx.op_randn(11, 4, 768, row0=0, step=3, stream=1)
    parts = torch.cat([ctx.op_randn(11, 2, 768, row0=0, step=3, stream=1), ctx.op_randn(11, 2, 768, row0=2, step=3, stream=1)])
    assert torch.equal(whole, parts)
    assert not torch.equal(whole[:2], whole[2:])


class _deterministic:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_deterministic(True)

    def __exit__(self, *exc):
        self.ctx.set_deterministic(False)


def _conds(ctx, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    cond = (torch.randn(B, 4, 512, generator=g) * 0.45).to(ctx.device)
    return cond, torch.zeros_like(cond)


def _ddpm_sched():
    s = odiff.Schedule()
    return {n: getattr(s, n).numpy() for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                               "posterior_mean_coef2", "posterior_log_variance_clipped")}


LATENT = (3, 16, 16)
PER_ROW = 3 * 16 * 16


def _stack(ctx, seed, B, steps, row0=0):
    x_T = ctx.op_randn(seed, B, PER_ROW, row0=row0, step=0, stream=0).reshape((B,) + LATENT)
    noise = torch.stack([ctx.op_randn(seed, B, PER_ROW, row0=row0, step=i, stream=1).reshape((B,) + LATENT) for i in range(steps)])
    return x_T, noise


@pytest.mark.parametrize("scale", [2.0, 1.0])
def test_seeded_ddim_loop_equals_the_stack_loop_bit_for_bit(tiny, scale):
    ctx, _, _ = tiny
    B, S, seed = 2, 4, 77
    cond, uncond = _conds(ctx, B)
    uc = uncond if scale > 1 else None
    ac = odiff.Schedule().alphas_cumprod
    kw = dict(eta=1.0, scale=scale, temperature=0.7, log_every_t=1, want_intermediates=True)
    with _deterministic(ctx):
        x_T, noise = _stack(ctx, seed, B, S)
        z0, xi0, pi0 = ctx.ddim_sample(S, x_T, cond, uc, ac, noise=noise, **kw)
        z1, xi1, pi1 = ctx.ddim_sample(S, None, cond, uc, ac, seed=seed, shape=LATENT, **kw)
        z2, _, _ = ctx.ddim_sample(S, x_T, cond, uc, ac, seed=seed, **kw)             # the start given, the step noise generated
        quiet = ctx.ddim_sample(S, x_T, cond, uc, ac, noise=torch.zeros_like(noise), **kw)[0]
    assert xi0.shape[0] == S and torch.isfinite(z0).all()
    assert not torch.equal(z0, quiet), "the noise stack has no effect: the comparison would show nothing"
    assert torch.equal(z0, z1) and torch.equal(xi0, xi1) and torch.equal(pi0, pi1)
    assert torch.equal(z0, z2)


@pytest.mark.parametrize("clip", [True, False])
def test_seeded_ddpm_loop_equals_the_stack_loop_bit_for_bit(tiny, clip):
    ctx, _, _ = tiny
    B, T, seed = 2, 6, 78
    cond, _ = _conds(ctx, B)
    sched = _ddpm_sched()
    with _deterministic(ctx):
        x_T, noise = _stack(ctx, seed, B, T)
        z0 = ctx.ddpm_sample(T, x_T, cond, noise, sched, clip_denoised=clip, temperature=0.7)
        z1 = ctx.ddpm_sample(T, None, cond, None, sched, clip_denoised=clip, temperature=0.7, seed=seed, shape=LATENT)
        last = noise.clone(); last[T - 1] = 0                                          # the final step (i == 0) consumes no noise
        z_last = ctx.ddpm_sample(T, x_T, cond, last, sched, clip_denoised=clip, temperature=0.7)
        quiet = ctx.ddpm_sample(T, x_T, cond, torch.zeros_like(noise), sched, clip_denoised=clip, temperature=0.7)
    assert torch.isfinite(z0).all() and not torch.equal(z0, quiet)
    assert torch.equal(z0, z1)
    assert torch.equal(z0, z_last)


def test_seeded_ddim_with_eta_zero_equals_the_unseeded_call(tiny):
    ctx, _, _ = tiny
    B, S = 2, 4
    cond, uncond = _conds(ctx, B)
    ac = odiff.Schedule().alphas_cumprod
    with _deterministic(ctx):
        x_T, _ = _stack(ctx, 5, B, 1)
        z0, xi0, pi0 = ctx.ddim_sample(S, x_T, cond, uncond, ac, eta=0.0, scale=2.0, log_every_t=1, want_intermediates=True)
        z1, xi1, pi1 = ctx.ddim_sample(S, x_T, cond, uncond, ac, eta=0.0, scale=2.0, log_every_t=1, want_intermediates=True, seed=5)
        z2 = ctx.ddim_sample(S, None, cond, uncond, ac, eta=0.0, scale=2.0, seed=5, shape=LATENT)[0]
    assert torch.equal(z0, z1) and torch.equal(xi0, xi1) and torch.equal(pi0, pi1) and torch.equal(z0, z2)


def test_seeded_ddim_rows_do_not_depend_on_the_sharding(tiny, model):
    """Deterministic mode is batch-invariant, and a row's noise is a function of its global index: rows [0, 4) in one call equal rows [0, 2)
    and [2, 4) in two, through the library context and through MinimalRETRODiffusion.sample_log."""
    ctx, _, _ = tiny
    cond, uncond = _conds(ctx, 4)
    ac = odiff.Schedule().alphas_cumprod
    kw = dict(eta=1.0, scale=2.0, seed=91, shape=LATENT)
    with _deterministic(ctx):
        whole = ctx.ddim_sample(4, None, cond, uncond, ac, **kw)[0]
        halves = [ctx.ddim_sample(4, None, cond[lo:lo + 2], uncond[lo:lo + 2], ac, row0=lo, **kw)[0] for lo in (0, 2)]
    assert torch.equal(whole, torch.cat(halves)) and not torch.equal(halves[0], halves[1])
    mkw = dict(ddim=True, ddim_steps=4, eta=1.0, unconditional_guidance_scale=2.0, noise_seed=91)
    with _deterministic(model.ctx):
        whole_m, inter = model.sample_log(cond=cond, batch_size=4, unconditional_conditioning=uncond, **mkw)
        halves_m = [model.sample_log(cond=cond[lo:lo + 2], batch_size=2, unconditional_conditioning=uncond[lo:lo + 2], noise_row0=lo, **mkw)[0]
                    for lo in (0, 2)]
    assert torch.equal(whole_m, torch.cat(halves_m))
    assert torch.equal(inter["x_inter"][0], model.ctx.op_randn(91, 4, PER_ROW).reshape((4,) + LATENT))       # the logged start is stream 0


def test_per_step_path_applies_the_same_noise(model):
    """DDIMSampler.sample(eta = 1, noise_seed, img_callback) takes the per-step path; its step i applies op_randn(step = i), the noise the
    native seeded loop generates.  Step 0 of the two runs starts from the same latent; the later steps are rebuilt from the native loop's
    logged x_inter (teacher-forced, as in test_gpu_plms.py) with the sampler's own p_sample_ddim and noise."""
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    ctx = model.ctx
    B, S, seed, scale = 2, 4, 123, 2.0
    cond, uncond = _conds(ctx, B, seed=9)
    sampler = DDIMSampler(model)
    common = dict(conditioning=cond, eta=1.0, temperature=0.7, log_every_t=1, verbose=False, unconditional_guidance_scale=scale,
                  unconditional_conditioning=uncond, noise_seed=seed)
    with _deterministic(ctx):
        z, inter = sampler.sample(S, B, LATENT, **common)
        seen = []
        z_ps, inter_ps = sampler.sample(S, B, LATENT, img_callback=lambda pred_x0, i: seen.append(i), **common)
        assert seen == list(range(S)) and len(inter["x_inter"]) == len(inter_ps["x_inter"]) == S + 1
        assert torch.equal(inter["x_inter"][0], inter_ps["x_inter"][0])
        worst = 0.0
        for i, step in enumerate(np.flip(sampler.ddim_timesteps)):
            index = S - 1 - i
            if i == 0:
                want_x, want_x0 = inter_ps["x_inter"][1], inter_ps["pred_x0"][1]
            else:
                ts = torch.full((B,), int(step), device=ctx.device, dtype=torch.long)
                want_x, want_x0 = sampler.p_sample_ddim(inter["x_inter"][i], cond, ts, index=index, temperature=0.7,
                                                        unconditional_guidance_scale=scale, unconditional_conditioning=uncond,
                                                        noise=sampler._device_randn((B,) + LATENT, seed, 0, step=i, stream=1))
            ex, e0 = rel_l2(inter["x_inter"][i + 1], want_x), rel_l2(inter["pred_x0"][i + 1], want_x0)
            worst = max(worst, ex, e0)
            assert ex <= UPDATE_TOL and e0 <= UPDATE_TOL, f"step {i}: x {ex:.3e}, pred_x0 {e0:.3e}"
    print(f"[device noise] per-step path vs native seeded loop, teacher-forced: worst {worst:.3e} (bound {UPDATE_TOL:.0e})")
    assert rel_l2(z_ps, z) <= 2e-2          # the free-running per-step latent, as test_gpu_plms.py bounds PLMS's


def test_seeded_ddpm_allocates_no_noise_stack(model):
    B, T = 2, 50
    cond, _ = _conds(model.ctx, B)
    stack_bytes = T * B * PER_ROW * 4
    model.sample(cond=cond, batch_size=B, timesteps=2, noise_seed=1)              # scratch and tables exist before the measurement

    def rise(**kw):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        z = model.sample(cond=cond, batch_size=B, timesteps=T, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(z).all()
        return torch.cuda.max_memory_allocated() - before

    seeded, stack = rise(noise_seed=1), rise()
    print(f"[device noise] DDPM {T} steps, B = {B}: torch peak rises by {seeded} B seeded, {stack} B with the stack ({stack_bytes} B)")
    assert seeded < stack_bytes <= stack


def test_errors_leave_the_context_usable(tiny):
    from rdm_amd import _lib
    from rdm_amd._lib import RdmError
    ctx, _, _ = tiny
    d = ctx.device
    out = torch.zeros(8, device=d)
    raw = lambda fn, *a: ctx._check(fn(ctx._h, *a))
    with pytest.raises(RdmError, match="reserved"):
        ctx.op_randn(1, 2, 4, stream=2)
    with pytest.raises(RdmError, match="reserved"):
        ctx.op_rng_words(1, 2, 4, stream=2)
    with pytest.raises(RdmError, match="32 bits"):                      # the binding ...
        ctx.op_randn(1, 2, 4, row0=2 ** 32 - 1)
    with pytest.raises(RdmError, match="32 bits"):                      # ... and the C ABI behind it
        raw(_lib.lib.rdm_op_randn, 1, 2 ** 32 - 1, 2, 4, 0, 0, _lib._ptr(out))
    with pytest.raises(RdmError, match="per_row"):
        ctx.op_randn(1, 2, 0)
    with pytest.raises(RdmError, match="per_row"):
        raw(_lib.lib.rdm_op_randn, 1, 0, 2, 0, 0, 0, _lib._ptr(out))
    with pytest.raises(RdmError, match="2\\^34"):
        raw(_lib.lib.rdm_op_randn, 1, 0, 1, 2 ** 34 + 1, 0, 0, _lib._ptr(out))
    assert (out == 0).all()
    cond, uncond = _conds(ctx, 2)
    ac = odiff.Schedule().alphas_cumprod
    x_T, noise = _stack(ctx, 4, 2, 4)
    with pytest.raises(RdmError, match="not both"):
        ctx.ddim_sample(4, x_T, cond, None, ac, eta=1.0, noise=noise, seed=4)
    with pytest.raises(RdmError, match="not both"):
        ctx.ddpm_sample(4, x_T, cond, noise, _ddpm_sched(), seed=4)
    with pytest.raises(RdmError, match="32 bits"):
        ctx.ddim_sample(4, None, cond, None, ac, eta=1.0, seed=4, row0=2 ** 32 - 2, shape=LATENT)
    with pytest.raises(RdmError, match="32 bits"):
        ctx.ddpm_sample(4, None, cond, None, _ddpm_sched(), seed=4, row0=-1, shape=LATENT)
    with pytest.raises(RdmError, match="shape"):
        ctx.ddim_sample(4, None, cond, None, ac, eta=1.0, seed=4)            # no x_T and no latent shape
    with pytest.raises(RdmError):
        ctx.ddim_sample(4, None, cond, None, ac, eta=1.0)                    # no x_T and no seed
    z = ctx.ddim_sample(4, None, cond, uncond, ac, eta=1.0, scale=2.0, seed=4, shape=LATENT)[0]
    torch.cuda.synchronize()
    assert z.shape == x_T.shape and torch.isfinite(z).all()
    assert torch.isfinite(ctx.op_randn(1, 2, 4)).all()
