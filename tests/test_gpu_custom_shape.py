"""Sampling at other image sizes (ldm's "convolutional sampling", sample_log(custom_shape=) at rdm/models/diffusion/ddpm.py:988-1011): the
UNet, the samplers and the first stage at non-square and non-training sizes against the fp32 CPU oracle, the 64-column strip form of the
3x3 conv at 192-wide output tiles, and the Python surface (MinimalRETRODiffusion, scripts/rdm_sample.py --height / --width).

Bounds are the project's stated ones (tests/test_gpu_models.py header), relative L2 against the fp32 oracle: one UNet forward 2.5e-2, a short
DDIM trajectory 4e-2, VQ decode / encode 2.5e-2; PLMS and DPM-Solver++ latents at the 2.5e-2 of their own test files; the conv op at
test_gpu_ops.py's 2^-7 max|ref|."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff
from oracle import unet as ounet
from oracle import vqdecoder as ovq

import _dpmpp_ref as dpmpp_ref
from _util import bf16_round, rel_l2, spec_to_unet_cfg, spec_to_vq_cfg
from test_gpu_ops import _close, _conv_ref, _pack_conv, _rand
from test_gpu_plms import _plms_loop, _schedule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

UNET_TOL, DDIM_TOL, VQ_TOL, SAMPLER_TOL = 2.5e-2, 4e-2, 2.5e-2, 2.5e-2
INDEX_AGREEMENT = 0.995
VQ_SEED = 5


def _within(what, value, bound):
    print(f"[custom shape] {what}: measured {value:.3e} (bound {bound:.1e})")
    assert value <= bound, f"{what}: {value} > {bound}"


def _vq_state_dict(vspec):
    shapes = dict(ovq.vq_param_shapes(vspec)); shapes.update(ovq.vq_encoder_param_shapes(vspec))
    return ounet.synth_state_dict(shapes, seed=VQ_SEED)


@pytest.fixture(scope="module")
def model(ctx):
    """The tiny UNet (down factor 4) and the tiny VQ-f4 first stage (decoder + encoder, factor 4) behind a MinimalRETRODiffusion on the session context."""
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    spec, vspec = ounet.tiny_spec(), ovq.tiny_vq_spec()
    fs = {"params": {"embed_dim": 3, "n_embed": vspec.n_embed, "ddconfig": {"z_channels": 3, "ch": vspec.ch, "ch_mult": vspec.ch_mult,
                                                                          "num_res_blocks": vspec.num_res_blocks, "resolution": vspec.resolution}}}
    up = dict(in_channels=spec.in_channels, out_channels=spec.out_channels, model_channels=spec.model_channels,
              num_res_blocks=spec.num_res_blocks, attention_resolutions=spec.attention_resolutions, channel_mult=spec.channel_mult,
              num_head_channels=spec.num_head_channels, context_dim=spec.context_dim)
    m = MinimalRETRODiffusion(unet_config={"params": up}, first_stage_config=fs, k_nn=4, image_size=16, ctx=ctx)
    m.sd_unet = ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234)
    m.sd_vq = _vq_state_dict(vspec)
    m.load_unet_state_dict(m.sd_unet)
    m.load_first_stage_state_dict(m.sd_vq)
    m.spec, m.vspec = spec, vspec
    return m


def _unet_inputs(B, H, W, seed, k=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    c = torch.randn(B, k, 512, generator=g) * 0.45
    c[B - 1] = 0                                  # one zero-context row (the unconditional half of a guided batch)
    return x, t, c


# ------------------------------------------------------------------------------------------------ 1. UNet forward
@pytest.mark.parametrize("H,W", [(16, 24), (24, 16), (20, 40), (8, 128)])
def test_unet_forward_non_square(model, H, W):
    """Tiny spec, B = 3 with one zero-context row, k = 4.  (20, 40): level pixel counts 800 / 200 / 50 (GroupNorm chunks that do not divide,
    self-attention with n % 32 != 0) and widths 40 / 20 / 5 (generic conv); (8, 128): wider than 64 (the strip conv where N % 128 == 0)."""
    ctx = model.ctx
    x, t, c = _unet_inputs(3, H, W, 100 + H * W)
    eps = ctx.unet_forward(x, t, c)
    assert tuple(eps.shape) == (3, 3, H, W)
    ref = ounet.unet_forward(model.sd_unet, model.spec, x, t, c)
    _within(f"unet forward at latent {H}x{W} vs oracle", rel_l2(eps, ref), UNET_TOL)
    if (H, W) == (20, 40):
        one = ctx.unet_forward(x[1:2], t[1:2], c[1:2])
        assert torch.equal(eps[1:2].cpu(), one.cpu()), "row 1 of the batch differs from the same sample run alone"


# ------------------------------------------------------------------------------------------------ 2. samplers
def _sampler_inputs(B, H, W, seed, device):
    rng = np.random.default_rng(seed)
    x_T = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).to(device)
    cond = torch.from_numpy((rng.standard_normal((B, 4, 512)) * 0.45).astype(np.float32)).to(device)
    return x_T, cond, torch.zeros_like(cond)


def _guided_eps(model, B, cond, uc, scale):
    c_cpu, u_cpu = cond.cpu(), uc.cpu()

    def eps(x, t):
        out = ounet.unet_forward(model.sd_unet, model.spec, torch.cat([x, x]), torch.full((2 * B,), t, dtype=torch.long), torch.cat([c_cpu, u_cpu]))
        return out[B:] + scale * (out[:B] - out[B:])
    return eps


def test_guided_ddim_non_square(model):
    B, S, scale = 2, 4, 2.0
    x_T, cond, uc = _sampler_inputs(B, 16, 24, 31, "cpu")
    sched = odiff.Schedule()
    z = model.ctx.ddim_sample(S, x_T, cond, uc, sched.alphas_cumprod, scale=scale)[0]
    assert tuple(z.shape) == (B, 3, 16, 24)
    apply = lambda x, t, c: ounet.unet_forward(model.sd_unet, model.spec, x, t, c)
    z_ref, _ = odiff.ddim_sample(apply, sched, S, x_T, cond, scale=scale, uncond=uc)
    _within("guided DDIM (4 steps, scale 2.0) at latent 16x24 vs oracle", rel_l2(z, z_ref), DDIM_TOL)


def test_plms_non_square(model):
    from rdm_amd.models.diffusion.plms import PLMSSampler
    B, S, scale = 2, 4, 2.0
    x_T, cond, uc = _sampler_inputs(B, 24, 16, 32, model.device)
    z, _ = PLMSSampler(model).sample(S, B, (3, 24, 16), conditioning=cond, x_T=x_T, verbose=False, unconditional_guidance_scale=scale,
                                     unconditional_conditioning=uc)
    assert tuple(z.shape) == (B, 3, 24, 16)
    z_ref = _plms_loop(_guided_eps(model, B, cond, uc, scale), S, x_T.cpu(), _schedule(S))
    _within("PLMS (4 steps, scale 2.0) at latent 24x16 vs the oracle PLMS loop", rel_l2(z, z_ref), SAMPLER_TOL)


def test_dpm_solver_non_square(model):
    from rdm_amd.models.diffusion.dpm_solver import DPMSolverSampler
    B, S, scale = 2, 4, 2.0
    x_T, cond, uc = _sampler_inputs(B, 24, 16, 33, model.device)
    z, _ = DPMSolverSampler(model).sample(S, B, (3, 24, 16), conditioning=cond, x_T=x_T, verbose=False, unconditional_guidance_scale=scale,
                                          unconditional_conditioning=uc)
    assert tuple(z.shape) == (B, 3, 24, 16)
    acp = odiff.Schedule().alphas_cumprod.numpy()
    nodes = dpmpp_ref.timesteps(acp, S, "logSNR")
    z_ref, _, _ = dpmpp_ref.sample(_guided_eps(model, B, cond, uc, scale), nodes, x_T.cpu(), acp, order=2, lower_order_final=True)
    _within("DPM-Solver++ (4 steps, scale 2.0) at latent 24x16 vs the oracle D-form loop", rel_l2(z, z_ref), SAMPLER_TOL)


# ------------------------------------------------------------------------------------------------ 3. first-stage decode
def _latent(B, h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((B, 3, h, w)).astype(np.float32))


def _check_decode(ctx, sd, vspec, z, what):
    """force_not_quantize image against the oracle; quantised path: index agreement with the oracle's arg-min, image against the oracle
    decoding the codebook rows of the library's OWN indices (a flipped near-tie can neither hide nor cause a failure)."""
    B, _, h, w = z.shape
    f = 1 << (len(vspec.ch_mult) - 1)
    img_nq = ctx.vq_decode(z, force_not_quantize=True)
    assert tuple(img_nq.shape) == (B, 3, f * h, f * w)
    _within(f"{what}: unquantised decode vs oracle", rel_l2(img_nq, ovq.vq_decode(sd, vspec, z, force_not_quantize=True)), VQ_TOL)
    img, idx = ctx.vq_decode(z, return_indices=True)
    idx = idx.cpu().long()
    _, idx_ref = ovq.vq_quantize(sd, z)
    agree = float((idx == idx_ref).float().mean())
    print(f"[custom shape] {what}: index agreement with the oracle arg-min {agree:.4f} (bound {INDEX_AGREEMENT})")
    assert agree >= INDEX_AGREEMENT
    zq = sd["quantize.embedding.weight"][idx].reshape(B, h, w, 3).permute(0, 3, 1, 2).contiguous()
    _within(f"{what}: quantised decode vs oracle on the library's indices", rel_l2(img, ovq.vq_decode(sd, vspec, zq, force_not_quantize=True)), VQ_TOL)


@pytest.mark.parametrize("h,w", [(16, 24), (24, 16), (8, 40), (5, 7)])
def test_vq_decode_non_square(model, h, w):
    """(5, 7): 35 latent pixels -- the mid AttnBlock on a token count that is no multiple of 64 (padded keys), odd widths on the generic conv."""
    _check_decode(model.ctx, model.sd_vq, model.vspec, _latent(2, h, w, 40 + h * w), f"tiny VQ decode at latent {h}x{w}")


def test_vq_decode_walked_in_ranges_non_square(model, tmp_path):
    """A child process with RDM_VQ_RANGE=2 decodes 3 latents of 16 x 24 in ranges of 2 and 1: bit for bit the one-range result."""
    z = _latent(3, 16, 24, 77)
    whole, whole_idx = model.ctx.vq_decode(z, return_indices=True)
    out = tmp_path / "ranges.npz"
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, numpy as np, torch\n"
        f"sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})\n"
        "import rdm_amd\nfrom rdm_amd import _lib, packing\nfrom oracle import vqdecoder as ovq, unet as ounet\nfrom _util import spec_to_vq_cfg\n"
        "torch.set_grad_enabled(False)\nctx = _lib.Context(0)\nspec = ovq.tiny_vq_spec()\n"
        "shapes = dict(ovq.vq_param_shapes(spec)); shapes.update(ovq.vq_encoder_param_shapes(spec))\n"
        f"sd = ounet.synth_state_dict(shapes, seed={VQ_SEED})\n"
        "cfg = spec_to_vq_cfg(spec)\nctx.load_vq(cfg, packing.pack('vq', cfg, sd))\n"
        "z = torch.from_numpy(np.random.default_rng(77).standard_normal((3, 3, 16, 24)).astype(np.float32))\n"
        "img, idx = ctx.vq_decode(z, return_indices=True)\n"
        f"np.savez({str(out)!r}, img=img.cpu().numpy(), idx=idx.cpu().numpy())\nctx.close()\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RDM_VQ_RANGE="2"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert np.array_equal(got["idx"], whole_idx.cpu().numpy())
    assert np.array_equal(got["img"], whole.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 4. quantise and encode
def test_vq_quantize_non_square(model):
    z = torch.from_numpy((np.random.default_rng(9).standard_normal((2, 3, 8, 40)) * 0.7).astype(np.float32))
    zq, idx = model.ctx.vq_quantize(z, return_indices=True)
    rq, ridx = ovq.vq_quantize(model.sd_vq, z)
    assert tuple(zq.shape) == (2, 3, 8, 40) and idx.numel() == 2 * 8 * 40
    agree = float((idx.cpu().long() == ridx).float().mean())
    print(f"[custom shape] vq_quantize at 8x40: index agreement {agree:.4f} (bound {INDEX_AGREEMENT})")
    assert agree >= INDEX_AGREEMENT
    own = model.sd_vq["quantize.embedding.weight"][idx.cpu().long()].reshape(2, 8, 40, 3).permute(0, 3, 1, 2)
    assert (zq.cpu() - (z + (own - z))).abs().max().item() <= 1e-6          # straight-through form on the library's own indices
    if agree == 1.0:
        assert (zq.cpu() - rq).abs().max().item() <= 1e-6


@pytest.mark.parametrize("H,W", [(64, 96), (32, 160)])
def test_vq_encode_non_square(model, H, W):
    x = torch.from_numpy(np.random.default_rng(H + W).uniform(-1.0, 1.0, (2, 3, H, W)).astype(np.float32))
    z = model.encode_first_stage(x)
    assert tuple(z.shape) == (2, 3, H // 4, W // 4)
    _within(f"tiny VQ encode of {H}x{W} images vs oracle", rel_l2(z, ovq.vq_encode(model.sd_vq, model.vspec, x)), VQ_TOL)


def test_vq_encode_refuses_sizes_the_downsamples_do_not_halve(model):
    from rdm_amd._lib import RdmError
    with pytest.raises(RdmError, match="multiples of 4"):
        model.ctx.vq_encode(torch.zeros(1, 3, 30, 64))
    with pytest.raises(RdmError):
        model.ctx.vq_encode(torch.zeros(1, 4, 32, 64))           # channel count
    with pytest.raises(RdmError):
        model.ctx.vq_decode(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RdmError):
        model.ctx.vq_quantize(torch.zeros(3, 8, 8))              # rank
    z = model.ctx.vq_encode(torch.zeros(1, 3, 32, 64))           # the context is still usable
    assert tuple(z.shape) == (1, 3, 8, 16)


# ------------------------------------------------------------------------------------------------ 5. shipped topology
def test_shipped_topology_wide_latents():
    """The only cases in which the 192-wide strip conv (UNet level 0 at a 128-wide latent) and the decoder's strip levels (128-, 256- and
    512-pixel-wide rows) run inside the models: shipped UNet at latent 32 x 128, B = 2 with one zero-context row; shipped VQ-f4 decode of
    one 16 x 128 latent (a 64 x 512 image)."""
    from rdm_amd import _lib, packing
    spec, vspec = ounet.shipped_spec(), ovq.shipped_vq_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=99)
    vsd = ounet.synth_state_dict(ovq.vq_param_shapes(vspec), seed=98)
    c2 = _lib.Context(0)
    try:
        cfg, vcfg = spec_to_unet_cfg(spec), spec_to_vq_cfg(vspec)
        c2.load_unet(cfg, packing.pack("unet", cfg, sd))
        c2.load_vq(vcfg, packing.pack("vq", vcfg, vsd))
        x, t, c = _unet_inputs(2, 32, 128, 8)
        eps = c2.unet_forward(x, t, c)
        _within("shipped UNet at latent 32x128 vs oracle", rel_l2(eps, ounet.unet_forward(sd, spec, x, t, c)), UNET_TOL)
        z = _latent(1, 16, 128, 12)
        img, idx = c2.vq_decode(z, return_indices=True)
        assert tuple(img.shape) == (1, 3, 64, 512)
        idx = idx.cpu().long()
        agree = float((idx == ovq.vq_quantize(vsd, z)[1]).float().mean())
        print(f"[custom shape] shipped VQ-f4 at latent 16x128: index agreement {agree:.4f} (bound {INDEX_AGREEMENT})")
        assert agree >= INDEX_AGREEMENT
        zq = vsd["quantize.embedding.weight"][idx].reshape(1, 16, 128, 3).permute(0, 3, 1, 2).contiguous()
        _within("shipped VQ-f4 decode of a 16x128 latent vs oracle on the library's indices",
                rel_l2(img, ovq.vq_decode(vsd, vspec, zq, force_not_quantize=True)), VQ_TOL)
    finally:
        c2.close()


# ------------------------------------------------------------------------------------------------ 6. strip form at N % 192
@pytest.mark.parametrize("B,H,W,C0,C1,N", [(1, 4, 128, 64, 0, 192), (2, 8, 192, 64, 64, 192), (1, 8, 128, 128, 0, 576), (1, 4, 256, 64, 0, 960)])
def test_conv3x3_strips_at_192_wide_tiles(ctx, B, H, W, C0, C1, N):
    """Images wider than 64 pixels with N % 192 == 0: plain, and with the per-sample row + residual (dual source where C1 > 0).  Inputs are
    random across the whole width: a strip that read zeros for its side halo fails."""
    d = ctx.device
    C = C0 + C1
    x0 = bf16_round(_rand((B, H, W, C0), 60))
    x1 = bf16_round(_rand((B, H, W, C1), 61)) if C1 else None
    w, b = bf16_round(_rand((N, C, 3, 3), 62, (9 * C) ** -0.5)), _rand((N,), 63, 0.1)
    xc = x0 if x1 is None else torch.cat([x0, x1], -1)
    ref = _conv_ref(xc, w, b)
    dev = lambda v: None if v is None else v.to(d, torch.bfloat16)
    out = ctx.op_conv3x3(dev(x0), dev(_pack_conv(w)), b.to(d), x1=dev(x1))
    assert tuple(out.shape) == (B, H, W, N)
    _close(out, ref, what="192-wide strip conv3x3")
    temb, res = _rand((B, N), 64), bf16_round(_rand((B, H, W, N), 65))
    out2 = ctx.op_conv3x3(dev(x0), dev(_pack_conv(w)), b.to(d), x1=dev(x1), rowvec=temb.to(d), residual=dev(res))
    _close(out2, ref + temb[:, None, None, :] + res, what="192-wide strip conv3x3 + row + residual")


# ------------------------------------------------------------------------------------------------ 7. surface
@pytest.fixture(scope="module")
def retriever(ctx):
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    rng = np.random.default_rng(21)
    N = 20_000
    pool = {"embedding": (rng.standard_normal((N, 512)) * 0.45).astype(np.float16), "img_id": np.arange(N) * 3,
            "patch_coords": rng.integers(0, 1200, (N, 4))}
    db = DatasetBuilder(data_pool=pool, k=20, ctx=ctx)
    db.train_searcher()
    return db


def test_sample_with_query_custom_shape(model, retriever):
    model.retriever = retriever
    model.unconditional_guidance_vex = torch.randn(512, device=model.device)
    q = torch.from_numpy((np.random.default_rng(23).standard_normal((2, 512)) * 0.45).astype(np.float32))
    latents = []
    real = model.sample_log
    model.sample_log = lambda **kw: (lambda r: (latents.append(r[0].clone()), r)[1])(real(**kw))       # the sample_log latent of the call
    try:
        torch.manual_seed(5)
        img = model.sample_with_query(query=q, query_embedded=True, k_nn=4, ddim=True, ddim_steps=4, unconditional_guidance_scale=2.0,
                                      unconditional_retro_guidance_label=0., visualize_nns=False, custom_shape=(3, 16, 24))["query_samples"]
    finally:
        model.sample_log = real
    assert tuple(img.shape) == (2, 3, 64, 96) and tuple(latents[0].shape) == (2, 3, 16, 24)
    assert bool(torch.isfinite(img).all()) and img.std().item() > 1e-3
    assert torch.equal(img.cpu(), model.decode_first_stage(latents[0]).cpu())
    with pytest.raises(ValueError, match="down factor 4"):
        model.sample_with_query(query=q, query_embedded=True, k_nn=4, ddim=True, ddim_steps=4, custom_shape=(3, 18, 24))
    with pytest.raises(ValueError, match="down factor 4"):
        model.sample_log(cond=torch.zeros(2, 4, 512), batch_size=2, ddim=True, ddim_steps=4, custom_shape=(3, 16, 22))


def test_ddpm_loop_takes_shape(model):
    """ldm's sample(shape=): the ancestral loop at a 24 x 16 latent for 4 timesteps, against the oracle's loop on the same noise."""
    rng = np.random.default_rng(41)
    B, T = 2, 4
    x_T = torch.from_numpy(rng.standard_normal((B, 3, 24, 16)).astype(np.float32))
    cond = torch.from_numpy((rng.standard_normal((B, 4, 512)) * 0.45).astype(np.float32))
    noise = torch.from_numpy(rng.standard_normal((T, B, 3, 24, 16)).astype(np.float32))
    z = model.sample(cond=cond, batch_size=B, shape=(B, 3, 24, 16), x_T=x_T, noise=noise, timesteps=T)
    assert tuple(z.shape) == (B, 3, 24, 16)
    apply = lambda x, t, c: ounet.unet_forward(model.sd_unet, model.spec, x, t, c)
    _within("DDPM loop (4 timesteps) at latent 24x16 vs oracle", rel_l2(z, odiff.ddpm_sample(apply, odiff.Schedule(), x_T, cond, noise, timesteps=T)), DDIM_TOL)
    z2 = model.sample(cond=cond.to(model.device), batch_size=B, shape=(B, 3, 24, 16), timesteps=T)       # noise drawn at the shape
    assert tuple(z2.shape) == (B, 3, 24, 16) and bool(torch.isfinite(z2).all())
    with pytest.raises(ValueError, match="down factor 4"):
        model.sample(cond=cond, batch_size=B, shape=(B, 3, 24, 18), timesteps=T)


def _script():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "rdm_sample.py")
    spec = importlib.util.spec_from_file_location("rdm_sample_native_sizes", path)
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_rdm_sample_script_height_width(tmp_path):
    """scripts/rdm_sample.py --height 128 --width 256 on the shipped architectures (seeded random weights / database): 256 x 128 PNGs."""
    from PIL import Image
    mod = _script()
    with pytest.raises(SystemExit):
        mod.parse_args(["--synthetic", "--gpu", "0", "--width", "200"])
    opt = mod.parse_args(["--synthetic", "--synthetic_db_rows", "20000", "--gpu", "0", "-bs", "2", "-n", "1", "--steps", "4",
                          "--height", "128", "--width", "256", "-s", str(tmp_path)])
    model = mod.load_model(opt)
    try:
        mod.sample_unconditional(model, opt)
        files = sorted(tmp_path.iterdir())
        assert len(files) == 2
        for f in files:
            im = Image.open(f)
            assert im.size == (256, 128)                          # PIL: (width, height)
            assert len(np.unique(np.asarray(im))) > 16            # not a constant image
    finally:
        model.ctx.close()
