"""The first-stage ENCODER held to oracle/vq_emul.py::vq_encode_emulated layer by layer: the models, the layer table and the teacher-forced
comparison, shared by tests/test_gpu_vq_encoder.py (the library's rdm_debug_tap blocks 1500 .. as "the library's taps") and
tests/test_vq_encoder_cpu.py (the taps of a deliberately ALTERED restatement in their place: the comparison must tell each alteration
apart, so the GPU test would fail on the same mistake in a kernel or in vqenc_body).

Teacher-forced: layer i of the restatement starts from the LIBRARY's value of layer i - 1, so each comparison is one layer deep and a
mistake shows at its own layer.  Bounds are tests/test_gpu_emul.py's: STAGE_TOL = 5e-4 for a layer that is one op (conv_in, a Downsample
conv, the wide tail's norm_out + swish and conv_out: one fp32 result, one bf16 rounding), 2 STAGE_TOL for a ResnetBlock or an AttnBlock
(4 - 6 roundings deep), STAGE_TOL for the returned latent against the restatement run from the library's last tapped layer."""
import contextlib
import functools

import torch

from oracle import unet as ounet
from oracle import vq_emul
from oracle import vqdecoder as ovq

from _util import rel_l2

STAGE_TOL = 5e-4               # tests/test_gpu_emul.py
TAP0 = 1500                    # rdm_debug_tap: the encoder's conv_in output
SEED = 17                      # the synthesis call of tests/test_gpu_training.py::test_vq_encode

# name -> (spec, image shape): the shipped VQ-f4 topology on a non-square batch of two (strip convs at 128 wide, halo convs at 64 and 32,
# both Downsamples, a 512-token AttnBlock at C = 512); the tiny VQ-f4 encoder at a 5 x 9 latent (45 tokens padded to 64, odd-width generic
# convs, conv_in on a partial wave); the tiny VQGAN wide encoder (a level AttnBlock, the wide tail)
MODELS = {"shipped": (ovq.shipped_vq_spec, (2, 3, 64, 128)), "tiny": (ovq.tiny_vq_spec, (2, 3, 20, 36)), "vqgan": (ovq.tiny_vqgan_spec, (2, 3, 32, 32))}
N_LAYERS = {"shipped": 12, "tiny": 9, "vqgan": 12}


def vq_cfg(spec):
    from rdm_amd import _lib
    return _lib.make_vq_cfg(embed_dim=spec.embed_dim, n_embed=spec.n_embed, z_channels=spec.z_channels, ch=spec.ch, ch_mult=spec.ch_mult,
                            num_res_blocks=spec.num_res_blocks, out_ch=spec.out_ch, resolution=spec.resolution, mid_attn=spec.mid_attn,
                            attn_resolutions=spec.attn_resolutions)


def layers(spec, shape):
    """[(name, kind, (B, H*W, C))] in execution order, from vq_encoder_param_shapes alone; kind "op" (one op) or "block" """
    p = ovq.vq_encoder_param_shapes(spec)
    B, _, H, W = shape
    out = [("conv_in", "op", (B, H * W, spec.ch))]
    nl = len(spec.ch_mult)
    for lvl in range(nl):
        for i in range(spec.num_res_blocks):
            pre = f"encoder.down.{lvl}.block.{i}"
            ch = p[pre + ".conv2.weight"][0]
            out.append((pre[8:], "block", (B, H * W, ch)))
            if f"encoder.down.{lvl}.attn.{i}.q.weight" in p:
                out.append((f"down.{lvl}.attn.{i}", "block", (B, H * W, ch)))
        if lvl != nl - 1:
            H, W = H // 2, W // 2
            out.append((f"down.{lvl}.downsample", "op", (B, H * W, p[f"encoder.down.{lvl}.downsample.conv.weight"][0])))
    ch = p["encoder.mid.block_1.conv2.weight"][0]
    out.append(("mid.block_1", "block", (B, H * W, ch)))
    if "encoder.mid.attn_1.q.weight" in p:
        out.append(("mid.attn_1", "block", (B, H * W, ch)))
    out.append(("mid.block_2", "block", (B, H * W, ch)))
    if spec.z_channels > 4:
        out.append(("norm_out + swish", "op", (B, H * W, ch)))
        out.append(("conv_out", "op", (B, H * W, spec.z_channels)))
    return out


def bound(kind):
    return STAGE_TOL if kind == "op" else 2 * STAGE_TOL


@functools.lru_cache(maxsize=None)
def model(name):
    """-> (spec, sd, x, free-running taps of the restatement, its latent, the fp32 oracle's latent); computed once, never written to"""
    torch.set_grad_enabled(False)
    mk, shape = MODELS[name]
    spec = mk()
    sd = ounet.synth_state_dict(ovq.vq_encoder_param_shapes(spec), seed=SEED)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1500 + shape[2])) * 2 - 1
    taps = []
    z_emu = vq_emul.vq_encode_emulated(sd, spec, x, taps=taps)
    return spec, sd, x, tuple(taps), z_emu, ovq.vq_encode(sd, spec, x)


def teacher_forced(name, lib_taps, lib_latent=None):
    """lib_taps: {i: [B, H*W, C]} 'the library's' layer outputs -> ([(layer name, kind, error)], error of lib_latent against the
    restatement run from the library's last layer, or None)"""
    spec, sd, x = model(name)[:3]
    own = []
    z_tf = vq_emul.vq_encode_emulated(sd, spec, x, taps=own, forced=lib_taps)
    table = layers(spec, tuple(x.shape))
    assert len(own) == len(table) == len(lib_taps), (len(own), len(table), len(lib_taps))
    rows = [(nm, kind, rel_l2(lib_taps[i], own[i])) for i, (nm, kind, _) in enumerate(table)]
    return rows, (None if lib_latent is None else rel_l2(lib_latent, z_tf))


def exceeding(rows):
    """names of the layers whose error is above their bound"""
    return [nm for nm, kind, e in rows if not e <= bound(kind)]


def report(tag, rows, e_latent=None):
    worst = max(rows, key=lambda r: r[2])
    for i, (nm, kind, e) in enumerate(rows):
        print(f"[vqenc] {tag} layer {i:2d} {nm:22s} {e:.3e} (bound {bound(kind):.0e})")
    print(f"[vqenc] {tag}, {len(rows)} layers teacher-forced: worst {worst[2]:.3e} at {worst[0]}" +
          ("" if e_latent is None else f"; latent from the library's last layer {e_latent:.3e}"))


# ------------------------------------------------------------------------------------------------ the 3-channel quantiser past its grid cap
# vq_quantize_kernel launches at most 1024 blocks of 256 threads: beyond 262 144 pixels a thread takes a second grid-stride trip.
QUANT_SHAPE = (1, 3, 520, 512)     # 266 240 pixels: 4 096 of them on a second trip
QUANT_U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def quantizer_case():
    """-> (decoder spec, its state dict (the tiny 512-entry codebook), z fp32 [1, 3, 520, 512]); computed once"""
    spec = ovq.tiny_vq_spec()
    sd = ounet.synth_state_dict(ovq.vq_param_shapes(spec), seed=5)
    z = torch.randn(QUANT_SHAPE, generator=torch.Generator().manual_seed(520)) * 0.6
    return spec, sd, z


def quantize_fp32_formula(z, e):
    """numpy fp32 evaluation of vq_quantize_kernel's formula: d_j = (|z|^2 + |e_j|^2) - 2 z.e_j with the kernel's association, first
    minimum; z_q = z + (e[idx] - z).  -> (zq NCHW fp32 tensor, idx int32 [pixels])"""
    import numpy as np
    zf = z.permute(0, 2, 3, 1).reshape(-1, 3).numpy().astype(np.float32)
    en = e.numpy().astype(np.float32)
    ew = (en[:, 0] * en[:, 0] + en[:, 1] * en[:, 1]) + en[:, 2] * en[:, 2]
    idx = np.empty(zf.shape[0], np.int32)
    for s in range(0, zf.shape[0], 16384):
        c = zf[s:s + 16384]
        zz = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        dot = (c[:, 0:1] * en[None, :, 0] + c[:, 1:2] * en[None, :, 1]) + c[:, 2:3] * en[None, :, 2]
        d = (zz[:, None] + ew[None, :]) - np.float32(2.0) * dot
        assert d.dtype == np.float32
        idx[s:s + 16384] = d.argmin(1)
    zq = zf + (en[idx] - zf)
    B, _, H, W = z.shape
    return torch.from_numpy(zq).reshape(B, H, W, 3).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(idx)


def check_quantized(z, e, zq, idx):
    """Every pixel, none exempt: with d the fp64 squared distance to each code, d[idx] - min d <= 8 u (|z|^2 + |e_idx|^2) (the fp32
    evaluation has fewer than eight roundings of terms that size); zq == z + (e[idx] - z) in fp32, bitwise.  -> worst (d[idx] - min d) / bound"""
    B, _, H, W = z.shape
    idx = idx.reshape(-1).long()
    assert idx.numel() == B * H * W and int(idx.min()) >= 0 and int(idx.max()) < e.shape[0]
    zf = z.permute(0, 2, 3, 1).reshape(-1, 3)
    zd, ed = zf.double(), e.double()
    worst = 0.0
    for s in range(0, zd.shape[0], 32768):
        c, ci = zd[s:s + 32768], idx[s:s + 32768]
        d = sum((c[:, k:k + 1] - ed[None, :, k]) ** 2 for k in range(3))
        gap = d.gather(1, ci[:, None])[:, 0] - d.min(1).values
        bnd = 8 * QUANT_U * ((c ** 2).sum(1) + (ed[ci] ** 2).sum(1))
        bad = int((gap > bnd).sum())
        assert bad == 0, f"{bad} pixels of [{s}, {s + c.shape[0]}) chose a code further than the bound allows (worst gap / bound {float((gap / bnd).max()):.3g})"
        worst = max(worst, float((gap / bnd).max()))
    want = (zf + (e[idx] - zf)).reshape(B, H, W, 3).permute(0, 3, 1, 2).contiguous()
    assert zq.shape == want.shape and torch.equal(zq.contiguous().view(torch.int32), want.view(torch.int32)), \
        f"zq differs from z + (e[idx] - z) in {int((zq != want).sum())} elements"
    return worst


# ------------------------------------------------------------------------------------------------ altered restatements (CPU near misses)
@contextlib.contextmanager
def _patched(attr, value):
    old = getattr(vq_emul, attr)
    setattr(vq_emul, attr, value)
    try:
        yield
    finally:
        setattr(vq_emul, attr, old)


def first_nin_shortcut(name):
    """(state-dict key of the first nin_shortcut bias, its block's layer name)"""
    sd = model(name)[1]
    key = sorted(k for k in sd if k.endswith("nin_shortcut.bias"))[0]
    return key, key[len("encoder."):-len(".nin_shortcut.bias")]


def altered_taps(name, how):
    """{i: taps} and latent of a free-running restatement that is wrong in one place: how = "pad" (Downsample padded (1, 0, 1, 0)),
    "nin_bias" (the first nin_shortcut's bias dropped), "eps" (every GroupNorm at eps 1e-5), "none" (unaltered)"""
    spec, sd, x = model(name)[:3]
    ctxm = contextlib.nullcontext()
    if how == "pad":
        ctxm = _patched("DOWN_PAD", (1, 0, 1, 0))
    elif how == "eps":
        ctxm = _patched("GN_EPS", 1e-5)
    elif how == "nin_bias":
        sd = dict(sd)
        key = first_nin_shortcut(name)[0]
        sd[key] = torch.zeros_like(sd[key])
    else:
        assert how == "none", how
    taps = []
    with ctxm:
        z = vq_emul.vq_encode_emulated(sd, spec, x, taps=taps)
    return dict(enumerate(taps)), z
