"""The first-stage ENCODER held to the CPU restatement of its own arithmetic (oracle/vq_emul.py::vq_encode_emulated), layer by layer
and teacher-forced through rdm_debug_tap blocks 1500, 1501, ... -- what tests/test_gpu_emul.py does for the UNet and the VQ-f4 decoder.
The whole-latent assertions elsewhere (2.5e-2 against the fp32 oracle: the bf16 storage distance) cannot see a GroupNorm epsilon of 1e-5
(1.2e-2 either way) and see a dropped bias or a mis-padded Downsample only by its size; here each layer starts from the LIBRARY's value of
the layer before it and is held at STAGE_TOL = 5e-4 (one op) / 2 STAGE_TOL (a ResnetBlock or AttnBlock), so such a mistake fails its own
line (tests/test_vq_encoder_cpu.py shows that on the CPU, through the same comparison: tests/_vqenc_ref.py).

Also here: the taps are inert (the latent is bitwise the same with one set) and exclusive (a decoder number leaves the buffer alone during
an encode, an encoder number during a decode), a short buffer receives exactly its own bytes; and the 3-channel quantiser past the 1024
blocks its launch is capped at, per pixel against fp64 distances.  The Downsample conv per element is in tests/test_gpu_forward_ops.py.

Measured on an MI355X (worst teacher-forced layer; latent from the library's last layer; free-running library / restatement vs fp32 oracle):
  shipped VQ-f4, 2 x 3 x 64 x 128:  8.2e-4 at down.2.block.1 (single ops <= 3.6e-5);  9.2e-5;  1.149e-2 / 1.152e-2
  tiny VQ-f4, 2 x 3 x 20 x 36:      6.3e-4 at down.0.block.0 (single ops <= 3.1e-5);  8.7e-7;  6.13e-3 / 6.09e-3
  tiny VQGAN, 2 x 3 x 32 x 32:      3.0e-4 at down.0.block.0 (single ops <= 1.9e-5);  4.5e-8;  9.89e-3 / 1.011e-2
  quantiser at 520 x 512: worst (d[idx] - min d) / bound 0.233, every index the fp32 oracle's argmin."""
import pytest
import torch

from oracle import unet as ounet
from oracle import vqdecoder as ovq

import _vqenc_ref as V
from _util import rel_l2, spec_to_vq_cfg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENTINEL = 0x7FC1                      # a bf16 NaN pattern no layer output holds (as int16)


def _load_encoder(ctx, name):
    from rdm_amd import packing
    spec, sd = V.model(name)[:2]
    cfg = V.vq_cfg(spec)
    ctx.load_vq_encoder(cfg, packing.pack("vqenc", cfg, sd))
    return spec, sd


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", list(V.MODELS))
def test_vq_encoder_layer_by_layer(ctx, name):
    """Every layer output of one encode -- conv_in, per level its ResnetBlocks (+ AttnBlocks) and the Downsample conv, the three mid layers,
    and the wide tail's norm_out + swish and conv_out -- teacher-forced; then the latent from the library's last tapped layer; then the
    free-running distances: library vs fp32 oracle <= 2.5e-2 and no further than 1.3 x the restatement's own distance."""
    _load_encoder(ctx, name)
    spec, sd, x, free, z_emu, z_ref = V.model(name)
    table = V.layers(spec, tuple(x.shape))
    lib, z0 = {}, None
    try:
        for i, (nm, kind, shp) in enumerate(table):
            buf = torch.empty(shp, device=ctx.device, dtype=torch.bfloat16)
            ctx.debug_tap(buf, V.TAP0 + i, 0)
            z = ctx.vq_encode(x)
            torch.cuda.synchronize()
            lib[i] = buf.float().cpu()
            z0 = z if z0 is None else z0
            assert torch.equal(_bits(z), _bits(z0)), f"the latent changed with the tap on layer {i} ({nm})"
    finally:
        ctx.debug_tap(None, -1)
    z = z0.cpu()
    rows, e_z = V.teacher_forced(name, lib, z)
    V.report(name, rows, e_z)
    assert V.exceeding(rows) == [], [(nm, f"{e:.3e}") for nm, kind, e in rows if not e <= V.bound(kind)]
    assert e_z <= V.STAGE_TOL, e_z
    e_lib, e_emu = rel_l2(z, z_ref), rel_l2(z_emu, z_ref)
    print(f"[vqenc] {name} free-running: library vs fp32 oracle {e_lib:.3e}, restatement vs fp32 oracle {e_emu:.3e}, library vs restatement {rel_l2(z, z_emu):.3e}")
    assert z.shape == z_ref.shape and e_lib <= 2.5e-2
    assert e_lib <= 1.3 * e_emu, "the library is further from fp32 than bf16 storage at its rounding points explains"


def test_taps_are_inert_exclusive_and_clipped(ctx):
    """The tiny VQ-f4 first stage, both halves loaded.  The latent with a tap set is bitwise the latent without one; a decoder block number
    set during an encode, and an encoder number during a decode, leave the buffer untouched (while the matching number does write); a
    buffer shorter than the layer receives exactly its first bytes, with the sentinel behind them intact."""
    from rdm_amd import packing
    spec, sd, x = V.model("tiny")[:3]
    _load_encoder(ctx, "tiny")
    dsd = ounet.synth_state_dict(ovq.vq_param_shapes(spec), seed=5)
    cfg = spec_to_vq_cfg(spec)
    ctx.load_vq(cfg, packing.pack("vq", cfg, dsd))
    table = V.layers(spec, tuple(x.shape))
    d = ctx.device
    fresh = lambda n: torch.full((n,), SENTINEL, device=d, dtype=torch.int16)
    untouched = lambda b: bool((b == SENTINEL).all())
    z_plain = ctx.vq_encode(x)
    zl = torch.randn(2, 3, 5, 9, generator=torch.Generator().manual_seed(59))
    img_plain = ctx.vq_decode(zl, force_not_quantize=True)
    torch.cuda.synchronize()
    i = 3                                                                    # down.1.block.0: a ResnetBlock with a nin_shortcut
    n = table[i][2][0] * table[i][2][1] * table[i][2][2]
    try:
        full = fresh(n)
        ctx.debug_tap(full.view(torch.bfloat16), V.TAP0 + i)
        z_tap = ctx.vq_encode(x)
        torch.cuda.synchronize()
        assert torch.equal(_bits(z_tap), _bits(z_plain)) and not bool((full == SENTINEL).any())
        img = ctx.vq_decode(zl, force_not_quantize=True)                       # an encoder number during a decode
        torch.cuda.synchronize()
        assert torch.equal(_bits(img), _bits(img_plain))
        for blk, run, fires in ((1001, lambda: ctx.vq_encode(x), False), (V.TAP0 + 1, lambda: ctx.vq_decode(zl, force_not_quantize=True), False),
                                (1001, lambda: ctx.vq_decode(zl, force_not_quantize=True), True), (V.TAP0 + len(table), lambda: ctx.vq_encode(x), False)):
            buf = fresh(64)
            ctx.debug_tap(buf.view(torch.bfloat16), blk)
            run()
            torch.cuda.synchronize()
            assert untouched(buf) != fires, f"block {blk}: buffer {'not written' if fires else 'written'}"
        short = 1000                                                         # elements: no multiple of the layer's width (128)
        buf = fresh(short + 256)
        ctx.debug_tap(buf[:short].view(torch.bfloat16), V.TAP0 + i)
        ctx.vq_encode(x)
        torch.cuda.synchronize()
        assert torch.equal(buf[:short], full[:short]) and untouched(buf[short:])
    finally:
        ctx.debug_tap(None, -1)


def test_quantiser_past_its_grid_cap(ctx):
    """rdm_vq_quantize_hw on 520 x 512 = 266 240 pixels (vq_quantize_kernel launches at most 1024 blocks of 256 threads: the last 4 096
    pixels are a second grid-stride trip) with the tiny 512-entry codebook.  Every pixel: d[idx] - min d <= 8 u (|z|^2 + |e_idx|^2) on fp64
    distances; zq is z + (e[idx] - z) in fp32, bitwise (tests/_vqenc_ref.py::check_quantized; the CPU test shows an fp32 evaluation of
    the kernel's formula inside the bound and a skipped second trip outside it)."""
    from rdm_amd import packing
    spec, sd, z = V.quantizer_case()
    cfg = spec_to_vq_cfg(spec)
    ctx.load_vq(cfg, packing.pack("vq", cfg, sd))
    zq, idx = ctx.vq_quantize(z, return_indices=True)
    torch.cuda.synchronize()
    worst = V.check_quantized(z, sd["quantize.embedding.weight"], zq.cpu(), idx.cpu())
    agree = float((idx.cpu().long() == ovq.vq_quantize(sd, z)[1]).float().mean())
    print(f"[vqenc] quantiser at {z.shape[2]} x {z.shape[3]}: worst (d[idx] - min d) / bound {worst:.3g}; agreement with the oracle's argmin {agree:.6f}")
