"""The first stage's streaming AttnBlock (csrc/vq_attn.hip): rdm_op_vq_attention element by element against fp64 (tests/_vq_attn_ref.py,
pinned on the CPU by tests/test_vq_attn_cpu.py), against the materialised chain it replaces, its refusals and its batch invariance; then
the executor beyond 4096 latent pixels, where the AttnBlock takes the kernel: the tiny VQ-f4 first stage (mid width 256) decoded at
64 x 72 and 66 x 70 latents against the fp32 oracle and layer by layer against the library's own arithmetic (oracle/vq_emul.py), encoded
from 256 x 288 images, walked in ranges, and decoded at 216 x 220 = 47520 latent pixels -- past the 46336 the materialised scores could
index -- with the AttnBlock's input and output tapped and 64 of its rows restated on the CPU.

Bounds: the op per element at the derived bound of _vq_attn_ref.VqAttention; one stage on the library's own inputs at test_gpu_emul.py's
STAGE_TOL = 5e-4 (a block of several stages at twice that); decode / encode against the fp32 oracle at test_gpu_custom_shape.py's 2.5e-2
with its index agreement."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet as ounet
from oracle import vqdecoder as ovq
from oracle.vq_emul import vq_decode_emulated

import _vq_attn_ref as R
from _train_ref import check
from _util import bf16_round as bf, rel_l2, spec_to_vq_cfg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

STAGE_TOL = 5e-4                      # tests/test_gpu_emul.py: one stage on the library's own inputs
VQ_TOL, INDEX_AGREEMENT = 2.5e-2, 0.995      # tests/test_gpu_custom_shape.py: first-stage decode / encode against the fp32 oracle
VQ_SEED = 5


def _within(what, value, bound):
    print(f"[vq attention] {what}: measured {value:.3e} (bound {bound:.1e})")
    assert value <= bound, f"{what}: {value} > {bound}"


# ------------------------------------------------------------------------------------------------ 1. the op
def _run(ctx, inp, strided=False):
    d = ctx.device
    dev = lambda t: t.to(d, torch.bfloat16)
    if strided:                                   # column blocks of one [B, n, 3C] tensor: row stride 3C
        qkv = torch.cat([dev(inp["q"]), dev(inp["k"]), dev(inp["v"])], 2).contiguous()
        C = inp["C"]
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        assert not q.is_contiguous()
    else:
        q, k, v = dev(inp["q"]), dev(inp["k"]), dev(inp["v"])
    out = ctx.op_vq_attention(q, k, v, bias_v=None if inp["bias"] is None else inp["bias"].to(d))
    torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_op_against_fp64_per_element(ctx, case):
    inp = R.make_case(case)
    out = _run(ctx, inp, strided=case[3].get("strided", False))
    worst, margin = check(R.VqAttention, inp, {"out": out})
    print(f"[vq attention] {R.case_id(case)}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    if case[0] > 1 and case[1] > 64:              # sample 1 is its own result, not sample 0's
        assert not torch.equal(out[0], out[1])


def test_op_refusals_leave_the_context_usable(ctx):
    from rdm_amd._lib import RdmError
    d = ctx.device
    mk = lambda n, C: torch.zeros(1, n, C, device=d, dtype=torch.bfloat16)
    for n, C, word in ((64, 192, "multiple of 128"), (0, 256, "n >= 1"), (64, 640, "multiple of 128")):
        with pytest.raises(RdmError) as e:
            ctx.op_vq_attention(mk(n, C), mk(n, C), mk(n, C))
        assert "rdm_op_vq_attention" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(RdmError):
        ctx.op_vq_attention(mk(64, 256), mk(32, 256), mk(64, 256))
    inp = R.make_case(R.CASES[1])
    check(R.VqAttention, inp, {"out": _run(ctx, inp)})


def test_op_against_the_materialised_chain(ctx):
    """(2, 256, 512): op_bmm(alpha) -> op_softmax -> op_bmm + bias_v, the chain vq_attn runs up to 4096 tokens, on the same inputs."""
    inp = R.VqAttention.make(2, 256, 512)
    d = ctx.device
    q, k, v = (inp[t].to(d, torch.bfloat16) for t in "qkv")
    s = ctx.op_bmm(q, k, alpha=R.VqAttention.scale(inp), out_f32=True)
    p = ctx.op_softmax(s)
    o = ctx.op_bmm(p, ctx.op_transpose_batched(v), out_f32=True)
    chain = (o + inp["bias"].to(d)).to(torch.bfloat16)
    out = ctx.op_vq_attention(q, k, v, bias_v=inp["bias"].to(d))
    _within("streaming op vs bmm -> softmax -> bmm + bias at (2, 256, 512)", rel_l2(out.float().cpu(), chain.float().cpu()), STAGE_TOL)


def test_op_batch_invariance(ctx):
    """rows of sample 1 of a B = 3 call are bit for bit those of a B = 1 call on that sample"""
    inp = R.VqAttention.make(3, 200, 256)
    d = ctx.device
    q, k, v = (inp[t].to(d, torch.bfloat16) for t in "qkv")
    b = inp["bias"].to(d)
    three = ctx.op_vq_attention(q, k, v, bias_v=b)
    one = ctx.op_vq_attention(q[1:2].contiguous(), k[1:2].contiguous(), v[1:2].contiguous(), bias_v=b)
    assert torch.equal(three[1:2].cpu(), one.cpu())


# ------------------------------------------------------------------------------------------------ 2. the executor beyond 4096 pixels
def _tiny():
    vs = ovq.tiny_vq_spec()
    shapes = dict(ovq.vq_param_shapes(vs)); shapes.update(ovq.vq_encoder_param_shapes(vs))
    return vs, ounet.synth_state_dict(shapes, seed=VQ_SEED)


@pytest.fixture(scope="module")
def tiny(ctx):
    from rdm_amd import packing
    vs, sd = _tiny()
    cfg = spec_to_vq_cfg(vs)
    ctx.load_vq(cfg, packing.pack("vq", cfg, sd))
    ctx.load_vq_encoder(cfg, packing.pack("vqenc", cfg, sd))
    return ctx, vs, sd


def _latent(B, h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((B, 3, h, w)).astype(np.float32))


@pytest.mark.parametrize("h,w", [(64, 72), (66, 70)])
def test_decode_against_the_oracle(tiny, h, w):
    """n = 4608 and n = 4620 (no multiple of 32): test_gpu_custom_shape.py's _check_decode -- the unquantised image against the oracle; index
    agreement with the oracle's arg-min; the quantised image against the oracle decoding the library's OWN indices."""
    ctx, vs, sd = tiny
    z = _latent(2, h, w, 40 + h * w)
    what = f"tiny VQ decode at latent {h}x{w}"
    img_nq = ctx.vq_decode(z, force_not_quantize=True)
    assert tuple(img_nq.shape) == (2, 3, 4 * h, 4 * w)
    _within(f"{what}: unquantised decode vs oracle", rel_l2(img_nq, ovq.vq_decode(sd, vs, z, force_not_quantize=True)), VQ_TOL)
    img, idx = ctx.vq_decode(z, return_indices=True)
    idx = idx.cpu().long()
    agree = float((idx == ovq.vq_quantize(sd, z)[1]).float().mean())
    print(f"[vq attention] {what}: index agreement with the oracle arg-min {agree:.4f} (bound {INDEX_AGREEMENT})")
    assert agree >= INDEX_AGREEMENT
    zq = sd["quantize.embedding.weight"][idx].reshape(2, h, w, 3).permute(0, 3, 1, 2).contiguous()
    _within(f"{what}: quantised decode vs oracle on the library's indices", rel_l2(img, ovq.vq_decode(sd, vs, zq, force_not_quantize=True)), VQ_TOL)


def test_decoder_layer_by_layer_on_the_streaming_block(tiny):
    """Latent 64 x 72, every layer tap teacher-forced against oracle/vq_emul.py (layer 2 is the mid AttnBlock: GroupNorm, q, k, v, the
    streaming kernel, proj_out + residual) at 2 STAGE_TOL per block, the image from the library's last layer at STAGE_TOL -- the method of
    test_gpu_emul.py::test_vq_decoder_layer_by_layer_on_padded_tokens."""
    ctx, vs, sd = tiny
    h, w = 64, 72
    z = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(100 * h + w))
    free = []
    vq_decode_emulated(sd, vs, z, force_not_quantize=True, taps=free)
    lib = {}
    for i, tp in enumerate(free):
        buf = torch.empty(tuple(tp.shape), device=ctx.device, dtype=torch.bfloat16)
        ctx.debug_tap(buf, 1000 + i, 0)
        img = ctx.vq_decode(z, force_not_quantize=True)
        torch.cuda.synchronize()
        lib[i] = buf.float().cpu()
    ctx.debug_tap(None, -1)
    own = []
    emu_tf = vq_decode_emulated(sd, vs, z, force_not_quantize=True, taps=own, forced=lib)
    errs = [rel_l2(lib[i], own[i]) for i in range(len(own))]
    e_img = rel_l2(img, emu_tf)
    print(f"[vq attention] tiny vq-f4 decoder at latent {h}x{w}, {len(own)} layers teacher-forced: worst {max(errs):.3e} (layer {int(np.argmax(errs))}), "
          f"mid AttnBlock {errs[2]:.3e}; image from the library's last layer {e_img:.3e}")
    assert max(errs) <= 2 * STAGE_TOL, errs
    assert e_img <= STAGE_TOL


def test_encode_against_the_oracle(tiny):
    """a pair of 256 x 288 images: the encoder's mid AttnBlock over 64 x 72 = 4608 pixels"""
    ctx, vs, sd = tiny
    x = torch.from_numpy(np.random.default_rng(256 + 288).uniform(-1.0, 1.0, (2, 3, 256, 288)).astype(np.float32))
    z = ctx.vq_encode(x)
    assert tuple(z.shape) == (2, 3, 64, 72)
    _within("tiny VQ encode of 256x288 images vs oracle", rel_l2(z, ovq.vq_encode(sd, vs, x)), VQ_TOL)


def test_decode_walked_in_ranges(tiny, tmp_path):
    """A child process with RDM_VQ_RANGE=2 decodes 3 latents of 64 x 72 in ranges of 2 and 1: bit for bit the one-range result."""
    ctx = tiny[0]
    z = _latent(3, 64, 72, 77)
    whole, whole_idx = ctx.vq_decode(z, return_indices=True)
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
        "z = torch.from_numpy(np.random.default_rng(77).standard_normal((3, 3, 64, 72)).astype(np.float32))\n"
        "img, idx = ctx.vq_decode(z, return_indices=True)\n"
        f"np.savez({str(out)!r}, img=img.cpu().numpy(), idx=idx.cpu().numpy())\nctx.close()\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RDM_VQ_RANGE="2"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert np.array_equal(got["idx"], whole_idx.cpu().numpy())
    assert np.array_equal(got["img"], whole.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 3. the size wall
def test_decode_past_46336_latent_pixels():
    """Latent 216 x 220 = 47520 pixels: its padded score matrix would pass 2^31 elements, which the materialised chain cannot index (the
    decode used to be refused: "beyond what one pass can index"), and would take 6 n^2 = 13.5 GB.  The decode must succeed without growing the
    device's memory use by that much; the mid AttnBlock's input and output are tapped (blocks 1001 / 1002, one decode each) and 64 of its rows
    restated on the CPU in oracle/vq_emul.py's arithmetic: GroupNorm of the tapped input, k and v for all rows, q and the scores for the 64."""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, packing
    vs, sd = _tiny()
    h, w = 216, 220
    n, C = h * w, vs.ch * vs.ch_mult[-1]
    z = _latent(1, h, w, 11)
    c2 = _lib.Context(0)
    try:
        cfg = spec_to_vq_cfg(vs)
        c2.load_vq(cfg, packing.pack("vq", cfg, sd))
        taps = {}
        for blk in (1001, 1002):
            buf = torch.empty((1, n, C), device=c2.device, dtype=torch.bfloat16)
            c2.debug_tap(buf, blk, 0)
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            img = c2.vq_decode(z, force_not_quantize=True)
            torch.cuda.synchronize()
            grown = free0 - torch.cuda.mem_get_info()[0]
            if blk == 1001:
                print(f"[vq attention] decode of a {h}x{w} latent grew device memory use by {grown / 1e9:.2f} GB (the scores alone would be {6 * n * n / 1e9:.1f} GB)")
                assert grown < 6 * n * n
            taps[blk] = buf.float().cpu()
        c2.debug_tap(None, -1)
        assert tuple(img.shape) == (1, 3, 4 * h, 4 * w) and bool(torch.isfinite(img).all())
    finally:
        c2.close()
    x, y = taps[1001][0], taps[1002][0]                                       # [n, C]
    pre = "decoder.mid.attn_1"
    hn = bf(F.group_norm(x.t().reshape(1, C, n), 32, sd[pre + ".norm.weight"], sd[pre + ".norm.bias"], 1e-6))[0].t().contiguous()
    Wb = lambda nm: bf(sd[f"{pre}.{nm}.weight"].float()).reshape(C, C)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:64]
    q = bf(F.linear(hn[rows], Wb("q"), sd[pre + ".q.bias"]))
    k = bf(F.linear(hn, Wb("k"), sd[pre + ".k.bias"]))
    v = bf(F.linear(hn, Wb("v")))
    p = bf(F.softmax(q @ k.t() * (float(C) ** -0.5), dim=1))                  # 64 x 47520
    ao = bf(p @ v + sd[pre + ".v.bias"])
    ref = bf(F.linear(ao, Wb("proj_out"), sd[pre + ".proj_out.bias"]) + x[rows])
    _within(f"mid AttnBlock over {n} pixels, 64 rows restated on the CPU", rel_l2(y[rows], ref), 2 * STAGE_TOL)
    print(f"[vq attention] the attention's own share of those rows (output minus the residual, both rounded at the output's size): rel L2 {rel_l2(y[rows] - x[rows], ref - x[rows]):.3e}")
