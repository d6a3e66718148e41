"""The shared guidance prefix through the first transformer's self-attention (csrc/unet_exec.hip, unet_body): in a guided sampler forward
the UNet batch is [x | x] with contexts [cond | uncond], and the first SpatialTransformer's norm, proj_in, norm1, q|k|v projection and
self-attention see the same rows in both halves, so they run once on the first half; attn1.to_out then runs on the whole batch and reads
its operand and its residual with a row wrap (lin4's a0_wrap_rows + res_wrap_rows) or, where lin4 does not take the shape, from copies.

rdm_debug_guidance_prefix(ctx, 0) gives the earlier prefix, which ends in front of that transformer.  Every row's arithmetic is the same in
both, and the shared stages choose their kernels as for the whole batch (LinearOp::choice_rows), so the two must agree BIT FOR BIT: on the
step's outputs, on every tap of the first transformer and on its block's output.  A tap that differs names the stage whose kernel is not
batch-position-invariant.

Shapes (shipped UNet, first transformer at 32 x 32: C = 384, 1024 tokens; one DDIM step, scale 2.0, k = 4):
  * guided B = 2: M = 4096 rows = 32 lin4 tiles of 128 x 384, fewer than lin4's 128-tile minimum: attn1.to_out runs on the generic GEMM and
    the COPY form (ao and t0 duplicated into full-size buffers) is what runs;
  * guided B = 8: the UNet batch is 16, M = 16384 = 128 tiles, the wrap 8192 rows = 64 whole tiles: the smallest batch at which the
    WRAPPED lin4 form runs.  (Which GEMM kernel ran is not visible from here.  lin4_supported takes exactly these parameters, the generic
    GEMM refuses a wrapped operand with an error, which would fail the step, and a kernel trace of this case shows every 384-wide GEMM of
    the 32 x 32 level on lin4_kernel<false, 1, false>: proj_in on 64 tiles, q|k|v on 192, attn1.to_out on 128.)
"""
import csv

import pytest
import torch

from oracle import diffusion as odiff
from oracle import unet as ounet

from _util import spec_to_unet_cfg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

K = 4
SENTINEL = 0x7F7F          # a bf16 bit pattern (3.4e38) no activation takes: rows a tap did not write keep it


@pytest.fixture(scope="module")
def shipped(ctx):
    from rdm_amd import packing
    spec = ounet.shipped_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234)
    cfg = spec_to_unet_cfg(spec)
    ctx.load_unet(cfg, packing.pack("unet", cfg, sd))
    yield ctx, spec
    ctx.debug_guidance_prefix(1)
    ctx.debug_tap(None, -1)
    ctx.prof_enable(())


def _first_transformer(spec):
    """-> (block index, layer index in the block, channels) of the first SpatialTransformer; it runs at 32 x 32 = 1024 tokens"""
    return next((bi, j, l[1]) for bi, (_, ls) in enumerate(spec.blocks) for j, l in enumerate(ls) if l[0] == "st")


def _inputs(B, zero_uncond=True):
    gen = torch.Generator().manual_seed(1000 + B)
    x_T = torch.randn(B, 3, 64, 64, generator=gen)
    cond = torch.randn(B, K, 512, generator=gen) * 0.45
    uncond = torch.zeros_like(cond) if zero_uncond else 0.1 * torch.randn(B, K, 512, generator=gen)
    return x_T, cond, uncond


def _step(ctx, inp):
    x_T, cond, uncond = inp
    z, _, pred = ctx.ddim_sample(1, x_T, cond, uncond, odiff.Schedule().alphas_cumprod, eta=0.0, scale=2.0, log_every_t=1, want_intermediates=True)
    torch.cuda.synchronize()
    return z.cpu(), pred.cpu()


def _tap_widths(C):
    return {1: C, 2: C, 3: C, 4: 3 * C, 5: C, 6: C, 7: C, 8: C, 9: 4 * C, 10: C}


def _run_mode(ctx, spec, inp, mode):
    """-> (z, pred_x0, {tap name: raw bf16 bits of the [2B, 1024, width] tensor}) of one guided DDIM step with the prefix in `mode`."""
    B = inp[0].shape[0]
    bi, j, C = _first_transformer(spec)
    n = 1024
    ctx.debug_guidance_prefix(mode)
    taps = {}
    try:
        for name, sub, width in [(f"stage {s}", 16 * j + s, w) for s, w in _tap_widths(C).items()] + [("block output", 0, C)]:
            buf = torch.full((2 * B, n, width), SENTINEL, dtype=torch.int16, device=ctx.device).view(torch.bfloat16)
            ctx.debug_tap(buf, bi, sub)
            _step(ctx, inp)
            taps[name] = buf.view(torch.int16).cpu()
        ctx.debug_tap(None, -1)
        z, pred = _step(ctx, inp)
    finally:
        ctx.debug_tap(None, -1)
        ctx.debug_guidance_prefix(1)
    return z, pred, taps


@pytest.mark.parametrize("B", [2, 8], ids=["B2-copy-form", "B8-wrapped-form"])
def test_prefix_through_attn1_is_bitwise_the_short_prefix(shipped, B):
    ctx, spec = shipped
    assert _first_transformer(spec)[2] == 384          # the tile counts in the module docstring are for C = 384
    inp = _inputs(B)
    z0, p0, t0 = _run_mode(ctx, spec, inp, 0)
    z1, p1, t1 = _run_mode(ctx, spec, inp, 1)
    for name in t0:
        assert not (t0[name] == SENTINEL).all(dim=-1).any(), f"{name}: the short prefix's tap left rows unwritten"
        same = torch.equal(t0[name], t1[name])
        if not same:
            halves = [torch.equal(t0[name][h * B:(h + 1) * B], t1[name][h * B:(h + 1) * B]) for h in (0, 1)]
            bad = (t0[name] != t1[name]).sum().item()
            print(f"[prefix] B={B} {name}: {bad} of {t0[name].numel()} elements differ; conditional half equal {halves[0]}, unconditional half equal {halves[1]}")
        assert same, f"guided B={B}, first transformer {name}: prefix through attn1 differs from the short prefix"
    assert torch.equal(z0, z1) and torch.equal(p0, p1), f"guided B={B}: z / pred_x0 differ between the two prefixes"


def _prof_rows(ctx, inp, mode, path):
    from rdm_amd import _lib
    ctx.debug_guidance_prefix(mode)
    try:
        ctx.prof_enable((_lib.PROF_LINEAR, _lib.PROF_ATTENTION))
        ctx.prof_reset()
        _step(ctx, inp)
        ctx.prof_dump(str(path))
    finally:
        ctx.prof_enable(())
        ctx.prof_reset()
        ctx.debug_guidance_prefix(1)
    return list(csv.DictReader(open(path)))


def test_the_shared_stages_run_on_half_the_rows(shipped, tmp_path):
    """Guided B = 8 (UNet batch 16, 16384 rows at 32 x 32): the first transformer's q|k|v GEMM covers 8192 rows and its self-attention 8 samples
    with the prefix through attn1, 16384 / 16 with the short prefix; attn1.to_out covers all 16384 rows in both."""
    from rdm_amd import _lib
    ctx, _ = shipped
    inp = _inputs(8)
    want = {1: (8192, 8, 16384), 0: (16384, 16, 16384)}
    for mode, (qkv_rows, attn_b, to_out_rows) in want.items():
        rows = _prof_rows(ctx, inp, mode, tmp_path / f"prof{mode}.csv")
        first = lambda kind, tag: next(r for r in rows if int(r["kind"]) == kind and r["tag"] == tag)
        qkv = first(_lib.PROF_LINEAR, "st.norm1+qkv")
        assert (int(qkv["d0"]), int(qkv["d1"]), int(qkv["d2"])) == (qkv_rows, 1152, 384), (mode, qkv)
        att = first(_lib.PROF_ATTENTION, "st.self_attention")
        assert (int(att["d0"]), int(att["d1"]), int(att["d2"])) == (attn_b, 1024, 384), (mode, att)
        to_out = first(_lib.PROF_LINEAR, "st.attn1.to_out")
        assert (int(to_out["d0"]), int(to_out["d1"]), int(to_out["d2"])) == (to_out_rows, 384, 384), (mode, to_out)
        # the later transformers are outside the prefix in both modes: full batch
        later = [r for r in rows if int(r["kind"]) == _lib.PROF_LINEAR and r["tag"] == "st.norm1+qkv"][1]
        assert int(later["d0"]) == 16384, (mode, later)


def test_unshared_context_takes_the_same_path(shipped):
    """A guided call whose unconditional context is not all-zero (no bias fold, cross-attention on every row): both prefixes give the same z."""
    ctx, _ = shipped
    inp = _inputs(2, zero_uncond=False)
    out = {}
    for mode in (0, 1):
        ctx.debug_guidance_prefix(mode)
        try:
            out[mode] = _step(ctx, inp)
        finally:
            ctx.debug_guidance_prefix(1)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_half_batch_tap_is_bounded_by_the_buffer(shipped):
    """A stage that ran on the first half is shown as the logical tensor, both copies bounded by the tap buffer: a buffer of 3 of the 4
    samples' rows receives samples 0, 1 and sample 0 again, and nothing behind it is written."""
    ctx, spec = shipped
    B, n = 2, 1024
    bi, j, C = _first_transformer(spec)
    inp = _inputs(B)
    full = torch.full((2 * B, n, C), SENTINEL, dtype=torch.int16, device=ctx.device).view(torch.bfloat16)
    part = torch.full((2 * B, n, C), SENTINEL, dtype=torch.int16, device=ctx.device).view(torch.bfloat16)
    try:
        ctx.debug_tap(full, bi, 16 * j + 1)
        _step(ctx, inp)
        ctx.debug_tap(part[:3], bi, 16 * j + 1)
        _step(ctx, inp)
    finally:
        ctx.debug_tap(None, -1)
    full, part = full.view(torch.int16).cpu(), part.view(torch.int16).cpu()
    assert torch.equal(full[:B], full[B:]) and not (full == SENTINEL).all(dim=-1).any()
    assert torch.equal(part[:3], full[:3]) and (part[3] == SENTINEL).all()
