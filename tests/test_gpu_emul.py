"""The parity window closed (verdict round 4, item 4): the library against the CPU restatement of ITS OWN arithmetic, stage by stage.

The fp32 goldens (tests/test_gpu_models.py, test_gpu_full.py) bound the library at the bf16 STORAGE distance -- 2.5e-2 per UNet forward,
measured 1.0-1.2e-2 -- wide enough to hide a mis-placed residual scale or an approximate GELU.  oracle/unet_emul.py / oracle/vq_emul.py
walk the same graph in fp32 and round to bf16 exactly where the library stores bf16 (with its re-associations done its way).

What this can and cannot bound (measured, tools/emul_probe.py):
  * ONE op on identical inputs: library and restatement agree to 1e-5 .. 8e-5 -- fp32 summation order, plus the few output roundings it flips;
  * FREE-RUNNING over many layers they decorrelate: a discrepancy d in front of a bf16 rounding comes out as ~sqrt(d ulp) behind it
    (a flip is a whole ulp; its probability is d / ulp): 1e-6 -> 6e-5 -> 5e-4 -> 1.4e-3 -> ... -> the rounding-noise floor.  After four
    blocks the two trajectories are as far from each other as each is from fp32 (1.0e-2): NO restatement short of bit-exact fp32 summation
    can hold a whole forward at 2e-3, and none is needed:
  * TEACHER-FORCED -- every stage of the restatement starts from the LIBRARY's value of the previous stage (rdm_debug_tap shows the
    executor's intermediate tensors: 25 block outputs, 5 stages per ResBlock, 10 per SpatialTransformer) -- each comparison is one op again.
    Bound: **5e-4 per stage** (measured <= 3e-4), 50 x tighter than the fp32 bound and LOCALISED: a wrong residual, bias, scale, norm
    epsilon, head split or weight slice in any of the 297 stages of the shipped UNet fails its own line.
Covered: (1) the direct forward of the shipped 400.9 M-parameter UNet, (2) the forward inside rdm_ddim_sample on a guided batch (shared
guidance prefix, zero-neighbour rows with attn2's bias folded into attn1.to_out, in-place cross-attention + norm3) and the CFG combine /
DDIM update that follows it, (3) the VQ-f4 decoder layer by layer, (4) tight op-level checks incl. the exact-erf GELU, (5) the free-running
distances with the statement above as assertions, (6) the same stage-by-stage comparison at sizes that are not the training size: the tiny UNet at
latent 36 x 40 and the tiny VQ-f4 decoder at latents 5 x 7 / 9 x 8 (the kernel paths only such sizes reach).  The emulators are pinned on the CPU: rounding off, they equal the fp32 oracle to 2e-5
(tests/test_oracle_cpu.py), and the fp32 oracle equals the reference's classes bit for bit (tools/gen_golden*.py).

Reference: rdm/modules/diffusionmodules/openaimodel.py:129 (fp32 compute), :335-371; rdm/modules/attention.py:77-196; ddim.py:217-268."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import diffusion as odiff
from oracle import unet as ounet
from oracle import vqdecoder as ovq
from oracle.unet_emul import _R, flash_attention, unet_forward_emulated
from oracle.vq_emul import vq_decode_emulated

from _util import bf16_round as bf, golden, rel_l2, spec_to_unet_cfg, spec_to_vq_cfg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

STAGE_TOL = 5e-4          # one stage on the library's own inputs (measured <= 3e-4)
OP_TOL = 2e-4             # one op on random inputs (measured <= 8e-5)


@pytest.fixture(scope="module")
def shipped(ctx):
    from rdm_amd import packing
    spec = ounet.shipped_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234)
    cfg = spec_to_unet_cfg(spec)
    ctx.load_unet(cfg, packing.pack("unet", cfg, sd))
    return ctx, spec, sd


def _library_stages(ctx, run, keys, rows_of):
    """One forward per key with the debug tap on that stage -> {key: [B, n, width] fp32 on the CPU}."""
    out = {}
    for key, shp in keys.items():
        buf = torch.empty((rows_of(key),) + tuple(shp[1:]), device=ctx.device, dtype=torch.bfloat16)
        ctx.debug_tap(buf, key[0], key[1])
        run()
        torch.cuda.synchronize()
        out[key] = buf.float().cpu()
    ctx.debug_tap(None, -1)
    return out


def _stage_name(spec, key):
    bi, sub = key
    name, layers = spec.blocks[bi]
    if sub == 0:
        return f"{name} output"
    j, st = sub // 16, sub % 16
    kind = layers[j][0]
    names = {"res": {1: "in_layers norm+SiLU", 2: "in_layers conv + emb", 3: "out_layers norm+SiLU", 4: "skip_connection", 5: "output"},
             "st": {1: "norm", 2: "proj_in", 3: "norm1", 4: "q|k|v", 5: "attn1 heads", 6: "x + attn1", 7: "x + attn2", 8: "norm3", 9: "GEGLU", 10: "output"}}
    return f"{name}.{j} ({kind}) {names[kind][st]}"


def test_unet_shipped_stage_by_stage(shipped):
    ctx, spec, sd = shipped
    g = golden("unet_shipped.npz")
    x, t, c = torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g["ctx"])
    B = x.shape[0]
    free = {}
    emu_free = unet_forward_emulated(sd, spec, x, t, c, taps=free)
    lib = _library_stages(ctx, lambda: ctx.unet_forward(x, t, c), {k: v.shape for k, v in free.items()}, lambda key: B)
    own = {}
    emu_tf = unet_forward_emulated(sd, spec, x, t, c, taps=own, forced=lib)
    eps = ctx.unet_forward(x, t, c)
    torch.cuda.synchronize()
    worst = max(((rel_l2(lib[k], own[k]), k) for k in lib), key=lambda p: p[0])
    print(f"[emul] shipped UNet, {len(lib)} stages teacher-forced: worst {worst[0]:.3e} at {_stage_name(spec, worst[1])}; eps (head on the library's last block) {rel_l2(eps, emu_tf):.3e}")
    for k in lib:
        e = rel_l2(lib[k], own[k])
        assert e <= STAGE_TOL, f"{_stage_name(spec, k)}: library vs its restatement on the library's own inputs {e:.3e}"
    assert rel_l2(eps, emu_tf) <= STAGE_TOL
    # free-running: both sit at the storage format's distance from fp32 -- the library no further than its restatement -- and from each other
    ref = torch.from_numpy(g["eps"])
    e_lib, e_emu, e_cross = rel_l2(eps, ref), rel_l2(emu_free, ref), rel_l2(eps, emu_free)
    print(f"[emul] shipped UNet free-running: library vs fp32 reference {e_lib:.3e}, restatement vs fp32 reference {e_emu:.3e}, library vs restatement {e_cross:.3e}")
    assert e_lib <= 2.5e-2 and e_emu <= 2.5e-2 and e_cross <= 2.5e-2
    assert e_lib <= 1.3 * e_emu, "the library is further from fp32 than bf16 storage at its rounding points explains"


def test_guided_sampler_forward_stage_by_stage_and_ddim_update(shipped):
    """The forward INSIDE rdm_ddim_sample (S = 1: one step at t = 1, CFG 2.0, k = 4): UNet batch [x | x], contexts [cond | 0]: the layers in
    front of the first SpatialTransformer run once on B samples (shared guidance prefix), the unconditional rows take attn2's bias in
    attn1.to_out's start values, the conditional rows the in-place cross-attention with norm3 emitted; then e = e_u + s (e_c - e_u) and the
    DDIM update (ddim.py:229-267) from the library's own pred_x0."""
    ctx, spec, sd = shipped
    gen = torch.Generator().manual_seed(77)
    B = 2
    x_T = torch.randn(B, 3, 64, 64, generator=gen)
    cond = torch.randn(B, 4, 512, generator=gen) * 0.45
    uncond = torch.zeros_like(cond)
    sched = odiff.Schedule()
    xx, tt, cc = torch.cat([x_T, x_T]), torch.full((2 * B,), 1, dtype=torch.long), torch.cat([cond, uncond])
    free = {}
    unet_forward_emulated(sd, spec, xx, tt, cc, ctx_rows=B, taps=free)
    first_st = next((bi, j) for bi, (_, ls) in enumerate(spec.blocks) for j, l in enumerate(ls) if l[0] == "st")
    in_prefix = lambda key: key[0] < first_st[0] or (key[0] == first_st[0] and key[1] != 0 and key[1] // 16 < first_st[1])
    run = lambda: ctx.ddim_sample(1, x_T, cond, uncond, sched.alphas_cumprod, eta=0.0, scale=2.0, log_every_t=1, want_intermediates=True)
    lib = _library_stages(ctx, run, {k: v.shape for k, v in free.items()}, lambda key: B if in_prefix(key) else 2 * B)
    forced = {k: (torch.cat([v, v]) if in_prefix(k) else v) for k, v in lib.items()}
    own = {}
    eps_tf = unet_forward_emulated(sd, spec, xx, tt, cc, ctx_rows=B, taps=own, forced=forced)
    worst = (0.0, None)
    for k in lib:
        for rows, what in ((slice(0, B), "conditional"), (slice(B, 2 * B), "unconditional")):
            e = rel_l2(forced[k][rows], own[k][rows])
            worst = max(worst, (e, k), key=lambda p: p[0])
            assert e <= STAGE_TOL, f"{_stage_name(spec, k)} ({what} rows): {e:.3e}"
    print(f"[emul] guided sampler forward, {len(lib)} stages x 2 halves teacher-forced: worst {worst[0]:.3e} at {_stage_name(spec, worst[1])}")
    # the step itself: CFG combine + DDIM update in fp32
    z, xi, pi = run()
    torch.cuda.synchronize()
    z, pred_x0 = z.cpu(), pi.cpu()[-1]
    sch = odiff.ddim_schedule(sched, 1, 0.0)
    a_t, a_prev, s1m = float(sch[1][0]), float(sch[2][0]), float(sch[4][0])
    e_cfg = eps_tf[B:] + 2.0 * (eps_tf[:B] - eps_tf[B:])
    want_x0 = (x_T - s1m * e_cfg) / a_t ** 0.5
    e_x0 = rel_l2(pred_x0, want_x0)
    e_lib = (x_T - a_t ** 0.5 * pred_x0) / s1m                                       # the eps the library used, from ITS pred_x0
    want_prev = a_prev ** 0.5 * pred_x0 + (1.0 - a_prev) ** 0.5 * e_lib
    e_up = rel_l2(z, want_prev)
    print(f"[emul] guided DDIM step: pred_x0 vs the restatement's (head + CFG on the library's last block) {e_x0:.3e}; update from the library's pred_x0 {e_up:.3e}")
    assert e_x0 <= STAGE_TOL and e_up <= 1e-5


def test_vq_decoder_shipped_layer_by_layer(ctx):
    """VQ-f4 decoder (no quantiser in front: a flipped near-tie code is a discrete event, covered by test_gpu_full.py's code agreement):
    every layer output -- conv_in, mid ResnetBlock / AttnBlock (4096 tokens, d = 512) / ResnetBlock, 9 ResnetBlocks, 2 Upsample convs --
    teacher-forced, then the image from the library's last layer."""
    from rdm_amd import packing
    g = golden("full_vq.npz")
    vs = ovq.shipped_vq_spec()
    sd = ounet.synth_state_dict(ovq.vq_param_shapes(vs), seed=int(g["seed"]))
    cfg = spec_to_vq_cfg(vs)
    ctx.load_vq(cfg, packing.pack("vq", cfg, sd))
    z = torch.from_numpy(g["z"])
    free = []
    emu_free = vq_decode_emulated(sd, vs, z, force_not_quantize=True, taps=free)
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
    print(f"[emul] vq-f4 decoder, {len(own)} layers teacher-forced: worst {max(errs):.3e} (layer {int(np.argmax(errs))}); image from the library's last layer {rel_l2(img, emu_tf):.3e}")
    assert max(errs) <= 2 * STAGE_TOL, errs            # (a ResnetBlock / AttnBlock is 4-6 roundings deep: two stage budgets)
    assert rel_l2(img, emu_tf) <= STAGE_TOL
    ref = ovq.vq_decode(sd, vs, z, force_not_quantize=True)
    e_lib, e_emu = rel_l2(img, ref), rel_l2(emu_free, ref)
    print(f"[emul] vq-f4 decoder free-running: library vs fp32 oracle {e_lib:.3e}, restatement vs fp32 oracle {e_emu:.3e}")
    assert e_lib <= 2.5e-2 and e_lib <= 1.3 * e_emu


def test_ops_against_their_own_arithmetic(ctx):
    """Single ops on random operands at the shipped shapes, against the restatement's formula for them: one bf16 rounding of an fp32 result.
    2e-4 is below what ANY formula change costs: tanh-GELU instead of erf 5e-4, a second rounding (e.g. of a residual sum) 2.4e-3."""
    from rdm_amd import _lib
    from rdm_amd.packing import _geglu_perm
    d = ctx.device
    g = torch.Generator().manual_seed(1)
    R = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    dev = lambda t: t.to(d, torch.bfloat16).contiguous()
    res = {}
    x = bf(R(2, 1024, 384) * 1.3 + 0.2); ga, be = 1 + 0.1 * R(384), 0.1 * R(384)
    ref = bf(F.silu(F.group_norm(x.permute(0, 2, 1).reshape(2, 384, 32, 32), 32, ga, be, 1e-5))).reshape(2, 384, 1024).permute(0, 2, 1)
    res["GroupNorm32 + SiLU"] = rel_l2(ctx.op_groupnorm(dev(x), ga.to(d), be.to(d), 1e-5, 1), ref)
    res["LayerNorm"] = rel_l2(ctx.op_layernorm(dev(x).reshape(2048, 384), ga.to(d), be.to(d)), bf(F.layer_norm(x, (384,), ga, be, 1e-5)).reshape(2048, 384))
    for M, N, K in ((49152, 384, 384), (8192, 960, 960)):
        a, w, b, r = bf(R(M, K)), bf(R(N, K, sc=K ** -0.5)), R(N, sc=0.3), bf(R(M, N))
        res[f"Linear + bias + residual {M}x{N}x{K}"] = rel_l2(ctx.op_linear(dev(a), dev(w), b.to(d), residual=dev(r)), bf(a @ w.t() + b + r))
    M, C = 32768, 384
    a, w, b = bf(R(M, C)), bf(R(8 * C, C, sc=C ** -0.5)), R(8 * C, sc=0.3)
    xg, gg = (a @ w.t() + b).chunk(2, dim=-1)
    perm = _geglu_perm(8 * C)
    out = ctx.op_linear(dev(a), dev(w[perm]), b[perm].contiguous().to(d), act=_lib.ACT_GEGLU)
    res["GEGLU (exact erf)"] = rel_l2(out, bf(xg * F.gelu(gg)))
    e_tanh = rel_l2(out, bf(xg * F.gelu(gg, approximate="tanh")))
    for B in (2, 16):                                          # fused read-out / split-K finisher
        H, C, N = 32, 384, 384
        xx, w, b, rv, r = bf(R(B, H, H, C)), bf(R(N, C, 3, 3, sc=(9 * C) ** -0.5)), R(N, sc=0.2), R(B, N, sc=0.3), bf(R(B, H, H, N))
        ref = bf(F.conv2d(xx.permute(0, 3, 1, 2), w, b, padding=1) + rv[:, :, None, None] + r.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        res[f"conv3x3 + bias + emb row + residual, batch {B}"] = rel_l2(
            ctx.op_conv3x3(dev(xx), dev(w.permute(0, 2, 3, 1)), b.to(d), rowvec=rv.to(d).contiguous(), residual=dev(r)), ref)
    B, n, heads = 2, 1024, 12; C = heads * 32
    qkv = bf(R(B, n, 3 * C))
    q, k, v = qkv.split(C, dim=-1); sp = lambda t: t.reshape(B, n, heads, 32).permute(0, 2, 1, 3)
    o = flash_attention(sp(q), sp(k), sp(v), 32 ** -0.5, _R(True))
    res["self-attention, d_head 32, 1024 tokens"] = rel_l2(ctx.op_self_attention_qkv(dev(qkv), heads), bf(o.permute(0, 2, 1, 3).reshape(B, n, C)))
    for k_, e in res.items():
        print(f"[emul] op {k_}: {e:.3e}")
    print(f"[emul] (the GEGLU output against a tanh-approximated GELU: {e_tanh:.3e})")
    assert max(res.values()) <= OP_TOL, res
    assert e_tanh > 2 * OP_TOL, "the GEGLU check would not tell erf from tanh"


# ------------------------------------------------------------------------------------------------ sizes that are not the training size
def _teacher_forced_unet(ctx, spec, sd, x, t, c):
    """-> ({stage: error}, error of eps from the library's last block): every tap of one direct forward against the restatement run on
    the library's own value of the previous stage"""
    B = x.shape[0]
    free = {}
    unet_forward_emulated(sd, spec, x, t, c, taps=free)
    lib = _library_stages(ctx, lambda: ctx.unet_forward(x, t, c), {k: v.shape for k, v in free.items()}, lambda key: B)
    own = {}
    emu_tf = unet_forward_emulated(sd, spec, x, t, c, taps=own, forced=lib)
    eps = ctx.unet_forward(x, t, c)
    torch.cuda.synchronize()
    return {k: rel_l2(lib[k], own[k]) for k in lib}, rel_l2(eps, emu_tf)


def test_unet_stage_by_stage_at_latent_36x40(ctx):
    """The tiny UNet with self-attention at every level, latent 36 x 40, B = 2 with one zero-context row, k = 4, direct forward.  Its levels:
    1440 pixels (flash_d32_kernel at n % 64 == 32, two-pass GroupNorm whose 22 chunks of 66 rows do not divide 1440, 40-wide generic convs),
    360 pixels (small self-attention with its keys in two LDS chunks, cross-attention as two skinny GEMMs), 90 pixels (small attention in
    one chunk, 10-wide convs); the 40-wide `out` conv falls to conv_out_kernel.  Every tap teacher-forced at STAGE_TOL, and eps from the
    library's last block."""
    from dataclasses import replace
    from rdm_amd import packing
    spec = replace(ounet.tiny_spec(), attention_resolutions=(1, 2, 4))
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=4321)
    cfg = spec_to_unet_cfg(spec)
    ctx.load_unet(cfg, packing.pack("unet", cfg, sd))
    g = torch.Generator().manual_seed(3640)
    x, t = torch.randn(2, 3, 36, 40, generator=g), torch.tensor([917, 12])
    c = torch.randn(2, 4, 512, generator=g) * 0.45
    c[1] = 0
    errs, e_eps = _teacher_forced_unet(ctx, spec, sd, x, t, c)
    worst = max(errs, key=errs.get)
    print(f"[emul] tiny UNet at latent 36x40, {len(errs)} stages teacher-forced: worst {errs[worst]:.3e} at {_stage_name(spec, worst)}; eps (conv_out_kernel head on the library's last block) {e_eps:.3e}")
    for k, e in errs.items():
        assert e <= STAGE_TOL, f"{_stage_name(spec, k)}: library vs its restatement on the library's own inputs {e:.3e}"
    assert e_eps <= STAGE_TOL


@pytest.mark.parametrize("h,w", [(5, 7), (9, 8)])
def test_vq_decoder_layer_by_layer_on_padded_tokens(ctx, h, w):
    """The tiny VQ-f4 decoder (force_not_quantize) at latents whose mid AttnBlock runs on padded tokens: 5 x 7 = 35 tokens in np = 64, 9 x 8 =
    72 tokens in np = 128 (two key tiles, the second mostly padding); odd widths on the generic conv, conv_in on a partial wave and the
    head on conv_out_kernel (image widths 28 / 32 x heights 20 / 36).  Every layer tap teacher-forced at 2 STAGE_TOL per block, the image
    from the library's last layer at STAGE_TOL."""
    from rdm_amd import packing
    vs = ovq.tiny_vq_spec()
    sd = ounet.synth_state_dict(ovq.vq_param_shapes(vs), seed=5)
    cfg = spec_to_vq_cfg(vs)
    ctx.load_vq(cfg, packing.pack("vq", cfg, sd))
    z = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(100 * h + w))
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
    print(f"[emul] tiny vq-f4 decoder at latent {h}x{w}, {len(own)} layers teacher-forced: worst {max(errs):.3e} (layer {int(np.argmax(errs))}); image from the library's last layer {e_img:.3e}")
    assert tuple(img.shape) == (2, 3, 4 * h, 4 * w)
    assert max(errs) <= 2 * STAGE_TOL, errs
    assert e_img <= STAGE_TOL
