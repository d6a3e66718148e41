"""GPU parity of the backward building blocks against torch autograd on the fp32 restatement of the same
ops (bf16-rounded operands): 3x3 conv dgrad / wgrad, GroupNorm(+SiLU) and LayerNorm backward, and a whole ResBlock
(rdm_amd/training.py) -- with and without the 1x1 skip projection -- through the C ABI.  Stated tolerance: 3e-2 relative L2 per
gradient (bf16 activation gradients between the stages, fp32 accumulation)."""
import pytest
import torch
import torch.nn.functional as F
import torch.nn.functional as F_

from _util import bf16_round, rel_l2

pytestmark = pytest.mark.gpu
TOL = 3e-2


@pytest.fixture(autouse=True)
def _autograd_on():
    # other test modules switch autograd off process-wide at import (collection imports them all): the references here need it
    with torch.enable_grad():
        yield


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("B,H,W,C,N", [(2, 64, 64, 192, 384), (3, 8, 32, 224, 96), (5, 16, 8, 64, 576), (3, 32, 32, 128, 64), (5, 16, 16, 64, 128),
                                       (2, 8, 64, 64, 64), (4, 16, 16, 576, 576), (1, 2, 16, 64, 64), (9, 4, 32, 192, 64), (8, 2, 16, 64, 64)])
def test_conv3x3_wgrad_tn(ctx, B, H, W, C, N):
    """The transpose-free wgrad kernels (csrc/wgrad.hip): the nine-tap kernel at widths 64 / 32 / 16 (row ring across sample boundaries:
    blocks spanning several samples in the 576-channel case, two-row images at (8, 2, 16, 64, 64), odd sample counts) and the per-tap
    kernel (widths that are not multiples of 64 channels, 8-pixel rows, partial 192-wide tiles, ragged row counts) -- against the fp32
    autograd of the same bf16 operands.  (1, 2, 16, 64, 64) has 32 pixels: below the kernels' floor of 256 it runs the transposed-copy
    fallback of csrc/backward.hip, not the nine-tap kernel.  Which path a shape takes, and the per-element checks of every path:
    tests/_wgrad_ref.py and test_gpu_training_ops.py."""
    d = ctx.device
    x = bf16_round(_rand((B, H, W, C), 11))
    w = torch.zeros((N, C, 3, 3), requires_grad=True)
    dy = bf16_round(_rand((B, H, W, N), 13))
    F.conv2d(x.permute(0, 3, 1, 2), w, None, padding=1).permute(0, 2, 3, 1).backward(dy)
    dw = ctx.op_conv3x3_wgrad(x.to(d, torch.bfloat16), dy.to(d, torch.bfloat16))
    e = rel_l2(dw, w.grad.permute(0, 2, 3, 1))
    print(f"conv wgrad B={B} {H}x{W} {C}->{N}: rel L2 {e:.2e}")
    assert e <= 1e-5          # exact bf16 products, fp32 sums in another order
    assert torch.equal(dw, ctx.op_conv3x3_wgrad(x.to(d, torch.bfloat16), dy.to(d, torch.bfloat16)))     # fixed-order planes: bitwise repeatable


@pytest.mark.parametrize("M,N,K", [(1000, 320, 96), (4096, 384, 1152), (300, 64, 512), (65536, 384, 384)])
def test_linear_wgrad_tn(ctx, M, N, K):
    d = ctx.device
    a, dy = bf16_round(_rand((M, K), 21)), bf16_round(_rand((M, N), 22))
    dw = ctx.op_linear_wgrad(dy.to(d, torch.bfloat16), a.to(d, torch.bfloat16))
    ref = dy.double().t() @ a.double()
    e = rel_l2(dw.double(), ref)
    print(f"linear wgrad M={M} {K}->{N}: rel L2 {e:.2e}")
    assert e <= 1e-5
    assert torch.equal(dw, ctx.op_linear_wgrad(dy.to(d, torch.bfloat16), a.to(d, torch.bfloat16)))


@pytest.mark.parametrize("B,H,C,N", [(2, 16, 64, 128), (3, 8, 128, 64), (1, 32, 64, 64), (4, 16, 192, 192)])
def test_conv3x3_dgrad_wgrad(ctx, B, H, C, N):
    d = ctx.device
    x = bf16_round(_rand((B, H, H, C), 1)).requires_grad_(True)
    w = bf16_round(_rand((N, C, 3, 3), 2, (9 * C) ** -0.5)).requires_grad_(True)
    dy = bf16_round(_rand((B, H, H, N), 3))
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, padding=1).permute(0, 2, 3, 1)
    y.backward(dy)
    wp = w.detach().permute(0, 2, 3, 1).contiguous().to(d, torch.bfloat16)
    dx = ctx.op_conv3x3_dgrad(dy.to(d, torch.bfloat16), wp)
    dw = ctx.op_conv3x3_wgrad(x.detach().to(d, torch.bfloat16), dy.to(d, torch.bfloat16))
    e_dx, e_dw = rel_l2(dx.float(), x.grad), rel_l2(dw, w.grad.permute(0, 2, 3, 1))
    print(f"conv B={B} {H}x{H} {C}->{N}: dgrad rel L2 {e_dx:.2e}, wgrad {e_dw:.2e}")
    assert e_dx <= TOL and e_dw <= 5e-3            # wgrad: fp32 output of exact bf16 products


@pytest.mark.parametrize("B,HW,C,silu", [(2, 64, 64, 1), (3, 256, 192, 1), (2, 1024, 96, 0)])
def test_groupnorm_backward(ctx, B, HW, C, silu):
    d = ctx.device
    x = bf16_round(_rand((B, HW, C), 4) * 1.5 + 0.3).requires_grad_(True)
    g = (1 + 0.1 * _rand((C,), 5)).requires_grad_(True); b = (0.1 * _rand((C,), 6)).requires_grad_(True)
    dy = bf16_round(_rand((B, HW, C), 7))
    y = F.group_norm(x.permute(0, 2, 1), 32, g, b, 1e-5).permute(0, 2, 1)
    if silu:
        y = F.silu(y)
    y.backward(dy)
    dx, dg, db = ctx.op_groupnorm_bwd(x.detach().to(d, torch.bfloat16), dy.to(d, torch.bfloat16), g.detach().to(d), b.detach().to(d), 1e-5, silu)
    e = (rel_l2(dx.float(), x.grad), rel_l2(dg, g.grad), rel_l2(db, b.grad))
    print(f"groupnorm bwd B={B} HW={HW} C={C} silu={silu}: dx {e[0]:.2e} dgamma {e[1]:.2e} dbeta {e[2]:.2e}")
    assert max(e) <= TOL


@pytest.mark.parametrize("M,C", [(100, 384), (513, 960), (7, 128)])
def test_layernorm_backward(ctx, M, C):
    d = ctx.device
    x = bf16_round(_rand((M, C), 8) * 1.5 + 0.3).requires_grad_(True)
    g = (1 + 0.1 * _rand((C,), 9)).requires_grad_(True); b = (0.1 * _rand((C,), 10)).requires_grad_(True)
    dy = bf16_round(_rand((M, C), 11))
    F.layer_norm(x, (C,), g, b, 1e-5).backward(dy)
    dx, dg, db = ctx.op_layernorm_bwd(x.detach().to(d, torch.bfloat16), dy.to(d, torch.bfloat16), g.detach().to(d))
    e = (rel_l2(dx.float(), x.grad), rel_l2(dg, g.grad), rel_l2(db, b.grad))
    print(f"layernorm bwd M={M} C={C}: dx {e[0]:.2e} dgamma {e[1]:.2e} dbeta {e[2]:.2e}")
    assert max(e) <= TOL


@pytest.mark.parametrize("Cin,Cout", [(64, 64), (128, 64)])
def test_resblock_backward_matches_autograd(ctx, Cin, Cout):
    """ldm ResBlock forward + backward on the native path vs torch autograd: gradients w.r.t. every parameter,
    the input and the (SiLU'd) time embedding."""
    from rdm_amd import training
    d = ctx.device
    B, H, E = 2, 16, 256
    f = {"gn1_g": 1 + 0.1 * _rand((Cin,), 20), "gn1_b": 0.1 * _rand((Cin,), 21), "gn2_g": 1 + 0.1 * _rand((Cout,), 22), "gn2_b": 0.1 * _rand((Cout,), 23),
         "w1": bf16_round(_rand((Cout, Cin, 3, 3), 24, (9 * Cin) ** -0.5)), "b1": 0.1 * _rand((Cout,), 25),
         "w2": bf16_round(_rand((Cout, Cout, 3, 3), 26, (9 * Cout) ** -0.5)), "b2": 0.1 * _rand((Cout,), 27),
         "emb_w": bf16_round(_rand((Cout, E), 28, E ** -0.5)), "emb_b": 0.1 * _rand((Cout,), 29)}
    if Cin != Cout:
        f["skip_w"] = bf16_round(_rand((Cout, Cin), 30, Cin ** -0.5)); f["skip_b"] = 0.1 * _rand((Cout,), 31)
    x = bf16_round(_rand((B, H, H, Cin), 32)); semb = bf16_round(F.silu(_rand((B, E), 33))); dout = bf16_round(_rand((B, H, H, Cout), 34))
    # fp32 autograd reference
    r = {k: v.clone().requires_grad_(True) for k, v in f.items()}
    xr, sr = x.clone().requires_grad_(True), semb.clone().requires_grad_(True)
    xc = xr.permute(0, 3, 1, 2)
    h = F.conv2d(F.silu(F.group_norm(xc, 32, r["gn1_g"], r["gn1_b"], 1e-5)), r["w1"], r["b1"], padding=1)
    h = h + F.linear(sr, r["emb_w"], r["emb_b"])[:, :, None, None]
    h = F.conv2d(F.silu(F.group_norm(h, 32, r["gn2_g"], r["gn2_b"], 1e-5)), r["w2"], r["b2"], padding=1)
    skip = F.conv2d(xc, r["skip_w"][:, :, None, None], r["skip_b"]) if Cin != Cout else xc
    out_ref = (skip + h).permute(0, 2, 3, 1)
    out_ref.backward(dout)
    # native
    p = {k: (v.permute(0, 2, 3, 1).contiguous().to(d, torch.bfloat16) if k in ("w1", "w2") else v.to(d, torch.bfloat16) if k in ("emb_w", "skip_w") else v.to(d))
         for k, v in f.items()}
    xd, sd, dd = x.to(d, torch.bfloat16), semb.to(d, torch.bfloat16), dout.to(d, torch.bfloat16)
    out, saved = training.resblock_forward(ctx, p, xd, sd)
    assert rel_l2(out.float(), out_ref.detach()) <= 1.5e-2
    g = training.resblock_backward(ctx, p, xd, sd, saved, dd)
    torch.cuda.synchronize()
    errs = {"dx": rel_l2(g["dx"].float(), xr.grad), "dsemb": rel_l2(g["dsemb"].float(), sr.grad)}
    for k in f:
        ref = r[k].grad.permute(0, 2, 3, 1) if k in ("w1", "w2") else r[k].grad
        errs[k] = rel_l2(g[k].float(), ref)
    print("resblock backward rel L2:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("M,F", [(300, 256), (64, 1536)])
def test_geglu_forward_backward(ctx, M, F):
    d = ctx.device
    pre = bf16_round(_rand((M, 2 * F), 40) * 1.5).requires_grad_(True)
    dh = bf16_round(_rand((M, F), 41))
    a, g = pre.chunk(2, dim=-1)
    h = a * F_.gelu(g)
    h.backward(dh)
    out = ctx.op_geglu(pre.detach().to(d, torch.bfloat16))
    dpre = ctx.op_geglu(pre.detach().to(d, torch.bfloat16), dh.to(d, torch.bfloat16))
    e = (rel_l2(out.float(), h.detach()), rel_l2(dpre.float(), pre.grad))
    print(f"geglu M={M} F={F}: forward {e[0]:.2e} backward {e[1]:.2e}")
    assert max(e) <= 1e-2


@pytest.mark.parametrize("M,C", [(512, 128), (192, 384)])
def test_feed_forward_block_backward(ctx, M, C):
    """x + ff(norm3(x)) of BasicTransformerBlock (GEGLU feed-forward, inner width 4 C): forward and every gradient vs autograd."""
    from rdm_amd import training
    d = ctx.device
    Fh = 4 * C
    x = bf16_round(_rand((M, C), 50)).requires_grad_(True)
    prm = {"ln_g": 1 + 0.1 * _rand((C,), 51), "ln_b": 0.1 * _rand((C,), 52), "w1": bf16_round(_rand((2 * Fh, C), 53, C ** -0.5)), "b1": 0.1 * _rand((2 * Fh,), 54),
           "w2": bf16_round(_rand((C, Fh), 55, Fh ** -0.5)), "b2": 0.1 * _rand((C,), 56)}
    ref_p = {k: v.clone().requires_grad_(True) for k, v in prm.items()}
    dout = bf16_round(_rand((M, C), 57))
    ln = F_.layer_norm(x, (C,), ref_p["ln_g"], ref_p["ln_b"], 1e-5)
    a, g = (ln @ ref_p["w1"].t() + ref_p["b1"]).chunk(2, dim=-1)
    out_ref = x + (a * F_.gelu(g)) @ ref_p["w2"].t() + ref_p["b2"]
    out_ref.backward(dout)
    dev = {k: (v.to(d, torch.bfloat16) if k in ("w1", "w2") else v.to(d)) for k, v in prm.items()}
    xd = x.detach().to(d, torch.bfloat16)
    out, saved = training.ff_forward(ctx, dev, xd)
    grads = training.ff_backward(ctx, dev, xd, saved, dout.to(d, torch.bfloat16))
    errs = {"out": rel_l2(out.float(), out_ref.detach()), "x": rel_l2(grads["x"].float(), x.grad)}
    for k in ("w1", "b1", "w2", "b2", "ln_g", "ln_b"):
        errs[k] = rel_l2(grads[k].float(), ref_p[k].grad)
    print(f"feed-forward block M={M} C={C}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL


@pytest.mark.parametrize("B,n,m,heads,d", [(2, 256, 256, 6, 32), (3, 64, 64, 4, 32), (2, 128, 64, 2, 64), (3, 1024, 4, 12, 32), (2, 300, 20, 6, 32), (2, 64, 32, 3, 32)])
def test_attention_forward_backward(ctx, B, n, m, heads, d):
    """softmax(q k^T / sqrt(d)) v per head (ldm CrossAttention core, self- and cross-shaped): output and dq / dk / dv vs autograd."""
    from rdm_amd import training
    dev = ctx.device
    C = heads * d
    q = bf16_round(_rand((B, n, C), 60)).requires_grad_(True)
    k = bf16_round(_rand((B, m, C), 61)).requires_grad_(True)
    v = bf16_round(_rand((B, m, C), 62)).requires_grad_(True)
    dout = bf16_round(_rand((B, n, C), 63))
    sp = lambda t, L: t.reshape(B, L, heads, d).permute(0, 2, 1, 3)
    att = (sp(q, n) @ sp(k, m).transpose(-1, -2) * d ** -0.5).softmax(-1)
    ref = (att @ sp(v, m)).permute(0, 2, 1, 3).reshape(B, n, C)
    ref.backward(dout)
    qd, kd, vd = (t.detach().to(dev, torch.bfloat16) for t in (q, k, v))
    out, saved = training.attention_forward(ctx, qd, kd, vd, heads)
    g = training.attention_backward(ctx, qd, kd, vd, heads, saved, dout.to(dev, torch.bfloat16))
    errs = {"out": rel_l2(out.float(), ref.detach()), "q": rel_l2(g["q"].float(), q.grad), "k": rel_l2(g["k"].float(), k.grad), "v": rel_l2(g["v"].float(), v.grad)}
    print(f"attention B={B} n={n} m={m} heads={heads} d={d}: " + " ".join(f"{kk} {vv:.2e}" for kk, vv in errs.items()))
    assert max(errs.values()) <= TOL


def test_basic_transformer_block_backward(ctx):
    """A whole BasicTransformerBlock (self-attention, cross-attention over k = 4 conditioning rows of width 512, GEGLU feed-forward; each
    with its LayerNorm and residual) forward + backward against torch autograd: output, dx, dcontext and every parameter gradient."""
    from rdm_amd import training
    dev = ctx.device
    B, n, C, heads, m, Cc = 2, 256, 192, 6, 4, 512
    Fh = 4 * C
    x = bf16_round(_rand((B, n, C), 70)).requires_grad_(True)
    cx = bf16_round(_rand((B, m, Cc), 71)).requires_grad_(True)
    def attn_params(seed, kc):
        return {"ln_g": 1 + 0.1 * _rand((C,), seed), "ln_b": 0.1 * _rand((C,), seed + 1), "wq": bf16_round(_rand((C, C), seed + 2, C ** -0.5)),
                "wk": bf16_round(_rand((C, kc), seed + 3, kc ** -0.5)), "wv": bf16_round(_rand((C, kc), seed + 4, kc ** -0.5)),
                "wo": bf16_round(_rand((C, C), seed + 5, C ** -0.5)), "bo": 0.1 * _rand((C,), seed + 6)}
    prm = {"attn1": attn_params(80, C), "attn2": attn_params(90, Cc),
           "ff": {"ln_g": 1 + 0.1 * _rand((C,), 100), "ln_b": 0.1 * _rand((C,), 101), "w1": bf16_round(_rand((2 * Fh, C), 102, C ** -0.5)), "b1": 0.1 * _rand((2 * Fh,), 103),
                  "w2": bf16_round(_rand((C, Fh), 104, Fh ** -0.5)), "b2": 0.1 * _rand((C,), 105)}}
    ref = {blk: {k: v.clone().requires_grad_(True) for k, v in d_.items()} for blk, d_ in prm.items()}
    dout = bf16_round(_rand((B, n, C), 110))
    def attn_ref(pp, xx, c):
        ln = F_.layer_norm(xx, (C,), pp["ln_g"], pp["ln_b"], 1e-5)
        c = ln if c is None else c
        sp = lambda t: t.reshape(t.shape[0], t.shape[1], heads, C // heads).permute(0, 2, 1, 3)
        q, k, v = sp(ln @ pp["wq"].t()), sp(c @ pp["wk"].t()), sp(c @ pp["wv"].t())
        a = (q @ k.transpose(-1, -2) * (C // heads) ** -0.5).softmax(-1) @ v
        return xx + a.permute(0, 2, 1, 3).reshape(xx.shape) @ pp["wo"].t() + pp["bo"]
    x1 = attn_ref(ref["attn1"], x, None)
    x2 = attn_ref(ref["attn2"], x1, cx)
    a, g = (F_.layer_norm(x2, (C,), ref["ff"]["ln_g"], ref["ff"]["ln_b"], 1e-5) @ ref["ff"]["w1"].t() + ref["ff"]["b1"]).chunk(2, dim=-1)
    out_ref = x2 + (a * F_.gelu(g)) @ ref["ff"]["w2"].t() + ref["ff"]["b2"]
    out_ref.backward(dout)
    to_dev = lambda d_: {k: (v.to(dev, torch.bfloat16) if k.startswith("w") else v.to(dev)) for k, v in d_.items()}
    dp = {blk: to_dev(d_) for blk, d_ in prm.items()}
    dp["attn1"]["heads"] = dp["attn2"]["heads"] = heads
    xd, cd = x.detach().to(dev, torch.bfloat16), cx.detach().to(dev, torch.bfloat16)
    out, saved = training.transformer_block_forward(ctx, dp, xd, cd)
    grads = training.transformer_block_backward(ctx, dp, xd, cd, saved, dout.to(dev, torch.bfloat16))
    errs = {"out": rel_l2(out.float(), out_ref.detach()), "x": rel_l2(grads["x"].float(), x.grad), "context": rel_l2(grads["context"].float(), cx.grad)}
    for blk in ("attn1", "attn2", "ff"):
        for k in prm[blk]:
            errs[f"{blk}.{k}"] = rel_l2(grads[blk][k].float(), ref[blk][k].grad)
    worst = max(errs, key=errs.get)
    print("transformer block: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert errs[worst] <= TOL, (worst, errs[worst])


def test_adamw_step_matches_torch(ctx):
    d = ctx.device
    n = 100003
    p0, g1, g2 = _rand((n,), 120), _rand((n,), 121, 0.1), _rand((n,), 122, 0.1)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    p, m, v = p0.clone().to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    pb = torch.empty(n, device=d, dtype=torch.bfloat16)
    for step, g in enumerate((g1, g2), start=1):
        ref.grad = g.clone(); opt.step()
        ctx.op_adamw(p, g.to(d), m, v, step, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05, p_bf16=pb)
    assert (p.cpu() - ref.detach()).abs().max().item() <= 2e-6
    assert torch.equal(pb.cpu(), p.cpu().to(torch.bfloat16))


def test_adamw_and_ema_over_tensor_lists(ctx):
    """rdm_op_adamw_multi / rdm_op_ema_multi: 120 tensors of 1 .. 300 k elements (three launches' worth, ragged last blocks, a tensor
    without a bf16 copy) give bit for bit what the per-tensor entries give."""
    d = ctx.device
    sizes = [1, 7, 2048, 2049, 300001] + [int(3 + 37 * i ** 1.7) for i in range(115)]
    mk = lambda seed, sc=1.0: [(_rand((n,), seed + i) * sc).to(d) for i, n in enumerate(sizes)]
    p1, g, m1, v1 = mk(1000), mk(2000, 0.1), [t.abs() * 0.01 for t in mk(3000)], [t.abs() * 0.01 for t in mk(4000)]
    p2, m2, v2 = [t.clone() for t in p1], [t.clone() for t in m1], [t.clone() for t in v1]
    b1 = [None if i == 3 else torch.empty_like(t, dtype=torch.bfloat16) for i, t in enumerate(p1)]
    b2 = [None if b is None else torch.empty_like(b) for b in b1]
    for step in (1, 2):
        for i in range(len(sizes)):
            ctx.op_adamw(p1[i], g[i], m1[i], v1[i], step, lr=2e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.03, p_bf16=b1[i])
        ctx.op_adamw_multi(p2, g, m2, v2, step, lr=2e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.03, p_bf16s=b2)
    for a, b in zip(p1 + m1 + v1 + [x for x in b1 if x is not None], p2 + m2 + v2 + [x for x in b2 if x is not None]):
        assert torch.equal(a, b)
    s1 = mk(5000); s2 = [t.clone() for t in s1]
    for i in range(len(sizes)):
        ctx.op_ema(s1[i], p1[i], 0.25)
    ctx.op_ema_multi(s2, p2, 0.25)
    assert all(torch.equal(a, b) for a, b in zip(s1, s2))


def _st_params(C, heads, Cc, seed):
    Fh = 4 * C
    def attn(sd, kc):
        return {"ln_g": 1 + 0.1 * _rand((C,), sd), "ln_b": 0.1 * _rand((C,), sd + 1), "wq": bf16_round(_rand((C, C), sd + 2, C ** -0.5)),
                "wk": bf16_round(_rand((C, kc), sd + 3, kc ** -0.5)), "wv": bf16_round(_rand((C, kc), sd + 4, kc ** -0.5)),
                "wo": bf16_round(_rand((C, C), sd + 5, C ** -0.5)), "bo": 0.1 * _rand((C,), sd + 6)}
    return {"gn_g": 1 + 0.1 * _rand((C,), seed), "gn_b": 0.1 * _rand((C,), seed + 1), "win": bf16_round(_rand((C, C), seed + 2, C ** -0.5)), "bin": 0.1 * _rand((C,), seed + 3),
            "wout": bf16_round(_rand((C, C), seed + 4, C ** -0.5)), "bout": 0.1 * _rand((C,), seed + 5),
            "block": {"attn1": attn(seed + 10, C), "attn2": attn(seed + 20, Cc),
                      "ff": {"ln_g": 1 + 0.1 * _rand((C,), seed + 30), "ln_b": 0.1 * _rand((C,), seed + 31), "w1": bf16_round(_rand((2 * Fh, C), seed + 32, C ** -0.5)),
                             "b1": 0.1 * _rand((2 * Fh,), seed + 33), "w2": bf16_round(_rand((C, Fh), seed + 34, Fh ** -0.5)), "b2": 0.1 * _rand((C,), seed + 35)}}}


def _torch_net(P, x, semb, cx, heads):
    """fp32 torch restatement of ResBlock -> SpatialTransformer on NHWC tensors (P: nested dict of requires_grad tensors)."""
    r, s = P["res"], P["st"]
    B, H, W, C = x.shape
    # (contiguous NCHW copies: torch's CPU group_norm / conv2d backward crashed on the permuted views)
    gn = lambda t, g, b, eps: F_.group_norm(t.permute(0, 3, 1, 2).contiguous(), 32, g, b, eps).permute(0, 2, 3, 1)
    conv = lambda t, w, b: F_.conv2d(t.permute(0, 3, 1, 2).contiguous(), w.permute(0, 3, 1, 2).contiguous(), b, padding=1).permute(0, 2, 3, 1)
    h = conv(F_.silu(gn(x, r["gn1_g"], r["gn1_b"], 1e-5)), r["w1"], r["b1"]) + (semb @ r["emb_w"].t() + r["emb_b"])[:, None, None, :]
    h = x + conv(F_.silu(gn(h, r["gn2_g"], r["gn2_b"], 1e-5)), r["w2"], r["b2"])
    t = gn(h, s["gn_g"], s["gn_b"], 1e-6).reshape(B, H * W, C) @ s["win"].t() + s["bin"]
    def attn(pp, xx, c):
        ln = F_.layer_norm(xx, (C,), pp["ln_g"], pp["ln_b"], 1e-5)
        c = ln if c is None else c
        sp = lambda u: u.reshape(u.shape[0], u.shape[1], heads, C // heads).permute(0, 2, 1, 3)
        a = (sp(ln @ pp["wq"].t()) @ sp(c @ pp["wk"].t()).transpose(-1, -2) * (C // heads) ** -0.5).softmax(-1) @ sp(c @ pp["wv"].t())
        return xx + a.permute(0, 2, 1, 3).reshape(xx.shape) @ pp["wo"].t() + pp["bo"]
    b = s["block"]
    t = attn(b["attn2"], attn(b["attn1"], t, None), cx)
    a, g = (F_.layer_norm(t, (C,), b["ff"]["ln_g"], b["ff"]["ln_b"], 1e-5) @ b["ff"]["w1"].t() + b["ff"]["b1"]).chunk(2, dim=-1)
    t = t + (a * F_.gelu(g)) @ b["ff"]["w2"].t() + b["ff"]["b2"]
    return h + (t @ s["wout"].t() + s["bout"]).reshape(B, H, W, C)


def test_training_step_resblock_plus_spatial_transformer(ctx):
    """Forward, MSE loss, backward through ResBlock -> SpatialTransformer and an AdamW step, all on the native ops: the gradients of the
    first step against autograd, then three steps of both optimisers side by side (loss values and final weights)."""
    from rdm_amd import training
    dev = ctx.device
    B, H, C, heads, m, Cc, E = 2, 16, 192, 6, 4, 512, 256
    res = {"gn1_g": 1 + 0.1 * _rand((C,), 130), "gn1_b": 0.1 * _rand((C,), 131), "gn2_g": 1 + 0.1 * _rand((C,), 132), "gn2_b": 0.1 * _rand((C,), 133),
           "w1": bf16_round(_rand((C, 3, 3, C), 134, (9 * C) ** -0.5)), "b1": 0.1 * _rand((C,), 135), "w2": bf16_round(_rand((C, 3, 3, C), 136, (9 * C) ** -0.5)),
           "b2": 0.1 * _rand((C,), 137), "emb_w": bf16_round(_rand((C, E), 138, E ** -0.5)), "emb_b": 0.1 * _rand((C,), 139)}
    master0 = {"res": res, "st": _st_params(C, heads, Cc, 150)}
    x, semb, cx = bf16_round(_rand((B, H, H, C), 200)), bf16_round(_rand((B, E), 201)), bf16_round(_rand((B, m, Cc), 202))
    target = bf16_round(_rand((B, H, H, C), 203))
    # torch side
    clone = lambda p: {k: (clone(v) if isinstance(v, dict) else v.clone().requires_grad_(True)) for k, v in p.items()}
    P = clone(master0)
    flatP = training.flatten_params(P)
    opt = torch.optim.AdamW(list(flatP.values()), lr=3e-4, weight_decay=1e-2)
    # native side
    to_dev = lambda p: {k: (to_dev(v) if isinstance(v, dict) else v.to(dev)) for k, v in p.items()}
    master = to_dev(master0)
    master["st"]["block"]["attn1"]["heads"] = master["st"]["block"]["attn2"]["heads"] = heads
    flatM = training.flatten_params(master)
    state = {"m": {k: torch.zeros_like(v) for k, v in flatM.items()}, "v": {k: torch.zeros_like(v) for k, v in flatM.items()}}
    xd, sd, cd, td = (t.to(dev, torch.bfloat16) for t in (x, semb, cx, target))
    losses = []
    for step in (1, 2, 3):
        opt.zero_grad()
        loss_ref = ((_torch_net(P, x, semb, cx, heads) - target) ** 2).mean()
        loss_ref.backward()
        loss, grads = training.training_step_demo(ctx, master, state, xd, sd, cd, td, step, lr=3e-4, weight_decay=1e-2)
        if step == 1:
            errs = {k: rel_l2(grads[k].float().reshape(v.shape), v.grad) for k, v in flatP.items()}
            worst = max(errs, key=errs.get)
            print(f"training step: loss {loss:.5f} vs {loss_ref.item():.5f}; worst gradient {worst} {errs[worst]:.2e} of {len(errs)}")
            assert errs[worst] <= TOL and abs(loss - loss_ref.item()) <= 2e-2 * loss_ref.item()
        opt.step()
        losses.append((loss, loss_ref.item()))
    # the two optimisers walk the same path: the loss after every step agrees, and moves in the same direction
    assert all(abs(a - b) <= 3e-2 * b for a, b in losses), losses
    assert (losses[2][0] < losses[0][0]) == (losses[2][1] < losses[0][1]), losses
    # after three steps the weights moved by ~3 lr per element; both optimisers must have moved them the same way
    drift = {k: rel_l2(flatM[k].float().cpu() - training.flatten_params(master0)[k], flatP[k].detach() - training.flatten_params(master0)[k]) for k in flatP}
    worst = max(drift, key=drift.get)
    print(f"training step: losses {losses}; worst update mismatch {worst} {drift[worst]:.2e}")
    assert drift[worst] <= 0.2           # sign flips of near-zero gradient elements under bf16 activations; the bulk moves identically


def test_whole_unet_loss_gradients(ctx):
    """The whole UNet (tiny topology twin of the shipped one: conv stem, ResBlocks, SpatialTransformers at two resolutions, Downsample,
    Upsample, skip concatenations, time-embedding MLP, GroupNorm + SiLU + conv head) in training form on the native ops: the MSE loss of
    ldm p_losses and its gradient w.r.t. EVERY parameter against torch autograd through the oracle's restatement of the same network."""
    from oracle import unet as ounet
    from rdm_amd import training_unet as TU
    dev = ctx.device
    spec = ounet.tiny_spec()
    sd = {k: bf16_round(v) if v.dim() >= 2 else v for k, v in ounet.synth_state_dict(ounet.param_shapes(spec), seed=7).items()}
    B, H = 2, 32
    x = bf16_round(_rand((B, 3, H, H), 300))
    cx = bf16_round(_rand((B, 4, 512), 301, 0.5))
    noise = bf16_round(_rand((B, 3, H, H), 302))
    tsteps = torch.tensor([37, 911])
    ref_sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    loss_ref = ((ounet.unet_forward(ref_sd, spec, x, tsteps, cx) - noise) ** 2).mean()
    loss_ref.backward()
    P = TU.params_from_state_dict(sd, dev)
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev, torch.bfloat16)
    loss, grads, _ = TU.unet_loss_and_grads(ctx, P, spec, to_nhwc(x), tsteps.to(dev), cx.to(dev, torch.bfloat16), to_nhwc(noise))
    g = TU.grads_to_state_dict_layout({k: v.cpu() for k, v in grads.items()}, sd)
    missing = sorted(set(sd) - set(g))
    assert not missing, missing
    errs = {k: rel_l2(g[k], ref_sd[k].grad) for k in sd}
    worst = sorted(errs, key=errs.get)[-3:]
    print(f"whole UNet: loss {loss:.5f} vs {loss_ref.item():.5f}; {len(errs)} parameter gradients, worst " + ", ".join(f"{k} {errs[k]:.2e}" for k in worst))
    assert abs(loss - loss_ref.item()) <= 2e-2 * loss_ref.item()
    assert errs[worst[-1]] <= 5e-2       # ~60 bf16 layers deep on both passes


def test_whole_unet_training_steps_track_torch(ctx):
    """Three AdamW steps of the whole (tiny-topology) UNet on the native ops beside torch.optim.AdamW on the oracle network: same loss
    curve (the ldm p_losses MSE on a fixed batch)."""
    from oracle import unet as ounet
    from rdm_amd import training_unet as TU
    dev = ctx.device
    spec = ounet.tiny_spec()
    sd = {k: bf16_round(v) if v.dim() >= 2 else v for k, v in ounet.synth_state_dict(ounet.param_shapes(spec), seed=11).items()}
    B, H = 2, 32
    x, cx, noise = bf16_round(_rand((B, 3, H, H), 310)), bf16_round(_rand((B, 4, 512), 311, 0.5)), bf16_round(_rand((B, 3, H, H), 312))
    tsteps = torch.tensor([120, 640])
    ref_sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.AdamW(list(ref_sd.values()), lr=2e-4, weight_decay=1e-2)
    P = TU.params_from_state_dict(sd, dev)
    state = {"m": {k: torch.zeros_like(v) for k, v in P.items()}, "v": {k: torch.zeros_like(v) for k, v in P.items()}}
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev, torch.bfloat16)
    xd, nd, cd, td = to_nhwc(x), to_nhwc(noise), cx.to(dev, torch.bfloat16), tsteps.to(dev)
    curve = []
    for step in (1, 2, 3):
        opt.zero_grad()
        loss_ref = ((ounet.unet_forward(ref_sd, spec, x, tsteps, cx) - noise) ** 2).mean()
        loss_ref.backward(); opt.step()
        curve.append((TU.unet_training_step(ctx, P, state, spec, xd, td, cd, nd, step, lr=2e-4, weight_decay=1e-2), loss_ref.item()))
    print(f"whole UNet training: loss curve native vs torch {[(round(a, 4), round(b, 4)) for a, b in curve]}")
    assert all(abs(a - b) <= 3e-2 * b for a, b in curve), curve
    assert curve[2][1] < curve[0][1] and curve[2][0] < curve[0][0], curve


def test_ema_matches_litema_formula(ctx):
    from rdm_amd import training_unet as TU
    d = ctx.device
    P = {"a": _rand((1000,), 400).to(d), "b": _rand((33, 7), 401).to(d)}
    ema = TU.Ema(P, decay=0.9999)
    ref = {k: v.clone().cpu() for k, v in P.items()}
    for n in range(1, 4):
        for k in P: P[k] += 0.1 * n
        ema.update(ctx, P)
        decay = min(0.9999, (1 + n) / (10 + n))
        for k in ref: ref[k] -= (1 - decay) * (ref[k] - P[k].cpu())
    for k in ref:
        assert (ema.shadow[k].cpu() - ref[k]).abs().max().item() <= 1e-6


def test_fused_and_unfused_attention_backward_agree(ctx):
    """The fused d_head = 32 backward (no score matrix) against the materialised-score path on the same inputs, n = 1024."""
    from rdm_amd import training
    dev = ctx.device
    B, n, heads = 2, 1024, 12
    C = heads * 32
    q, k, v, dout = (bf16_round(_rand((B, n, C), 500 + i)).to(dev, torch.bfloat16) for i in range(4))
    out, saved = training.attention_forward(ctx, q, k, v, heads)          # flash forward
    fused = training.attention_backward(ctx, q, k, v, heads, saved, dout)
    training._UNFUSED_ATTENTION_BWD = True
    try:
        out_p, saved_p = training.attention_forward(ctx, q, k, v, heads)  # materialised scores
        plain = training.attention_backward(ctx, q, k, v, heads, saved_p, dout)
    finally:
        training._UNFUSED_ATTENTION_BWD = False
    assert "p" not in saved and "p" in saved_p and rel_l2(out.float(), out_p.float()) <= 6e-3
    for key in ("q", "k", "v"):
        e = rel_l2(fused[key].float(), plain[key].float())
        print(f"fused vs unfused d{key}: {e:.2e}")
        assert e <= 6e-3
