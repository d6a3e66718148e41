"""The inference forward kernels (linear / lin4 / sgemm / mgemm, the LayerNorm-folded projection, conv3x3 on every launch path, the
stem conv, GroupNorm, LayerNorm, flash and small attention, the fused cross-attention, the head conv and its VALU fallback) called through the C ABI and held to a
float64 CPU restatement of the same operation, element by element (tests/_fwd_ref.py states each bound and near miss).  Every case
also shows that its bound discriminates: the kernel output must fall outside the bound against each near-miss reference.  Kernels that
sum in a fixed order are called twice and must agree bitwise; for the batched tile geometries, changing one sample's input must leave
every other sample's output bitwise unchanged.  The three forms only the CLIP towers run -- the tiled GEMM adding an fp32 residual into
its fp32 output (called with the output aliased to the residual and apart: bitwise equal), LayerNorm fp32 -> fp32, small attention on
the column thirds of one fused q|k|v buffer -- are cases like the others."""
import os
import subprocess
import sys

import pytest
import torch

import _fwd_ref as R
from _train_ref import check

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
torch.set_num_threads(min(16, torch.get_num_threads()))

# paths whose kernels promise a fixed summation order (one-pass / two-pass GroupNorm, the K-split finisher, lin4, halo4, flash)
REPEATABLE = ("gn_", "K-split", "lin4", "halo4", "flash")


def _run(ctx, case, inp):
    from rdm_amd import _lib
    from rdm_amd.packing import _geglu_perm
    d = ctx.device
    b = lambda t: t.to(d, BF).contiguous()
    f = lambda t: t.to(d, torch.float32).contiguous()
    o = lambda t: None if t is None else f(t)
    if case is R.Linear:
        w, bias = inp["w"], inp["b"]
        if inp["act"] == R.ACT_GEGLU:
            perm = _geglu_perm(w.shape[0])
            w = w[perm]; bias = None if bias is None else bias[perm]
        if inp.get("res_f32"):      # the towers' x += proj(h): once into a fresh tensor, once over the residual itself -- bitwise the same
            sep = ctx.op_linear_res_f32(b(inp["a"]), b(w), o(bias), f(inp["res"]), act=inp["act"])
            x = f(inp["res"]).clone()
            inplace = ctx.op_linear_res_f32(b(inp["a"]), b(w), o(bias), x, act=inp["act"], inplace=True)
            assert inplace.data_ptr() == x.data_ptr() and sep.data_ptr() != x.data_ptr()
            assert torch.equal(sep, inplace), "out aliased to the residual differs from out in a buffer of its own"
            return {"out": sep}
        res = None if inp["res"] is None else b(inp["res"])
        if inp["rows"] is not None:
            return {"out": ctx.op_linear_rowvec(b(inp["a"]), b(w), o(bias), f(inp["rv"]), inp["rows"], residual=res)}
        return {"out": ctx.op_linear(b(inp["a"]), b(w), o(bias), residual=res, act=inp["act"], alpha=inp["alpha"], out_f32=inp["f32"])}
    if case is R.LinearLN:
        w, bias = inp["w"], inp["b"]
        if inp["act"] == R.ACT_GEGLU:
            perm = _geglu_perm(w.shape[0])
            w = w[perm]; bias = None if bias is None else bias[perm]
        return {"out": ctx.op_linear_ln(b(inp["x"]), b(w), o(bias), f(inp["gamma"]), f(inp["beta"]), act=inp["act"], eps=inp["eps"])}
    if case is R.Conv3x3:
        x, C0 = inp["x"], inp["C0"]
        x1 = b(x[..., C0:]) if x.shape[3] > C0 else None
        if inp["asym"]:             # the first-stage encoder's Downsample: its own entry point, exactly vqenc_body's call
            return {"out": ctx.op_conv3x3_down(b(x), b(inp["w"].permute(0, 2, 3, 1)), f(inp["b"]))}
        return {"out": ctx.op_conv3x3(b(x[..., :C0]), b(inp["w"].permute(0, 2, 3, 1)), f(inp["b"]), x1=x1, rowvec=o(inp.get("t")),
                                      residual=b(inp["res"]) if "res" in inp else None, stride=inp["stride"], ups=inp["ups"])}
    if case is R.GroupNorm:
        x, C0 = inp["x"], inp["C0"]
        x1 = b(x[..., C0:]) if x.shape[2] > C0 else None
        return {"out": ctx.op_groupnorm(b(x[..., :C0]), f(inp["gamma"]), f(inp["beta"]), inp["eps"], inp["silu"], x1)}
    if case is R.LayerNorm:
        if inp.get("out_f32"):
            return {"out": ctx.op_layernorm_f32(f(inp["x"]), f(inp["gamma"]), f(inp["beta"]), inp["eps"])}
        return {"out": ctx.op_layernorm(f(inp["x"]) if inp["f32"] else b(inp["x"]), f(inp["gamma"]), f(inp["beta"]), inp["eps"])}
    if case is R.SelfAttention:
        q, k, v = inp["q"], inp["k"], inp["v"]
        if inp["mode"] == "qkv":
            return {"out": ctx.op_self_attention_qkv(b(torch.cat([q, k, v], -1)), inp["H"])}
        return {"out": ctx.op_self_attention(b(torch.cat([q, k], -1)), b(v.transpose(1, 2)), inp["H"])}
    if case is R.SmallAttention:
        if inp.get("fused"):        # one [B, n, 3 H D] buffer; q, k, v its column thirds at the row pitch 3 H D
            W = inp["H"] * inp["D"]
            qkv = b(torch.cat([inp["q"], inp["k"], inp["v"]], -1))
            return {"out": ctx.op_small_attention(qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:], inp["H"], inp["D"], inp["causal"], inp["scale"])}
        return {"out": ctx.op_small_attention(b(inp["q"]), b(inp["k"]), b(inp["v"]), inp["H"], inp["D"], inp["causal"], inp["scale"])}
    if case is R.XattnFused:
        ln = (f(inp["gamma"]), f(inp["beta"]), inp["eps"]) if inp["ln"] else None
        res = None if inp["ln"] or inp["res"] is None else b(inp["res"])
        return {"out": ctx.op_xattn_fused(b(inp["x"]), b(inp["G"]), b(inp["U"]), o(inp["bias"]), res, inp["ncols"], inp["k"], ln=ln)}
    if case is R.HeadConv:
        gn = (f(inp["gamma"]), f(inp["beta"]), inp["eps"]) if inp["norm"] else None
        return {"out": ctx.op_head_conv(b(inp["x"]), f(inp["w"]), f(inp["bias"]), gn=gn)}
    if case is R.ConvIn:
        return {"out": ctx.op_conv_in(f(inp["x"]), f(inp["w"]), f(inp["b"]))}
    if case is R.ConvOut:
        return {"out": ctx.op_conv_out(b(inp["x"]), f(inp["w"]), f(inp["b"]))}
    raise AssertionError(case.name)


_GPU_CASES = [e for e in R.CASES if not e[1].get("mgemm")]
_MGEMM_CASES = [e for e in R.CASES if e[1].get("mgemm")]


@pytest.mark.parametrize("entry", _GPU_CASES, ids=[R.case_id(e) for e in _GPU_CASES])
def test_forward_op_matches_fp64_restatement(ctx, entry):
    case, kw, path = entry
    inp = case.make(**kw)
    out = _run(ctx, case, inp)
    torch.cuda.synchronize()
    host = {k: v.float().cpu() for k, v in out.items()}
    worst, margin = check(case, inp, host)
    print(f"{path}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    if any(tag in path for tag in REPEATABLE):
        again = _run(ctx, case, inp)
        for k in out:
            assert torch.equal(out[k], again[k]), f"{path}: two calls differ (fixed summation order expected)"


def test_linear_mgemm_matches_fp64_restatement(ctx):
    """mgemm.hip through rdm_op_linear in a child process with the RDM_MGEMM_ANY=64 test hook (plain ops of >= 64 rows take it)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})\n"
            "import torch, rdm_amd\nfrom rdm_amd import _lib\nimport _fwd_ref as R, test_gpu_forward_ops as T\nfrom _train_ref import check\n"
            "ctx = _lib.Context(0)\n"
            "for case, kw, path in T._MGEMM_CASES:\n"
            "    inp = case.make(**kw)\n"
            "    out = T._run(ctx, case, inp); torch.cuda.synchronize()\n"
            "    worst, margin = check(case, inp, {k: v.float().cpu() for k, v in out.items()})\n"
            "    print(R.case_id((case, kw, path)), path, 'worst error / bound %.3g, closest near miss %.3g' % (worst, margin))\n"
            "print('OK')\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RDM_MGEMM_ANY="64"), capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_conv3x3_down_refuses_odd_sizes_and_the_context_stays_usable(ctx):
    """rdm_op_conv3x3_down: an odd Hin or Win is an argument error and no launch (the output keeps its sentinel); the next call on the same
    context runs and is held to the bound."""
    from rdm_amd import _lib
    d = ctx.device
    g = torch.Generator().manual_seed(9)
    w, bias = torch.randn(64, 3, 3, 64, generator=g).to(d, BF), torch.randn(64, generator=g).to(d)
    for H, W in ((5, 6), (6, 5), (1, 1)):
        x = torch.randn(1, H, W, 64, generator=g).to(d, BF)
        out = torch.full((1, max(H // 2, 1), max(W // 2, 1), 64), 7.0, device=d, dtype=BF)
        rc = _lib.lib.rdm_op_conv3x3_down(ctx._h, x.data_ptr(), 64, w.data_ptr(), bias.data_ptr(), out.data_ptr(), 1, H, W, 64)
        torch.cuda.synchronize()
        assert rc != 0 and bool((out == 7.0).all()), (H, W, rc)
        with pytest.raises(_lib.RdmError, match="rdm_op_conv3x3_down"):
            ctx.op_conv3x3_down(x, w, bias)
    inp = R.Conv3x3.make(B=3, H=6, W=10, C0=64, N=64, stride=2, asym=1)
    out = _run(ctx, R.Conv3x3, inp)
    torch.cuda.synchronize()
    check(R.Conv3x3, inp, {k: v.float().cpu() for k, v in out.items()})


def test_xattn_ln3_matches_layernorm_of_its_own_rows(ctx):
    """rdm_op_xattn_fused_ln3: x <- the LN-form cross-attention in place (held to XattnFused's bound) and norm3 of the finished rows,
    held to LayerNorm's bound against a LayerNorm of the kernel's OWN bf16 rows (the statistics are taken on the rounded values)."""
    d = ctx.device
    inp = R.XattnFused.make(B=2, n=96, heads=6, k=4, ln=True, seed=7)
    g = torch.Generator().manual_seed(8)
    C = inp["x"].shape[2]
    g3, b3 = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    x = inp["x"].to(d, BF).contiguous()
    l3 = ctx.op_xattn_fused_ln3(x, inp["G"].to(d, BF).contiguous(), inp["U"].to(d, BF).contiguous(), inp["bias"].to(d),
                                inp["ncols"], inp["k"], ln=(inp["gamma"].to(d), inp["beta"].to(d), inp["eps"]), ln3=(g3.to(d), b3.to(d)))
    torch.cuda.synchronize()
    worst, margin = check(R.XattnFused, inp, {"out": x.float().cpu()})
    print(f"xattn_ln_fused_kernel (in place): worst {worst:.3g}, closest near miss {margin:.3g}")
    rows = x.float().cpu().reshape(-1, C)
    li = R.LayerNorm.make(rows.shape[0], C, x=rows, gamma=g3, beta=b3)
    worst, margin = check(R.LayerNorm, li, {"out": l3.float().cpu().reshape(-1, C)})
    print(f"xattn_ln_fused_kernel norm3: worst {worst:.3g}, closest near miss {margin:.3g}")


# batch independence: a tile holding several samples (8x8 halo4: four per tile), the strip kernel, GroupNorm's XCD-grouped block
# order (B = 8) and flash: a change to sample 1's input leaves every other sample's output bitwise unchanged
_INDEP = [(R.Conv3x3, dict(B=4, H=8, W=8, C0=128, N=192), "x"), (R.Conv3x3, dict(B=2, H=8, W=128, C0=64, N=128), "x"),
          (R.GroupNorm, dict(B=8, HW=1024, C0=384, silu=1), "x"), (R.SelfAttention, dict(B=3, n=128, H=2), "q")]


@pytest.mark.parametrize("case,kw,key", _INDEP, ids=["halo4-8x8-four-samples", "halo4-strip", "gn_onepass-B8", "flash"])
def test_other_samples_unchanged_when_one_sample_changes(ctx, case, kw, key):
    inp = case.make(**kw)
    out = _run(ctx, case, inp)["out"]
    t = inp[key].clone()
    t[1] = R.bfr(torch.randn(t[1].shape, generator=torch.Generator().manual_seed(5)) + 0.5)
    inp[key] = t
    out2 = _run(ctx, case, inp)["out"]
    keep = [i for i in range(out.shape[0]) if i != 1]
    assert not torch.equal(out[1], out2[1])
    assert torch.equal(out[keep], out2[keep]), f"{case.name}: another sample's output changed"
