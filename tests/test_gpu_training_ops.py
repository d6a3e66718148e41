"""The training-path primitives (csrc/backward.hip, misc.hip, the implicit-GEMM bmm) called one by one through the C ABI and held to a
float64 CPU restatement of the same operation, element by element (tests/_train_ref.py states each bound and near miss).  Every case
also shows that its bound discriminates: the kernel output must fall outside the bound against each near-miss reference.  Kernels
whose comments promise a fixed summation order are called twice and must agree bitwise."""
import ctypes

import pytest
import torch

import _train_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# outputs whose kernels sum in a fixed order (colsum stages, GN / LN affine partials, the small-attention block partials)
REPEATABLE = {"colsum", "colsum_samples", "layernorm_bwd", "groupnorm_bwd", "small_attention_bwd"}


def _run(ctx, case, inp):
    d = ctx.device
    b = lambda t: t.to(d, BF).contiguous()
    f = lambda t: t.to(d, torch.float32).contiguous()
    name = case.name
    if name == "add":
        return {"out": ctx.op_add(b(inp["a"]), b(inp["b"]))}
    if name == "silu":
        return {"out": ctx.op_silu(f(inp["x"]), f(inp["dy"]) if inp["grad"] else None)}
    if name == "sumpool2":
        return {"out": ctx.op_sumpool2(b(inp["x"]))}
    if name == "colsum":
        return {"out": ctx.op_colsum(b(inp["x"]))}
    if name == "colsum_samples":
        return {"out": ctx.op_colsum_samples(b(inp["x"]))}
    if name == "transpose":
        x = b(inp["x"])
        return {"out": ctx.op_transpose_batched(x) if x.ndim == 3 else ctx.op_transpose(x)}
    if name == "heads":
        return {"out": ctx.op_heads(b(inp["x"]), inp["H"], inp["D"], inp["mode"])}
    if name == "expand2":
        return {"out": ctx.op_expand2(b(inp["x"]), inp["mode"])}
    if name == "bmm":
        return {"out": ctx.op_bmm(b(inp["a"]), b(inp["w"]), alpha=inp["alpha"], out_f32=inp["f32"])}
    if name == "softmax":
        return {"out": ctx.op_softmax(f(inp["s"]), n_valid=inp["n_valid"])}
    if name == "softmax_bwd":
        return {"out": ctx.op_softmax_bwd(b(inp["p"]), f(inp["dp"]))}
    if name == "geglu":
        return {"out": ctx.op_geglu(b(inp["pre"]), b(inp["dh"]) if inp["bwd"] else None)}
    if name == "layernorm_bwd":
        dx, dg, db = ctx.op_layernorm_bwd(b(inp["x"]), b(inp["dy"]), f(inp["gamma"]), inp["eps"], residual=b(inp["res"]) if "res" in inp else None)
        return {"dx": dx, "dgamma": dg, "dbeta": db}
    if name == "groupnorm_bwd":
        dx, dg, db = ctx.op_groupnorm_bwd(b(inp["x"]), b(inp["dy"]), f(inp["gamma"]), f(inp["beta"]), inp["eps"], inp["silu"],
                                          residual=b(inp["res"]) if "res" in inp else None)
        return {"dx": dx, "dgamma": dg, "dbeta": db}
    if name == "conv3x3_dgrad":
        return {"out": ctx.op_conv3x3_dgrad(b(inp["dy"]), b(inp["w"]))}
    if name == "attention_bwd":
        dq, dk, dv = ctx.op_attention_bwd(b(inp["q"]), b(inp["k"]), b(inp["v"]), b(inp["o"]), b(inp["do"]), inp["H"])
        return {"dq": dq, "dk": dk, "dv": dv}
    if name == "small_attention_bwd":
        # row pitches larger than C go straight to the C ABI (the wrapper passes contiguous rows)
        from rdm_amd import _lib
        q, kv, do = b(inp["q"]), b(inp["kv"]), b(inp["do"])
        B, nq, ldq = q.shape; nkv = kv.shape[1]; H = inp["H"]; C = 32 * H
        ldkv = kv.shape[2] // 2
        dq = torch.empty((B, nq, C), device=d, dtype=BF); dk = torch.empty((B, nkv, C), device=d, dtype=BF); dv = torch.empty_like(dk)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        ctx._check(_lib.lib.rdm_op_small_attention_bwd(ctx._h, P(q), ldq, P(kv), ctypes.c_void_p(kv.data_ptr() + 2 * ldkv), ldkv * 2, P(do),
                                                       do.shape[2], B, nq, nkv, H, float(inp["scale"]), P(dq), P(dk), P(dv)))
        return {"dq": dq, "dk": dk, "dv": dv}
    raise AssertionError(name)


@pytest.mark.parametrize("entry", R.CASES, ids=[R.case_id(e) for e in R.CASES])
def test_training_op_matches_fp64_restatement(ctx, entry):
    case, kw, path = entry
    inp = case.make(**kw)
    out = _run(ctx, case, inp)
    torch.cuda.synchronize()
    host = {k: v.float().cpu() for k, v in out.items()}
    worst, margin = R.check(case, inp, host)
    print(f"{path}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    if case.name in REPEATABLE:
        again = _run(ctx, case, inp)
        for k in out:
            assert torch.equal(out[k], again[k]), f"{case.name}.{k}: two calls differ (fixed summation order expected)"
