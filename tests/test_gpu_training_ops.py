"""The training-path primitives (csrc/backward.hip, misc.hip, the implicit-GEMM bmm) called one by one through the C ABI and held to a
float64 CPU restatement of the same operation, element by element (tests/_train_ref.py states each bound and near miss).  Every case
also shows that its bound discriminates: the kernel output must fall outside the bound against each near-miss reference.  Kernels
whose comments promise a fixed summation order are called twice and must agree bitwise.

The two weight-gradient ops (csrc/wgrad.hip, the fallbacks of csrc/backward.hip) take their cases from tests/_wgrad_ref.py: every case names
the kernel path it is for and the test first asks the host-only selector that the path is the one the library takes; integer operands
make dW equal its reference bit for bit, one Gaussian case per path is held to the per-element chain bound."""
import ctypes

import pytest
import torch

import _train_ref as R
import _wgrad_ref as WG

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# outputs whose kernels sum in a fixed order (colsum stages, GN / LN affine partials, the small-attention block partials)
REPEATABLE = {"colsum", "colsum_samples", "layernorm_bwd", "groupnorm_bwd", "small_attention_bwd", "mse_loss"}


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
    if name in ("conv3x3_wgrad", "linear_wgrad"):
        from rdm_amd import _lib
        if name == "conv3x3_wgrad":
            B, H, W, C = inp["x"].shape
            assert _lib.wgrad_select(B, H, W, C, inp["dy"].shape[3]) == inp["form"], "the case is for another kernel path than the library takes"
            return {"dw": ctx.op_conv3x3_wgrad(b(inp["x"]), b(inp["dy"]))}
        M, K = inp["a"].shape
        assert _lib.wgrad_select(M, inp["dy"].shape[1], K) == inp["form"], "the case is for another kernel path than the library takes"
        return {"dw": ctx.op_linear_wgrad(b(inp["dy"]), b(inp["a"]))}
    if name == "adamw":
        p, g, m, v = (f(inp[k]).clone() for k in "pgmv")
        pb = torch.zeros(p.shape, device=d, dtype=BF)
        kw = dict(lr=inp["lr"], betas=inp["betas"], eps=inp["eps"], weight_decay=inp["wd"])
        if len(inp["sizes"]) == 1:
            ctx.op_adamw(p, g, m, v, inp["step"], p_bf16=pb, **kw)
        else:                                                # separate allocations, as the parameters of a model are
            parts = [[t.clone() for t in x.split(inp["sizes"])] for x in (p, g, m, v, pb)]
            ctx.op_adamw_multi(parts[0], parts[1], parts[2], parts[3], inp["step"], p_bf16s=parts[4], **kw)
            p, m, v, pb = (torch.cat(parts[i]) for i in (0, 2, 3, 4))
        return {"p": p, "m": m, "v": v, "pb": pb}
    if name == "ema":
        sh, p = f(inp["s"]).clone(), f(inp["p"])
        if len(inp["sizes"]) == 1:
            ctx.op_ema(sh, p, inp["omd"])
            return {"out": sh}
        shs, ps = [t.clone() for t in sh.split(inp["sizes"])], [t.clone() for t in p.split(inp["sizes"])]
        ctx.op_ema_multi(shs, ps, inp["omd"])
        return {"out": torch.cat(shs)}
    if name == "q_sample":
        # through the C ABI into outputs filled with 7 beforehand: the zero padding channels must be WRITTEN, not found zero
        from rdm_amd import _lib
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        x0, noise, ca, cb = f(inp["x0"]), f(inp["noise"]), f(inp["a"]), f(inp["b"])
        B, C, H, W = x0.shape
        out = torch.full_like(x0, 7.0) if inp["nchw"] else None
        nhwc = torch.full((B, H, W, inp["cpad"]), 7.0, device=d, dtype=BF) if inp["cpad"] else None
        ctx._check(_lib.lib.rdm_op_q_sample(ctx._h, P(x0), P(noise), P(ca), P(cb), P(out), P(nhwc), B, C, H, W, inp["cpad"]))
        return {k: v for k, v in (("out", out), ("nhwc", nhwc)) if v is not None}
    if name == "mse_loss":
        from rdm_amd import _lib
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        eps, target = b(inp["eps"]), f(inp["target"])
        coef = f(inp["coef"]) if inp["coef"] is not None else None
        B, H, W, ldc = eps.shape
        se = torch.full((B,), 7.0, device=d)
        deps = torch.full_like(eps, 7.0) if coef is not None else None
        ctx._check(_lib.lib.rdm_op_mse_loss(ctx._h, P(eps), P(target), P(coef), P(se), P(deps), B, target.shape[1], H, W, ldc))
        return {"se": se, "deps": deps} if deps is not None else {"se": se}
    if name == "where_rows":
        return {"out": ctx.op_where_rows(inp["mask"], f(inp["a"]), f(inp["x"]))}
    if name == "timestep_embedding":
        # through the C ABI into a buffer of one more row: the row after the last must come back as it went in
        from rdm_amd import _lib
        B, ld = inp["t"].shape[0], inp["ld"]
        buf = torch.full((B + 1, ld), 7.0, device=d, dtype=BF)
        t = inp["t"].to(d, torch.int64).contiguous()
        ctx._check(_lib.lib.rdm_op_timestep_embedding(ctx._h, ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(buf.data_ptr()), B, inp["dim"], ld))
        return {"out": buf[:B], "guard": buf[B]}
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


@pytest.mark.parametrize("entry", WG.CASES, ids=[WG.case_id(e) for e in WG.CASES])
def test_weight_gradient_matches_its_reference(ctx, entry):
    """integer cases: bitwise equal to the integer reference; Gaussian cases: worst error / bound <= 1, every near miss > 1; both: the
    selector names the case's path, and two calls agree bitwise (fixed-order planes)"""
    case, kw, path = entry
    inp = case.make(**kw)
    out = _run(ctx, case, inp)
    torch.cuda.synchronize()
    worst, margin = R.check(case, inp, {k: v.float().cpu() for k, v in out.items()})
    print(f"{path}: " + (f"bitwise equal, {margin} elements of the closest near miss differ" if case.exact
                         else f"worst error / bound {worst:.3g}, closest near miss {margin:.3g}"))
    again = _run(ctx, case, inp)
    assert torch.equal(out["dw"], again["dw"]), f"{path}: two calls differ (fixed-order planes expected)"


@pytest.mark.parametrize("first,second", WG.SCRATCH_REUSE, ids=[f"{a[0]}-z{a[1]}-then-z1" for a, _ in WG.SCRATCH_REUSE])
def test_weight_gradient_scratch_reuse(ctx, first, second):
    """a many-plane case leaves its planes in the context's scratch; a one-plane case of the same path right after it must still be exact"""
    for form in (first, second):
        case, kw, path = WG.exact_case(form)
        inp = case.make(**kw)
        out = _run(ctx, case, inp)
        torch.cuda.synchronize()
        assert torch.equal(out["dw"].cpu().double(), case.ref(inp, R.F64)["dw"]), path
