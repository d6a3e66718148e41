"""CPU check of the training-op references (tests/_train_ref.py) that tests/test_gpu_training_ops.py holds the HIP kernels to: an fp32
torch restatement of each op stands in for the kernel.  It must pass every per-element bound and fall outside the bound against every
near miss -- so the bounds are wide enough for honest fp32 arithmetic and narrow enough to catch the bugs the near misses encode."""
import math

import pytest
import torch

import torch.nn.functional as F

import _train_ref as R
import _wgrad_ref as WG

# the largest shapes exist for the GPU launch geometry; on the CPU their smaller siblings carry the same checks
_CPU_CASES = [e for e in R.CASES if not (e[0] is R.Colsum and e[1]["M"] > 1_000_000)]


@pytest.mark.parametrize("entry", _CPU_CASES, ids=[R.case_id(e) for e in _CPU_CASES])
def test_fp32_restatement_within_bound_and_near_misses_outside(entry):
    case, kw, path = entry
    inp = case.make(**kw)
    worst, margin = R.check(case, inp, R.standin(case, inp))
    print(f"{path}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def test_every_primitive_is_parametrised():
    names = {e[0].name for e in R.CASES}
    assert names == {"add", "silu", "sumpool2", "colsum", "colsum_samples", "transpose", "heads", "expand2", "bmm", "softmax", "softmax_bwd",
                     "geglu", "layernorm_bwd", "groupnorm_bwd", "conv3x3_dgrad", "attention_bwd", "small_attention_bwd", "adamw", "ema", "q_sample",
                     "mse_loss", "where_rows", "timestep_embedding"}
    assert {e[0].name for e in WG.CASES} == {"conv3x3_wgrad", "linear_wgrad"}


def test_colsum_geometry_reaches_both_chunk_clamps():
    assert R.colsum_chunk(1000, 64) == 64 and R.colsum_chunk(4_300_000, 8) == 4096
    assert R.colsum_chunk(100, 64) is None and R.colsum_chunk(1000, 36) is None
    assert 64 < R.colsum_chunk(300_000, 320) < 4096


def test_one_pass_layernorm_statistics_fall_outside_the_bound():
    """The defect the LayerNorm backward had: E[x^2] - mean^2 in fp32 on rows whose mean is 60-100x their spread.  An fp32 emulation of
    it (the kernel's lane-strided partial sums) must fail the dgamma bound on the offset-row case."""
    inp = R.LayerNormBwd.make(M=8, C=320, offset=True)
    x = inp["x"]
    M, C = x.shape
    lanes = x.reshape(M, C // 64, 64)                    # element c goes to lane c % 64
    s = lanes.sum(1).sum(1, keepdim=True); ss = (lanes * lanes).sum(1).sum(1, keepdim=True)
    mean = s / C
    rstd = torch.rsqrt(torch.clamp(ss / C - mean * mean, min=0) + inp["eps"])
    xh = (x - mean) * rstd
    out = R.standin(R.LayerNormBwd, inp)
    out["dgamma"] = (inp["dy"] * xh).sum(0)
    with pytest.raises(AssertionError, match="dgamma"):
        R.check(R.LayerNormBwd, inp, out)


# ---------------------------------------------------------------------------------------------- weight gradients (tests/_wgrad_ref.py)
def _shape(kw):
    return tuple(kw[k] for k in (("B", "H", "W", "C", "N") if "B" in kw else ("M", "N", "K")))


@pytest.mark.parametrize("entry", WG.CASES, ids=[WG.case_id(e) for e in WG.CASES])
def test_weight_gradient_reference_and_near_misses(entry):
    """the reference agrees with torch autograd of the same operands; integer cases stay below 2^24 and are exact in fp32 in any order; the
    fp32 stand-in passes the check, every near miss fails it -- and differs from the exact answer where the bug it encodes would show"""
    case, kw, path = entry
    inp = case.make(**kw)
    ref = case.ref(inp, R.F64)["dw"]
    with torch.enable_grad():
        if case.name == "conv3x3_wgrad":
            w = torch.zeros((kw["N"], kw["C"], 3, 3), dtype=R.F64, requires_grad=True)
            F.conv2d(inp["x"].double().permute(0, 3, 1, 2), w, None, padding=1).permute(0, 2, 3, 1).backward(inp["dy"].double())
            auto = w.grad.permute(0, 2, 3, 1)
        else:
            w = torch.zeros((kw["N"], kw["K"]), dtype=R.F64, requires_grad=True)
            F.linear(inp["a"].double(), w).backward(inp["dy"].double())
            auto = w.grad
    terms = case.terms(inp)
    if kw["exact"]:
        assert torch.equal(ref, auto)
        assert float(terms.max()) < 2 ** 24, "a partial sum could leave the integers fp32 holds exactly"
        assert torch.equal(ref, ref.round()) and kw["chain"] is None
    else:
        assert float(((ref - auto).abs() / terms).max()) < 1e-14
        assert kw["chain"] == WG.chain_of(kw["form"])
    worst, margin = R.check(case, inp, R.standin(case, inp, lambda *a: False))
    where = {}
    for label, m in case.misses(inp):
        diff = (m["dw"] != ref)
        assert diff.any(), label
        where[label] = diff
    if case.name == "conv3x3_wgrad":
        taps = lambda d: {(ky, kx) for ky in range(3) for kx in range(3) if d[:, ky, kx].any()}
        assert taps(where["corner pixel of tap (0, 0) dropped"]) == {(0, 0)}
        if kw["B"] >= 2:
            assert taps(where["next sample's first row let in at the bottom edge"]) == {(2, 0), (2, 1), (2, 2)}
        assert taps(where["taps transposed"]) == {(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)}
        assert len(taps(where["last chunk dropped"])) >= 4
        assert ("one Z plane skipped" in where) == (kw["form"][1] >= 2)
        if kw["form"][1] >= 2:
            assert len(taps(where["one Z plane skipped"])) == 9
            # the planes partition the pixels: every pixel in exactly one
            cover = sum(case.plane_mask(inp, z).long() for z in range(kw["form"][1]))
            assert torch.equal(cover, torch.ones_like(cover)), path
    else:
        assert ("one Z plane skipped" in where) == (kw["form"][1] >= 2) and ("last chunk dropped" in where) == (kw["M"] > 1)
    print(f"{path}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def test_every_weight_gradient_case_reaches_the_path_it_names():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    for case, kw, path in WG.CASES:
        assert _lib.wgrad_select(*_shape(kw)) == kw["form"], (path, _lib.wgrad_select(*_shape(kw)))
    for fa, fb in WG.SCRATCH_REUSE:
        assert WG.exact_case(fa)[1]["form"] == fa and WG.exact_case(fb)[1]["form"] == fb
        assert fa[0] == fb[0] and fb[1] == 1 and (fa[1] >= 8 or fa[0] == "linear_fallback" and fa[1] > 1)
    with pytest.raises(_lib.RdmError):
        _lib.wgrad_select(1, 2, 3, 4)
    with pytest.raises(_lib.RdmError):
        _lib.wgrad_select(2, 8, 8, 63, 64)                # the op refuses odd C
    with pytest.raises(_lib.RdmError):
        _lib.wgrad_select(0, 64, 64)


# every conv3x3 (C, N) of the shipped UNet (model_channels 192, mult 1 2 3 5) and of the tiny one (64, mult 1 2 3), stem and head padded to 64
_SHIPPED = [(64, 192), (192, 192), (192, 384), (384, 384), (384, 576), (576, 576), (576, 960), (960, 960), (1920, 960), (1536, 960), (1536, 576),
            (1152, 576), (960, 576), (960, 384), (768, 384), (576, 384), (576, 192), (384, 192), (192, 64)]
_TINY = [(64, 64), (64, 128), (128, 128), (128, 192), (192, 192), (384, 192), (320, 192), (320, 128), (256, 128), (192, 128), (192, 64), (128, 64)]


def test_every_answer_of_the_weight_gradient_selector_has_a_case():
    """H, W in 2 .. 64, B in 1 .. 9, the conv channel pairs of both configs; linear: M in 1 .. 5000 at a few (N, K).  Every distinct
    (path, Z = 1 / 2-7 / >= 8, remap form) must be named by a GPU case."""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    seen = {}
    for C, N in sorted(set(_SHIPPED + _TINY)):
        for H in range(2, 65):
            for W in range(2, 65):
                for B in range(1, 10):
                    seen.setdefault(WG.answer_class(_lib.wgrad_select(B, H, W, C, N)), (B, H, W, C, N))
    for N, K in ((192, 768), (768, 192), (384, 384), (64, 64), (1536, 384), (320, 96), (34, 64)):
        for M in range(1, 5001):
            seen.setdefault(WG.answer_class(_lib.wgrad_select(M, N, K)), (M, N, K))
    cased = {WG.answer_class(kw["form"]) for _, kw, _ in WG.CASES if kw["exact"]}
    unnamed = {k: v for k, v in seen.items() if k not in cased}
    assert not unnamed, f"selector answers without an exact GPU case (first shape reaching each): {unnamed}"
    assert {k[0] for k in seen} == {"conv9<4>", "conv9<5>", "conv9<6>", "tn9", "tn1", "conv_fallback", "linear_fallback"}
    # and one Gaussian case per path
    assert {kw["form"][0] for _, kw, _ in WG.CASES if not kw["exact"]} == {k[0] for k in seen}


def test_adamw_bound_tells_fp32_bias_corrections_from_exact_ones():
    """The defect the optimizer had: 1 - beta and 1 - beta^step taken in fp32 from fp32 betas.  An emulation of that kernel falls outside
    the m and v bounds at step 1 (v by the 1.3e-5 that 1 - 0.999f is short of 1e-3); its p stays inside, because v and bc2 are short by
    the same factor there."""
    inp = R.AdamW.make(sizes=(2049,), step=1, betas=(0.9, 0.999), wd=1e-2)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    b1, b2, lr, eps, wd = f32(0.9), f32(0.999), f32(1e-3), f32(1e-8), f32(1e-2)
    p, g, m, v = (inp[k] for k in "pgmv")
    m1 = (b1.double() * m.double() + ((1 - b1) * g).double()).float()
    v1 = (b2.double() * v.double() + ((1 - b2) * g * g).double()).float()
    bc1, bc2 = 1 - b1, 1 - b2                               # step 1
    assert abs(float(bc2) / 1e-3 - 1) > 1.2e-5
    p1 = p * (1 - lr * wd) - (lr / bc1) * m1 / (v1.sqrt() / bc2.sqrt() + eps)
    ref = R.AdamW.ref(inp, R.F64)
    a_m, a_v, a_p, _ = R.AdamW.bound_terms(inp, False)
    assert R.ratio(m1, ref["m"], a_m) > 1 and R.ratio(v1, ref["v"], a_v) > 40 and R.ratio(p1, ref["p"], a_p) <= 1
    # the explicit term: with fp32 corrections it would be most of the p bound at this step
    _, _, a_p32, part = R.AdamW.bound_terms(inp, True)
    assert float((part / a_p32).max()) > 0.9 and R.bc_rel_error(0.999, 1, True) > 2.9e-5


# ---------------------------------------------------------------------- the optimizer / loss-side references against torch's own operations
def _independent(case, inp):
    """the same quantity from torch's own implementation in fp64 (not from the case's formula)"""
    D = R.F64
    if case is R.AdamW:
        p = torch.nn.Parameter(inp["p"].double())
        p.grad = inp["g"].double()
        opt = torch.optim.AdamW([p], lr=inp["lr"], betas=inp["betas"], eps=inp["eps"], weight_decay=inp["wd"], amsgrad=False, foreach=False)
        st = opt.state[p]
        st["step"] = torch.tensor(float(inp["step"] - 1))
        st["exp_avg"], st["exp_avg_sq"] = inp["m"].double().clone(), inp["v"].double().clone()
        opt.step()
        return {"p": p.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"], "pb": p.detach()}
    if case is R.Ema:
        return {"out": torch.lerp(inp["s"].double(), inp["p"].double(), inp["omd"])}
    if case is R.QSample:
        v = torch.einsum("b,bchw->bchw", inp["a"].double(), inp["x0"].double()) + torch.einsum("b,bchw->bchw", inp["b"].double(), inp["noise"].double())
        out = {"out": v} if inp["nchw"] else {}
        if inp["cpad"]:
            out["nhwc"] = F.pad(v.permute(0, 2, 3, 1), (0, inp["cpad"] - v.shape[1]))
        return out
    if case is R.MseLoss:
        B, C, H, W = inp["target"].shape
        with torch.enable_grad():
            eps = inp["eps"].double().requires_grad_(True)
            se = F.mse_loss(eps[..., :C].permute(0, 3, 1, 2), inp["target"].double(), reduction="none").mean((1, 2, 3))
            if inp["coef"] is None:
                return {"se": se.detach()}
            # deps = coef[b] (eps - target) is the gradient of sum_b coef[b] (C H W / 2) se[b]
            (se * inp["coef"].double() * (C * H * W / 2)).sum().backward()
        return {"se": se.detach(), "deps": eps.grad}
    if case is R.WhereRows:
        out = inp["x"].double().clone()
        out[inp["mask"]] = inp["a"].double()[inp["mask"]]
        return {"out": out}
    if case is R.TimestepEmbedding:                          # ldm.modules.diffusionmodules.util.timestep_embedding, in fp64, zero-padded to ld
        half = inp["dim"] // 2
        freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=D) / half)
        args = inp["t"][:, None].double() * freqs[None]
        emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
        return {"out": F.pad(emb, (0, inp["ld"] - 2 * half)), "guard": torch.full((inp["ld"],), 7.0, dtype=D)}
    raise AssertionError(case.name)


_GLUE = [e for e in R.CASES if e[0] in (R.AdamW, R.Ema, R.QSample, R.MseLoss, R.WhereRows, R.TimestepEmbedding)]


@pytest.mark.parametrize("entry", _GLUE, ids=[R.case_id(e) for e in _GLUE])
def test_reference_agrees_with_torch(entry):
    """torch.optim.AdamW stepped in fp64 from the preset state, lerp, F.mse_loss and its autograd, masked assignment, ldm's embedding
    formula: each must give what the case's reference gives, to 1e-6 of the case's bound (fp64 re-association only)"""
    case, kw, path = entry
    inp = case.make(**kw)
    ref, ind = case.ref(inp, R.F64), _independent(case, inp)
    assert set(ref) == set(ind)
    for k in ref:
        assert ind[k].shape == ref[k].shape and ind[k].dtype == R.F64, (k, ind[k].shape, ref[k].shape)
        if case.exact:
            assert torch.equal(ind[k], ref[k]), k
        else:
            r, a = case.bound(inp, ref)[k]
            q = R.ratio(ind[k], ref[k], r * ref[k].abs() + a)
            assert q < 1e-6, f"{path}: {k} differs from torch's own computation by {q:.3g} of the bound"
