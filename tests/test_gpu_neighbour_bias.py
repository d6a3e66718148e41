"""The neighbour bias on the GPU (include/rdm_hip.h rdm_set_neighbour_bias): the two biased kernels through their op entries against
the float64 restatements of tests/_nnbias_ref.py (bound, near misses, bitwise properties), the UNet executor and every sampler entry
under a bias against the fp32 oracle with the bias restated, the errors, and the Python surface (nn_counts, short subsets).

Bounds are the project's: one UNet forward 2.5e-2 and a short DDIM trajectory 4e-2 relative L2 against the fp32 oracle
(tests/test_gpu_custom_shape.py)."""
import math

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff
from oracle import unet as ounet
from oracle import vqdecoder as ovq

import _fwd_ref as R
import _nnbias_ref as N
import _step_ref as step_ref
from _train_ref import check
from _util import rel_l2, spec_to_unet_cfg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
torch.set_num_threads(min(16, torch.get_num_threads()))
BF = torch.bfloat16
NEG = float("-inf")
UNET_TOL, DDIM_TOL = 2.5e-2, 4e-2


def _within(what, value, bound):
    print(f"[neighbour bias] {what}: measured {value:.3e} (bound {bound:.1e})")
    assert value <= bound, f"{what}: {value} > {bound}"


def _outside(what, value, bound):
    print(f"[neighbour bias] {what}: measured {value:.3e} (must exceed {bound:.1e})")
    assert value > bound, f"{what}: {value} <= {bound}"


# ================================================================================================ op level: the fused kernels
def _run_xattn(ctx, inp, key_bias="own", ln3=None):
    d = ctx.device
    b = lambda t: t.to(d, BF).contiguous()
    f = lambda t: None if t is None else t.to(d, torch.float32).contiguous()
    kb = inp["key_bias"] if isinstance(key_bias, str) else key_bias
    ln = (f(inp["gamma"]), f(inp["beta"]), inp["eps"]) if inp["ln"] else None
    if ln3 is not None:
        x = b(inp["x"])
        l3 = ctx.op_xattn_fused_ln3(x, b(inp["G"]), b(inp["U"]), f(inp["bias"]), inp["ncols"], inp["k"], ln=ln, ln3=(f(ln3[0]), f(ln3[1])),
                                    key_bias=None if kb is None else f(kb))
        return x, l3
    res = None if inp["ln"] or inp["res"] is None else b(inp["res"])
    return ctx.op_xattn_fused(b(inp["x"]), b(inp["G"]), b(inp["U"]), f(inp["bias"]), res, inp["ncols"], inp["k"], ln=ln,
                              key_bias=None if kb is None else f(kb))


# (B, n, heads, k): one block per sample; NB = ceil(heads k / 32) = 1, 1, 4 (and 1 at k = 1).  Patterns per sample.
_FUSED = [(2, 32, 2, 4, ("finite", "first")), (2, 32, 2, 4, ("one", "finite")),
          (2, 96, 6, 2, ("finite", "first")), (2, 96, 6, 2, ("one", "finite")),
          (2, 32, 30, 4, ("finite", "first")), (2, 32, 30, 4, ("one", "finite"))]


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("B,n,heads,k,patterns", _FUSED, ids=[f"n{c[1]}-h{c[2]}-k{c[3]}-{'+'.join(c[4])}" for c in _FUSED])
def test_fused_biased_matches_fp64_restatement(ctx, B, n, heads, k, patterns, ln):
    inp = N.XattnFusedBiased.make(B, n, heads, k, patterns, ln=ln)
    out = _run_xattn(ctx, inp)
    torch.cuda.synchronize()
    worst, margin = check(N.XattnFusedBiased, inp, {"out": out.float().cpu()})
    print(f"xattn fused biased ({'ln' if ln else 'plain'}, NB {math.ceil(heads * k / 32)}, {patterns}): worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    if "one" in patterns:             # all but one masked: the probabilities are exactly 1 and 0, so the kept column of U arrives unweighted
        b0 = patterns.index("one")
        keep = int(torch.isfinite(inp["key_bias"][b0]).nonzero()[0])
        cols = torch.arange(heads) * k + keep
        want = inp["U"][b0][:, cols].double().sum(-1) + inp["bias"].double() + (inp["x"][b0] if ln else inp["res"][b0]).double()
        got = out[b0].double().cpu()
        assert bool(((got - want).abs() <= 2.0 ** -8 * want.abs() + (heads + 4) * 2.0 ** -24 * (inp["U"][b0][:, cols].double().abs().sum(-1) + want.abs())).all())


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
def test_fused_group_one_is_bitwise_the_unbiased_result(ctx, ln):
    """(2, 64, 4, 1): a softmax over one neighbour is 1 whatever finite bias its score carries."""
    inp = N.XattnFusedBiased.make(2, 64, 4, 1, ("finite", "finite"), ln=ln)
    assert bool(torch.isfinite(inp["key_bias"]).all()) and bool((inp["key_bias"] != 0).all())
    out = _run_xattn(ctx, inp)
    plain = _run_xattn(ctx, inp, key_bias=None)
    assert torch.equal(out, plain)
    check(R.XattnFused, inp, {"out": out.float().cpu()})


def test_fused_norm3_form_biased(ctx):
    """The in-place LN + norm3 form at (2, 96, 6, 4) under a bias: x against the biased restatement, norm3 against a LayerNorm of the kernel's
    own rows."""
    inp = N.XattnFusedBiased.make(2, 96, 6, 4, ("first", "one"), ln=True, seed=7)
    g = torch.Generator().manual_seed(8)
    C = inp["x"].shape[2]
    g3, b3 = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    x, l3 = _run_xattn(ctx, inp, ln3=(g3, b3))
    torch.cuda.synchronize()
    worst, margin = check(N.XattnFusedBiased, inp, {"out": x.float().cpu()})
    print(f"xattn ln3 biased: worst {worst:.3g}, closest near miss {margin:.3g}")
    rows = x.float().cpu().reshape(-1, C)
    check(R.LayerNorm, R.LayerNorm.make(rows.shape[0], C, x=rows, gamma=g3, beta=b3), {"out": l3.float().cpu().reshape(-1, C)})
    x0, l30 = _run_xattn(ctx, inp, key_bias=torch.zeros(2, 4), ln3=(g3, b3))
    xp, l3p = _run_xattn(ctx, inp, key_bias=None, ln3=(g3, b3))
    assert torch.equal(x0, xp) and torch.equal(l30, l3p), "a zero bias differs from the unbiased norm3 form"


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("B,n,heads,k", [(2, 32, 2, 4), (2, 96, 6, 2), (2, 32, 30, 4)], ids=["nb1-k4", "nb1-k2", "nb4-k4"])
def test_fused_bitwise_properties(ctx, B, n, heads, k, ln):
    inp = N.XattnFusedBiased.make(B, n, heads, k, ("first", "finite"), ln=ln)
    out = _run_xattn(ctx, inp)
    # a zero bias is the unbiased entry
    assert torch.equal(_run_xattn(ctx, inp, key_bias=torch.zeros(B, k)), _run_xattn(ctx, inp, key_bias=None))
    # a masked neighbour's finite data has no influence: its G rows and U columns replaced (sample 0, neighbour 0)
    cols = torch.arange(heads) * k
    other = dict(inp)
    g = torch.Generator().manual_seed(77)
    Gm, Um = inp["G"].clone(), inp["U"].clone()
    Gm[0, cols] = R.bfr(torch.randn(heads, Gm.shape[2], generator=g) * 3)
    Um[0][:, cols] = R.bfr(torch.randn(Um.shape[1], heads, generator=g) * 3)
    other["G"], other["U"] = Gm, Um
    assert torch.equal(_run_xattn(ctx, other), out), "a masked neighbour's G rows / U columns changed the output"
    assert not torch.equal(_run_xattn(ctx, other, key_bias=None), _run_xattn(ctx, inp, key_bias=None))
    # sample 1's bias changed: every other sample's output is bit-identical
    kb = inp["key_bias"].clone(); kb[1] = N.bias_rows("finite", k, 991)
    out2 = _run_xattn(ctx, inp, key_bias=kb)
    assert torch.equal(out2[0], out[0]) and not torch.equal(out2[1], out[1])


# ================================================================================================ op level: small attention
def _run_small(ctx, inp, key_bias="own"):
    b = lambda t: t.to(ctx.device, BF).contiguous()
    kb = inp["key_bias"] if isinstance(key_bias, str) else key_bias
    return ctx.op_small_attention(b(inp["q"]), b(inp["k"]), b(inp["v"]), inp["H"], inp["D"], 0, inp["scale"],
                                  key_bias=None if kb is None else kb.to(ctx.device))


# key 0 masked (the NaN trap of the online softmax); 50 odd queries x 16 keys; 300 keys: chunks of 256, masked keys on both sides of the
# boundary, the boundary keys themselves among them
_SMALL = [dict(B=2, nq=16, nkv=3, H=4, D=32, masked=[[0], [1, 2]]),
          dict(B=2, nq=50, nkv=16, H=6, D=32, masked=[[0, 5, 15], []]),
          dict(B=2, nq=40, nkv=300, H=2, D=32, masked=[[0, 100, 254, 255, 256, 257, 299], list(range(256, 300))])]


@pytest.mark.parametrize("kw", _SMALL, ids=["k3-first-masked", "k16-odd-queries", "k300-two-chunks"])
def test_small_attention_biased_matches_fp64_restatement(ctx, kw):
    inp = N.SmallAttentionBiased.make(**kw)
    out = _run_small(ctx, inp)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()), "a masked key poisoned the row"
    worst, margin = check(N.SmallAttentionBiased, inp, {"out": out.float().cpu()})
    print(f"small attention biased {kw['nkv']} keys: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    # a zero bias is the unbiased entry
    assert torch.equal(_run_small(ctx, inp, key_bias=torch.zeros_like(inp["key_bias"])), _run_small(ctx, inp, key_bias=None))
    # a masked key's k / v rows replaced
    other = dict(inp)
    g = torch.Generator().manual_seed(5)
    m0 = kw["masked"][0]
    kk, vv = inp["k"].clone(), inp["v"].clone()
    kk[0, m0] = R.bfr(torch.randn(len(m0), kk.shape[2], generator=g) * 4); vv[0, m0] = R.bfr(torch.randn(len(m0), vv.shape[2], generator=g) * 4)
    other["k"], other["v"] = kk, vv
    assert torch.equal(_run_small(ctx, other), out), "a masked key's k / v rows changed the output"
    # sample 1's bias changed
    kb = inp["key_bias"].clone(); kb[1] = torch.rand(kb.shape[1], generator=g) * 6 - 3
    out2 = _run_small(ctx, inp, key_bias=kb)
    assert torch.equal(out2[0], out[0]) and not torch.equal(out2[1], out[1])


def test_small_attention_biased_refuses_the_causal_mask(ctx):
    from rdm_amd._lib import RdmError
    inp = N.SmallAttentionBiased.make(B=1, nq=8, nkv=8, H=1, D=32, masked=[[]])
    b = lambda t: t.to(ctx.device, BF).contiguous()
    with pytest.raises(RdmError, match="causal"):
        ctx.op_small_attention(b(inp["q"]), b(inp["k"]), b(inp["v"]), 1, 32, 1, inp["scale"], key_bias=inp["key_bias"].to(ctx.device))


# ================================================================================================ model level
_MODELS = {}


def _use(ctx, name):
    """Load the named synthetic UNet on the session context unless it is the one this module loaded last."""
    from rdm_amd import packing
    if name not in _MODELS:
        spec = ounet.tiny_spec() if name == "tiny" else ounet.shipped_spec()
        _MODELS[name] = (spec, ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234))
    spec, sd = _MODELS[name]
    if _MODELS.get("loaded") != name:
        cfg = spec_to_unet_cfg(spec)
        ctx.load_unet(cfg, packing.pack("unet", cfg, sd))
        _MODELS["loaded"] = name
    ctx.set_neighbour_bias(None)
    return spec, sd


@pytest.fixture(scope="module", autouse=True)
def _fresh_module():
    _MODELS.pop("loaded", None)           # another module has loaded its own UNet on the session context
    yield


@pytest.fixture(autouse=True)
def _clean_context(ctx):
    yield
    ctx.set_neighbour_bias(None)


def _oracle(sd, spec, x, t, c, bias, monkeypatch):
    with monkeypatch.context() as mp:
        if bias is not None:
            mp.setattr(ounet, "cross_attention", N.biased_cross_attention(bias))
        return ounet.unet_forward(sd, spec, x, t, c)


def _inputs(B, H, k, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, H, H, generator=g), torch.tensor([500, 37][:B]), torch.randn(B, k, 512, generator=g) * 1.0


@pytest.mark.parametrize("name,H", [("tiny", 16), ("shipped", 32)])
def test_unet_forward_under_mask_and_weights(ctx, monkeypatch, name, H):
    """rdm_unet_forward under the mask and under the weights against the biased oracle; the same output against the unbiased oracle lies
    outside the bound; the two references differ by at least 4 x the bound.  Tiny at 16 x 16: the fused kernel at its 64-token level (and
    256), the generic branch in place of the two-GEMM form at its 16-token level."""
    spec, sd = _use(ctx, name)
    x, t, c = _inputs(2, H, 4)
    plain = _oracle(sd, spec, x, t, c, None, monkeypatch)
    nat_plain = ctx.unet_forward(x, t, c)
    _within(f"{name}: unbiased forward vs oracle", rel_l2(nat_plain, plain), UNET_TOL)
    for what, rows in (("mask", N.MASK_ROWS), ("weights [4, 1, 1, 1/4]", N.WEIGHT_ROWS)):
        bias = torch.tensor(rows)
        ref = _oracle(sd, spec, x, t, c, bias, monkeypatch)
        _outside(f"{name}, {what}: biased oracle vs unbiased oracle", rel_l2(ref, plain), 4 * UNET_TOL)
        with ctx.neighbour_bias(bias):
            eps = ctx.unet_forward(x, t, c)
        assert ctx.get_neighbour_bias() is None
        _within(f"{name}, {what}: native under the bias vs biased oracle", rel_l2(eps, ref), UNET_TOL)
        _outside(f"{name}, {what}: native under the bias vs unbiased oracle", rel_l2(eps, plain), UNET_TOL)
    assert torch.equal(ctx.unet_forward(x, t, c), nat_plain), "after set_neighbour_bias(None) a call is not what it was before"


@pytest.mark.parametrize("k,rows", [(3, [[NEG, 0.0, 1.0], [0.5, NEG, NEG]]), (16, [[NEG] * 5 + [0.0] * 11, [1.0, -1.0] * 8])], ids=["k3-first-masked", "k16"])
def test_unet_forward_generic_path_under_a_bias(ctx, monkeypatch, k, rows):
    spec, sd = _use(ctx, "tiny")
    x, t, c = _inputs(2, 16, k, seed=5)
    bias = torch.tensor(rows)
    ref = _oracle(sd, spec, x, t, c, bias, monkeypatch)
    plain = _oracle(sd, spec, x, t, c, None, monkeypatch)
    with ctx.neighbour_bias(bias):
        eps = ctx.unet_forward(x, t, c)
    assert bool(torch.isfinite(eps).all())
    _within(f"k = {k}: native under the bias vs biased oracle", rel_l2(eps, ref), UNET_TOL)
    _outside(f"k = {k}: native under the bias vs unbiased oracle", rel_l2(eps, plain), UNET_TOL)
    want = ctx.unet_forward(x, t, c)
    with ctx.neighbour_bias(torch.zeros(2, k)):       # the generic branch with and without the operand: no dispatch change
        assert torch.equal(ctx.unet_forward(x, t, c), want)


def test_zero_bias_is_bitwise_no_bias_where_the_dispatch_stays(ctx):
    """Latent 32 x 32 on the tiny spec: levels of 1024 / 256 / 64 tokens, all on the fused kernel with or without a bias."""
    _use(ctx, "tiny")
    x, t, c = _inputs(2, 32, 4, seed=9)
    want = ctx.unet_forward(x, t, c)
    with ctx.neighbour_bias(torch.zeros(2, 4)):
        assert torch.equal(ctx.unet_forward(x, t, c), want)


@pytest.mark.parametrize("zero_uncond", [True, False], ids=["zero-uncond", "given-uncond"])
def test_guided_forward_never_biases_the_unconditional_half(ctx, monkeypatch, zero_uncond):
    spec, sd = _use(ctx, "tiny")
    x, _, c = _inputs(2, 16, 4, seed=11)
    uc = torch.zeros_like(c) if zero_uncond else torch.randn(2, 4, 512, generator=torch.Generator().manual_seed(12))
    bias = torch.tensor(N.MASK_ROWS)
    plain = ctx.unet_forward_guided(x, 500, c, uc)
    with ctx.neighbour_bias(bias):
        out = ctx.unet_forward_guided(x, 500, c, uc)
    assert torch.equal(out[2:], plain[2:]), "the unconditional rows' eps moved under a bias"
    assert not torch.equal(out[:2], plain[:2])
    ref = _oracle(sd, spec, torch.cat([x, x]), torch.full((4,), 500), torch.cat([c, uc]), bias, monkeypatch)
    _within("guided forward under the mask vs biased oracle", rel_l2(out, ref), UNET_TOL)


def test_deterministic_mode_honours_the_bias(ctx, monkeypatch):
    spec, sd = _use(ctx, "tiny")
    x, t, c = _inputs(2, 16, 4)
    bias = torch.tensor(N.MASK_ROWS)
    ref = _oracle(sd, spec, x, t, c, bias, monkeypatch)
    ctx.set_deterministic(True)
    try:
        with ctx.neighbour_bias(bias):
            eps = ctx.unet_forward(x, t, c)
        with ctx.neighbour_bias(bias[1:]):
            one = ctx.unet_forward(x[1:], t[1:], c[1:])
    finally:
        ctx.set_deterministic(False)
    assert torch.equal(eps[1:], one), "deterministic mode: row 1 of the biased batch differs from the same sample run alone under its own row"
    # the guided forward as the samplers run it in deterministic mode: every row takes the cross-attention, the unconditional ones unbiased
    uc = torch.zeros_like(c)
    ctx.set_deterministic(True)
    try:
        plain_g = ctx.unet_forward_guided(x, 500, c, uc)
        with ctx.neighbour_bias(bias):
            out = ctx.unet_forward_guided(x, 500, c, uc)
    finally:
        ctx.set_deterministic(False)
    assert torch.equal(out[2:], plain_g[2:]) and not torch.equal(out[:2], plain_g[:2])
    ref_g = _oracle(sd, spec, torch.cat([x, x]), torch.full((4,), 500), torch.cat([c, uc]), bias, monkeypatch)
    _within("deterministic mode, guided forward under the mask vs biased oracle", rel_l2(out, ref_g), UNET_TOL)
    _within("deterministic mode under the mask vs biased oracle", rel_l2(eps, ref), UNET_TOL)


# ---- every sampler entry, 2 - 3 steps on the tiny spec, neighbour 3 masked
ACP = odiff.Schedule().alphas_cumprod


def _sampler_entries(ctx):
    sched = odiff.Schedule()
    ddpm = {n: getattr(sched, n).numpy() for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                                   "posterior_mean_coef2", "posterior_log_variance_clipped")}
    nodes = [999, 600, 200, 1]
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(2, 3, 16, 16, generator=g)
    mask = (torch.rand(2, 1, 16, 16, generator=g) < 0.5).float()
    return {
        "ddim": lambda x, c, u: ctx.ddim_sample(2, x, c, u, ACP, scale=2.0)[0],
        "plms": lambda x, c, u: ctx.plms_sample(2, x, c, u, ACP, scale=2.0)[0],
        "dpmpp": lambda x, c, u: ctx.dpmpp_sample(nodes, x, c, u, ACP, scale=2.0)[0],
        "unipc": lambda x, c, u: ctx.unipc_sample(nodes, x, c, u, ACP, scale=2.0)[0],
        "sde-seeded": lambda x, c, u: ctx.dpmpp_sde_sample(nodes, x, c, u, ACP, scale=2.0, seed=7)[0],
        "ddpm-seeded": lambda x, c, u: ctx.ddpm_sample(3, x, c, None, ddpm, seed=7),
        "decode": lambda x, c, u: ctx.ddim_decode(4, 2, x, c, u, ACP, scale=2.0)[0],
        "encode": lambda x, c, u: ctx.ddim_encode(4, 2, x, c, u, ACP, scale=2.0)[0],
        "inpaint-seeded": lambda x, c, u: ctx.ddim_inpaint(4, 2, x, x0, mask, c, u, ACP, scale=2.0, seed=7)[0],
    }


@pytest.mark.parametrize("entry", ["ddim", "plms", "dpmpp", "unipc", "sde-seeded", "ddpm-seeded", "decode", "encode", "inpaint-seeded"])
def test_every_sampler_entry_honours_the_bias(ctx, entry):
    _use(ctx, "tiny")
    run = _sampler_entries(ctx)[entry]
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 3, 16, 16, generator=g)
    c = torch.randn(2, 4, 512, generator=g)
    u = torch.zeros_like(c)
    c2 = c.clone(); c2[:, 3] = torch.randn(2, 512, generator=g) * 2
    bias = torch.tensor([[0.0, 0.0, 0.0, NEG]] * 2)
    plain = run(x, c, u)
    with ctx.neighbour_bias(bias):
        a = run(x, c, u)
        b = run(x, c2, u)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b), f"{entry}: the masked neighbour's content changed the latent"
    assert not torch.equal(a, plain), f"{entry}: the bias was not honoured"
    assert not torch.equal(run(x, c2, u), plain)


def test_ddim_native_loop_is_the_callers_loop_and_holds_the_oracle(ctx, monkeypatch):
    """The native guided DDIM loop under a bias, bit for bit the caller's loop over rdm_unet_forward_guided + rdm_op_ddim_step under the same
    bias, and within DDIM_TOL of oracle.diffusion.ddim_sample with the biased forward.  (A 3-step 'uniform' schedule does not exist at
    T = 1000 -- S = 3 yields the timestep 1000 --, so the schedule is S = 4: its first 3 steps and the 4th are all compared.)"""
    spec, sd = _use(ctx, "tiny")
    S, scale, B = 4, 2.0, 2
    g = torch.Generator().manual_seed(41)
    x_T = torch.randn(B, 3, 16, 16, generator=g)
    c = torch.randn(B, 4, 512, generator=g)
    u = torch.zeros_like(c)
    bias = torch.tensor(N.MASK_ROWS)
    with ctx.neighbour_bias(bias):
        z, xi, _ = ctx.ddim_sample(S, x_T, c, u, ACP, scale=scale, log_every_t=1, want_intermediates=True)
        x = x_T.to(ctx.device).clone()
        n_steps = step_ref.ddim_steps(S)
        for i in range(n_steps):
            index = n_steps - 1 - i
            t, a_t, a_prev, sigma, s1m = step_ref.ddim_scalars(S, index, 0.0)
            eps = ctx.unet_forward_guided(x, t, c, u)
            ctx.op_ddim_step(x, eps, None, True, scale, a_t, a_prev, sigma, s1m, 1.0, x)
            torch.cuda.synchronize()
            assert torch.equal(x, xi[i]), f"step {i}: the caller's loop differs from the native loop"
    assert torch.equal(x, z)
    with monkeypatch.context() as mp:
        mp.setattr(ounet, "cross_attention", N.biased_cross_attention(bias))
        z_ref, _ = odiff.ddim_sample(lambda xx, tt, cc: ounet.unet_forward(sd, spec, xx, tt, cc), odiff.Schedule(), S, x_T, c, scale=scale, uncond=u)
    z_plain, _ = odiff.ddim_sample(lambda xx, tt, cc: ounet.unet_forward(sd, spec, xx, tt, cc), odiff.Schedule(), S, x_T, c, scale=scale, uncond=u)
    _within("guided DDIM under the mask vs biased oracle", rel_l2(z, z_ref), DDIM_TOL)
    _outside("guided DDIM under the mask vs unbiased oracle", rel_l2(z, z_plain), DDIM_TOL)


def test_sampler_classes_take_the_bias_on_the_native_and_the_per_step_path(ctx):
    """DDIMSampler.sample(neighbour_bias=): the native loop, and with a callback the per-step path, whose guided forward runs the doubled
    batch under [bias | zeros]; PLMSSampler's per-step path orders the batch [uc | c].  Both paths agree (2.5e-2, the samplers' bound) and
    differ from the unbiased call; the context is left without a bias."""
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    from rdm_amd.models.diffusion.plms import PLMSSampler
    m = _surface_model(ctx)
    g = torch.Generator().manual_seed(51)
    x_T = torch.randn(2, 3, 16, 16, generator=g).to(m.device)
    c = torch.randn(2, 4, 512, generator=g).to(m.device)
    kw = dict(S=4, batch_size=2, shape=(3, 16, 16), conditioning=c, x_T=x_T, verbose=False, unconditional_guidance_scale=2.0,
              unconditional_conditioning=torch.zeros_like(c))
    bias = torch.tensor(N.MASK_ROWS)
    for cls in (DDIMSampler, PLMSSampler):
        plain, _ = cls(m).sample(**kw)
        native, _ = cls(m).sample(neighbour_bias=bias, **kw)
        per_step, _ = cls(m).sample(neighbour_bias=bias, callback=lambda i: None, **kw)
        assert ctx.get_neighbour_bias() is None
        _within(f"{cls.__name__}: per-step path vs native loop under the mask", rel_l2(per_step, native), 2.5e-2)
        _outside(f"{cls.__name__}: native loop under the mask vs unbiased", rel_l2(native, plain), 0.1)
    z = m.sample_log(cond=c, batch_size=2, ddim=True, ddim_steps=4, x_T=x_T, unconditional_guidance_scale=2.0,
                     unconditional_conditioning=torch.zeros_like(c), neighbour_bias=bias)[0]
    assert torch.equal(z, DDIMSampler(m).sample(neighbour_bias=bias, **kw)[0])
    with pytest.raises(ValueError, match="no finite entry"):
        DDIMSampler(m).sample(neighbour_bias=torch.full((2, 4), NEG), **kw)


# ---- errors
def test_bias_errors_leave_the_context_usable(ctx):
    from rdm_amd._lib import RdmError
    _use(ctx, "tiny")
    x, t, c = _inputs(2, 16, 4)
    want = ctx.unet_forward(x, t, c)
    # a (rows, k) mismatch; a bias left set from another shape
    ctx.set_neighbour_bias(torch.zeros(3, 4))
    with pytest.raises(RdmError, match="neighbour bias"):
        ctx.unet_forward(x, t, c)
    with pytest.raises(RdmError, match="neighbour bias"):
        ctx.ddim_sample(2, x, c, torch.zeros_like(c), ACP, scale=2.0)
    ctx.set_neighbour_bias(torch.zeros(2, 2))
    with pytest.raises(RdmError, match="neighbour bias"):
        ctx.unet_forward_guided(x, 500, c, torch.zeros_like(c))
    assert ctx.get_neighbour_bias() == (2, 2)
    # refused values: the bias in force stays
    for bad, word in ((torch.tensor([[0.0, float("nan")], [0.0, 0.0]]), "NaN"), (torch.tensor([[0.0, float("inf")], [0.0, 0.0]]), "inf"),
                      (torch.tensor([[0.0, 0.0], [NEG, NEG]]), "finite")):
        with pytest.raises(RdmError, match=word):
            ctx.set_neighbour_bias(bad)
        assert ctx.get_neighbour_bias() == (2, 2)
    ctx.set_neighbour_bias(None)
    assert ctx.get_neighbour_bias() is None
    assert torch.equal(ctx.unet_forward(x, t, c), want)
    with pytest.raises(RdmError):
        with ctx.neighbour_bias(torch.zeros(5, 4)):
            ctx.unet_forward(x, t, c)
    assert ctx.get_neighbour_bias() is None, "the context manager did not clear the bias on the way out"


# ================================================================================================ the Python surface
def _surface_model(ctx):
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    spec, vspec = ounet.tiny_spec(), ovq.tiny_vq_spec()
    unet = dict(in_channels=spec.in_channels, out_channels=spec.out_channels, model_channels=spec.model_channels,
                num_res_blocks=spec.num_res_blocks, attention_resolutions=spec.attention_resolutions, channel_mult=spec.channel_mult,
                num_head_channels=spec.num_head_channels, context_dim=spec.context_dim)
    fs = {"params": {"embed_dim": 3, "n_embed": vspec.n_embed, "ddconfig": {"z_channels": 3, "ch": vspec.ch, "ch_mult": vspec.ch_mult,
                                                                          "num_res_blocks": vspec.num_res_blocks, "resolution": vspec.resolution}}}
    m = MinimalRETRODiffusion(unet_config={"params": unet}, first_stage_config=fs, k_nn=4, image_size=16, ctx=ctx)
    m.load_unet_state_dict(ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234))
    m.load_first_stage_state_dict(ounet.synth_state_dict(ovq.vq_param_shapes(vspec), seed=5))
    _MODELS["loaded"] = "tiny"
    return m


def test_short_subsets_and_mixed_counts_on_the_surface(ctx):
    """A subset of 2 rows at k_nn = 4: "mask" samples finite images, equal bit for bit to the same neighbours given explicitly with nn_counts
    (the masked places then hold OTHER finite rows: they cannot matter); the default raises; nn_counts = [4, 1] in one batch is the two
    samples run in separate calls at those counts (deterministic mode: the batch invariance test_gpu_custom_shape demands of unet_forward)."""
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    was = ctx.deterministic
    ctx.set_deterministic(True)
    try:
        m = _surface_model(ctx)
        rng = np.random.default_rng(57)
        n = 503
        pool = {"embedding": (rng.standard_normal((n, 512)) * 0.45).astype(np.float16), "img_id": np.arange(n), "patch_coords": np.zeros((n, 4), np.int64)}
        qs = (rng.standard_normal((2, 512)) * 0.45).astype(np.float32)
        x_T = torch.from_numpy(rng.standard_normal((2, 3, 16, 16)).astype(np.float32))
        two = np.array([5, 400])
        kw = dict(query_embedded=True, k_nn=4, ddim=True, ddim_steps=2, unconditional_guidance_scale=2.0, unconditional_retro_guidance_label=0.)
        db = DatasetBuilder(data_pool=pool, k=4, ctx=ctx)
        db.define_subset("two", two)
        db.train_searcher()
        m.retriever = db
        q = torch.from_numpy(qs)
        with pytest.raises(ValueError, match=r"subset 'two' allows 2 rows, fewer than k = 4"):
            m.sample_with_query(query=q, x_T=x_T, db_subset="two", **kw)
        masked = m.sample_with_query(query=q, x_T=x_T, db_subset="two", short_subsets="mask", **kw)["query_samples"]
        assert bool(torch.isfinite(masked).all()) and ctx.get_neighbour_bias() is None
        nn = db.search_k_nearest(qs, k=4, query_embedded=True, subset="two", short_ok=True)
        assert nn["counts"].tolist() == [2, 2] and bool((nn["embeddings"][:, 2:] == 0).all())
        # the same neighbours given explicitly: a database of the two rows and two rows opposite to both queries (they rank last)
        junk = np.stack([-(qs[0] + qs[1]), -2 * (qs[0] + qs[1])]).astype(np.float16)
        small = DatasetBuilder(data_pool={"embedding": np.concatenate([pool["embedding"][two], junk]), "img_id": np.arange(4),
                                          "patch_coords": np.zeros((4, 4), np.int64)}, k=4, ctx=ctx)
        small.train_searcher()
        got = small.search_k_nearest(qs, k=4, query_embedded=True)
        assert np.array_equal(two[got["nns"][:, :2]], nn["nns"][:, :2]), "the stand-in database does not rank the two rows first"
        m.retriever = small
        explicit = m.sample_with_query(query=q, x_T=x_T, nn_counts=3, **kw)["query_samples"]        # the query + the two rows
        assert torch.equal(masked, explicit)
        assert not torch.equal(masked, m.sample_with_query(query=q, x_T=x_T, **kw)["query_samples"])
        # sample_from_rdata: the retrieved neighbours alone are the conditioning
        db.train_searcher()
        m.retriever = db
        rkw = dict(qids=np.array([1, 2]), x_T=x_T, k_nn=4, ddim=True, ddim_steps=2, unconditional_guidance_scale=2.0, unconditional_retro_guidance_label=0.)
        rd = m.sample_from_rdata(2, db_subset="two", short_subsets="mask", **rkw)["samples_with_sampled_nns"]
        nn_rd = db.search_k_nearest(pool["embedding"][rkw["qids"]], k=4, query_embedded=True, subset="two", short_ok=True)
        given = torch.from_numpy(np.asarray(nn_rd["embeddings"])).float()
        given[:, 2:] = torch.randn(2, 2, 512, generator=torch.Generator().manual_seed(1))
        assert torch.equal(rd, m.sample_from_rdata(2, nn_embeddings=given.to(m.device), nn_counts=2, **rkw)["samples_with_sampled_nns"])
        # mixed counts in one batch
        mixed = m.sample_with_query(query=q, x_T=x_T, nn_counts=[4, 1], **kw)["query_samples"]
        for j, cnt in enumerate((4, 1)):
            alone = m.sample_with_query(query=q[j:j + 1], x_T=x_T[j:j + 1], nn_counts=cnt, **kw)["query_samples"]
            assert torch.equal(mixed[j:j + 1], alone), (j, cnt)
        # (count 4 is a zero bias row, but no bit-for-bit twin of the call without a bias: the 16-token level takes the generic branch under a
        #  bias, and the first stage's quantiser turns a last-bit difference of a latent into another code)
    finally:
        ctx.set_deterministic(was)
        ctx.set_neighbour_bias(None)
