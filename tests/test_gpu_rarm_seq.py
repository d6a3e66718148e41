"""GPU suite of the RARM whole-sequence pass through the C ABI: the causal d_head-64 attention kernel and the token-NLL kernel element by
element against fp64 (tests/_rarm_seq_ref.py states the bounds and near misses), rdm_rarm_forward_seq against the committed goldens of the
reference's RetrievalPatchTransformer and against the stepwise rdm_rarm_forward, rdm_rarm_nll against reference values formed from those
goldens, the sampler with a prefilled prefix teacher-forced through the pass, and the LatentImageRETRO / script surface.

Stated tolerances: logits rel L2 <= 2e-2 (tiny) / 2.5e-2 (shipped size) against the reference, the bounds of test_gpu_rarm.py; two summation
orders of the same bf16 operands (whole-sequence pass vs decode steps, fast-mode range walk) <= 1.5e-2 overall and <= 5e-2 on the worst
sequence, the bounds of test_rarm_mid_size_gemm_against_skinny_kernel; a greedy token may differ from the teacher-forced arg-max only at a
near-tie (the two logits within 4e-2 of the row's RMS, test_gpu_vq_codes.py), and on at most 1 position in 4."""
import numpy as np
import pytest
import torch

from oracle import rarm as orarm
from oracle import unet as ounet

import _rarm_seq_ref as S
from _train_ref import check
from _util import golden, rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BF = torch.bfloat16

# |rarm_nll - reference NLL| per token, reference = fp64 logsumexp - target logit of the golden's REFERENCE logits.  Measured on an MI355X:
# worst 3.152e-2 nats over the 36 tiny positions (2.24e-2 of the row's logit RMS, mean RMS 1.50) and 1.297e-1 nats over the 8 shipped-size points
# (2.82e-2 of the row's logit RMS, mean RMS 4.70; the synthetic weights give NLLs near 21 nats).  Asserted: twice the worst measured value rounded
# up to one significant digit, and in no case looser than 4e-2 of the row's logit RMS (the near-tie allowance of test_gpu_vq_codes.py: 2e-2, the
# logits bound, once for the log-sum and once for the target logit) -- at these logit scales the second clause is the one that binds.
NLL_TOL_TINY, NLL_TOL_SHIPPED = 7e-2, 3e-1


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("shape", S.CAUSAL_SHAPES, ids=["x".join(map(str, s)) for s in S.CAUSAL_SHAPES])
def test_causal_attention_matches_fp64_restatement_and_fills_the_cache(ctx, shape):
    """causal_d64_kernel against fp64 per element, every near miss outside the bound; two calls agree bitwise; with caches of L = n + 5
    rows pre-filled with a sentinel, rows 0 .. n-1 receive the bf16 K / V columns of qkv bit for bit, rows n .. L-1 keep the sentinel, and
    `out` has the bits of the call without caches."""
    B, n, H = shape
    inp = S.CausalAttention.make(*shape)
    d = ctx.device
    qkv = S.qkv_of(inp).to(d, BF).contiguous()
    out = ctx.op_causal_attention_d64(qkv, H, S.CausalAttention.SCALE)
    torch.cuda.synchronize()
    worst, margin = check(S.CausalAttention, inp, {"out": out.float().cpu()})
    print(f"causal_d64_kernel {shape}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    assert torch.equal(ctx.op_causal_attention_d64(qkv, H, S.CausalAttention.SCALE), out)
    L, sentinel = n + 5, -7.0
    kc = torch.full((B, H, L, 64), sentinel, device=d, dtype=BF); vc = torch.full((B, H, L, 64), sentinel, device=d, dtype=BF)
    out2 = ctx.op_causal_attention_d64(qkv, H, S.CausalAttention.SCALE, kcache=kc, vcache=vc)
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
    C = H * 64
    for cache, col0 in ((kc, C), (vc, 2 * C)):
        want = qkv[:, :, col0:col0 + C].reshape(B, n, H, 64).permute(0, 2, 1, 3)
        assert torch.equal(cache[:, :, :n], want)
        assert bool((cache[:, :, n:] == sentinel).all())


@pytest.mark.parametrize("shape", S.NLL_SHAPES, ids=["x".join(map(str, s)) for s in S.NLL_SHAPES])
def test_nll_kernel_matches_fp64_restatement(ctx, shape):
    inp = S.Nll.make(*shape)
    out = ctx.op_rarm_nll(inp["logits"], inp["targets"])
    torch.cuda.synchronize()
    worst, margin = check(S.Nll, inp, {"nll": out.float().cpu()})
    print(f"rarm_nll_kernel {shape}: worst error / bound {worst:.3g}, near miss {margin:.3g}")
    assert torch.equal(ctx.op_rarm_nll(inp["logits"], inp["targets"]), out)
    # a row that starts 8 bytes past a 16-byte boundary (odd row of an even V that is no multiple of 4): V = 1002
    if shape[1] == 1000:
        lg = torch.cat([inp["logits"], inp["logits"][:, :2]], 1).contiguous()
        got = ctx.op_rarm_nll(lg, inp["targets"]).double().cpu()
        ref = S.nll64(lg, inp["targets"])
        assert bool(((got - ref).abs() <= 2.0 ** -21 * (4 + lg.double().abs().max(-1).values + ref.abs())).all())


def test_c_abi_refuses_bad_arguments(ctx):
    from rdm_amd import _lib
    _ensure(ctx, "tiny", 1)
    d = ctx.device
    tok = torch.zeros((2, 12), dtype=torch.long, device=d); cx = torch.zeros((2, 4, 512), device=d); big = torch.zeros((2, 129, 512), device=d)
    lg = torch.zeros((2, 12, 1000), device=d); nl = torch.zeros((2, 12), device=d); out = torch.zeros((2, 4), dtype=torch.long, device=d)
    u = torch.zeros((4, 2), device=d)
    P = _lib._ptr
    L = _lib.lib
    for args in ((None, 2, 12, P(cx), 4, P(lg)), (P(tok), 2, 12, None, 4, P(lg)), (P(tok), 2, 12, P(cx), 4, None),
                 (P(tok), 2, 25, P(cx), 4, P(lg)), (P(tok), 2, 12, P(big), 129, P(lg)), (P(tok), 0, 12, P(cx), 4, P(lg))):
        assert L.rdm_rarm_forward_seq(ctx._h, *args) != 0
    for args in ((None, P(tok), 2, 12, P(cx), 4, P(nl)), (P(tok), None, 2, 12, P(cx), 4, P(nl)), (P(tok), P(tok), 2, 12, P(cx), 4, None),
                 (P(tok), P(tok), 2, 25, P(cx), 4, P(nl)), (P(tok), P(tok), 2, 12, P(big), 129, P(nl))):
        assert L.rdm_rarm_nll(ctx._h, *args) != 0
    import ctypes as C
    a = _lib.RarmSampleArgs(batch=2, k=4, cond_len=12, steps=14, temperature=1.0, top_k=0, guidance_scale=1.0)        # 12 + 14 - 1 = 25 > 24
    assert L.rdm_rarm_sample_prefill(ctx._h, C.byref(a), 1.0, P(tok), P(cx), P(u), P(out)) != 0
    a = _lib.RarmSampleArgs(batch=2, k=129, cond_len=12, steps=4, temperature=1.0, top_k=0, guidance_scale=1.0)
    assert L.rdm_rarm_sample_prefill(ctx._h, C.byref(a), 1.0, P(tok), P(big), P(u), P(out)) != 0
    a = _lib.RarmSampleArgs(batch=2, k=4, cond_len=12, steps=4, temperature=1.0, top_k=0, guidance_scale=1.0)
    assert L.rdm_rarm_sample_prefill(ctx._h, C.byref(a), 0.0, P(tok), P(cx), P(u), P(out)) != 0
    assert L.rdm_rarm_sample_prefill(ctx._h, C.byref(a), 1.0, None, P(cx), P(u), P(out)) != 0
    qkv = torch.zeros((1, 8, 192), device=d, dtype=BF); o = torch.zeros((1, 8, 64), device=d, dtype=BF); kc = torch.zeros((1, 1, 8, 64), device=d, dtype=BF)
    assert L.rdm_op_causal_attention_d64(ctx._h, None, 192, 1, 8, 1, 0.125, P(o), 64, None, None, 0) != 0
    assert L.rdm_op_causal_attention_d64(ctx._h, P(qkv), 192, 1, 1025, 1, 0.125, P(o), 64, None, None, 0) != 0
    assert L.rdm_op_causal_attention_d64(ctx._h, P(qkv), 192, 1, 8, 1, 0.125, P(o), 64, P(kc), None, 8) != 0
    assert L.rdm_op_causal_attention_d64(ctx._h, P(qkv), 192, 1, 8, 1, 0.125, P(o), 64, P(kc), P(kc), 7) != 0
    assert L.rdm_op_rarm_nll(ctx._h, None, 2, 1000, P(tok), P(nl)) != 0
    assert L.rdm_op_rarm_nll(ctx._h, P(lg), 2, 999, P(tok), P(nl)) != 0
    with pytest.raises(_lib.RdmError, match="targets must lie in"):
        ctx.rarm_nll(tok, torch.full((2, 12), 1000, dtype=torch.long), cx)


# ------------------------------------------------------------------------------------------------ the pass against the reference class
def _cfg(spec):
    from rdm_amd import _lib
    return _lib.make_rarm_cfg(in_channels=spec.vocab_in, out_channels=spec.vocab_out, n_heads=spec.n_heads, d_head=spec.d_head,
                              depth=spec.depth, context_dim=spec.context_dim, sequence_length=spec.sequence_length)


_LOADED = {}


def _ensure(ctx, which, seed):
    """Load the tiny / shipped-size transformer with seeded weights unless this very load is still the context's current one."""
    from rdm_amd import packing
    key = (which, seed)
    if _LOADED.get("key") == key and ctx.rarm_cfg is _LOADED.get("cfg"):
        return _LOADED["spec"]
    spec = orarm.tiny_rarm_spec() if which == "tiny" else orarm.shipped_rarm_spec()
    cfg = _cfg(spec)
    ctx.load_rarm(cfg, packing.pack("rarm", cfg, ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=seed)))
    _LOADED.update(key=key, cfg=cfg, spec=spec)
    return spec


def _two_orders(a, b, what):
    e = rel_l2(a, b)
    worst = max(rel_l2(a[i], b[i]) for i in range(a.shape[0]))
    print(f"{what}: rel L2 {e:.3e}, worst sequence {worst:.3e}")
    assert e <= 1.5e-2 and worst <= 5e-2


def test_forward_seq_tiny_golden_and_stepwise(ctx):
    g = golden("rarm_tiny.npz")
    _ensure(ctx, "tiny", int(g["seed"]))
    tok, cx = torch.from_numpy(g["tokens"]), torch.from_numpy(g["ctx"])
    logits = ctx.rarm_forward_seq(tok, cx)
    torch.cuda.synchronize()
    ref = torch.from_numpy(g["logits"])
    e = rel_l2(logits, ref)
    per = [rel_l2(logits[:, i], ref[:, i]) for i in range(ref.shape[1])]
    print(f"rarm_forward_seq tiny: rel L2 vs reference golden {e:.3e}, worst position {max(per):.3e}")
    assert logits.shape == ref.shape and e <= 2e-2 and max(per) <= 2e-2
    _two_orders(logits.cpu(), ctx.rarm_forward(tok, cx).cpu(), "whole-sequence pass vs decode steps, tiny 3 x 12")


def test_forward_seq_shipped_golden_and_stepwise(ctx):
    g = golden("rarm_shipped.npz")
    _ensure(ctx, "shipped", int(g["seed"]))
    tok, cx = torch.from_numpy(g["tokens"]), torch.from_numpy(g["ctx"])
    logits = ctx.rarm_forward_seq(tok, cx)
    torch.cuda.synchronize()
    e = rel_l2(logits[:, -2:], torch.from_numpy(g["logits_last"]))
    print(f"rarm_forward_seq shipped 2 x 8 (last 2 positions): rel L2 vs reference golden {e:.3e}")
    assert e <= 2.5e-2
    _two_orders(logits.cpu(), ctx.rarm_forward(tok, cx).cpu(), "whole-sequence pass vs decode steps, shipped 2 x 8")


@pytest.fixture(scope="module")
def deep():
    return golden("rarm_shipped_deep.npz")


def test_forward_seq_shipped_deep_golden(ctx, deep):
    """t = 256: every query tile count of the causal kernel up to the shipped sequence; a row with eight random neighbours and a row with
    zero neighbours (the unconditional half of a guided batch)."""
    g = deep
    _ensure(ctx, "shipped", int(g["seed"]))
    logits = ctx.rarm_forward_seq(torch.from_numpy(g["tokens"]), torch.from_numpy(g["ctx"]))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all())
    ref = torch.from_numpy(g["logits_at"])
    for r in range(2):
        for j, p in enumerate(g["positions"].tolist()):
            e = rel_l2(logits[r, p], ref[r, j])
            print(f"rarm_forward_seq shipped, row {r} ({'zero' if r else 'random'} neighbours), position {p}: rel L2 {e:.3e}")
            assert e <= 2.5e-2


def _random_batch(spec, b, t, seed, k=8):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, spec.vocab_out, (b, t), generator=gen), torch.randn((b, k, spec.context_dim), generator=gen) * 0.45


def test_forward_seq_repeats_bitwise(ctx, deep):
    spec = _ensure(ctx, "shipped", int(deep["seed"]))
    tok, cx = _random_batch(spec, 4, 40, 5)
    first = ctx.rarm_forward_seq(tok, cx)
    assert bool(torch.isfinite(first).all())
    for rep in range(4):
        assert torch.equal(ctx.rarm_forward_seq(tok, cx), first), f"repeat {rep + 1}: the pass gave different bits"


def test_deterministic_mode_rows_do_not_depend_on_the_batch(ctx, deep):
    """Shipped size, 70 sequences x 40 tokens (2800 rows: tall GEMM tiles) against the same rows run alone (80, 40 and 40 rows: short tiles,
    and row counts at which fast mode would take the skinny kernels): bit for bit in deterministic mode."""
    spec = _ensure(ctx, "shipped", int(deep["seed"]))
    tok, cx = _random_batch(spec, 70, 40, 6)
    assert not ctx.deterministic
    ctx.set_deterministic(True)
    try:
        big = ctx.rarm_forward_seq(tok, cx)
        for lo, hi in ((0, 2), (33, 34), (69, 70)):
            small = ctx.rarm_forward_seq(tok[lo:hi], cx[lo:hi])
            assert torch.equal(small, big[lo:hi]), f"sequences {lo}:{hi} differ between a {hi - lo}-sequence and a 70-sequence call in deterministic mode"
    finally:
        ctx.set_deterministic(False)


def test_range_walk_tiny(ctx):
    """1400 sequences x 24 tokens = 33 600 rows: two ranges (1365 sequences, then a ragged one of 35).  Sequences 0, 1365 (the first of the
    second range) and 1399 equal a 3-sequence call bit for bit in deterministic mode and to two summation orders' distance in fast mode."""
    g = golden("rarm_tiny.npz")
    spec = _ensure(ctx, "tiny", int(g["seed"]))
    tok, cx = _random_batch(spec, 1400, 24, 7, k=4)
    pick = torch.tensor([0, 1365, 1399])
    fast_big = ctx.rarm_forward_seq(tok, cx)[pick.to(ctx.device)].cpu()
    fast_small = ctx.rarm_forward_seq(tok[pick], cx[pick]).cpu()
    assert bool(torch.isfinite(fast_big).all())
    _two_orders(fast_big, fast_small, "range walk, fast mode, sequences 0 / 1365 / 1399")
    ctx.set_deterministic(True)
    try:
        big = ctx.rarm_forward_seq(tok, cx)[pick.to(ctx.device)]
        small = ctx.rarm_forward_seq(tok[pick], cx[pick])
        assert torch.equal(big, small)
        nl_big = ctx.rarm_nll(tok, tok.clamp(max=spec.vocab_out - 1), cx)[pick.to(ctx.device)]
        nl_small = ctx.rarm_nll(tok[pick], tok[pick].clamp(max=spec.vocab_out - 1), cx[pick])
        assert torch.equal(nl_big, nl_small)
    finally:
        ctx.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ NLL end to end
def _nll_report(what, got, ref, rms, tol):
    err = (got.double() - ref).abs()
    print(f"{what}: worst |nll - reference| {float(err.max()):.3e} nats (in units of the row's logit RMS: {float((err / rms).max()):.3e}); "
          f"mean reference NLL {float(ref.mean()):.4f}, mean logit RMS {float(rms.mean()):.3f}")
    assert bool((err <= torch.minimum(torch.full_like(rms, tol), 4e-2 * rms)).all())


def test_nll_tiny_golden(ctx):
    """All 36 positions of the tiny golden against fp64 NLLs of the REFERENCE logits.  Measured worst deviation 3.152e-2 nats = 2.24e-2 of the
    row's logit RMS; asserted min(7e-2, 4e-2 RMS) per token (NLL_TOL_TINY above)."""
    g = golden("rarm_tiny.npz")
    spec = _ensure(ctx, "tiny", int(g["seed"]))
    tgt = S.tiny_nll_targets(g, spec.vocab_out)
    got = ctx.rarm_nll(torch.from_numpy(g["tokens"]), tgt, torch.from_numpy(g["ctx"])).cpu()
    assert got.shape == tgt.shape and got.dtype == torch.float32
    _nll_report("rarm_nll tiny, 36 positions", got, S.nll64(g["logits"], tgt), S.logit_rms(g["logits"]), NLL_TOL_TINY)


def test_nll_shipped_deep_golden_and_own_logits(ctx, deep):
    """The 8 (row, position) points of the deep golden that carry reference logits: measured worst deviation 1.297e-1 nats = 2.82e-2 of the
    row's logit RMS, asserted min(3e-1, 4e-2 RMS) per token (NLL_TOL_SHIPPED above); and in deterministic mode
    rarm_nll equals the fp64 NLL of rarm_forward_seq's OWN logits at all 512 positions within the NLL kernel's bound -- both entries run the
    same kernels on the same rows, the head GEMM of the NLL entry in pieces of 2048 rows."""
    g = deep
    spec = _ensure(ctx, "shipped", int(g["seed"]))
    tok, cx = torch.from_numpy(g["tokens"]), torch.from_numpy(g["ctx"])
    tgt = S.deep_nll_targets(g, spec.vocab_out)
    got = ctx.rarm_nll(tok, tgt, cx).cpu()
    pos = torch.from_numpy(g["positions"])
    _nll_report("rarm_nll shipped, positions 0 / 31 / 127 / 255 of 2 rows", got[:, pos], S.nll64(g["logits_at"], tgt[:, pos]),
                S.logit_rms(g["logits_at"]), NLL_TOL_SHIPPED)
    ctx.set_deterministic(True)
    try:
        mine = ctx.rarm_nll(tok, tgt, cx).double().cpu()
        lg = ctx.rarm_forward_seq(tok, cx).cpu()
    finally:
        ctx.set_deterministic(False)
    ref = S.nll64(lg, tgt)
    q = ((mine - ref).abs() / (2.0 ** -21 * (4 + lg.double().abs().max(-1).values + ref.abs()))).max()
    print(f"rarm_nll vs fp64 NLL of rarm_forward_seq's own logits, deterministic mode: worst error / kernel bound {float(q):.3g}")
    assert float(q) <= 1.0


# ------------------------------------------------------------------------------------------------ sampler with prefill
@pytest.mark.parametrize("scale", [1.0, 2.0], ids=["unguided", "guided"])
def test_prefill_with_one_conditioning_token_is_the_plain_sampler(ctx, scale):
    g = golden("rarm_tiny.npz")
    spec = _ensure(ctx, "tiny", int(g["seed"]))
    steps, B = g["uniforms"].shape
    cond = torch.full((B, 1), spec.vocab_in - 1, dtype=torch.long)
    kw = dict(temperature=float(g["temperature"]), top_k=int(g["top_k"]), guidance_scale=scale)
    plain = ctx.rarm_sample(cond, torch.from_numpy(g["ctx"]), steps, torch.from_numpy(g["uniforms"]), **kw)
    pre = ctx.rarm_sample(cond, torch.from_numpy(g["ctx"]), steps, torch.from_numpy(g["uniforms"]), prefill=True, **kw)
    assert torch.equal(pre, plain)


def _near_tie_check(lg, emitted, what):
    """lg: teacher-forced logits of the completed positions; emitted: the tokens the sampler wrote.  -> share of near-tie positions"""
    greedy = lg.argmax(-1)
    differ = greedy != emitted
    share = float(differ.float().mean())
    print(f"{what}: positions whose teacher-forced arg-max is another token: {int(differ.sum())} of {differ.numel()} (share {share:.3f})")
    if bool(differ.any()):
        top = lg.max(-1).values; mine = lg.gather(-1, emitted[..., None])[..., 0]; rms = lg.pow(2).mean(-1).sqrt()
        assert bool(((top - mine)[differ] <= 4e-2 * rms[differ]).all())
    assert share <= 0.25
    return share


@pytest.mark.parametrize("scale", [1.0, 2.0], ids=["unguided", "guided"])
def test_prefilled_completion_is_greedy_decoding_behind_the_given_prefix(ctx, scale):
    """test_completion_is_greedy_decoding_behind_the_given_prefix with prefill=True, teacher-fed through rarm_forward_seq; guided: the
    conditional and zero-neighbour logits combined as the sampler combines them (the duplicated unconditional half of the prefill)."""
    import test_gpu_vq_codes as T
    vspec = T.ovq.tiny_vqgan_spec()
    m, batch = T._mirror(ctx, (vspec, T._first_stage_sd(vspec)))
    x = batch["image"].permute(0, 3, 1, 2)
    r = batch["nn_embeddings"].to(ctx.device)
    _, z = m.encode_to_z(x)
    _, c = m.encode_to_c(torch.zeros((4, 0)))
    out = m.sample(z[:, :32], r, c, steps=32, guidance_scale=scale, prefill=True)
    assert out.shape == (4, 64) and torch.equal(out[:, :32], z[:, :32])
    assert int(out.min()) >= 0 and int(out.max()) < 512
    seq = torch.cat([c.to(ctx.device), out[:, :-1]], dim=1)
    lg = ctx.rarm_forward_seq(seq, r)[:, 32:]                                # logits that predict positions 32 .. 63
    if scale > 1.0:
        lu = ctx.rarm_forward_seq(seq, torch.zeros_like(r))[:, 32:]
        lg = lu + scale * (lg - lu)
    _near_tie_check(lg, out[:, 32:], f"prefilled completion, guidance {scale}")
    assert torch.equal(m.sample(z[:, :32], r, c, steps=32, guidance_scale=scale, prefill=True), out)


def test_prefilled_completion_shipped_size(ctx, deep):
    """The deep golden's two sequences, prefix = sos + 128 codes (129 positions: four full query tiles and a ragged one filled into the
    cache), four greedy steps behind it."""
    g = deep
    _ensure(ctx, "shipped", int(g["seed"]))
    tok, cx = torch.from_numpy(g["tokens"]), torch.from_numpy(g["ctx"]).to(ctx.device)
    cond = tok[:, :129]
    u = torch.zeros((4, 2))
    out = ctx.rarm_sample(cond, cx, 4, u, top_k=1, prefill=True)
    assert out.shape == (2, 4) and int(out.min()) >= 0 and int(out.max()) < 16384
    seq = torch.cat([cond.to(ctx.device), out[:, :-1]], 1)
    lg = ctx.rarm_forward_seq(seq, cx)[:, 128:]
    _near_tie_check(lg, out, "prefilled completion, shipped size, 129-token prefix")


# ------------------------------------------------------------------------------------------------ surface
def test_validation_step_equals_compute_loss_of_forward(ctx):
    import test_gpu_vq_codes as T
    vspec = T.ovq.tiny_vqgan_spec()
    m, batch = T._mirror(ctx, (vspec, T._first_stage_sd(vspec)))
    ctx.set_deterministic(True)
    try:
        val = m.validation_step(batch, 0)
        x, c = m.get_xc(batch)
        logits, target = m.forward(x, c, m.get_r(batch))
        loss, log = m.compute_loss(logits, target, split="val")
        per_token = m.nll(x, m.get_r(batch))
    finally:
        ctx.set_deterministic(False)
    assert list(val) == ["val/loss"] and logits.shape == (4, 64, 512) and target.shape == (4, 64) and per_token.shape == (4, 64)
    ref = S.nll64(logits.cpu(), target.cpu())
    bound = 2.0 ** -21 * (4 + logits.double().abs().max(-1).values.cpu() + ref.abs())
    assert bool(((per_token.double().cpu() - ref).abs() <= bound).all())
    print(f"validation_step {float(val['val/loss']):.6f}, compute_loss(forward) {float(loss):.6f}, fp64 {float(ref.mean()):.6f}")
    assert abs(float(val["val/loss"]) - float(ref.mean())) <= float(bound.mean()) + 2.0 ** -22 * float(ref.mean())
    assert abs(float(loss) - float(ref.mean())) <= 1e-4
    assert abs(float(val["val/loss"]) - float(loss)) <= 2 * float(bound.mean()) + 1e-6
    with pytest.raises(NotImplementedError):
        m.training_step(batch, 0)


def test_rarm_sample_script_score(tmp_path, capsys):
    """scripts/rarm_sample.py --synthetic --score on two generated images: two finite per-image lines and the mean, no PNG written."""
    from PIL import Image
    import test_gpu_vq_codes as T
    src = tmp_path / "src"; src.mkdir()
    rng = np.random.default_rng(12)
    for i, (h, w) in enumerate(((300, 400), (256, 256))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / f"im{i}.png")
    dst = tmp_path / "out"; dst.mkdir()
    mod = T._rarm_script()
    opt = mod.parse_args(["--synthetic", "--synthetic_db_rows", "20000", "--gpu", "0", "-bs", "2", "--seed", "7", "--score", str(src), "-s", str(dst)])
    model = mod.load_model(opt)
    capsys.readouterr()
    nll = mod.sample(model, opt)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    model.ctx.close()
    assert nll.shape == (2, 256) and bool(torch.isfinite(nll).all())
    per_image = [ln for ln in lines if ln.startswith("image ")]
    assert len(per_image) == 2 and all("nats/code" in ln and "bits/code" in ln for ln in per_image)
    for i, ln in enumerate(per_image):
        nats = float(ln.split("nll ")[1].split()[0]); bits = float(ln.split("nats/code, ")[1].split()[0])
        assert np.isfinite(nats) and abs(nats - float(nll[i].mean())) <= 1e-3 and abs(bits - nats / np.log(2.0)) <= 1e-3
    mean = [ln for ln in lines if ln.startswith("val/loss ")]
    assert len(mean) == 1 and abs(float(mean[0].split()[1]) - float(nll.mean())) <= 1e-3
    assert list(dst.iterdir()) == []
