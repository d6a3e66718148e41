"""GPU suite of the RARM training step through the C ABI: the backward of the causal d_head-64 attention, the gradient of the mean token NLL
and the gradient of the token embedding element by element against fp64 (tests/_rarm_train_ref.py states the bounds and near misses), one
transformer block forward + backward and the whole tiny model against autograd of the oracle, three AdamW steps beside torch.optim.AdamW,
and the LatentImageRETRO surface (configure_optimizers / training_step / sync_sampling_weights / validation_step).

Tolerances are the project's own, from tests/test_gpu_backward.py: 3e-2 relative L2 per gradient tensor of one block (its TOL), 2e-2 on
the loss and 5e-2 per tensor of a whole model (test_whole_unet_loss_gradients), 3e-2 per loss of a three-step curve
(test_whole_unet_training_steps_track_torch)."""
import ctypes

import pytest
import torch

from oracle import rarm as orarm
from oracle import unet as ounet

import _rarm_seq_ref as S
import _rarm_train_ref as TR
from _train_ref import check
from _util import rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BF = torch.bfloat16
ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("shape", S.CAUSAL_SHAPES, ids=ids(S.CAUSAL_SHAPES))
def test_causal_attention_bwd_matches_fp64_restatement(ctx, shape):
    """causal_bwd_*_kernel against fp64 per element, every near miss outside the bound; two calls agree bitwise; with row pitches larger than
    the packed widths (ldq, lddo + 8, ldo + 4, ldd + 12) the same bits arrive and the padding columns keep their sentinel."""
    from rdm_amd._lib import lib
    B, n, H = shape
    C = H * 64
    inp = TR.CausalAttentionBwd.make(*shape)
    d = ctx.device
    qkv, o, do = S.qkv_of(inp).to(d, BF).contiguous(), inp["o"].to(d, BF).contiguous(), inp["do"].to(d, BF).contiguous()
    dqkv = ctx.op_causal_attention_d64_bwd(qkv, o, do, H, TR.CausalAttentionBwd.SCALE)
    torch.cuda.synchronize()
    out = {"dq": dqkv[..., :C].float().cpu(), "dk": dqkv[..., C:2 * C].float().cpu(), "dv": dqkv[..., 2 * C:].float().cpu()}
    worst, margin = check(TR.CausalAttentionBwd, inp, out)
    print(f"causal_bwd kernels {shape}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    assert torch.equal(ctx.op_causal_attention_d64_bwd(qkv, o, do, H, TR.CausalAttentionBwd.SCALE), dqkv)
    sentinel = -7.0
    pad = lambda t, extra: torch.cat([t, torch.full(t.shape[:-1] + (extra,), sentinel, device=d, dtype=BF)], -1).contiguous()
    qkv2, o2, do2 = pad(qkv, 8), pad(o, 4), pad(do, 8)
    out2 = torch.full((B, n, 3 * C + 12), sentinel, device=d, dtype=BF)
    rc = lib.rdm_op_causal_attention_d64_bwd(ctx._h, _p(qkv2), 3 * C + 8, _p(o2), C + 4, _p(do2), C + 8, B, n, H, TR.CausalAttentionBwd.SCALE, _p(out2), 3 * C + 12)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(out2[..., :3 * C], dqkv) and bool((out2[..., 3 * C:] == sentinel).all())
    if n == 1:
        assert not dqkv[..., :2 * C].any() and torch.equal(dqkv[..., 2 * C:], do)


@pytest.mark.parametrize("shape", TR.NLL_BWD_SHAPES, ids=ids(TR.NLL_BWD_SHAPES))
def test_nll_bwd_matches_fp64_restatement(ctx, shape):
    """rarm_nll_bwd_kernel against fp64 per element, the near misses outside; two calls agree bitwise; nll_out has op_rarm_nll's bits"""
    inp = TR.NllBwd.make(*shape)
    d = ctx.device
    lg, tg = inp["logits"].to(d), inp["targets"].to(d)
    dl, nll = ctx.op_rarm_nll_bwd(lg, tg, inp["gscale"], want_nll=True)
    torch.cuda.synchronize()
    worst, margin = check(TR.NllBwd, inp, {"dlogits": dl.float().cpu()})
    print(f"rarm_nll_bwd_kernel {shape}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    assert torch.equal(ctx.op_rarm_nll_bwd(lg, tg, inp["gscale"]), dl)
    assert torch.equal(nll, ctx.op_rarm_nll(lg, tg))


@pytest.mark.parametrize("shape", TR.EMBED_SHAPES, ids=ids(TR.EMBED_SHAPES))
def test_embedding_grad_matches_fp64_restatement(ctx, shape):
    """embedding_grad_kernel against fp64 per element into an output pre-filled with a sentinel (unused rows must be WRITTEN as zero); two calls
    agree bitwise"""
    M, V, C, dup = shape
    inp = TR.EmbeddingGrad.make(*shape)
    d = ctx.device
    tok, dy = inp["tokens"].to(d), inp["dy"].to(d, BF).contiguous()
    out = torch.full((V, C), -7.0, device=d, dtype=torch.float32)
    ctx.op_embedding_grad(tok, dy, V, out=out)
    torch.cuda.synchronize()
    worst, margin = check(TR.EmbeddingGrad, inp, {"dw": out.cpu()})
    print(f"embedding_grad_kernel {shape}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    assert torch.equal(ctx.op_embedding_grad(tok, dy, V), out)


def test_argument_refusals(ctx):
    """null pointers, n = 1025, an odd vocabulary and M < 1 return nonzero (nothing is launched), and the Python wrappers refuse bad ids first"""
    from rdm_amd._lib import RdmError, lib
    d = ctx.device
    H, n, B = 1, 4, 1
    qkv = torch.zeros((B, n, 192), device=d, dtype=BF); o = torch.zeros((B, n, 64), device=d, dtype=BF); out = torch.full((B, n, 192), -7.0, device=d, dtype=BF)
    call = lambda q, oo, do, nn, dq: lib.rdm_op_causal_attention_d64_bwd(ctx._h, _p(q), 192, _p(oo), 64, _p(do), 64, B, nn, H, 0.125, _p(dq), 192)
    for args in ((None, o, o, n, out), (qkv, None, o, n, out), (qkv, o, None, n, out), (qkv, o, o, n, None), (qkv, o, o, 1025, out), (qkv, o, o, 0, out)):
        assert call(*args) != 0
    assert lib.rdm_op_causal_attention_d64_bwd(ctx._h, _p(qkv), 196, _p(o), 64, _p(o), 64, B, n, H, 0.125, _p(out), 192) != 0      # ldq not a multiple of 8
    lg = torch.zeros((2, 10), device=d); tg = torch.zeros((2,), device=d, dtype=torch.int64); dl = torch.full((2, 10), -7.0, device=d, dtype=BF)
    assert lib.rdm_op_rarm_nll_bwd(ctx._h, None, 2, 10, _p(tg), 0.5, _p(dl), None) != 0
    assert lib.rdm_op_rarm_nll_bwd(ctx._h, _p(lg), 2, 10, None, 0.5, _p(dl), None) != 0
    assert lib.rdm_op_rarm_nll_bwd(ctx._h, _p(lg), 2, 10, _p(tg), 0.5, None, None) != 0
    assert lib.rdm_op_rarm_nll_bwd(ctx._h, _p(lg), 2, 9, _p(tg), 0.5, _p(dl), None) != 0
    assert lib.rdm_op_rarm_nll_bwd(ctx._h, _p(lg), 0, 10, _p(tg), 0.5, _p(dl), None) != 0
    dy = torch.zeros((2, 8), device=d, dtype=BF); dw = torch.full((4, 8), -7.0, device=d)
    assert lib.rdm_op_embedding_grad(ctx._h, None, _p(dy), 2, 8, 4, _p(dw)) != 0
    assert lib.rdm_op_embedding_grad(ctx._h, _p(tg), None, 2, 8, 4, _p(dw)) != 0
    assert lib.rdm_op_embedding_grad(ctx._h, _p(tg), _p(dy), 2, 8, 4, None) != 0
    assert lib.rdm_op_embedding_grad(ctx._h, _p(tg), _p(dy), 0, 8, 4, _p(dw)) != 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((dl == -7.0).all()) and bool((dw == -7.0).all())
    with pytest.raises(RdmError, match="targets must lie"):
        ctx.op_rarm_nll_bwd(lg, tg + 10, 0.5)
    with pytest.raises(RdmError, match="tokens must lie"):
        ctx.op_embedding_grad(tg + 4, dy, 4)
    with pytest.raises(RdmError, match="1 <= n <= 1024"):
        ctx.op_causal_attention_d64_bwd(torch.zeros((1, 1025, 192), device=d, dtype=BF), torch.zeros((1, 1025, 64), device=d, dtype=BF),
                                        torch.zeros((1, 1025, 64), device=d, dtype=BF), 1, 0.125)


# ------------------------------------------------------------------------------------------------ one block
@pytest.mark.parametrize("C,H,b,t,k", [(128, 2, 3, 12, 4), (768, 12, 2, 36, 8)], ids=["C128", "C768"])
def test_block_forward_backward_matches_autograd(ctx, C, H, b, t, k):
    """one BasicTransformerBlock (causal attn1, cross attn2 on k neighbours, GEGLU ff) forward and backward on the native ops against fp32
    autograd of the oracle's block on the same bf16-rounded operands: output and every gradient tensor within 3e-2 relative L2"""
    from rdm_amd import training as T
    from rdm_amd import training_rarm as TRN
    spec = orarm.RarmSpec(vocab_in=66, vocab_out=64, n_heads=H, d_head=64, depth=1, context_dim=512, sequence_length=t)
    sd = {k_: TR.bfr(torch.as_tensor(v).float()) for k_, v in ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=77).items()
          if k_.startswith("transformer_blocks.0.")}
    g = torch.Generator().manual_seed(5)
    x, cx, dy = TR.bfr(torch.randn(b, t, C, generator=g)), TR.bfr(torch.randn(b, k, 512, generator=g) * 0.45), TR.bfr(torch.randn(b, t, C, generator=g))
    tb = "transformer_blocks.0"
    with torch.enable_grad():
        p = {k_: v.clone().requires_grad_(True) for k_, v in sd.items()}
        xr = x.clone().requires_grad_(True)
        ln = lambda nm, y: torch.nn.functional.layer_norm(y, y.shape[-1:], p[f"{tb}.{nm}.weight"], p[f"{tb}.{nm}.bias"])
        y = orarm.causal_self_attention(p, tb + ".attn1", ln("norm1", xr), H) + xr
        y = ounet.cross_attention(p, tb + ".attn2", ln("norm2", y), cx, H) + y
        y = ounet.feed_forward(p, tb + ".ff", ln("norm3", y)) + y
        (y * dy).sum().backward()
    d = ctx.device
    P = TRN.params_from_state_dict(sd, d)
    names = TRN._block_names(0)
    pp = TRN._gather(P, names, heads=H)
    xd, cd, dyd = x.to(d, BF), cx.to(d, BF), dy.to(d, BF)
    x1, s1 = T.attn_block_forward(ctx, pp["attn1"], xd, causal=True)
    x2, s2 = T.attn_block_forward(ctx, pp["attn2"], x1, cd)
    x3, s3 = T.ff_forward(ctx, pp["ff"], x2.reshape(b * t, C))
    gr = T.transformer_block_backward(ctx, pp, xd, cd, {"x1": x1, "x2": x2, "attn1": s1, "attn2": s2, "ff": s3}, dyd)
    torch.cuda.synchronize()
    grads = {}
    TRN._scatter(grads, {"attn1": gr["attn1"], "attn2": gr["attn2"], "ff": gr["ff"]}, names)
    errs = {"out": rel_l2(x3.reshape(b, t, C).float().cpu(), y.detach()), "dx": rel_l2(gr["x"].float().cpu(), xr.grad)}
    errs.update({k_: rel_l2(grads[k_].float().cpu().reshape(sd[k_].shape), p[k_].grad) for k_ in sd})
    print(f"block C={C}: worst " + ", ".join(f"{k_} {e:.3g}" for k_, e in sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
    assert set(grads) == set(sd)
    for k_, e in errs.items():
        assert e <= 3e-2, (k_, e)


# ------------------------------------------------------------------------------------------------ the whole tiny model
@pytest.fixture(scope="module")
def problem():
    return TR.tiny_problem()


def test_whole_model_loss_and_gradients(ctx, problem):
    """depth 2, b = 3, t = 12, k = 4: loss within 2e-2, all 44 parameter tensors within 5e-2 relative L2 of fp64 autograd"""
    from rdm_amd import training_rarm as TRN
    spec, sd, tokens, targets, context = problem
    P = TRN.params_from_state_dict(sd, ctx.device)
    loss, grads, nll = TRN.rarm_loss_and_grads(ctx, P, spec, tokens, targets, context)
    torch.cuda.synchronize()
    grads = {k: v.cpu() for k, v in TRN.grads_to_state_dict_layout(grads, sd).items()}
    loss64, g64 = TR.autograd_loss_and_grads(sd, spec, tokens, targets, context, torch.float64)
    errs = sorted(((rel_l2(grads[k], g64[k]), k) for k in g64), reverse=True)
    print(f"whole tiny RARM: loss {loss:.5f} (fp64 {loss64:.5f}); worst three: " + ", ".join(f"{k} {e:.3g}" for e, k in errs[:3]))
    assert set(grads) == set(g64) and len(g64) == 44
    assert abs(loss - loss64) <= 2e-2 * abs(loss64), (loss, loss64)
    for e, k in errs:
        assert grads[k].shape == sd[k].shape and e <= 5e-2, (k, e)
    loss2, grads2, _ = TRN.rarm_loss_and_grads(ctx, P, spec, tokens, targets, context)
    assert loss2 == loss and all(torch.equal(grads2[k].cpu().reshape(grads[k].shape), grads[k]) for k in grads)       # no atomics anywhere


def _tiny_mirror(ctx, spec):
    from rdm_amd.models.autoregression.transformer import LatentImageRETRO
    cfg = dict(in_channels=spec.vocab_in, out_channels=spec.vocab_out, n_heads=spec.n_heads, d_head=spec.d_head, depth=spec.depth,
               context_dim=spec.context_dim, sequence_length=spec.sequence_length)
    return LatentImageRETRO({"params": cfg}, sos_token=spec.vocab_in - 1, mask_token=spec.vocab_in - 2, ctx=ctx, p_mask_max=0.0)


def test_three_training_steps_track_torch_and_reach_the_sampler(ctx, monkeypatch):
    """three steps of LatentImageRETRO.training_step beside torch.optim.AdamW(betas=(0.9, 0.95)): each loss within 3e-2; after
    sync_sampling_weights() validation_step on the same batch is within 3e-2 of torch's loss after the steps, and repeats bitwise after
    release_scratch().  fp32 start weights (tiny_problem says why); the first stage is replaced by the batch's own codes."""
    spec, sd, tokens, targets, context = TR.tiny_problem(round_weights=False)
    want, final, _ = TR.torch_adamw_losses(sd, spec, tokens, targets, context, 3, 1e-4)
    assert final <= 0.9 * want[0], (want, final)
    m = _tiny_mirror(ctx, spec)
    monkeypatch.setattr(m, "encode_to_z", lambda x: (None, targets.to(ctx.device)))
    batch = {"image": torch.zeros((tokens.shape[0], 4, 4, 3)), "nn_embeddings": context}
    with pytest.raises(NotImplementedError, match="backward"):
        m.training_step(batch, 0)
    m.load_transformer_state_dict(sd)
    state = m.configure_optimizers(lr=1e-4)
    got = [m.training_step(batch, i) for i in range(3)]
    print("native " + " ".join(f"{v:.4f}" for v in got) + " | torch " + " ".join(f"{v:.4f}" for v in want) + f" -> {final:.4f}")
    for a, b in zip(got, want):
        assert abs(a - b) <= 3e-2 * abs(b), (got, want)
    assert state.step == 3
    before = float(m.validation_step(batch, 0)["val/loss"])
    assert abs(before - want[0]) <= 3e-2 * want[0]                           # the sampler still holds the weights it was loaded with
    m.sync_sampling_weights()
    val = m.validation_step(batch, 0)["val/loss"]
    print(f"validation after sync {float(val):.4f}")
    assert abs(float(val) - final) <= 3e-2 * final, (float(val), final)
    ctx.release_scratch()
    assert torch.equal(m.validation_step(batch, 0)["val/loss"], val)
    out = m.state_dict()
    assert out["transformer.proj_out.weight"].shape == sd["proj_out.weight"].shape and out["transformer.positional_encoding"].shape == sd["positional_encoding"].shape
