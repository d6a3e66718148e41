"""CPU suite of the RARM training step: fp32 restatements of the three new kernels held to the bounds tests/test_gpu_rarm_train.py holds the
HIP kernels to (tests/_rarm_train_ref.py), the whole graph of rdm_amd.training_rarm run through the TorchOps stand-in against fp64
autograd of oracle.rarm.rarm_forward, three AdamW steps against torch.optim.AdamW, and what LatentImageRETRO.configure_optimizers /
training_step hand down to the context.

Tolerances (the project's own, from the UNet training tests): loss 2e-2 relative, every parameter tensor 5e-2 relative L2, each loss of
the three-step curve 3e-2 relative."""
import pytest
import torch

import _rarm_seq_ref as S
import _rarm_train_ref as TR
from _train_ref import check
from _util import rel_l2

torch.set_num_threads(min(16, torch.get_num_threads()))
ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


# ------------------------------------------------------------------------------------------------ the kernels' references
@pytest.mark.parametrize("shape", S.CAUSAL_SHAPES, ids=ids(S.CAUSAL_SHAPES))
def test_causal_attention_bwd_restatement_within_bound_and_near_misses_outside(shape):
    inp = TR.CausalAttentionBwd.make(*shape)
    worst, margin = check(TR.CausalAttentionBwd, inp, TR.CausalAttentionBwd.standin(inp))
    print(f"causal attention bwd {shape}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def test_causal_attention_bwd_single_token():
    """n = 1: the softmax is 1, so dq = dk = 0 and dv = dO"""
    inp = TR.CausalAttentionBwd.make(3, 1, 2)
    ref = TR.CausalAttentionBwd.ref(inp, torch.float64)
    assert not ref["dq"].any() and not ref["dk"].any() and torch.equal(ref["dv"], inp["do"].double())


@pytest.mark.parametrize("shape", TR.NLL_BWD_SHAPES, ids=ids(TR.NLL_BWD_SHAPES))
def test_nll_bwd_restatement_within_bound_and_near_misses_outside(shape):
    inp = TR.NllBwd.make(*shape)
    worst, margin = check(TR.NllBwd, inp, TR.NllBwd.standin(inp))
    print(f"nll bwd {shape}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


@pytest.mark.parametrize("shape", TR.EMBED_SHAPES, ids=ids(TR.EMBED_SHAPES))
def test_embedding_grad_restatement_within_bound_and_near_misses_outside(shape):
    inp = TR.EmbeddingGrad.make(*shape)
    assert int((inp["tokens"] == shape[1] - 1).sum()) == shape[3]
    worst, margin = check(TR.EmbeddingGrad, inp, TR.EmbeddingGrad.standin(inp))
    print(f"embedding grad {shape}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def test_signatures_declare_the_new_entries():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    for name in ("rdm_op_causal_attention_d64_bwd", "rdm_op_rarm_nll_bwd", "rdm_op_embedding_grad"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    for name in ("op_causal_attention_d64_bwd", "op_rarm_nll_bwd", "op_embedding_grad"):
        assert hasattr(_lib.Context, name), name


# ------------------------------------------------------------------------------------------------ the graph through the stand-in
@pytest.fixture(scope="module")
def problem():
    return TR.tiny_problem()


def test_whole_graph_matches_fp64_autograd(problem):
    """loss within 2e-2, every one of the 44 parameter tensors within 5e-2 relative L2 of fp64 autograd; the graph ran the fused causal path"""
    import rdm_amd  # noqa: F401
    from rdm_amd import training_rarm as TRN
    spec, sd, tokens, targets, context = problem
    ops = TR.TorchOps()
    P = TRN.params_from_state_dict(sd, "cpu")
    with torch.no_grad():
        loss, grads, nll = TRN.rarm_loss_and_grads(ops, P, spec, tokens, targets, context)
    grads = TRN.grads_to_state_dict_layout(grads, sd)
    loss64, g64 = TR.autograd_loss_and_grads(sd, spec, tokens, targets, context, torch.float64)
    assert set(grads) == set(g64) and len(g64) == 44
    assert nll.shape == tokens.shape and abs(float(nll.mean()) - loss) <= 1e-6 * abs(loss)
    assert abs(loss - loss64) <= 2e-2 * abs(loss64), (loss, loss64)
    errs = sorted(((rel_l2(grads[k], g64[k]), k) for k in g64), reverse=True)
    print(f"loss {loss:.5f} (fp64 {loss64:.5f}); worst tensors: " + ", ".join(f"{k} {e:.3g}" for e, k in errs[:3]))
    for e, k in errs:
        assert grads[k].shape == sd[k].shape, k
        assert e <= 5e-2, (k, e)
    assert ops.calls.count("op_causal_attention_d64") == spec.depth and ops.calls.count("op_causal_attention_d64_bwd") == spec.depth
    assert ops.calls.count("op_embedding_grad") == 1
    assert not grads["positional_encoding"][:, tokens.shape[1]:].any() and grads["positional_encoding"][:, :tokens.shape[1]].any()


def test_attention_forward_causal_takes_the_fused_kernels():
    """training.attention_forward(causal=True) / attention_backward: the fused op on [q | k | v], its backward split into dq, dk, dv;
    the default (causal=False) keeps the materialised path; anything but d_head-64 self-attention is refused"""
    import rdm_amd  # noqa: F401
    from rdm_amd import training as T
    inp = TR.CausalAttentionBwd.make(2, 33, 2)
    ops = TR.TorchOps()
    b16 = lambda k: inp[k].to(torch.bfloat16)
    out, saved = T.attention_forward(ops, b16("q"), b16("k"), b16("v"), 2, causal=True)
    g = T.attention_backward(ops, b16("q"), b16("k"), b16("v"), 2, saved, b16("do"))
    assert ops.calls == ["op_causal_attention_d64", "op_causal_attention_d64_bwd"]
    assert torch.equal(out.float(), S.CausalAttention.standin(inp)["out"])
    want = TR.CausalAttentionBwd.standin({**inp, "o": out.float()})
    assert all(torch.equal(g[k].float(), want["d" + k]) and g[k].is_contiguous() for k in "qkv")
    out2, saved2 = T.attention_forward(ops, b16("q"), b16("k"), b16("v"), 2)
    assert "p" in saved2 and out2.shape == out.shape and len(ops.calls) == 2
    with pytest.raises(NotImplementedError, match="d_head = 64"):
        T.attention_forward(ops, b16("q"), b16("k"), b16("v"), 4, causal=True)


def test_three_adamw_steps_track_torch():
    """each loss within 3e-2 of torch.optim.AdamW(betas=(0.9, 0.95)) on fp32 autograd; that curve itself falls by at least 10 %.
    fp32 start weights (tiny_problem says why)."""
    import rdm_amd  # noqa: F401
    from rdm_amd import training_rarm as TRN
    spec, sd, tokens, targets, context = TR.tiny_problem(round_weights=False)
    want, final, _ = TR.torch_adamw_losses(sd, spec, tokens, targets, context, 3, 1e-4)
    assert final <= 0.9 * want[0], (want, final)
    ops = TR.TorchOps()
    state = TRN.TrainState(TRN.params_from_state_dict(sd, "cpu"))
    with torch.no_grad():
        got = [TRN.rarm_training_step(ops, state, spec, tokens, targets, context, lr=1e-4) for _ in range(3)]
        after, _, _ = TRN.rarm_loss_and_grads(ops, state.params(), spec, tokens, targets, context)
    print("native " + " ".join(f"{v:.4f}" for v in got + [after]) + " | torch " + " ".join(f"{v:.4f}" for v in want + [final]))
    for a, b in zip(got + [after], want + [final]):
        assert abs(a - b) <= 3e-2 * abs(b), (got, after, want, final)
    assert state.step == 3
    sdn = TRN.state_dict_from_params(state.P, sd)
    assert sdn["proj_out.weight"].shape == sd["proj_out.weight"].shape and sdn["positional_encoding"].shape == sd["positional_encoding"].shape
    assert torch.equal(state.work["proj_out.weight"], state.P["proj_out.weight"].to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ the surface against a fake context
V = 512


class _FakeCtx(TR.TorchOps):
    def vq_encode_indices(self, x, return_quant=False):
        b = x.shape[0]
        return torch.zeros((b, 64, 2, 2)), (torch.arange(b * 4).reshape(b, 4) * 37 + 11) % V

    def load_rarm(self, cfg, packed):
        self.calls.append("load_rarm")


def _mirror(monkeypatch=None):
    import rdm_amd  # noqa: F401
    from rdm_amd.models.autoregression.transformer import LatentImageRETRO
    fake = _FakeCtx()
    m = LatentImageRETRO({"params": dict(in_channels=V + 2, out_channels=V, n_heads=2, d_head=64, depth=1, context_dim=512, sequence_length=8)},
                         sos_token=V + 1, mask_token=V, ctx=fake, p_mask_max=1.0)
    return m, fake


def _batch(b=3):
    return {"image": torch.zeros((b, 4, 4, 3)), "nn_embeddings": torch.ones((b, 2, 512))}


def _sd():
    from oracle import rarm as orarm
    from oracle import unet as ounet
    spec = orarm.RarmSpec(vocab_in=V + 2, vocab_out=V, n_heads=2, d_head=64, depth=1, context_dim=512, sequence_length=8)
    return {k: torch.from_numpy(v).float() if not torch.is_tensor(v) else v.float()
            for k, v in ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=5).items()}


def test_training_step_needs_configure_optimizers():
    m, _ = _mirror()
    with pytest.raises(NotImplementedError, match=r"backward.*configure_optimizers"):
        m.training_step(_batch(), 0)
    with pytest.raises(RuntimeError, match="no transformer weights"):
        m.configure_optimizers()


def test_training_step_feeds_sos_and_shifted_codes_and_the_masked_neighbours(monkeypatch):
    import numpy as np
    from rdm_amd import training_rarm as TRN
    m, fake = _mirror()
    sd = _sd()
    state = m.configure_optimizers({"transformer." + k: v for k, v in sd.items()}, lr=3e-4)
    assert torch.equal(state.P["proj_out.weight"], sd["proj_out.weight"][:, :, 0]) and state.step == 0
    seen = {}
    real = TRN.rarm_training_step

    def spy(ctx, st, spec, tokens, targets, context, **kw):
        seen.update(tokens=tokens.clone(), targets=targets.clone(), context=context.clone(), kw=kw, st=st)
        return real(ctx, st, spec, tokens, targets, context, **kw)

    monkeypatch.setattr(TRN, "rarm_training_step", spy)
    monkeypatch.setattr(np.random, "uniform", lambda lo, hi: hi)             # get_mask_prob() -> p_mask_max = 1: every entry masked
    batch = _batch()
    loss = m.training_step(batch, 0)
    codes = (torch.arange(12).reshape(3, 4) * 37 + 11) % V
    assert torch.equal(seen["targets"], codes)
    assert torch.equal(seen["tokens"], torch.cat([torch.full((3, 1), V + 1), codes[:, :-1]], 1))
    assert torch.equal(seen["context"], torch.full((3, 2, 512), float(V)))          # r under p_mask = 1: the mask token everywhere
    assert seen["kw"]["lr"] == 3e-4 and seen["kw"]["betas"] == (0.9, 0.95) and seen["kw"]["eps"] == 1e-8 and seen["kw"]["weight_decay"] == 1e-2
    assert seen["st"] is state and state.step == 1 and isinstance(loss, float) and loss > 0
    m.training_step(batch, 1, lr=1e-5)
    assert seen["kw"]["lr"] == 1e-5 and state.step == 2
    out = m.state_dict()
    assert set(out) == {"transformer." + k for k in sd} and out["transformer.proj_out.weight"].shape == sd["proj_out.weight"].shape
    assert not torch.equal(out["transformer.proj_out.bias"], sd["proj_out.bias"])


def test_load_keeps_a_reference_and_sync_reloads(monkeypatch):
    from rdm_amd import packing
    m, fake = _mirror()
    sd = _sd()
    packed = []
    monkeypatch.setattr(packing, "pack", lambda kind, cfg, tsd: packed.append((kind, tsd)) or b"")
    with pytest.raises(RuntimeError, match="configure_optimizers"):
        m.sync_sampling_weights()
    m.load_transformer_state_dict(sd)
    assert m._transformer_sd is sd
    state = m.configure_optimizers()
    assert torch.equal(state.P["positional_encoding"], sd["positional_encoding"]) and state.P["positional_encoding"] is not sd["positional_encoding"]
    state.P["proj_out.bias"].add_(1.0)
    m.sync_sampling_weights()
    assert fake.calls.count("load_rarm") == 2 and packed[-1][0] == "rarm"
    assert torch.equal(packed[-1][1]["proj_out.bias"], sd["proj_out.bias"] + 1.0) and packed[-1][1]["proj_out.weight"].shape == sd["proj_out.weight"].shape
