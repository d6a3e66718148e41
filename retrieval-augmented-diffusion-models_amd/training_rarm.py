"""The RARM transformer in training form on the native ops: forward with saved activations, the mean cross-entropy of the next code, backward
to every parameter, and the AdamW step -- what autograd and `configure_optimizers` do under `LatentImageRETRO.training_step`
(rdm/models/autoregression/transformer.py:46-57, 106-119, 207-222) for RetrievalPatchTransformer (rdm/modules/attention.py:199-272:
token embedding + learned positions, `depth` BasicTransformerBlocks of causal self-attention, cross-attention to the k neighbours and a
GEGLU feed-forward, a 1x1 Conv1d head).  The counterpart of training_unet.py for the autoregressive model.

Every arithmetic step of a block, of the head and of the loss is a C-ABI call (rdm_amd._lib / rdm_amd.training): the causal attention and
its fused backward (rdm_op_causal_attention_d64 / _bwd) on ONE fused q | k | v projection, the cross-attention on the materialised-score
path, the loss gradient (rdm_op_rarm_nll_bwd) and the embedding gradient (rdm_op_embedding_grad).  torch holds device memory and does
layout plumbing: the embedding-row gather with the position rows added to it (one [b t, C] tensor), concatenating the three projection
weights, zero padding, transposes of the position table, the mean of the per-token losses.

The head runs in row pieces of at most HEAD_ROWS rows, so the fp32 logits of a piece ([2048, 16384]: 128 MB) are the largest fp32
tensor; the bf16 gradient of all logits is held whole for the head's two gradient GEMMs.

Parameters live in a dict keyed by the reference's state-dict names, fp32 masters in the native layouts (`params_from_state_dict`:
proj_out.weight [V, C]; everything else as in the state dict, positional_encoding [C, L]); `grads_to_state_dict_layout` maps back.
No EMA and no dropout (the shipped configs train with dropout 0.0); the LambdaLR scheduler is the caller's (`lr=`)."""
import torch

from . import training as T
from .training_unet import TrainState, _as_params, _attn_names, _gather, _scatter, apply_gradients

HEAD_ROWS = 2048
BETAS = (0.9, 0.95)              # transformer.py:106-107: AdamW(betas=(0.9, 0.95)), torch's eps and weight_decay, over all parameters


def params_from_state_dict(sd, device):
    """reference state dict of `transformer.*` (fp32, PyTorch layouts) -> native-layout fp32 masters on `device`."""
    out = {}
    for k, v in sd.items():
        v = torch.as_tensor(v).detach().float()
        if k == "proj_out.weight":
            v = v.reshape(v.shape[0], v.shape[1])
        out[k] = v.contiguous().to(device).clone()
    return out


def grads_to_state_dict_layout(grads, shapes):
    """native-layout gradients -> the shapes of the reference's state dict (`shapes`: name -> shape or tensor)."""
    out = {}
    for k, g in grads.items():
        ref = shapes[k]
        out[k] = g.float().reshape(tuple(ref.shape) if hasattr(ref, "shape") else tuple(ref))
    return out


def state_dict_from_params(P, shapes):
    """native-layout masters -> host tensors in the reference's state-dict layouts."""
    return {k: v.detach().float().cpu().reshape(tuple(shapes[k].shape) if hasattr(shapes[k], "shape") else tuple(shapes[k])).contiguous()
            for k, v in P.items()}


def _block_names(i):
    tb = f"transformer_blocks.{i}"
    return {"attn1": _attn_names(tb, "attn1", 1), "attn2": _attn_names(tb, "attn2", 2),
            "ff": {"ln_g": tb + ".norm3.weight", "ln_b": tb + ".norm3.bias", "w1": tb + ".ff.net.0.proj.weight", "b1": tb + ".ff.net.0.proj.bias",
                   "w2": tb + ".ff.net.2.weight", "b2": tb + ".ff.net.2.bias"}}


def _pad_cols(t, mult=64):
    """[M, K] -> [M, ceil(K / mult) * mult] with zero columns (a GEMM's contraction length is a multiple of 64)."""
    k = t.shape[1]
    kp = (k + mult - 1) // mult * mult
    if kp == k:
        return t
    out = torch.zeros((t.shape[0], kp), device=t.device, dtype=t.dtype)
    out[:, :k] = t
    return out


def rarm_train_forward(ctx, P, spec, tokens, context):
    """tokens int64 [b, t] (t <= sequence_length), context [b, k, context_dim] -> (x bf16 [b, t, C]: the input of the head, tape)."""
    P = _as_params(P)
    b, t = tokens.shape
    C, heads = spec.n_heads * spec.d_head, spec.n_heads
    if spec.d_head != 64 or t < 1 or t > min(1024, spec.sequence_length):
        raise NotImplementedError(f"rarm training: d_head 64 and 1 <= t <= min(1024, sequence_length) (d_head {spec.d_head}, t {t})")
    dev = P["proj_in.weight"].device
    tok = tokens.to(dev).long().contiguous()
    ctx._check_ids("rarm_train_forward", tok, spec.vocab_in, "tokens")
    x = (P["proj_in.weight"][tok] + P["positional_encoding"][:, :t].t()[None]).to(torch.bfloat16)      # attention.py:252-258
    cb = context.to(device=dev, dtype=torch.bfloat16).contiguous()
    tape = {"tokens": tok, "context": cb, "blocks": []}
    for i in range(spec.depth):
        p = _gather(P, _block_names(i), heads=heads)
        x1, s1 = T.attn_block_forward(ctx, p["attn1"], x, causal=True)
        x2, s2 = T.attn_block_forward(ctx, p["attn2"], x1, cb)
        x3, s3 = T.ff_forward(ctx, p["ff"], x2.reshape(b * t, C))
        tape["blocks"].append((p, x, {"x1": x1, "x2": x2, "attn1": s1, "attn2": s2, "ff": s3}))
        x = x3.reshape(b, t, C)
    tape["x_out"] = x
    return x, tape


def rarm_head_loss(ctx, P, spec, x, targets):
    """proj_out + the mean cross-entropy (transformer.py:46-48) in row pieces: x bf16 [b, t, C], targets int64 [b, t] ->
    (loss, dlogits bf16 [b t, V] = (softmax - onehot) / (b t), nll f32 [b, t])."""
    P = _as_params(P)
    b, t, C = x.shape
    M, V = b * t, spec.vocab_out
    xf = x.reshape(M, C)
    tg = targets.to(x.device).long().reshape(M).contiguous()
    w, bias = P.w("proj_out.weight"), P["proj_out.bias"]
    dlogits = torch.empty((M, V), device=x.device, dtype=torch.bfloat16)
    nll = torch.empty((M,), device=x.device, dtype=torch.float32)
    for r0 in range(0, M, HEAD_ROWS):
        r1 = min(M, r0 + HEAD_ROWS)
        logits = ctx.op_linear(xf[r0:r1], w, bias, out_f32=True)
        ctx.op_rarm_nll_bwd(logits, tg[r0:r1], 1.0 / M, out=dlogits[r0:r1], nll_out=nll[r0:r1])
    return float(nll.mean()), dlogits, nll.reshape(b, t)


def rarm_train_backward(ctx, P, spec, tape, dlogits):
    """dlogits bf16 [b t, V] -> {state-dict name: fp32 gradient in the native layout} for every parameter."""
    P = _as_params(P)
    x = tape["x_out"]
    b, t, C = x.shape
    grads = {}
    w = P.w("proj_out.weight")
    grads["proj_out.weight"] = ctx.op_linear_wgrad(dlogits, x.reshape(b * t, C))
    grads["proj_out.bias"] = ctx.op_colsum(dlogits)
    d = ctx.op_linear(_pad_cols(dlogits), _pad_cols(ctx.op_transpose(w))).reshape(b, t, C)
    for i in range(spec.depth - 1, -1, -1):
        p, xin, saved = tape["blocks"][i]
        g = T.transformer_block_backward(ctx, p, xin, tape["context"], saved, d)
        _scatter(grads, {"attn1": g["attn1"], "attn2": g["attn2"], "ff": g["ff"]}, _block_names(i))
        d = g["x"]
    dflat = d.reshape(b * t, C).contiguous()
    grads["proj_in.weight"] = ctx.op_embedding_grad(tape["tokens"].reshape(-1), dflat, spec.vocab_in)
    dpos = ctx.op_colsum(d.reshape(b, t * C)).reshape(t, C)                                      # the batch sum per (position, channel)
    gp = torch.zeros((C, spec.sequence_length), device=d.device, dtype=torch.float32)             # positions >= t saw no token
    gp[:, :t] = dpos.t()
    grads["positional_encoding"] = gp
    return grads


def rarm_loss_and_grads(ctx, P, spec, tokens, targets, context):
    """-> (mean cross-entropy, gradients in the native layout, per-token nll f32 [b, t])."""
    x, tape = rarm_train_forward(ctx, P, spec, tokens, context)
    loss, dlogits, nll = rarm_head_loss(ctx, P, spec, x, targets)
    return loss, rarm_train_backward(ctx, P, spec, tape, dlogits), nll


def rarm_training_step(ctx, state, spec, tokens, targets, context, lr=1e-4, betas=BETAS, eps=1e-8, weight_decay=1e-2):
    """One optimisation step on a TrainState (fp32 masters and moments, bf16 working copies refreshed by the optimiser kernel): forward,
    loss, backward, AdamW over ALL parameters (norms, biases, embedding and position table included, as the reference's single
    parameter group).  -> loss before the update."""
    loss, grads, _ = rarm_loss_and_grads(ctx, state.params(), spec, tokens, targets, context)
    apply_gradients(ctx, state, grads, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    return loss
