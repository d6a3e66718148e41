"""The neighbour bias (include/rdm_hip.h rdm_set_neighbour_bias) restated: float64 references, per-element bounds and near misses of the
two biased kernels in the style of tests/_fwd_ref.py, and the fp32 oracle's cross-attention with the bias, for the model-level tests
(oracle.unet.cross_attention is replaced for the duration of a test; basic_transformer_block calls it through the module global).

Bounds: XattnFused's and SmallAttention's, extended by the one fp32 addition the bias costs: u (|S| + |bias|) on the score of every kept
column.  A masked column (-inf) has probability exactly 0 and contributes exactly 0 to the reference, to the bound and to the kernel."""
import math

import torch
import torch.nn.functional as F

import _fwd_ref as R
from _train_ref import BF, F64, U, _cdiv, bfr

NEG = float("-inf")


# ------------------------------------------------------------------------------------------------ bias rows
def bias_rows(pattern, k, seed):
    """One row [k] of the named pattern: 'finite' (values in [-3, 3]), 'first' (neighbour 0 masked, the rest finite), 'one' (all but one
    masked: probabilities exactly 1 and 0), 'zero'."""
    g = torch.Generator().manual_seed(seed)
    row = torch.rand(k, generator=g) * 6 - 3
    if pattern == "zero":
        return torch.zeros(k)
    if pattern == "first" and k > 1:
        row[0] = NEG
    elif pattern == "one" and k > 1:
        keep = int(torch.randint(0, k, (1,), generator=g))
        row = torch.where(torch.arange(k) == keep, row, torch.full((k,), NEG))
    return row


def make_bias(patterns, k, seed=1):
    """[B, k]: one pattern name per sample"""
    return torch.stack([bias_rows(p, k, seed + 17 * i) for i, p in enumerate(patterns)])


def _finite(t):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


# ------------------------------------------------------------------------------------------------ fused cross-attention
class XattnFusedBiased:
    """R.XattnFused with key_bias [B, k] added to the score columns h k + j before the group softmax (xattn_fused_kernel<NB, true> /
    xattn_ln_fused_kernel<NB, true>).  e_S gains u (|S| + |bias|) on kept columns; masked columns carry no error and no probability.
    Near misses: the bias dropped; the next sample's row; the bias indexed by head instead of by neighbour; the weights exp(bias)
    applied after the softmax without renormalising; -inf treated as 0."""
    name = "xattn_fused_biased"
    exact = False

    @staticmethod
    def make(B, n, heads, k, patterns, ln=False, seed=101, bias_seed=1):
        inp = R.XattnFused.make(B, n, heads, k, ln=ln, seed=seed)
        inp["key_bias"] = make_bias(patterns, k, bias_seed)
        return inp

    @staticmethod
    def scores(inp, dt):
        nc = inp["ncols"]
        return R.XattnFused.xn(inp, dt) @ inp["G"][:, :nc].to(dt).transpose(1, 2)

    @staticmethod
    def cols(inp, kb, dt):
        """[B, 1, ncols]: the bias of column h k + j is kb[b][j]"""
        return kb.to(dt).repeat(1, inp["heads"])[:, None, :]

    @staticmethod
    def probs(inp, dt, mode=None):
        k, nc, H = inp["k"], inp["ncols"], inp["heads"]
        kb = inp["key_bias"]
        s = XattnFusedBiased.scores(inp, dt)
        B, n, _ = s.shape
        sm = lambda t: torch.softmax(t.reshape(B, n, nc // k, k), -1).reshape(B, n, nc)
        if mode == "dropped":
            return sm(s)
        if mode == "next sample":
            return sm(s + XattnFusedBiased.cols(inp, kb.roll(-1, 0), dt))
        if mode == "by head":                    # column h k + j takes entry h mod k
            byh = torch.stack([kb[:, h % k] for h in range(H)], 1).repeat_interleave(k, 1)
            return torch.nan_to_num(sm(s + byh.to(dt)[:, None, :]))        # (a head whose whole group is masked: no probability at all)
        if mode == "after softmax":
            return sm(s) * torch.exp(XattnFusedBiased.cols(inp, kb, dt))
        if mode == "-inf as 0":
            return sm(s + XattnFusedBiased.cols(inp, _finite(kb), dt))
        return sm(s + XattnFusedBiased.cols(inp, kb, dt))

    @staticmethod
    def ref(inp, dt, mode=None):
        o = XattnFusedBiased.probs(inp, dt, mode) @ inp["U"][:, :, : inp["ncols"]].to(dt).transpose(1, 2)
        if inp["bias"] is not None:
            o = o + inp["bias"].to(dt)
        if inp["ln"]:
            o = o + inp["x"].to(dt)
        elif inp["res"] is not None:
            o = o + inp["res"].to(dt)
        return {"out": o}

    @staticmethod
    def bound(inp, ref):
        nc, k, C = inp["ncols"], inp["k"], inp["x"].shape[2]
        G, Um = inp["G"][:, :nc].double(), inp["U"][:, :, :nc].double()
        xn = R.XattnFused.xn(inp, F64)
        e_S = (C + 4) * U * (xn.abs() @ G.abs().transpose(1, 2))
        if inp["ln"]:
            x = inp["x"].double()
            d = _cdiv(C, 64) + 14
            mean = x.mean(-1, keepdim=True); rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + inp["eps"])
            e_xn = 2.0 ** -9 * xn.abs() + inp["gamma"].double().abs() * U * (d * x.abs().mean(-1, keepdim=True) * rstd + (d + 8) * ((x - mean) * rstd).abs())
            e_S = e_S + e_xn @ G.abs().transpose(1, 2)
        S = xn @ G.transpose(1, 2)
        B, n, _ = S.shape
        kbc = XattnFusedBiased.cols(inp, inp["key_bias"], F64).expand(B, n, nc)
        kept = torch.isfinite(kbc)
        Sb = torch.where(kept, S + _finite(kbc), torch.zeros_like(S))                      # the biased score of a kept column
        e_S = torch.where(kept, e_S + U * (S.abs() + _finite(kbc).abs()), torch.zeros_like(e_S))     # the one addition
        P = XattnFusedBiased.probs(inp, F64)
        assert bool((P[~kept] == 0).all()), "a masked column has probability exactly 0"
        e_Sg = e_S.reshape(B, n, nc // k, k).amax(-1, keepdim=True).expand(B, n, nc // k, k).reshape(B, n, nc)
        e_P = P * (BF + 2.0 ** -22 * (4 + Sb.abs()) + 2 * e_Sg + k * U)
        tot = P @ Um.abs().transpose(1, 2)
        if inp["bias"] is not None:
            tot = tot + inp["bias"].double().abs()
        if inp["ln"]:
            tot = tot + inp["x"].double().abs()
        elif inp["res"] is not None:
            tot = tot + inp["res"].double().abs()
        return {"out": (BF, e_P @ Um.abs().transpose(1, 2) + (nc + 4) * U * tot)}

    @staticmethod
    def misses(inp):
        return [(m, XattnFusedBiased.ref(inp, F64, m)) for m in ("dropped", "next sample", "by head", "after softmax", "-inf as 0")]


# ------------------------------------------------------------------------------------------------ small attention
class SmallAttentionBiased:
    """R.SmallAttention (not causal) with key_bias [B, nkv] added to every head's scaled score of key j (small_attention_kernel<D, true>:
    masked keys are skipped).  e_P gains u (|scale S| + |bias|) per kept key.  Near misses: the bias dropped; the next sample's row; -inf
    treated as 0; the weights applied after the softmax without renormalising; and beyond one LDS chunk: the keys beyond the first chunk
    dropped, the last chunk alone."""
    name = "small_attention_biased"
    exact = False

    @staticmethod
    def make(B, nq, nkv, H, D, masked, seed=91, bias_seed=3):
        """masked: per sample, the list of masked key indices"""
        inp = R.SmallAttention.make(B, nq, nkv, H, D, seed=seed)
        g = torch.Generator().manual_seed(bias_seed)
        kb = torch.rand(B, nkv, generator=g) * 6 - 3
        for b, idx in enumerate(masked):
            kb[b, list(idx)] = NEG
        inp["key_bias"] = kb
        return inp

    @staticmethod
    def ref(inp, dt, mode=None, keys=None):
        H, D, kb = inp["H"], inp["D"], inp["key_bias"]
        s = R._heads(inp["q"].to(dt), H, D) @ R._heads(inp["k"].to(dt), H, D).transpose(-1, -2) * inp["scale"]
        vh = R._heads(inp["v"].to(dt), H, D)
        col = lambda t: t.to(dt)[:, None, None, :]
        if mode == "dropped":
            P = torch.softmax(s, -1)
        elif mode == "next sample":
            P = torch.softmax(s + col(kb.roll(-1, 0)), -1)
        elif mode == "-inf as 0":
            P = torch.softmax(s + col(_finite(kb)), -1)
        elif mode == "after softmax":
            P = torch.softmax(s, -1) * torch.exp(col(kb))
        else:
            sb = s + col(kb)
            if keys is not None:
                sb = sb.clone(); sb[..., : keys[0]] = NEG; sb[..., keys[1]:] = NEG
            P = torch.nan_to_num(torch.softmax(sb, -1))
        return {"out": R._unheads(P @ vh)}

    @staticmethod
    def bound(inp, ref):
        H, D, scale, kb = inp["H"], inp["D"], inp["scale"], inp["key_bias"].double()
        qh, kh, vh = (R._heads(t.double(), H, D) for t in (inp["q"], inp["k"], inp["v"]))
        m = kh.shape[2]
        S = qh @ kh.transpose(-1, -2)
        kbc = kb[:, None, None, :].expand_as(S)
        kept = torch.isfinite(kbc)
        sb = torch.where(kept, S * scale + _finite(kbc), torch.zeros_like(S))
        P = torch.softmax(S * scale + kbc, -1)
        assert bool((P[~kept] == 0).all())
        e_P = P * (2.0 ** -22 * (4 + sb.abs()) + 2 * D * U * scale * (qh.abs() @ kh.abs().transpose(-1, -2)) + m * U
                   + U * ((S * scale).abs() + _finite(kbc).abs()))
        o = P @ vh
        return {"out": (BF, R._unheads(e_P @ vh.abs() + (m + 4) * U * (P @ vh.abs()) + 4 * U * o.abs()))}

    @staticmethod
    def misses(inp):
        m = [(l, SmallAttentionBiased.ref(inp, F64, l)) for l in ("dropped", "next sample", "-inf as 0", "after softmax")]
        nkv = inp["k"].shape[1]
        kc = R.small_attention_chunk(nkv, inp["D"])
        if nkv > kc:
            m += [("keys beyond the first chunk dropped", SmallAttentionBiased.ref(inp, F64, keys=(0, kc))),
                  ("the last chunk alone", SmallAttentionBiased.ref(inp, F64, keys=((nkv - 1) // kc * kc, nkv)))]
        return m


# ------------------------------------------------------------------------------------------------ the oracle's cross-attention, biased
def biased_cross_attention(bias):
    """oracle.unet.cross_attention with bias [rows, k] added to every head's score of neighbour j of sample b < rows, after the 1 / sqrt(d)
    scale and before the softmax; samples >= rows (the unconditional half of a guided batch) and self-attention are untouched."""
    bias = torch.as_tensor(bias, dtype=torch.float32)

    def cross_attention(sd, pre, x, context, heads):
        q = F.linear(x, sd[pre + ".to_q.weight"])
        ctx = x if context is None else context
        k = F.linear(ctx, sd[pre + ".to_k.weight"])
        v = F.linear(ctx, sd[pre + ".to_v.weight"])
        B, n, C = q.shape
        d = C // heads
        split = lambda t: t.reshape(B, t.shape[1], heads, d).permute(0, 2, 1, 3)
        q, k, v = split(q), split(k), split(v)
        sim = torch.einsum("bhid,bhjd->bhij", q, k) * d ** -0.5
        if context is not None:
            assert bias.shape[1] == context.shape[1] and bias.shape[0] <= B
            full = torch.zeros(B, bias.shape[1], dtype=sim.dtype)
            full[: bias.shape[0]] = bias.to(sim.dtype)
            sim = sim + full[:, None, None, :]
        out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), v)
        out = out.permute(0, 2, 1, 3).reshape(B, n, C)
        return F.linear(out, sd[pre + ".to_out.0.weight"], sd[pre + ".to_out.0.bias"])
    return cross_attention


MASK_ROWS = [[0.0, 0.0, NEG, NEG], [NEG, 0.0, 0.0, 0.0]]             # the issue's mask: two of four neighbours, then the first one
WEIGHT_ROWS = [[math.log(w) for w in (4.0, 1.0, 1.0, 0.25)]] * 2   # the issue's weights [4, 1, 1, 1/4]
