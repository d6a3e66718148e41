"""Float64 restatements, per-element bounds and near misses of the two kernels of the RARM whole-sequence pass -- the causal d_head-64
attention (csrc/attention.hip: causal_d64_kernel) and the token NLL (csrc/rarm.hip: rarm_nll_kernel) -- and the reference values of the
pass itself, formed from the committed goldens of the reference's RetrievalPatchTransformer.  Shared by tests/test_gpu_rarm_seq.py (the
HIP kernels through the C ABI) and tests/test_rarm_seq_cpu.py (fp32 torch restatements standing in for them).  Same CASE contract as
tests/_fwd_ref.py: `make / ref / bound / misses`, held together by _train_ref.check()."""
import numpy as np
import torch

import _fwd_ref as R
from _train_ref import BF, F64, bfr


# ============================================================================================================ causal attention, d_head 64
class CausalAttention:
    """causal_d64_kernel: flash_d32's arithmetic at d_head 64 with a causal tile walk.  Operands as SmallAttention.make at D = 64, scale
    64^-0.5.  Bound: r = 2^-8 (bf16 output), a = _attn_bound with the bf16-P term and the causal mask.  Near misses: the diagonal masked
    (a query does not see itself), one key ahead visible, no mask at all, the scale applied twice, the head order reversed, k and v
    swapped.  (At n = 1 the mask and scale misses other than the first coincide with the reference; check() drops those.)"""
    name = "causal_attention_d64"
    exact = False
    D = 64
    SCALE = 64 ** -0.5

    @staticmethod
    def make(B, n, H, seed=93):
        return R.SmallAttention.make(B, n, n, H, 64, causal=1, seed=seed)

    @staticmethod
    def ref(inp, dt, scale=None, swap=False, reverse=False, diagonal=1, pb=False):
        """diagonal: keys j >= i + diagonal are masked (1: causal; 0: the diagonal too; 2: one key ahead visible; None: no mask).
        pb: the unnormalised probabilities are rounded to bf16 for the PV product, the normaliser is their unrounded sum (the kernel)."""
        k, v = (inp["v"], inp["k"]) if swap else (inp["k"], inp["v"])
        H, D = inp["H"], 64
        s = R._heads(inp["q"].to(dt), H, D) @ R._heads(k.to(dt), H, D).transpose(-1, -2) * (CausalAttention.SCALE if scale is None else scale)
        if diagonal is not None:
            s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(diagonal), float("-inf"))
        vh = R._heads(v.to(dt), H, D)
        if pb:
            p = torch.exp(s - s.max(-1, keepdim=True).values)
            o = (bfr(p.float()).to(dt) @ vh) / p.sum(-1, keepdim=True)
        else:
            o = torch.nan_to_num(torch.softmax(s, -1)) @ vh
        o = R._unheads(o)
        if reverse:
            o = R._unheads(R._heads(o, H, D).flip(1))
        return {"out": o}

    @staticmethod
    def bound(inp, ref):
        return {"out": (BF, R._attn_bound(inp["q"], inp["k"], inp["v"], inp["H"], 64, CausalAttention.SCALE, True, True))}

    @staticmethod
    def misses(inp):
        f = CausalAttention.ref
        return [("diagonal masked", f(inp, F64, diagonal=0)), ("one key ahead visible", f(inp, F64, diagonal=2)), ("no mask", f(inp, F64, diagonal=None)),
                ("scale applied twice", f(inp, F64, scale=CausalAttention.SCALE ** 2)), ("heads reversed", f(inp, F64, reverse=True)),
                ("k and v swapped", f(inp, F64, swap=True))]

    @staticmethod
    def standin(inp):
        """fp32 arithmetic, P rounded to bf16, the output rounded to bf16"""
        return {"out": bfr(CausalAttention.ref(inp, torch.float32, pb=True)["out"])}


# (B, n, H): single token | the tiny golden's t | exactly one tile | one row into the second tile | ragged last tile, odd head count |
# sos + 128 kept codes at the shipped head count | the shipped sequence
CAUSAL_SHAPES = [(3, 1, 2), (3, 12, 2), (2, 32, 2), (2, 33, 2), (2, 95, 3), (2, 129, 12), (1, 256, 12)]


def qkv_of(inp):
    """the fused projection layout the kernel reads: [B, n, q | k | v]"""
    return torch.cat([inp["q"], inp["k"], inp["v"]], -1)


# ============================================================================================================ token NLL
class Nll:
    """rarm_nll_kernel: nll = logsumexp(row) - row[target], all fp32.  Rows: N(0, s) for s in {1, 3, 12} in turn; row 3 is dominated by
    one logit 60 above the rest, row 4 is constant; targets include 0 and V - 1.  Bound per element (fp32 output: r = 0):
    a = 2^-21 (4 + max |row| + |nll64|) -- a few fp32 roundings of the maximum-shifted exponentials' sum, of the logarithm and of the
    two differences, whose operands are at most max |row| and |nll|.  Near miss: the logit of target + 1."""
    name = "rarm_nll"
    exact = False

    @staticmethod
    def make(rows, V, seed=97):
        g = torch.Generator().manual_seed(seed)
        s = torch.tensor([1.0, 3.0, 12.0])[torch.arange(rows) % 3]
        lg = torch.randn(rows, V, generator=g) * s[:, None]
        lg[3] = torch.randn(V, generator=g); lg[3, V // 3] = lg[3].max() + 60.0
        lg[4] = 1.25
        tg = torch.randint(0, V, (rows,), generator=g)
        tg[0] = 0; tg[1] = V - 1; tg[3] = V // 3; tg[5] = (V // 3) % V
        return {"logits": lg.contiguous(), "targets": tg}

    @staticmethod
    def ref(inp, dt, shift=0):
        lg = inp["logits"].to(dt)
        tg = (inp["targets"] + shift) % lg.shape[1]
        return {"nll": torch.logsumexp(lg, -1) - lg.gather(1, tg[:, None])[:, 0]}

    @staticmethod
    def bound(inp, ref):
        return {"nll": (0.0, 2.0 ** -21 * (4 + inp["logits"].double().abs().max(-1).values + ref["nll"].double().abs()))}

    @staticmethod
    def misses(inp):
        return [("target + 1", Nll.ref(inp, F64, shift=1))]

    @staticmethod
    def standin(inp):
        return Nll.ref(inp, torch.float32)


NLL_SHAPES = [(64, 1000), (64, 4096), (64, 16384)]


# ============================================================================================================ the pass: reference NLL values
def nll64(logits, targets):
    """fp64 logsumexp(logits) - logits[target] over the last axis"""
    lg = torch.as_tensor(logits).double()
    tg = torch.as_tensor(targets).long()
    return torch.logsumexp(lg, -1) - lg.gather(-1, tg[..., None])[..., 0]


def logit_rms(logits):
    return torch.as_tensor(logits).double().pow(2).mean(-1).sqrt()


def tiny_nll_targets(g, vocab):
    """rarm_tiny.npz: the next tokens where they exist (positions 0 .. t-2), seeded random codes for the last position"""
    tok = torch.from_numpy(g["tokens"])
    last = torch.from_numpy(np.random.default_rng(101).integers(0, vocab, (tok.shape[0], 1)))
    return torch.cat([tok[:, 1:], last], 1)


def deep_nll_targets(g, vocab):
    """rarm_shipped_deep.npz: a full [2, 256] target matrix -- the next tokens, seeded random codes at the last position"""
    tok = torch.from_numpy(g["tokens"])
    last = torch.from_numpy(np.random.default_rng(102).integers(0, vocab, (tok.shape[0], 1)))
    return torch.cat([tok[:, 1:], last], 1).clamp_(0, vocab - 1)
