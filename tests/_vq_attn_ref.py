"""Float64 restatement of the first stage's streaming AttnBlock attention (rdm_op_vq_attention, csrc/vq_attn.hip), its per-element bound
and its near misses, in the CASE contract of tests/_fwd_ref.py (`make` / `ref` / `bound` / `misses`, checked by _train_ref.check).  Shared
by tests/test_gpu_vq_attn.py (the HIP kernel through the C ABI) and tests/test_vq_attn_cpu.py (an fp32 torch restatement of the kernel's
arithmetic standing in for it).

One head of D = C channels: out = softmax(q k^T C^-1/2) v + bias_v.  The bound is SelfAttention's, derived, not measured:
(2^-8, _attn_bound(q, k, v, 1, C, scale, True)) -- b = 2^-8 for the normalised probability rounded to bf16 before the P.V MFMA, the score
and P.V chains in fp32, r = 2^-8 |ref| for the bf16 output (the fp32 add of bias_v is one more rounding of 2^-24 |ref|, far inside r).

Inputs: q, v ~ N(0, 1), k ~ N(0, 2^2), bf16-rounded, bias_v ~ N(0, 1) fp32.  `kmul` = 8 multiplies the keys once more: scale |s| then
reaches tens (the softmax is close to one-hot), and an exponential taken against anything but the exact row maximum can overflow."""
import torch

from _fwd_ref import _attn, _attn_bound
from _train_ref import BF, F64, bfr


def _softmax_pv(q, k, v, scale, dt, pad64=False, tail_out_of_sum=False):
    """softmax(q k^T scale) v with the two padding bugs: pad64 -- the softmax runs over n rounded up to 64 with zero keys (score 0: they take
    probability); tail_out_of_sum -- the normaliser counts the first n - n % 32 keys only (the last key tile's share is left out)"""
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    n = k.shape[1]
    s = q @ k.transpose(1, 2) * scale
    if pad64:
        s = torch.cat([s, torch.zeros(s.shape[0], s.shape[1], -n % 64, dtype=dt)], 2)
    e = torch.exp(s - s.max(2, keepdim=True).values)
    nsum = n - n % 32 if tail_out_of_sum else s.shape[2]
    p = e / e[:, :, :nsum].sum(2, keepdim=True)
    return p[:, :, :n] @ v


class VqAttention:
    """rdm_op_vq_attention: vq_attn_stream_kernel<C / 128>.  Near misses: scale C^-1; k and v swapped; padding keys leaking probability; the
    last key tile left out of the normaliser; bias_v omitted.  (A near miss that coincides with the reference at a shape -- no padding at
    n % 64 == 0, no ragged tile at n % 32 == 0, no bias -- is skipped by check(), as everywhere.)"""
    name = "vq_attention"
    exact = False

    @staticmethod
    def make(B, n, C, kmul=1, bias=True, seed=91):
        g = torch.Generator().manual_seed(seed + n + C)
        q, k, v = (bfr(torch.randn(B, n, C, generator=g) * s) for s in (1.0, 2.0 * kmul, 1.0))
        return {"q": q, "k": k, "v": v, "bias": torch.randn(C, generator=g) if bias else None, "C": C, "kmul": kmul}

    @staticmethod
    def scale(inp):
        return float(inp["C"]) ** -0.5

    @staticmethod
    def ref(inp, dt, scale=None, swap=False, no_bias=False, **bug):
        k, v = (inp["v"], inp["k"]) if swap else (inp["k"], inp["v"])
        sc = VqAttention.scale(inp) if scale is None else scale
        n = k.shape[1]
        bug = {b: on for b, on in bug.items() if on and n % (64 if b == "pad64" else 32)}       # nothing to pad, no ragged tile: the reference itself
        o = _softmax_pv(inp["q"], k, v, sc, dt, **bug) if bug else _attn(inp["q"].to(dt), k.to(dt), v.to(dt), 1, inp["C"], sc)
        if inp["bias"] is not None and not no_bias:
            o = o + inp["bias"].to(dt)
        return {"out": o}

    @staticmethod
    def bound(inp, ref):
        return {"out": (BF, _attn_bound(inp["q"], inp["k"], inp["v"], 1, inp["C"], VqAttention.scale(inp), True))}

    @staticmethod
    def misses(inp):
        m = [("scale C^-1", VqAttention.ref(inp, F64, scale=1.0 / inp["C"])), ("k and v swapped", VqAttention.ref(inp, F64, swap=True)),
             ("last key tile out of the normaliser", VqAttention.ref(inp, F64, tail_out_of_sum=True)), ("bias_v omitted", VqAttention.ref(inp, F64, no_bias=True))]
        # Zero-score padding keys take the share pad / (pad + sum_j e^(s_j)) of a row, and every p shrinks by that factor.  The bound grants each
        # probability a bf16 rounding (2^-8 P), so a share of that order is no different from honest rounding in ANY arithmetic: 27 zero keys
        # among 1061 real ones, or any number of them under row maxima of 30 and more (the keys x 8 case, which stands for the maximum
        # subtraction instead).  The miss is listed where the largest share of a row passes four roundings.
        s = inp["q"].double() @ inp["k"].double().transpose(1, 2) * VqAttention.scale(inp)
        pad = -s.shape[2] % 64
        if pad and float((pad / (pad + torch.exp(s).sum(2))).max()) > 4 * BF:
            m.append(("padding keys leak probability", VqAttention.ref(inp, F64, pad64=True)))
        return m


def kernel_arithmetic(inp):
    """fp32 restatement of the kernel: fp32 scores scaled in fp32, the NORMALISED probability rounded to bf16, fp32 P.V + bias_v, one rounding"""
    q, k, v = inp["q"], inp["k"], inp["v"]
    s = q @ k.transpose(1, 2) * torch.tensor(VqAttention.scale(inp), dtype=torch.float32)
    e = torch.exp(s - s.max(2, keepdim=True).values)
    p = bfr(e * (1.0 / e.sum(2, keepdim=True)))
    o = p @ v
    if inp["bias"] is not None:
        o = o + inp["bias"]
    return {"out": bfr(o)}


# (B, n, C, extra make() arguments, what the shape is for) -- the strided case passes q, k, v as column blocks of one [n, 3C] tensor (GPU test)
CASES = [
    (2, 64, 512, {}, "one tile"),
    (1, 35, 256, {}, "fewer keys than a tile, ragged in both axes"),
    (2, 200, 512, {}, "several key tiles and a ragged tail of 8"),
    (2, 1061, 512, {}, "several query blocks per sample, n odd"),
    (1, 200, 512, {"kmul": 8}, "keys x 8"),
    (1, 200, 256, {"strided": True}, "q k v as column blocks of one n x 3C tensor"),
    (1, 200, 512, {"bias": False}, "no bias_v"),
]


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[4].replace(', ', ' ').replace(' ', '_')}"


def make_case(c):
    kw = {k: v for k, v in c[3].items() if k != "strided"}
    return VqAttention.make(c[0], c[1], c[2], **kw)
