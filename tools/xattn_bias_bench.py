#!/usr/bin/env python3
"""What the neighbour bias costs in the fused cross-attention kernels, through the op entries at the shipped levels: (rows per sample, C)
= (1024, 384), (256, 768), (64, 960), k = 4, B' = 64 samples, in the LN + norm3 form (what a guided forward launches on its conditional
rows) and in the plain form on LayerNorm'd rows.  Per level and form, microseconds per launch of
  * the unbiased entry (rdm_op_xattn_fused / _ln3), measured twice per round -- first and last: their difference is the A/A spread,
  * rdm_op_xattn_fused_biased with a zero bias,
  * rdm_op_xattn_fused_biased with half the neighbours masked ([0, 0, -inf, -inf]),
the variants alternating over `rounds` rounds of `reps` launches; the figure is the median over the rounds of a round's mean.  Only the
fused kernel's launch is timed (the library's HIP-event profiler brackets it; the G / U packing of the op entry is outside).  The box's
calibration probe is printed on every line.

usage: xattn_bias_bench.py [rounds [reps]]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rdm_amd  # noqa: F401
from rdm_amd import _lib

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, K, NP = 64, 4, 128
ctx = _lib.Context(0)
d = ctx.device
tf, gb = ctx.calib_probe()
cal = f"[mfma probe {tf:.1f} TFLOP/s, hbm stream {gb:.1f} GB/s]"
g = torch.Generator(device=d).manual_seed(11)
rnd = lambda *s, scale=1.0: (torch.randn(s, device=d, generator=g) * scale)
out = {"B": B, "k": K, "rounds": rounds, "reps": reps, "calibration": {"mfma_probe_tflops": round(tf, 1), "hbm_stream_gbps": round(gb, 1)}, "us": {}}

for n, Cc in ((1024, 384), (256, 768), (64, 960)):
    heads = Cc // 32
    ncols = heads * K
    G = torch.zeros(B, NP, Cc, device=d); G[:, :ncols] = rnd(B, ncols, Cc, scale=4.0 / Cc ** 0.5)
    U = torch.zeros(B, Cc, NP, device=d); U[:, :, :ncols] = rnd(B, Cc, ncols)
    G, U = G.bfloat16().contiguous(), U.bfloat16().contiguous()
    x = (rnd(B, n, Cc, scale=1.7)).bfloat16().contiguous()
    res = rnd(B, n, Cc).bfloat16().contiguous()
    bias, ga, be, g3, b3 = rnd(Cc), 1 + 0.1 * rnd(Cc), 0.1 * rnd(Cc), 1 + 0.1 * rnd(Cc), 0.1 * rnd(Cc)
    zero = torch.zeros(B, K, device=d)
    half = torch.tensor([0.0, 0.0, float("-inf"), float("-inf")], device=d).repeat(B, 1).contiguous()
    forms = {
        "ln+norm3": lambda kb: ctx.op_xattn_fused_ln3(x.clone(), G, U, bias, ncols, K, ln=(ga, be, 1e-5), ln3=(g3, b3), key_bias=kb),
        "plain": lambda kb: ctx.op_xattn_fused(x, G, U, bias, res, ncols, K, key_bias=kb),
    }
    for form, call in forms.items():
        variants = [("unbiased", None), ("zero bias", zero), ("half masked", half), ("unbiased again", None)]
        for _, kb in variants:                       # warm-up: code objects, the per-device attribute calls
            call(kb)
        torch.cuda.synchronize()
        per = {name: [] for name, _ in variants}
        for _ in range(rounds):
            for name, kb in variants:
                ctx.prof_reset()
                ctx.prof_enable((_lib.PROF_LINEAR,))
                for _ in range(reps):
                    call(kb)
                torch.cuda.synchronize()
                cnt, ms, _ = ctx.prof_collect(_lib.PROF_LINEAR)
                ctx.prof_enable(())
                assert cnt == reps, (cnt, reps)
                per[name].append(ms / cnt * 1e3)
        med = {name: statistics.median(v) for name, v in per.items()}
        spread = abs(med["unbiased again"] - med["unbiased"])
        line = ", ".join(f"{name} {med[name]:.2f}" for name, _ in variants)
        worst = max(med["zero bias"], med["half masked"]) - min(med["unbiased"], med["unbiased again"])
        verdict = "within the A/A spread" if worst <= spread else f"{worst:.2f} us above the faster unbiased run (A/A spread {spread:.2f} us)"
        print(f"n={n} C={Cc} heads={heads} {form}: us per launch: {line}; biased: {verdict} {cal}", flush=True)
        out["us"][f"n{n} C{Cc} {form}"] = {name: round(v, 3) for name, v in med.items()}
print(json.dumps(out))
