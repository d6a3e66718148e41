#!/usr/bin/env python3
"""The first stage's AttnBlock attention through the C ABI: the streaming kernel (rdm_op_vq_attention, csrc/vq_attn.hip) against the
materialised chain it replaces beyond 4096 tokens (V^T transpose, rdm_op_bmm with alpha -> rdm_op_softmax -> rdm_op_bmm) at
(B, n, C) = (64, 4096, 512), (8, 9216, 512), (4, 16384, 512), the streaming kernel alone at (1, 65536, 512) -- the chain cannot index
that size -- and the whole VQ-f4 decode of 512 x 512 and 1024 x 1024 images at B = 4 on the shipped synthetic first stage.
Prints one line per measurement, the box's calibration probe first, and one JSON line at the end.

    python tools/vq_attn_bench.py [--no-decode] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()

    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, synthetic
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion

    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    d = ctx.device
    tf, gb = ctx.calib_probe()
    print(f"calibration: mfma probe {tf:.1f} TFLOP/s, hbm stream {gb:.1f} GB/s", flush=True)
    res = {"calibration": {"mfma_probe_tflops": round(tf, 1), "hbm_stream_gbps": round(gb, 1)}, "op": [], "decode": []}
    g = torch.Generator(device=d).manual_seed(0)
    for B, n, C, chain in ((64, 4096, 512, True), (8, 9216, 512, True), (4, 16384, 512, True), (1, 65536, 512, False)):
        q, k, v = (torch.randn(B, n, C, device=d, generator=g).mul_(s).bfloat16() for s in (1.0, 2.0, 1.0))
        reps = max(2, a.reps if B * n * n <= 2 ** 31 else a.reps // 2)
        ts, out = timed(lambda: ctx.op_vq_attention(q, k, v), reps)      # no bias_v: the chain below has none either (the executor folds it into the P.V epilogue)
        row = {"B": B, "n": n, "C": C, "stream_ms": round(ts * 1e3, 3), "stream_tflops": round(6.0 * B * n * n * C / ts / 1e12, 1)}
        line = f"vq attention B={B} n={n} C={C}: streaming {ts * 1e3:9.3f} ms ({row['stream_tflops']:6.1f} TFLOP/s over its 3 products)"
        if chain:
            def run_chain():
                s = ctx.op_bmm(q, k, alpha=C ** -0.5, out_f32=True)
                p = ctx.op_softmax(s)
                del s
                return ctx.op_bmm(p, ctx.op_transpose_batched(v))
            tc, ref = timed(run_chain, reps)
            diff = float((out.float() - ref.float()).norm() / ref.float().norm())
            row.update(chain_ms=round(tc * 1e3, 3), chain_tflops=round(4.0 * B * n * n * C / tc / 1e12, 1), rel_l2=diff)
            line += f"; chain {tc * 1e3:9.3f} ms ({row['chain_tflops']:6.1f} TFLOP/s over its 2, {6.0 * B * n * n / 1e9:.1f} GB of scores); streaming / chain {ts / tc:.2f}; rel L2 {diff:.1e}"
            del ref
        print(line, flush=True)
        res["op"].append(row)
        del q, k, v, out
        torch.cuda.empty_cache()
    if not a.no_decode:
        model = MinimalRETRODiffusion(unet_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, k_nn=4, ctx=ctx)
        model.load_first_stage_state_dict(synthetic.vq_state_dict(model.vq_cfg))
        f = 1 << (model.vq_cfg.n_ch_mult - 1)
        for H, W in ((512, 512), (1024, 1024)):
            z = torch.randn(4, model.vq_cfg.embed_dim, H // f, W // f, device=d, generator=g)
            t, img = timed(lambda: ctx.vq_decode(z), 2)
            assert tuple(img.shape[2:]) == (H, W) and bool(torch.isfinite(img).all())
            print(f"vq decode of 4 images {H}x{W} (latent {H // f}x{W // f}, AttnBlock over {H // f * (W // f)} pixels): {t * 1e3:9.1f} ms, {t * 1e3 / 4:.1f} ms per image", flush=True)
            res["decode"].append({"H": H, "W": W, "B": 4, "ms": round(t * 1e3, 1)})
            del img
            torch.cuda.empty_cache()
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
