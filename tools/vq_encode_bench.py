#!/usr/bin/env python3
"""VQGAN-f16 encode to code indices at the shipped size, through the C ABI: `vq_encode_indices` on 64 images (encoder + nearest-code
search) and the nearest-code op alone at M = N = 16384, E = 256 (the search of those 64 images), with its share of the fp32-input
MFMA floor 2 M N E / 155 TF.  Device-event times around calls that end in a synchronise.  GPU box only.
  python tools/vq_encode_bench.py [--images 64] [--reps 5] [--only op|encode]
(kernel times: run it with --only op under `rocprofv3 --kernel-trace --stats`; the op call also holds the |e|^2 and merge kernels)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import rdm_amd  # noqa: E402,F401
from rdm_amd import _lib, packing, synthetic  # noqa: E402

F32_MFMA_PEAK_TF = 155.0          # 64 FLOP/clk/SIMD x 4 SIMDs x 256 CUs x 2.4 GHz


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("op", "encode"), default=None)
    opt = ap.parse_args()
    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    ctx.use_current_stream()
    cfg = _lib.make_vqgan_f16_cfg()
    g = torch.Generator().manual_seed(0)
    if opt.only != "encode":
        M = opt.images * (cfg.resolution >> (cfg.n_ch_mult - 1)) ** 2
        N, E = cfg.n_embed, cfg.embed_dim
        cb = (torch.randn((N, E), generator=g) / E ** 0.5).to(ctx.device)
        z = (torch.randn((M, E), generator=g) / E ** 0.5).to(ctx.device)
        ms, idx = timed(lambda: ctx.vq_nearest_code(z, cb), opt.reps * 4)
        flop = 2.0 * M * N * E
        floor_ms = flop / (F32_MFMA_PEAK_TF * 1e12) * 1e3
        print(f"nearest-code op M={M} N={N} E={E}: {ms:.3f} ms per call = {flop / ms / 1e9:.1f} TFLOP/s, fp32-MFMA floor {floor_ms:.3f} ms "
              f"-> {floor_ms / ms:.3f} of it (checksum {int(idx.long().sum())})")
    if opt.only != "op":
        sd = synthetic.vq_state_dict(cfg, synthetic.VQGAN_SEED); sd.update(synthetic.vq_encoder_state_dict(cfg))
        ctx.load_vq(cfg, packing.pack("vq", cfg, sd)); ctx.load_vq_encoder(cfg, packing.pack("vqenc", cfg, sd))
        x = (torch.rand((opt.images, 3, cfg.resolution, cfg.resolution), generator=g) * 2 - 1).to(ctx.device)
        ms, idx = timed(lambda: ctx.vq_encode_indices(x), opt.reps)
        ms_z, _ = timed(lambda: ctx.vq_encode(x), opt.reps)
        print(f"vq_encode_indices, {opt.images} images: {ms:.2f} ms per call ({ms / opt.images:.3f} ms per image); vq_encode alone {ms_z:.2f} ms "
              f"(checksum {int(idx.sum())})")
    ctx.close()


if __name__ == "__main__":
    main()
