#!/usr/bin/env python3
"""The RARM decode of bench.py --config 5 (shipped architecture, seeded random weights, 8 random neighbours per sequence, top-k 256,
temperature 1, guidance 1) with a nucleus mass, for a per-kernel profile of the top_p < 1 sampler beside the top_p = 1 one:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/rarm_top_p_profile.py --batch 2048 --top_p 0.9

Runs `--warmup` + `--steps` calls of 256 tokens each and prints one JSON line with the synchronised per-token time of the timed calls
and the share of tokens that differ from the top_p = 1 run with the same uniforms.  (bench.py itself has no such flag: its workload is
fixed.)"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=2048)
    p.add_argument("--top_p", type=float, default=0.9)
    p.add_argument("--top_k", type=int, default=256)
    p.add_argument("--tokens", type=int, default=256)
    p.add_argument("--steps", type=int, default=1)
    p.add_argument("--warmup", type=int, default=1)
    a = p.parse_args()
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, packing, synthetic
    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    dev = ctx.device
    rcfg = _lib.make_rarm_cfg()
    ctx.load_rarm(rcfg, packing.pack("rarm", rcfg, synthetic.rarm_state_dict(rcfg)))
    gen = torch.Generator(device=dev).manual_seed(7)
    nbrs = torch.randn((a.batch, 8, rcfg.context_dim), device=dev, generator=gen) * 0.45
    u = torch.rand((a.tokens, a.batch), device=dev, generator=gen).clamp(0.0, 0.99999994)
    sos = torch.full((a.batch, 1), 16385, dtype=torch.long, device=dev)
    kw = dict(temperature=1.0, top_k=a.top_k, guidance_scale=1.0)
    tok = None
    for i in range(a.warmup + a.steps):
        if i == a.warmup:
            torch.cuda.synchronize(); t0 = time.perf_counter()
        tok = ctx.rarm_sample(sos, nbrs, a.tokens, u, top_p=a.top_p, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / max(a.steps, 1)
    plain = ctx.rarm_sample(sos, nbrs, a.tokens, u, **kw)
    print(json.dumps({"batch": a.batch, "top_k": a.top_k, "top_p": a.top_p, "tokens": a.tokens, "us_per_token_step": dt / a.tokens * 1e6,
                      "sequences_per_s": a.batch / dt, "tokens_differing_from_top_p_1": float((tok != plain).float().mean())}))
    ctx.close()


if __name__ == "__main__":
    main()
