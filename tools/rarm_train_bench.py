#!/usr/bin/env python3
"""One optimisation step of the RARM transformer at the shipped size (18 x 768, vocabulary 16384; synthetic weights), t = 256 tokens,
k = 8 neighbours, at 64 and at 8 sequences:
  (a) ms per step of rdm_amd.training_rarm.rarm_training_step (forward, loss, backward, AdamW): the median of --steps steps after 2 warm-ups;
  (b) the teacher-forced rarm_nll pass on the same batch, in the same run;
  (c) the causal d_head-64 attention backward alone at (64, 256, 12) beside its forward, and from them the backward-to-forward ratio and
      the attention backward's share of a step (18 layers).
Device-event times.  Prints one JSON line and writes it to --json (a run is committed as profiles/rarm_train_bench.json).  GPU box only.
  python tools/rarm_train_bench.py [--batches 64,8] [--steps 5] [--json profiles/rarm_train_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import rdm_amd  # noqa: E402,F401
from rdm_amd import _lib, packing, synthetic, training_rarm  # noqa: E402


def times(fn, reps, warmup=2):
    """per-call device times in ms"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "rarm_train_bench.json"))
    opt = ap.parse_args()
    if opt.steps < 5:
        ap.error("--steps: at least 5 timed steps")
    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    cfg = _lib.make_rarm_cfg()
    sd = synthetic.rarm_state_dict(cfg)
    ctx.load_rarm(cfg, packing.pack("rarm", cfg, sd))
    T, K, H = cfg.sequence_length, 8, cfg.n_heads
    res = {"tool": "rarm_train_bench", "tokens": T, "neighbours": K, "timed_steps": opt.steps, "warmup": 2, "batches": {}}

    # (c) the attention kernels alone
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn((64, T, 3 * H * 64), generator=g).to(ctx.device, torch.bfloat16)
    do = torch.randn((64, T, H * 64), generator=g).to(ctx.device, torch.bfloat16)
    o = ctx.op_causal_attention_d64(qkv, H, 0.125)
    fwd = statistics.median(times(lambda: ctx.op_causal_attention_d64(qkv, H, 0.125), 20))
    bwd = statistics.median(times(lambda: ctx.op_causal_attention_d64_bwd(qkv, o, do, H, 0.125), 20))
    res["causal_attention_64x256x12"] = {"forward_ms": round(fwd, 4), "backward_ms": round(bwd, 4), "backward_to_forward": round(bwd / fwd, 2)}
    del qkv, do, o

    for B in [int(v) for v in opt.batches.split(",")]:
        g = torch.Generator().manual_seed(0)
        codes = torch.randint(0, cfg.vocab_out, (B, T), generator=g)
        tokens = torch.cat([torch.full((B, 1), cfg.vocab_in - 1), codes[:, :-1]], 1).to(ctx.device)
        targets = codes.to(ctx.device)
        context = (torch.randn((B, K, cfg.context_dim), generator=g) * 0.45).to(ctx.device)
        state = training_rarm.TrainState(training_rarm.params_from_state_dict(sd, ctx.device))
        losses = []
        ts = times(lambda: losses.append(training_rarm.rarm_training_step(ctx, state, cfg, tokens, targets, context, lr=1e-4)), opt.steps)
        nll = times(lambda: ctx.rarm_nll(tokens, targets, context), 3, warmup=1)
        step = statistics.median(ts)
        entry = {"step_ms": round(step, 2), "step_ms_all": [round(v, 2) for v in ts], "tokens_per_s": round(B * T / step * 1e3),
                 "rarm_nll_ms": round(statistics.median(nll), 2), "loss_first": round(losses[0], 4), "loss_last": round(losses[-1], 4),
                 "peak_memory_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
        if B == 64:
            entry["attention_backward_share"] = round(cfg.depth * bwd / step, 4)
        res["batches"][str(B)] = entry
        del state
        ctx.release_scratch()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if opt.json:
        with open(opt.json, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
