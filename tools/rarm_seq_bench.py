#!/usr/bin/env python3
"""The RARM whole-sequence pass at the shipped size (18 x 768, vocabulary 16384; synthetic weights), 64 sequences, k = 8 neighbours:
  (a) rarm_forward (256 decode steps) against rarm_forward_seq (one pass) at t = 256, and their logits' distance;
  (b) image completion behind 8 kept code rows (sos + 128 codes given, 128 sampled) with the prefix fed token by token and with prefill;
  (c) rarm_nll at t = 256.
Device-event times around calls, after warm-up.  Prints one JSON line (a run is committed as profiles/rarm_seq_bench.json, its kernel statistics as profiles/rarm_seq_kernel_stats.csv).  GPU box only.
  python tools/rarm_seq_bench.py [--seqs 64] [--reps 3] [--only forward|seq|prefill|nll] [--json PATH]
(kernel shares: `rocprofv3 --kernel-trace --stats -- python tools/rarm_seq_bench.py --only seq`; causal_d64_kernel is the new attention)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import rdm_amd  # noqa: E402,F401
from rdm_amd import _lib, packing, synthetic  # noqa: E402


def timed(fn, reps, warmup=1):
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
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("forward", "seq", "prefill", "nll"), default=None)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    opt = ap.parse_args()
    torch.set_grad_enabled(False)
    ctx = _lib.Context(0)
    ctx.use_current_stream()
    cfg = _lib.make_rarm_cfg()
    ctx.load_rarm(cfg, packing.pack("rarm", cfg, synthetic.rarm_state_dict(cfg)))
    B, T, K = opt.seqs, cfg.sequence_length, 8
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, cfg.vocab_out, (B, T), generator=g)
    tokens = torch.cat([torch.full((B, 1), cfg.vocab_in - 1), codes[:, :-1]], 1).to(ctx.device)       # [sos | codes][:, :-1]
    targets = codes.to(ctx.device)
    context = (torch.randn((B, K, cfg.context_dim), generator=g) * 0.45).to(ctx.device)
    res = {"tool": "rarm_seq_bench", "sequences": B, "tokens": T, "neighbours": K, "reps": opt.reps}
    want = lambda name: opt.only in (None, name)
    seq_logits = None
    if want("seq"):
        ms, seq_logits = timed(lambda: ctx.rarm_forward_seq(tokens, context), opt.reps)
        res["forward_seq_ms"] = round(ms, 3)
    if want("forward"):
        ms, step_logits = timed(lambda: ctx.rarm_forward(tokens, context), max(1, opt.reps // 3))
        res["forward_stepwise_ms"] = round(ms, 3)
        if seq_logits is not None:
            d = (seq_logits.double() - step_logits.double()).norm() / step_logits.double().norm()
            res["forward_seq_vs_stepwise_rel_l2"] = float(f"{float(d):.3e}")
            res["forward_speedup"] = round(res["forward_stepwise_ms"] / res["forward_seq_ms"], 2)
            res["forward_gate_5x"] = bool(res["forward_speedup"] >= 5.0)
        del step_logits
    del seq_logits
    if want("nll"):
        ms, nll = timed(lambda: ctx.rarm_nll(tokens, targets, context), opt.reps)
        res["nll_ms"] = round(ms, 3); res["nll_mean"] = round(float(nll.mean()), 4)
    if want("prefill"):
        kept = T // 2
        cond = tokens[:, :kept + 1].contiguous()                    # sos + 8 code rows
        u = torch.rand((T - kept, B), generator=g).to(ctx.device)
        kw = dict(temperature=1.0, top_k=256)
        ms0, _ = timed(lambda: ctx.rarm_sample(cond, context, T - kept, u, **kw), opt.reps)
        ms1, _ = timed(lambda: ctx.rarm_sample(cond, context, T - kept, u, prefill=True, **kw), opt.reps)
        res.update(completion_kept_rows=8, completion_stepwise_prefix_ms=round(ms0, 3), completion_prefill_ms=round(ms1, 3),
                   completion_speedup=round(ms0 / ms1, 3), prefill_gate_not_slower=bool(ms1 <= ms0))
    line = json.dumps(res)
    print(line)
    if opt.json:
        with open(opt.json, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
