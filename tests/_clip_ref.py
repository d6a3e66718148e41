"""The CLIP towers stage by stage, TEACHER-FORCED: every tensor rdm_debug_tap shows of a tower (include/rdm_hip.h: block 2000 text, 3000
image) is compared with a float64 restatement of ITS op on the tapped tensors in front of it.  GEMMs, LayerNorms and the attention are
held to the per-element bounds of tests/_fwd_ref.py through `check(case, inp, out)` -- the same bound, the same near misses, no other
tolerance -- and the glue stages (embedding adds, gathers, the patch matrix: fp32 adds and pure copies have ONE correct answer) bitwise.
Shared by tests/test_gpu_clip.py (the library's taps) and tests/test_clip_emul_cpu.py (the taps of oracle/clip_emul.py standing in for
them, and of its near-miss towers, which must fail at the stage they break)."""
import torch

import _fwd_ref as R
from _train_ref import bfr, check
from oracle.clip_emul import IMAGE, TEXT, eot_columns, patchify, stage_name


def text_tokens(spec, B, seed=5):
    """B >= 3 token rows [B, L]: every row its own EOT column; row 0's maximum in column 0, row 1's in column L - 1, row 2 holding its
    maximum id twice (columns 7 and 40: the first counts); further rows an EOT at a column of their own"""
    assert B >= 3
    g = torch.Generator().manual_seed(seed)
    L, V = spec.context_length, spec.vocab_size
    t = torch.randint(1, V - 2, (B, L), generator=g)
    t[0, 0] = V - 1
    t[1, L - 1] = V - 1
    t[2, 7] = V - 1; t[2, 40] = V - 1
    for b in range(3, B):
        t[b, 2 + (11 * b) % (L - 4)] = V - 1
    return t


def tap_shapes(spec, tower, B):
    """{(block, sub): (rows, width, dtype)} of every stage of a tower, in execution order"""
    bf, f32 = torch.bfloat16, torch.float32
    if tower == TEXT:
        rows, Wd, layers = B * spec.context_length, spec.transformer_width, spec.transformer_layers
        head = {1: (rows, Wd, f32)}
        tail = {2: (B, Wd, f32), 3: (B, Wd, bf), 4: (B, spec.embed_dim, f32)}
    else:
        GG = (spec.image_resolution // spec.vision_patch_size) ** 2
        rows, Wd, layers = B * (GG + 1), spec.vision_width, spec.vision_layers
        head = {1: (B * GG, 3 * spec.vision_patch_size ** 2, bf), 2: (B * GG, Wd, f32), 3: (rows, Wd, f32), 4: (rows, Wd, f32)}
        tail = {5: (B, Wd, f32), 6: (B, Wd, bf), 7: (B, spec.embed_dim, f32)}
    out = {(tower, s): v for s, v in head.items()}
    for i in range(layers):
        for s, (w, dt) in {1: (Wd, bf), 2: (3 * Wd, bf), 3: (Wd, bf), 4: (Wd, f32), 5: (Wd, bf), 6: (4 * Wd, bf), 7: (Wd, f32)}.items():
            out[(tower, 16 * (i + 1) + s)] = (rows, w, dt)
    out.update({(tower, s): v for s, v in tail.items()})
    return out


def _lin(a, w, b=None, act=R.ACT_NONE, f32=False, res=None):
    return {"a": a.float(), "w": bfr(w.float()), "b": b, "act": act, "f32": f32, "alpha": 1.0, "rows": None, "mgemm": False, "res": res,
            "res_f32": res is not None}


def _ln(x, sd, pre, out_f32=False):
    return {"x": x.float(), "f32": True, "gamma": sd[pre + ".weight"], "beta": sd[pre + ".bias"], "eps": 1e-5, "small_var": False, "out_f32": out_f32}


def _exact(key, got, want):
    got, want = got.float(), want.float()
    assert got.shape == want.shape, f"{stage_name(key)}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = int((got != want).sum())
    assert bad == 0, f"{stage_name(key)}: {bad} of {got.numel()} elements differ (bitwise equality expected)"
    return 0.0, float("inf")


def _op(key, case, inp, got):
    try:
        return check(case, inp, {"out": got.float()})
    except AssertionError as e:
        raise AssertionError(f"{stage_name(key)}: {e}") from None


def _blocks(sd, pre, layers, tower, taps, x_in, B, L, heads, causal, report):
    for i in range(layers):
        p, k = f"{pre}.resblocks.{i}", lambda s: (tower, 16 * (i + 1) + s)
        Wd = x_in.shape[1]
        report[k(1)] = _op(k(1), R.LayerNorm, _ln(x_in, sd, p + ".ln_1"), taps[k(1)])
        report[k(2)] = _op(k(2), R.Linear, _lin(taps[k(1)], sd[p + ".attn.in_proj_weight"], sd[p + ".attn.in_proj_bias"]), taps[k(2)])
        qkv = taps[k(2)].float().reshape(B, L, 3 * Wd)
        att = {"q": qkv[..., :Wd], "k": qkv[..., Wd:2 * Wd], "v": qkv[..., 2 * Wd:], "H": heads, "D": Wd // heads, "causal": causal,
               "scale": (Wd // heads) ** -0.5, "fused": True}
        report[k(3)] = _op(k(3), R.SmallAttention, att, taps[k(3)].reshape(B, L, Wd))
        report[k(4)] = _op(k(4), R.Linear, _lin(taps[k(3)], sd[p + ".attn.out_proj.weight"], sd[p + ".attn.out_proj.bias"], f32=True, res=x_in.float()),
                           taps[k(4)])
        report[k(5)] = _op(k(5), R.LayerNorm, _ln(taps[k(4)], sd, p + ".ln_2"), taps[k(5)])
        report[k(6)] = _op(k(6), R.Linear, _lin(taps[k(5)], sd[p + ".mlp.c_fc.weight"], sd[p + ".mlp.c_fc.bias"], act=R.ACT_QUICKGELU), taps[k(6)])
        report[k(7)] = _op(k(7), R.Linear, _lin(taps[k(6)], sd[p + ".mlp.c_proj.weight"], sd[p + ".mlp.c_proj.bias"], f32=True, res=taps[k(4)].float()),
                           taps[k(7)])
        x_in = taps[k(7)]
    return x_in


def check_text_stages(sd, spec, tokens, taps):
    """-> {key: (worst error / bound, closest near miss)}; AssertionError naming the first stage that fails"""
    B, L = tokens.shape
    Wd = spec.transformer_width
    k = lambda s: (TEXT, s)
    rep = {}
    rep[k(1)] = _exact(k(1), taps[k(1)], (sd["token_embedding.weight"][tokens] + sd["positional_embedding"]).reshape(B * L, Wd))
    x = _blocks(sd, "transformer", spec.transformer_layers, TEXT, taps, taps[k(1)], B, L, spec.transformer_heads, 1, rep)
    rep[k(2)] = _exact(k(2), taps[k(2)], x.reshape(B, L, Wd)[torch.arange(B), eot_columns(tokens)])
    rep[k(3)] = _op(k(3), R.LayerNorm, _ln(taps[k(2)], sd, "ln_final"), taps[k(3)])
    rep[k(4)] = _op(k(4), R.Linear, _lin(taps[k(3)], sd["text_projection"].t(), f32=True), taps[k(4)])
    return rep


def check_image_stages(sd, spec, image, taps):
    B = image.shape[0]
    P, Wd = spec.vision_patch_size, spec.vision_width
    GG = (spec.image_resolution // P) ** 2
    k = lambda s: (IMAGE, s)
    rep = {}
    rep[k(1)] = _exact(k(1), taps[k(1)], bfr(patchify(image.float(), P)))
    rep[k(2)] = _op(k(2), R.Linear, _lin(taps[k(1)], sd["visual.conv1.weight"].reshape(Wd, -1), f32=True), taps[k(2)])
    cls = sd["visual.class_embedding"].expand(B, 1, Wd)
    rep[k(3)] = _exact(k(3), taps[k(3)], (torch.cat([cls, taps[k(2)].float().reshape(B, GG, Wd)], 1) + sd["visual.positional_embedding"]).reshape(-1, Wd))
    rep[k(4)] = _op(k(4), R.LayerNorm, _ln(taps[k(3)], sd, "visual.ln_pre", out_f32=True), taps[k(4)])
    x = _blocks(sd, "visual.transformer", spec.vision_layers, IMAGE, taps, taps[k(4)], B, GG + 1, spec.vision_heads, 0, rep)
    rep[k(5)] = _exact(k(5), taps[k(5)], x.reshape(B, GG + 1, Wd)[:, 0])
    rep[k(6)] = _op(k(6), R.LayerNorm, _ln(taps[k(5)], sd, "visual.ln_post"), taps[k(6)])
    rep[k(7)] = _op(k(7), R.Linear, _lin(taps[k(6)], sd["visual.proj"].t(), f32=True), taps[k(7)])
    return rep


def summary(rep):
    """the per-stage report as one line per stage"""
    return "\n".join(f"  {stage_name(key)}: worst error / bound {w:.3g}, closest near miss {m:.3g}" for key, (w, m) in rep.items())
