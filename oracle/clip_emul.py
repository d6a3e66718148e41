"""The LIBRARY's arithmetic for the two CLIP towers, restated on the CPU (oracle -- test infrastructure only; the companion of
oracle/unet_emul.py and oracle/vq_emul.py, same purpose and method: fp32 math on bf16 weights, one bf16 rounding exactly where
csrc/first_stage.hip `clip_tower` / `clip_text_body` / `clip_image_body` store a bf16 tensor).

  * the residual stream stays fp32 from the embedding to the pooled row: token + positional embedding, the patch embeddings (bf16 pixels
    against bf16 conv1 weights, fp32 out), cls | patches + positional, ln_pre (fp32 -> fp32), and both residual adds of a resblock
    (x += out_proj(heads), x += c_proj(hidden): the projection's fp32 result added to the fp32 x, no rounding to bf16 in between);
  * bf16 where a GEMM or the attention reads: ln_1, ln_2, ln_final, ln_post, the fused q|k|v rows, the attention heads, the QuickGELU
    hidden x sigmoid(1.702 x) -- all projection weights bf16, biases and LayerNorm parameters fp32;
  * attention as small_attention_kernel forms it: q scaled by d^-1/2 in fp32 BEFORE the dot products, fp32 scores, p = exp(s - max) NOT
    rounded, (p v) / sum p in fp32, heads = column blocks of 64 of each third of the q|k|v rows (head-major);
  * the EOT row is the FIRST maximum of the token ids (torch.argmax's rule, pinned in tests/test_clip_emul_cpu.py).
With rounding=False it is exact algebra and must equal oracle/clip.py (tests/test_clip_emul_cpu.py).

taps: dict receiving every stage under the key (block, sub) rdm_debug_tap shows it at (include/rdm_hip.h): block 2000 the text tower,
3000 the image tower; sub = 16 * layer + stage, layer 0 the tower's own stages, layer i + 1 resblock i.  Tensors are [rows, width] as the
library holds them.  forced: {key: tensor} teacher forcing -- the stage's own value is recorded, then the given one is carried on.
variant: one deliberate defect (the near-miss towers of tests/test_clip_emul_cpu.py), None for the library's arithmetic.

Follows (through oracle/clip.py) rdm/modules/custom_clip/model.py:152-235, 307-320."""
import math

import torch
import torch.nn.functional as F

from .clip import ClipSpec
from .unet_emul import _R

TEXT, IMAGE = 2000, 3000
VARIANTS = ("pos_shift", "cls_last", "no_causal", "erf_gelu", "heads_d_major", "patch_yxc", "eot_last")
TEXT_STAGES = {1: "token + positional embedding", 2: "EOT rows", 3: "ln_final", 4: "text projection"}
IMAGE_STAGES = {1: "patch matrix", 2: "patch embeddings", 3: "cls | patches + positional", 4: "ln_pre", 5: "cls rows", 6: "ln_post",
                7: "image projection"}
BLOCK_STAGES = {1: "ln_1", 2: "q|k|v", 3: "attention heads", 4: "x + out_proj", 5: "ln_2", 6: "QuickGELU hidden", 7: "x + c_proj"}


def stage_name(key):
    block, sub = key
    tower = "text" if block == TEXT else "image"
    layer, st = sub // 16, sub % 16
    if layer == 0:
        return f"{tower} {(TEXT_STAGES if block == TEXT else IMAGE_STAGES)[st]}"
    return f"{tower} resblock {layer - 1} {BLOCK_STAGES[st]}"


class _Walk:
    def __init__(self, block, taps, forced):
        self.block, self.taps, self.forced, self.layer = block, taps, forced, 0

    def __call__(self, stage, t):
        key = (self.block, 16 * self.layer + stage)
        if self.taps is not None:
            self.taps[key] = t
        if self.forced is not None and key in self.forced:
            return self.forced[key].float().reshape(t.shape)
        return t


def _ln(x, sd, pre):
    return F.layer_norm(x, x.shape[-1:], sd[pre + ".weight"], sd[pre + ".bias"], 1e-5)


def attention(qkv, B, L, heads, causal, variant=None):
    """qkv [B L, 3 W] (bf16 values) -> heads [B L, W] fp32, unrounded"""
    Wd = qkv.shape[1] // 3
    d = Wd // heads
    if variant == "heads_d_major":
        sp = lambda t: t.reshape(B, L, d, heads).permute(0, 3, 1, 2)
    else:
        sp = lambda t: t.reshape(B, L, heads, d).permute(0, 2, 1, 3)
    q, k, v = (sp(qkv[:, i * Wd:(i + 1) * Wd]) for i in range(3))
    s = (q * torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32)) @ k.transpose(-1, -2)
    if causal and variant != "no_causal":
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (p @ v) / p.sum(-1, keepdim=True)
    if variant == "heads_d_major":
        return o.permute(0, 2, 3, 1).reshape(B * L, Wd)
    return o.permute(0, 2, 1, 3).reshape(B * L, Wd)


def _tower(sd, pre, layers, x, B, L, heads, causal, R, walk, variant):
    bf = R.bf
    Wb = lambda k: bf(sd[k].float())
    for i in range(layers):
        p = f"{pre}.resblocks.{i}"
        walk.layer = i + 1
        ln = walk(1, bf(_ln(x, sd, p + ".ln_1")))
        qkv = walk(2, bf(F.linear(ln, Wb(p + ".attn.in_proj_weight"), sd[p + ".attn.in_proj_bias"])))
        ao = walk(3, bf(attention(qkv, B, L, heads, causal, variant)))
        x = walk(4, F.linear(ao, Wb(p + ".attn.out_proj.weight"), sd[p + ".attn.out_proj.bias"]) + x)
        ln = walk(5, bf(_ln(x, sd, p + ".ln_2")))
        h = F.linear(ln, Wb(p + ".mlp.c_fc.weight"), sd[p + ".mlp.c_fc.bias"])
        act = 0.5 * h * (1 + torch.erf(h / math.sqrt(2))) if variant == "erf_gelu" else h * torch.sigmoid(1.702 * h)
        hid = walk(6, bf(act))
        x = walk(7, F.linear(hid, Wb(p + ".mlp.c_proj.weight"), sd[p + ".mlp.c_proj.bias"]) + x)
    walk.layer = 0
    return x


def eot_columns(tokens, last=False):
    """column of the maximum id of every row: the first one (torch.argmax; clip_gather_eot_kernel), or the last (a near miss)"""
    if last:
        return tokens.shape[1] - 1 - tokens.flip(1).argmax(dim=-1)
    return tokens.argmax(dim=-1)


def clip_text_emulated(sd, spec: ClipSpec, tokens, rounding=True, taps=None, forced=None, variant=None):
    """tokens int64 [B, context_length] -> [B, embed_dim] fp32 (un-normalised), as rdm_clip_encode_text computes it"""
    assert variant is None or variant in VARIANTS
    R = _R(rounding)
    walk = _Walk(TEXT, taps, forced)
    B, L = tokens.shape
    Wd = spec.transformer_width
    pos = sd["positional_embedding"]
    if variant == "pos_shift":
        pos = pos.roll(-1, 0)
    x = walk(1, (sd["token_embedding.weight"][tokens] + pos).reshape(B * L, Wd))
    x = _tower(sd, "transformer", spec.transformer_layers, x, B, L, spec.transformer_heads, True, R, walk, variant)
    col = eot_columns(tokens, last=variant == "eot_last")
    eot = walk(2, x.reshape(B, L, Wd)[torch.arange(B), col])
    ln = walk(3, R.bf(_ln(eot, sd, "ln_final")))
    return walk(4, ln @ R.bf(sd["text_projection"].float()))


def patchify(image, P, variant=None):
    """[B, 3, R, R] -> [B G^2, 3 P^2], columns in (c, py, px) order: conv1's weight flattening"""
    B, C, Rr, _ = image.shape
    G = Rr // P
    t = image.reshape(B, C, G, P, G, P)                      # b c gy py gx px
    if variant == "patch_yxc":
        return t.permute(0, 2, 4, 3, 5, 1).reshape(B * G * G, C * P * P)
    return t.permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, C * P * P)


def clip_image_emulated(sd, spec: ClipSpec, x, rounding=True, taps=None, forced=None, variant=None):
    """x f32 [B, 3, R, R] (already CLIP-normalised) -> [B, embed_dim] fp32, as rdm_clip_encode_image computes it"""
    assert variant is None or variant in VARIANTS
    R = _R(rounding)
    walk = _Walk(IMAGE, taps, forced)
    B = x.shape[0]
    P, Wd = spec.vision_patch_size, spec.vision_width
    GG = (spec.image_resolution // P) ** 2
    patches = walk(1, R.bf(patchify(x.float(), P, variant)))
    pe = walk(2, patches @ R.bf(sd["visual.conv1.weight"].float()).reshape(Wd, -1).t())
    cls = sd["visual.class_embedding"].expand(B, 1, Wd)
    pos = sd["visual.positional_embedding"]
    if variant == "pos_shift":
        pos = pos.roll(-1, 0)
    seq = [pe.reshape(B, GG, Wd), cls] if variant == "cls_last" else [cls, pe.reshape(B, GG, Wd)]
    x0 = walk(3, (torch.cat(seq, 1) + pos).reshape(B * (GG + 1), Wd))
    h = walk(4, _ln(x0, sd, "visual.ln_pre"))
    h = _tower(sd, "visual.transformer", spec.vision_layers, h, B, GG + 1, spec.vision_heads, False, R, walk, variant)
    c = walk(5, h.reshape(B, GG + 1, Wd)[:, GG if variant == "cls_last" else 0])
    ln = walk(6, R.bf(_ln(c, sd, "visual.ln_post")))
    return walk(7, ln @ R.bf(sd["visual.proj"].float()))
