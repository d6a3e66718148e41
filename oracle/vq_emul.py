"""The LIBRARY's arithmetic for the first stage, restated on the CPU (oracle — test infrastructure only; the companion of oracle/unet_emul.py,
same purpose and method: fp32 math, one bf16 rounding wherever csrc/first_stage.hip stores a bf16 tensor).

Decode (`vq_body` / `vq_trunk`, the VQ-f4 decoder):
  * quantisation + post_quant_conv and conv_in in fp32 (vq_quantize_kernel, conv_in_kernel), conv_in's output rounded;
  * ResnetBlock: bf16(swish(GroupNorm eps 1e-6)), bf16 3x3 weights, bias / shortcut added in fp32, one rounding per conv;
  * AttnBlock: bf16 q, k and V^T (b_v added after P.V: rows of P sum to 1), fp32 scores, NORMALISED probabilities rounded to bf16
    (softmax_rows_kernel), bf16(P V + b_v), proj_out + residual in one rounding;
  * Upsample convs by output phase on pre-summed weights (oracle/unet_emul.py::_phase_weights);
  * norm_out + swish rounded, conv_out against fp32 weights, fp32 image.
Encode (`vqenc_body`, VQ-f4 and the wide VQGAN-f16 form): see vq_encode_emulated.
With rounding=False both are exact algebra and must equal oracle/vqdecoder.py (tests/test_oracle_cpu.py, tests/test_vq_encoder_cpu.py).

Follows (through oracle/vqdecoder.py): ldm VQModelInterface.decode / encode, Decoder / Encoder / ResnetBlock / AttnBlock / Upsample /
Downsample, taming VectorQuantizer2, reached from rdm/models/diffusion/ddpm.py:840 and :390-391."""
import torch
import torch.nn.functional as F

from .unet_emul import _R, _upsample_conv
from .vqdecoder import VQSpec, vq_quantize

# what the encoder restatement states about the library, by name: tests/_vqenc_ref.py alters them to show that the layer-by-layer
# comparison tells each alteration apart
GN_EPS = 1e-6                  # every GroupNorm of the first stage (ldm Normalize)
DOWN_PAD = (0, 1, 0, 1)        # [ldm] Downsample(with_conv): zero column on the right, zero row at the bottom, then an unpadded stride-2 conv


def _swish(x):
    return x * torch.sigmoid(x)


def _blocks(sd, R, eps):
    """-> (Wb, gn, resnet, attn): the ResnetBlock / AttnBlock arithmetic both halves of the first stage share (vq_res, vq_attn)"""
    bf = R.bf
    Wb = lambda k: bf(sd[k].float())
    gn = lambda x, pre: F.group_norm(x, 32, sd[pre + ".weight"], sd[pre + ".bias"], eps)

    def resnet(pre, x):
        h = bf(_swish(gn(x, pre + ".norm1")))
        h = bf(F.conv2d(h, Wb(pre + ".conv1.weight"), sd[pre + ".conv1.bias"], padding=1))
        h = bf(_swish(gn(h, pre + ".norm2")))
        res = x
        if (pre + ".nin_shortcut.weight") in sd:
            res = bf(F.conv2d(x, Wb(pre + ".nin_shortcut.weight"), sd[pre + ".nin_shortcut.bias"]))
        return bf(F.conv2d(h, Wb(pre + ".conv2.weight"), sd[pre + ".conv2.bias"], padding=1) + res)

    def attn(pre, x):
        b, c, hh, ww = x.shape
        n = hh * ww
        hn = bf(gn(x, pre + ".norm")).permute(0, 2, 3, 1).reshape(b, n, c)
        lin = lambda nm, bias=True: F.linear(hn, Wb(f"{pre}.{nm}.weight").reshape(c, c), sd[f"{pre}.{nm}.bias"] if bias else None)
        q, k, v = bf(lin("q")), bf(lin("k")), bf(lin("v", bias=False))
        s = torch.bmm(q, k.transpose(1, 2)) * (float(c) ** -0.5)
        p = bf(F.softmax(s, dim=2))
        ao = bf(torch.bmm(p, v) + sd[pre + ".v.bias"])
        out = F.linear(ao, Wb(pre + ".proj_out.weight").reshape(c, c), sd[pre + ".proj_out.bias"])
        return bf(out.reshape(b, hh, ww, c).permute(0, 3, 1, 2) + x)

    return Wb, gn, resnet, attn


def _layers(taps, forced):
    """-> layer(img): records the layer's own output as tokens [B, H*W, C] and hands on `forced[i]` in its place where one is given"""
    cnt = [0]

    def layer(img):
        tok = img.permute(0, 2, 3, 1).reshape(img.shape[0], img.shape[2] * img.shape[3], img.shape[1])
        i = cnt[0]; cnt[0] += 1
        if taps is not None:
            taps.append(tok)
        if forced is not None and i in forced:
            return forced[i].float().reshape(img.shape[0], img.shape[2], img.shape[3], img.shape[1]).permute(0, 3, 1, 2)
        return img

    return layer


def vq_decode_emulated(sd, spec: VQSpec, z, force_not_quantize=False, rounding=True, taps=None, forced=None):
    """taps: list receiving every layer's output [B, H*W, C] in execution order (conv_in, mid.block_1, mid.attn_1, mid.block_2, then per
    level its blocks (+ attn) and the upsample conv) -- the library shows the same tensors as rdm_debug_tap blocks 1000, 1001, ...;
    forced: {index: tensor} teacher forcing as in oracle/unet_emul.py."""
    R = _R(rounding)
    layer = _layers(taps, forced)
    bf = R.bf
    Wb, gn, resnet, attn = _blocks(sd, R, 1e-6)

    if not force_not_quantize:
        z, _ = vq_quantize(sd, z)
    h = F.conv2d(z, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"])                      # fp32 (vq_quantize_kernel)
    h = layer(bf(F.conv2d(h, sd["decoder.conv_in.weight"], sd["decoder.conv_in.bias"], padding=1)))        # fp32 weights (conv_in_kernel)
    h = layer(resnet("decoder.mid.block_1", h))
    if spec.mid_attn:
        h = layer(attn("decoder.mid.attn_1", h))
    h = layer(resnet("decoder.mid.block_2", h))
    for lvl in reversed(range(len(spec.ch_mult))):
        for i in range(spec.num_res_blocks + 1):
            h = layer(resnet(f"decoder.up.{lvl}.block.{i}", h))
            if f"decoder.up.{lvl}.attn.{i}.q.weight" in sd:
                h = layer(attn(f"decoder.up.{lvl}.attn.{i}", h))
        if lvl != 0:
            h = layer(bf(_upsample_conv(h, Wb(f"decoder.up.{lvl}.upsample.conv.weight"), sd[f"decoder.up.{lvl}.upsample.conv.bias"], R)))
    h = bf(_swish(gn(h, "decoder.norm_out")))
    return F.conv2d(h, sd["decoder.conv_out.weight"], sd["decoder.conv_out.bias"], padding=1)


def vq_encode_emulated(sd, spec: VQSpec, x, rounding=True, taps=None, forced=None):
    """csrc/first_stage.hip `vqenc_body` restated: image fp32 [B, out_ch, H, W] -> latent fp32 [B, embed_dim, H / f, W / f] (not quantised).

      * conv_in in fp32 on fp32 weights, output rounded (conv_in_kernel);
      * ResnetBlock and AttnBlock as in the decoder (vq_res, vq_attn; an AttnBlock on a token count that is no multiple of 64 runs on zero
        padding whose keys get probability 0: the same values);
      * Downsample: bf16(conv2d(pad(h, (0, 1, 0, 1)), bf16 W, stride 2) + bias) -- the generic implicit GEMM with IgemmParams::asym;
      * VQ-f4 tail (z_channels <= 4): norm_out + swish rounded, conv_out against fp32 weights in fp32, quant_conv in fp32
        (vq_quantize_kernel with no codebook).  At the encoder's widths (ch * ch_mult[-1] = 256 and 512, above head_conv_kernel's 240) the
        head is Ops::head's GroupNorm pass + conv_out_kernel: bf16 activations, fp32 weights, fp32 accumulation.  A narrower encoder whose
        image size head_conv_kernel takes (C <= 240, W % 32 == 0, H even) would add that kernel's own roundings -- its fp32 weights carried
        as bf16 hi + lo pairs, 2^-16 relative -- which this restatement does not state; none of the models the suite loads reaches it;
      * wide tail (VQGAN-f16, z_channels > 4): GroupNorm + swish rounded, conv_out as a bf16 3x3 conv rounded, quant_conv as a bf16-weight
        GEMM on those bf16 rows with fp32 output.

    taps: list receiving every layer's output [B, H*W, C] in execution order -- conv_in; per level its ResnetBlocks (each followed by its
    AttnBlock where the level has one) and the Downsample conv; mid.block_1, mid.attn_1, mid.block_2; for a wide latent also norm_out + swish
    and conv_out -- the library shows the same tensors as rdm_debug_tap blocks 1500, 1501, ...; forced: {index: tensor} teacher forcing.
    With rounding=False it is exact algebra and equals oracle/vqdecoder.py::vq_encode (tests/test_vq_encoder_cpu.py)."""
    R = _R(rounding)
    layer = _layers(taps, forced)
    bf = R.bf
    Wb, gn, resnet, attn = _blocks(sd, R, GN_EPS)
    nl = len(spec.ch_mult)

    h = layer(bf(F.conv2d(x, sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"], padding=1)))        # fp32 weights (conv_in_kernel)
    for lvl in range(nl):
        for i in range(spec.num_res_blocks):
            h = layer(resnet(f"encoder.down.{lvl}.block.{i}", h))
            if f"encoder.down.{lvl}.attn.{i}.q.weight" in sd:
                h = layer(attn(f"encoder.down.{lvl}.attn.{i}", h))
        if lvl != nl - 1:
            pre = f"encoder.down.{lvl}.downsample.conv"
            h = layer(bf(F.conv2d(F.pad(h, DOWN_PAD), Wb(pre + ".weight"), sd[pre + ".bias"], stride=2)))
    h = layer(resnet("encoder.mid.block_1", h))
    if spec.mid_attn:
        h = layer(attn("encoder.mid.attn_1", h))
    h = layer(resnet("encoder.mid.block_2", h))
    if spec.z_channels > 4:
        h = layer(bf(_swish(gn(h, "encoder.norm_out"))))
        h = layer(bf(F.conv2d(h, Wb("encoder.conv_out.weight"), sd["encoder.conv_out.bias"], padding=1)))
        return F.conv2d(h, Wb("quant_conv.weight"), sd["quant_conv.bias"])
    h = bf(_swish(gn(h, "encoder.norm_out")))
    h = F.conv2d(h, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"], padding=1)
    return F.conv2d(h, sd["quant_conv.weight"], sd["quant_conv.bias"])
