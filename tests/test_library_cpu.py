"""CPU suite: the C-ABI library loads, exports every symbol include/rdm_hip.h declares, refuses to run
without a GPU (no fallback), and its weight manifests agree with the reference's state_dict layout."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import clip as oclip
from oracle import unet as ounet
from oracle import vqdecoder as ovq

from _util import spec_to_clip_cfg, spec_to_unet_cfg, spec_to_vq_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rdm_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    syms = _header_symbols()
    assert len(syms) >= 25 and "rdm_op_conv3x3_down" in syms and "rdm_op_conv3x3" in syms
    for s in syms:
        assert hasattr(_lib.lib, s), f"librdm_hip.so does not export {s}"
    assert set(_lib.SIGNATURES) == set(syms), set(_lib.SIGNATURES) ^ set(syms)
    assert b"gfx950" in _lib.lib.rdm_version()


def test_native_library_reads_only_the_kept_environment_switches():
    """The library's environment switches are a closed list: the deterministic mode and four test / tool hooks (csrc/common.h, rdm_env_int).
    A new `getenv("RDM_...")` in csrc/ must be driven by a test or not be added."""
    import glob
    csrc = os.path.join(ROOT, "retrieval-augmented-diffusion-models_amd", "csrc")
    names = set()
    for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
        names |= set(re.findall(r'getenv\("(RDM_[A-Z0-9_]+)', open(path).read()))
    assert names == {"RDM_DETERMINISTIC", "RDM_MGEMM_ANY", "RDM_MGEMM_FROM", "RDM_VQ_RANGE", "RDM_OP_FRAG_CACHE"}, sorted(names)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    with pytest.raises(_lib.RdmError):
        _lib.Context(0)


def _check_manifest(kind, cfg, shapes):
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, packing
    entries, blob_bytes = _lib.manifest(kind, cfg)
    # every reference key exactly once among the plain entries; derived entries (products of two reference tensors, e.g. the
    # fused ff.net.2 * proj_out map) may re-use keys
    used = [s for e in entries if not e[2].startswith("fuse_") for s in e[3]]
    assert sorted(used) == sorted(shapes), set(used) ^ set(shapes)
    assert all(s in shapes for e in entries for s in e[3])
    ends = [off + nb for off, nb, _, _ in entries]
    offs = [off for off, _, _, _ in entries]
    assert all(o % 256 == 0 for o in offs) and all(a <= b for a, b in zip(ends[:-1], offs[1:])) and ends[-1] <= blob_bytes
    sd = ounet.synth_state_dict(shapes, seed=1)
    blob = packing.pack(kind, cfg, sd)
    assert blob.nbytes == blob_bytes
    return entries, blob, sd


def test_unet_manifest_padding_recipes():
    """A UNet whose widths are multiples of 32 only (models/rdm/ffhq: model_channels 224): the manifest's kinds carry the padding
    recipe and the packer executes it -- every reference tensor is used, padded segments end in zeros, logical values sit where
    the recipe says (checked on a skip-concat conv: [N][ky][kx][C0 pad | C1 pad]); the ImageNet config has no recipe at all."""
    from rdm_amd import _lib
    spec = ounet.UNetSpec(model_channels=96, num_res_blocks=1, attention_resolutions=(2, 4), channel_mult=(1, 2, 3), num_head_channels=32, context_dim=512)
    entries, blob, sd = _check_manifest("unet", spec_to_unet_cfg(spec), ounet.param_shapes(spec))
    assert any("|R=" in e[2] or "|C=" in e[2] for e in entries)
    assert not any("|" in e[2] for e in _lib.manifest("unet", spec_to_unet_cfg(ounet.shipped_spec()))[0])
    ffhq = ounet.UNetSpec(model_channels=224, channel_mult=(1, 2, 3, 4))
    e2, nbytes = _lib.manifest("unet", spec_to_unet_cfg(ffhq))
    assert sorted(s for e in e2 if not e[2].startswith("fuse_") for s in e[3]) == sorted(ounet.param_shapes(ffhq))
    # a decoder ResBlock conv over [h | skip]: 'conv3|R=n>np|C=c0>p0,c1>p1'
    off, nb, kd, srcs = next(e for e in entries if e[2].startswith("conv3") and e[2].count(">") == 3)
    from rdm_amd.packing import _parse_kind
    _, rows, cols = _parse_kind(kd)
    (n, npad), ((c0, p0), (c1, p1)) = rows[0], cols
    w = sd[srcs[0]]
    assert w.shape == (n, c0 + c1, 3, 3) and nb == npad * 9 * (p0 + p1) * 2
    got = torch.from_numpy(blob[off:off + nb].view(np.int16).copy()).view(torch.bfloat16).float().reshape(npad, 3, 3, p0 + p1)
    ref = w.permute(0, 2, 3, 1).to(torch.bfloat16).float()
    assert torch.equal(got[:n, :, :, :c0], ref[..., :c0]) and torch.equal(got[:n, :, :, p0:p0 + c1], ref[..., c0:])
    assert not got[n:].any() and not got[:, :, :, c0:p0].any() and not got[:, :, :, p0 + c1:].any()


def test_unet_manifest_matches_reference_state_dict():
    spec = ounet.tiny_spec()
    entries, blob, sd = _check_manifest("unet", spec_to_unet_cfg(spec), ounet.param_shapes(spec))
    # spot-check the conv3 layout: [N][ky][kx][C]
    off, nb, kd, srcs = next(e for e in entries if e[2] == "conv3")
    w = sd[srcs[0]]
    got = torch.from_numpy(blob[off:off + nb].view(np.int16).copy()).view(torch.bfloat16).float().reshape(w.shape[0], 3, 3, w.shape[1])
    assert torch.equal(got, w.permute(0, 2, 3, 1).to(torch.bfloat16).float())
    # the shipped config's manifest covers all 688 tensors
    full = ounet.shipped_spec()
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    e2, nbytes = _lib.manifest("unet", spec_to_unet_cfg(full))
    assert sorted(s for e in e2 if not e[2].startswith("fuse_") for s in e[3]) == sorted(ounet.param_shapes(full))
    assert 0.79e9 < nbytes < 0.99e9          # ~0.80 GB bf16 + the derived ff.net.2 x proj_out product weights (0.13 GB)
    # the derived entry is the product map: [W_out W_2 | W_out] and W_out b_2 + b_out
    off, nb, kd, srcs = next(e for e in entries if e[2] == "fuse_w")
    w2, wo = sd[srcs[0]].double(), sd[srcs[1]].reshape(sd[srcs[1]].shape[0], -1).double()
    got = torch.from_numpy(blob[off:off + nb].view(np.int16).copy()).view(torch.bfloat16).float().reshape(wo.shape[0], -1)
    assert torch.equal(got, torch.cat([wo @ w2, wo], dim=1).float().to(torch.bfloat16).float())


def test_vq_and_clip_manifests():
    _check_manifest("vq", spec_to_vq_cfg(ovq.tiny_vq_spec()), ovq.vq_param_shapes(ovq.tiny_vq_spec()))
    _check_manifest("clip", spec_to_clip_cfg(oclip.tiny_clip_spec()), oclip.clip_param_shapes(oclip.tiny_clip_spec()))


def test_rarm_and_vqgan_manifests():
    """RARM transformer (rdm/modules/attention.py:206-249 keys) and the taming VQGAN-f16 decoder (per-level AttnBlocks, wide latent)."""
    import rdm_amd  # noqa: F401
    from oracle import rarm as orarm
    from rdm_amd import _lib
    spec = orarm.tiny_rarm_spec()
    cfg = _lib.make_rarm_cfg(in_channels=spec.vocab_in, out_channels=spec.vocab_out, n_heads=spec.n_heads, depth=spec.depth,
                             sequence_length=spec.sequence_length)
    entries, blob, sd = _check_manifest("rarm", cfg, orarm.rarm_param_shapes(spec))
    off, nb, kd, srcs = next(e for e in entries if e[2] == "f32_t")      # positional_encoding [C, L] stored as [L][C]
    got = torch.from_numpy(blob[off:off + nb].view(np.float32).copy()).reshape(spec.sequence_length, spec.inner_dim)
    assert torch.equal(got, sd["positional_encoding"].t())
    vs = ovq.tiny_vqgan_spec()
    vcfg = _lib.make_vq_cfg(embed_dim=vs.embed_dim, n_embed=vs.n_embed, z_channels=vs.z_channels, ch=vs.ch, ch_mult=vs.ch_mult,
                            num_res_blocks=vs.num_res_blocks, resolution=vs.resolution, attn_resolutions=vs.attn_resolutions)
    e2, _, _ = _check_manifest("vq", vcfg, ovq.vq_param_shapes(vs))
    assert any(e[2] == "conv3" and e[3] == ["decoder.conv_in.weight"] for e in e2)          # wide latent: conv_in is a GEMM-class conv
    full = _lib.make_vqgan_f16_cfg()
    e3, nbytes = _lib.manifest("vq", full)
    assert sorted(s for e in e3 for s in e[3]) == sorted(ovq.vq_param_shapes(ovq.vqgan_f16_spec()))


def test_manifests_are_byte_for_byte_the_recorded_ones():
    """tests/golden/manifest_digests.json (tools/manifest_digests.py) holds, for all five model kinds and every cfg the suite loads,
    the sha256 of the manifest text and blob_bytes: entry order, offsets, sizes, kinds and source keys of every blob layout stay
    what packed checkpoints were written against."""
    import hashlib
    import json
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest_digests.json")))
    assert {r["kind"] for r in rows} == {"unet", "vq", "vqenc", "clip", "rarm"} and len(rows) >= 25
    types = {"unet": _lib.UNetCfg, "vq": _lib.VqCfg, "vqenc": _lib.VqCfg, "clip": _lib.ClipCfg, "rarm": _lib.RarmCfg}
    for r in rows:
        cfg = types[r["kind"]]()
        assert sorted(r["cfg"]) == sorted(n for n, _ in cfg._fields_)
        for name, v in r["cfg"].items():
            if isinstance(v, list):
                getattr(cfg, name)[:] = v
            else:
                setattr(cfg, name, v)
        text, blob_bytes = _lib.manifest_text(r["kind"], cfg)
        assert (hashlib.sha256(text.encode()).hexdigest(), blob_bytes) == (r["sha256"], r["blob_bytes"]), (r["kind"], r["cfg"])


def test_ema_key_mapping():
    import rdm_amd  # noqa: F401
    from rdm_amd import packing
    ck = {"model.diffusion_model.out.2.weight": torch.zeros(1), "model_ema.diffusion_modelout2weight": torch.ones(1),
          "model.diffusion_model.out.2.bias": torch.zeros(1), "first_stage_model.x": torch.zeros(1)}
    sd = packing.ema_unet_state_dict(ck)
    assert sd["out.2.weight"].item() == 1.0 and sd["out.2.bias"].item() == 0.0 and len(sd) == 2


def test_vq_encoder_manifest():
    """First-stage ENCODER (`encoder.*`, `quant_conv.*` -- taming/ldm Encoder + quant_conv, ldm/models/autoencoder.py:96-110): every
    reference tensor consumed once; the stride-2 Downsample conv is a 3x3 conv entry like the others ([N][ky][kx][C])."""
    spec = ovq.tiny_vq_spec()
    shapes = ovq.vq_encoder_param_shapes(spec)
    entries, blob, sd = _check_manifest("vqenc", spec_to_vq_cfg(spec), shapes)
    off, nb, kd, srcs = next(e for e in entries if e[3] == ["encoder.down.0.downsample.conv.weight"])
    w = sd[srcs[0]]
    got = torch.from_numpy(blob[off:off + nb].view(np.int16).copy()).view(torch.bfloat16).float().reshape(w.shape[0], 3, 3, -1)
    assert torch.equal(got[..., :w.shape[1]], w.permute(0, 2, 3, 1).to(torch.bfloat16).float())
    full = ovq.vq_encoder_param_shapes(ovq.shipped_vq_spec())
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    e2, _ = _lib.manifest("vqenc", spec_to_vq_cfg(ovq.shipped_vq_spec()))
    assert sorted(s for e in e2 for s in e[3]) == sorted(full)


def test_training_layout_round_trip():
    """Masters in the native layouts ([N][ky][kx][C] convs, [N][C] 1x1 convs) and back: state_dict_from_params inverts
    params_from_state_dict, and grads_to_state_dict_layout maps a native-layout gradient onto the reference's parameter shapes."""
    import rdm_amd  # noqa: F401
    from rdm_amd import training_unet as tu
    spec = ounet.tiny_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=3)
    P = tu.params_from_state_dict(sd, "cpu")
    k3 = next(k for k, v in sd.items() if v.dim() == 4 and v.shape[2:] == (3, 3))
    assert P[k3].shape == (sd[k3].shape[0], 3, 3, sd[k3].shape[1]) and torch.equal(P[k3][:, 1, 2, :], sd[k3][:, :, 1, 2])
    back = tu.state_dict_from_params(P, sd)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k].float()) for k in sd)
    g = tu.grads_to_state_dict_layout({k3: P[k3].reshape(P[k3].shape[0], -1)}, sd)
    assert torch.equal(g[k3], sd[k3].float())
    pr = tu._Params(P, {k3: P[k3].to(torch.bfloat16) * 0})
    assert not pr.w(k3).any() and pr[k3] is P[k3] and k3 in pr
    kb = next(k for k in sd if k.endswith(".bias"))
    assert pr.w(kb).dtype == torch.bfloat16 and torch.equal(pr.w(kb).float(), P[kb].to(torch.bfloat16).float())
