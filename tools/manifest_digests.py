#!/usr/bin/env python3
"""Writes tests/golden/manifest_digests.json: for every model kind and every cfg the suite loads, the cfg's fields, the sha256 of the
manifest text the library writes for it, and blob_bytes (tests/test_library_cpu.py recomputes and compares them).  The blob layout
is part of what a packed checkpoint is: re-run this only for a change that is meant to move it.  Needs no GPU."""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rdm_amd  # noqa: F401
from rdm_amd import _lib
from oracle import clip as oclip, rarm as orarm, unet as ounet, vqdecoder as ovq
from _util import spec_to_clip_cfg, spec_to_unet_cfg, spec_to_vq_cfg


def vq_cfg(spec, **kw):
    return _lib.make_vq_cfg(embed_dim=spec.embed_dim, n_embed=spec.n_embed, z_channels=spec.z_channels, ch=spec.ch, ch_mult=spec.ch_mult,
                            num_res_blocks=spec.num_res_blocks, out_ch=spec.out_ch, resolution=spec.resolution, mid_attn=spec.mid_attn,
                            attn_resolutions=spec.attn_resolutions, **kw)


def rarm_cfg(spec):
    return _lib.make_rarm_cfg(in_channels=spec.vocab_in, out_channels=spec.vocab_out, n_heads=spec.n_heads, d_head=spec.d_head, depth=spec.depth,
                              context_dim=spec.context_dim, sequence_length=spec.sequence_length)


def cases():
    U = ounet.UNetSpec
    unets = [ounet.tiny_spec(), ounet.shipped_spec(), U(model_channels=224, channel_mult=(1, 2, 3, 4)),
             U(model_channels=96, num_res_blocks=1, attention_resolutions=(2, 4), channel_mult=(1, 2, 3), num_head_channels=32, context_dim=512),
             U(model_channels=32, num_res_blocks=1, attention_resolutions=(2, 4), channel_mult=(1, 3, 5), num_head_channels=32, context_dim=512)]
    out = [("unet", spec_to_unet_cfg(s)) for s in unets] + [("unet", _lib.make_unet_cfg())]
    V = ovq.VQSpec
    stages = [ovq.tiny_vq_spec(), ovq.shipped_vq_spec(), ovq.tiny_vqgan_spec(), ovq.vqgan_f16_spec(),
              V(n_embed=512, ch=64, ch_mult=(1, 2), num_res_blocks=1, resolution=64),
              V(embed_dim=256, n_embed=512, z_channels=256, ch=64, ch_mult=(1, 2, 4), num_res_blocks=1, resolution=64, attn_resolutions=(16,))]
    for s in stages:
        out += [("vq", vq_cfg(s)), ("vqenc", vq_cfg(s))]
    t = ovq.tiny_vq_spec()
    out += [("vq", _lib.make_vq_cfg()), ("vqenc", _lib.make_vq_cfg()), ("vq", _lib.make_vqgan_f16_cfg()), ("vqenc", _lib.make_vqgan_f16_cfg()),
            ("vq", vq_cfg(t, kl=True)), ("vq", _lib.make_vq_cfg(kl=True)), ("vq", spec_to_vq_cfg(t)),
            ("vq", vq_cfg(ovq.VQSpec(n_embed=512, ch=64, ch_mult=(1, 2, 4), num_res_blocks=2, resolution=64)))]
    out += [("clip", spec_to_clip_cfg(oclip.tiny_clip_spec())), ("clip", spec_to_clip_cfg(oclip.vitb32_spec())), ("clip", _lib.make_clip_cfg())]
    R = orarm.RarmSpec
    rarms = [orarm.tiny_rarm_spec(), orarm.shipped_rarm_spec(),
             R(vocab_in=514, vocab_out=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64),
             R(vocab_in=514, vocab_out=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=256),
             R(vocab_in=4098, vocab_out=4096, n_heads=1, d_head=64, depth=1, context_dim=64, sequence_length=40)]
    out += [("rarm", rarm_cfg(s)) for s in rarms] + [("rarm", _lib.make_rarm_cfg())]
    return out


def cfg_fields(cfg):
    return {name: (list(v) if hasattr(v, "__len__") else v) for name, _ in cfg._fields_ for v in [getattr(cfg, name)]}


def main():
    rows, seen = [], set()
    for kind, cfg in cases():
        fields = cfg_fields(cfg)
        ident = json.dumps([kind, fields])
        if ident in seen:
            continue
        seen.add(ident)
        text, blob_bytes = _lib.manifest_text(kind, cfg)
        rows.append({"kind": kind, "cfg": fields, "sha256": hashlib.sha256(text.encode()).hexdigest(), "blob_bytes": blob_bytes})
    path = os.path.join(ROOT, "tests", "golden", "manifest_digests.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} manifests -> {path}")


if __name__ == "__main__":
    main()
