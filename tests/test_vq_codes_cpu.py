"""CPU suite of the VQGAN-f16 encode path (image -> code indices, RARM image completion): the C ABI's declarations, the encoder
manifests of wide-latent first stages, packing, the synthetic encoder shapes and the script's flags.  (Kernels and executors:
tests/test_gpu_vq_codes.py.)"""
import importlib.util
import os
import re

import numpy as np
import torch

from oracle import unet as ounet
from oracle import vqdecoder as ovq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rdm_vq_encode_indices", "rdm_op_vq_nearest_code")


def _cfg(spec):
    from rdm_amd import _lib
    return _lib.make_vq_cfg(embed_dim=spec.embed_dim, n_embed=spec.n_embed, z_channels=spec.z_channels, ch=spec.ch, ch_mult=spec.ch_mult,
                            num_res_blocks=spec.num_res_blocks, resolution=spec.resolution, attn_resolutions=spec.attn_resolutions)


def test_header_declares_the_new_entries_and_the_binding_carries_them():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["rdm_vq_encode_indices"][1]) == 5
    assert len(_lib.SIGNATURES["rdm_op_vq_nearest_code"][1]) == 7
    for method in ("vq_encode_indices", "vq_nearest_code"):
        assert callable(getattr(_lib.Context, method))
    # the call-site table of INTEGRATION.md names them
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in integ


def _check_manifest(spec):
    from rdm_amd import _lib
    entries, blob_bytes = _lib.manifest("vqenc", _cfg(spec))
    want = ovq.vq_encoder_param_shapes(spec)
    seen = [s for _, _, _, srcs in entries for s in srcs]
    assert sorted(seen) == sorted(want), "every encoder.* / quant_conv.* key exactly once"
    kinds = {s: kd for _, _, kd, srcs in entries for s in srcs}
    assert kinds["encoder.conv_out.weight"] == "conv3" and kinds["quant_conv.weight"] == "bf16"
    assert not any(k.startswith("quantize.") for k in seen)          # the codebook stays with the decoder blob
    for off, nbytes, kd, srcs in entries:
        elt = 4 if kd.startswith("f32") else 2
        assert nbytes == sum(int(np.prod(want[s])) for s in srcs) * elt and off + nbytes <= blob_bytes
    return entries


def test_tiny_vqgan_encoder_manifest_consumes_every_key_once():
    _check_manifest(ovq.tiny_vqgan_spec())


def test_shipped_vqgan_f16_encoder_manifest():
    from rdm_amd import _lib
    spec = ovq.vqgan_f16_spec()
    _check_manifest(spec)
    entries, _ = _lib.manifest("vqenc", _lib.make_vqgan_f16_cfg())
    assert sorted(s for _, _, _, srcs in entries for s in srcs) == sorted(ovq.vq_encoder_param_shapes(spec))


def test_three_channel_encoder_manifest_is_unchanged():
    """VQ-f4: conv_out and quant_conv stay fp32 entries (the fused head conv + the 3 x 3 quantiser kernel read them)."""
    from rdm_amd import _lib
    entries, _ = _lib.manifest("vqenc", _lib.make_vq_cfg())
    kinds = {s: kd for _, _, kd, srcs in entries for s in srcs}
    assert kinds["encoder.conv_out.weight"] == "f32" and kinds["quant_conv.weight"] == "f32"
    assert sorted(kinds) == sorted(ovq.vq_encoder_param_shapes(ovq.VQSpec()))


def test_unsupported_encoder_cfgs_are_rejected():
    from rdm_amd import _lib
    import pytest
    for bad in (dict(embed_dim=96, z_channels=64), dict(embed_dim=64, z_channels=3), dict(embed_dim=64, z_channels=64, kl=True)):
        with pytest.raises(ValueError):
            _lib.manifest("vqenc", _lib.make_vq_cfg(ch=64, ch_mult=(1, 2), resolution=32, **bad))


def test_pack_vqenc_round_trips_the_wide_tail():
    """encoder.conv_out of the tiny VQGAN through packing.pack: bf16 [N][ky][kx][C] at the manifest's offset; quant_conv as bf16 [E][Z]."""
    from rdm_amd import _lib, packing
    spec = ovq.tiny_vqgan_spec()
    cfg = _cfg(spec)
    sd = ounet.synth_state_dict(ovq.vq_encoder_param_shapes(spec), seed=888)
    blob = packing.pack("vqenc", cfg, sd)
    entries, blob_bytes = _lib.manifest("vqenc", cfg)
    assert blob.nbytes == blob_bytes
    by_src = {srcs[0]: (off, nbytes) for off, nbytes, _, srcs in entries}

    def bf16_at(name):
        off, nbytes = by_src[name]
        bits = blob[off:off + nbytes].view(np.uint16).astype(np.uint32) << 16
        return torch.from_numpy(bits.view(np.float32).copy())

    w = sd["encoder.conv_out.weight"]
    assert torch.equal(bf16_at("encoder.conv_out.weight").reshape(w.shape[0], 3, 3, w.shape[1]), w.permute(0, 2, 3, 1).bfloat16().float())
    q = sd["quant_conv.weight"]
    assert torch.equal(bf16_at("quant_conv.weight").reshape(q.shape[0], q.shape[1]), q.reshape(q.shape[0], -1).bfloat16().float())


def test_synthetic_encoder_shapes_equal_the_oracles():
    from rdm_amd import _lib, synthetic
    for spec, cfg in ((ovq.tiny_vqgan_spec(), _cfg(ovq.tiny_vqgan_spec())), (ovq.vqgan_f16_spec(), _lib.make_vqgan_f16_cfg()),
                      (ovq.VQSpec(), _lib.make_vq_cfg())):
        assert synthetic.vq_encoder_param_shapes(cfg) == ovq.vq_encoder_param_shapes(spec)
    cfg = _cfg(ovq.tiny_vqgan_spec())
    sd = synthetic.vq_encoder_state_dict(cfg, seed=3)
    assert sorted(sd) == sorted(ovq.vq_encoder_param_shapes(ovq.tiny_vqgan_spec()))
    assert not set(sd) & set(synthetic.vq_param_shapes(cfg))         # disjoint from the decoder's keys: one dict can carry both


def _script():
    path = os.path.join(ROOT, "scripts", "rarm_sample.py")
    spec = importlib.util.spec_from_file_location("rarm_sample_native_cpu", path)
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_script_complete_from_flag_parses_and_old_defaults_stay():
    mod = _script()
    opt = mod.parse_args(["--complete_from", "some/dir", "--keep_rows", "5"])
    assert str(opt.complete_from) == os.path.join("some", "dir") and opt.keep_rows == 5
    opt = mod.parse_args(["--complete_from", "img.png"])
    assert opt.keep_rows is None
    d = mod.parse_args([])
    assert d.complete_from is None and d.keep_rows is None
    assert (d.batch_size, d.n_runs, d.seed, d.guidance_scale, d.top_k, d.top_p, d.temperature, d.top_m, d.k_nn) == (4, 2, None, 1.0, 256, 1.0, 1.0, 0.01, 4)
    assert str(d.savepath) == os.path.join("out", "rarm") and d.gpu == -1 and d.caption == "" and not d.synthetic
    assert "--complete_from" in mod.__doc__ and "--keep_rows" in mod.__doc__


def test_load_images_centre_crops_and_scales(tmp_path):
    from PIL import Image
    mod = _script()
    a = np.zeros((40, 60, 3), np.uint8); a[:, 10:50] = 255            # the centre 40 x 40 square is white, the margins black
    Image.fromarray(a).save(tmp_path / "b.png")
    Image.fromarray(np.full((16, 16, 3), 0, np.uint8)).save(tmp_path / "a.png")
    (tmp_path / "notes.txt").write_text("not an image")
    x = mod.load_images(tmp_path, 32)
    assert x.shape == (2, 3, 32, 32) and x.dtype == torch.float32
    assert float(x[0].max()) == -1.0 and float(x[1].min()) == 1.0      # sorted by name: a.png (black), b.png (white square)
    assert mod.load_images(tmp_path / "b.png", 8).shape == (1, 3, 8, 8)


def test_mirror_log_images_call_pattern():
    """log_images against a recording context: encode once, the five key families, the half run keeps the first half of the codes as
    its prefix, and get_r's Bernoulli masking replaces entries of r by the mask token."""
    import rdm_amd  # noqa: F401
    from rdm_amd.models.autoregression.transformer import LatentImageRETRO

    class Ctx:
        device = torch.device("cpu")

        def __init__(self):
            self.calls = []

        def vq_encode_indices(self, img, return_quant=False):
            idx = torch.arange(img.shape[0] * 16).reshape(img.shape[0], 16) % 512
            return (torch.zeros(img.shape[0], 64, 4, 4), idx) if return_quant else idx

        def rarm_sample(self, cond_tokens, context, steps, uniforms, **kw):
            self.calls.append(dict(kw, steps=steps, cond=cond_tokens.clone(), context=context.clone()))
            return torch.full((cond_tokens.shape[0], steps), 7, dtype=torch.long)

        def vq_decode_indices(self, idx):
            self.decoded = idx.clone()
            return torch.zeros((idx.shape[0], 3, 16, 16))

    mock = Ctx()
    m = LatentImageRETRO({"params": dict(in_channels=514, out_channels=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=16)},
                         None, mask_token=512, sos_token=513, ctx=mock)
    batch = {"image": torch.zeros(5, 16, 16, 3), "nn_embeddings": torch.ones(5, 2, 512)}
    log = m.log_images(batch, N=3, top_k=20)
    assert sorted(log) == ["inputs", "reconstructions", "samples_full", "samples_full_p_0.50", "samples_full_p_1.00", "samples_half"]
    assert log["inputs"].shape == (3, 3, 16, 16) and all(v.shape == (3, 3, 16, 16) for k, v in log.items() if k != "inputs")
    full, half, p50, p100 = mock.calls
    assert full["steps"] == 16 and full["cond"].shape == (3, 1) and bool((full["cond"] == 513).all()) and full["top_k"] == 20
    assert half["steps"] == 8 and half["cond"].shape == (3, 9) and torch.equal(half["cond"][:, 1:], mock.vq_encode_indices(torch.zeros(3, 1))[:, :8])
    assert bool((full["context"] == 1).all()) and bool((p100["context"] == 512).all())
    frac = float((p50["context"] == 512).float().mean())
    assert 0.4 < frac < 0.6 and bool(((p50["context"] == 512) | (p50["context"] == 1)).all())
    assert torch.equal(mock.decoded, mock.vq_encode_indices(torch.zeros(3, 1)))          # reconstructions: decoded last, from the image's own codes
    # sample() hands back the given prefix followed by the new tokens (transformer.py:268-269)
    out = m.sample(torch.arange(6).reshape(2, 3), torch.zeros(2, 1, 512), torch.full((2, 1), 513), steps=4)
    assert out.shape == (2, 7) and torch.equal(out[:, :3], torch.arange(6).reshape(2, 3)) and bool((out[:, 3:] == 7).all())
