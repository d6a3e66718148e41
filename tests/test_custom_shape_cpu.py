"""CPU side of sampling at other image sizes: the size-per-call first-stage entries are declared and bound, MinimalRETRODiffusion hands
sizes through to the library context unchanged (decode / quantise / encode, sample_log(custom_shape=), the DDPM loop's shape=), the
sharded path draws its per-row noise at the custom shape, and scripts/rdm_sample.py validates --height / --width."""
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW_SYMBOLS = ("rdm_vq_decode_hw", "rdm_vq_quantize_hw", "rdm_vq_encode_hw")


def test_hw_entries_are_declared_and_bound():
    """Declared in the header (tests/test_library_cpu.py then requires the library to export them) with the argument lists the binding uses."""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdm_hip.h")).read(), flags=re.S)
    for name in HW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/rdm_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(","))
        assert getattr(_lib.lib, name) is not None
    # the square entries keep their signatures
    for name, nargs in (("rdm_vq_decode", 6), ("rdm_vq_quantize", 5), ("rdm_vq_encode", 4)):
        assert len(_lib.SIGNATURES[name][1]) == nargs


class StubCtx:
    """Stands in for the library context: records what reaches it, returns tensors of the shapes the library would."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def vq_decode(self, z, force_not_quantize=False, return_indices=False):
        self.calls.append(("vq_decode", z, force_not_quantize))
        return z.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)

    def vq_quantize(self, z, return_indices=False):
        self.calls.append(("vq_quantize", z))
        return z.round()

    def vq_encode(self, x):
        self.calls.append(("vq_encode", x))
        return x[:, :, ::4, ::4].contiguous()

    def ddim_sample(self, S, x_T, cond, uncond, alphas_cumprod, eta=0.0, scale=1.0, noise=None, log_every_t=100, temperature=1.0,
                    want_intermediates=False):
        self.calls.append(("ddim_sample", x_T, noise))
        return x_T * 0.5, x_T[None], x_T[None]

    def plms_sample(self, S, x_T, cond, uncond, alphas_cumprod, scale=1.0, log_every_t=100, want_intermediates=False, **kw):
        self.calls.append(("plms_sample", x_T, None))
        return x_T * 0.5, x_T[None], x_T[None]

    def ddpm_sample(self, timesteps, x_T, cond, noise, sched, clip_denoised=True, temperature=1.0):
        self.calls.append(("ddpm_sample", x_T, noise))
        return x_T * 0.25


def _model(ctx, image_size=8):
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    # default UNet cfg: four levels, down factor 8; default first stage: VQ-f4
    return MinimalRETRODiffusion(unet_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, ctx=ctx, image_size=image_size)


def test_first_stage_methods_hand_sizes_through():
    ctx = StubCtx()
    m = _model(ctx)
    z = torch.randn(2, 3, 5, 7)
    img = m.decode_first_stage(z)
    assert ctx.calls[-1][0] == "vq_decode" and torch.equal(ctx.calls[-1][1], z) and tuple(img.shape) == (2, 3, 20, 28)
    m.quantize_first_stage(z)
    assert ctx.calls[-1][0] == "vq_quantize" and torch.equal(ctx.calls[-1][1], z)
    x = torch.randn(2, 3, 32, 160)
    lat = m.encode_first_stage(x)
    assert ctx.calls[-1][0] == "vq_encode" and torch.equal(ctx.calls[-1][1], x) and tuple(lat.shape) == (2, 3, 8, 40)


def test_sample_log_custom_shape_reaches_every_sampler():
    ctx = StubCtx()
    m = _model(ctx)
    cond = torch.zeros(2, 4, 512)
    for kw, entry in ((dict(ddim=True), "ddim_sample"), (dict(ddim=True, plms=True), "plms_sample"), (dict(ddim=False, timesteps=3), "ddpm_sample")):
        ctx.calls.clear()
        z, _ = m.sample_log(cond=cond, batch_size=2, ddim_steps=4, custom_shape=(3, 16, 24), **kw)
        name, x_T, noise = ctx.calls[-1]
        assert name == entry and tuple(x_T.shape) == (2, 3, 16, 24) and tuple(z.shape) == (2, 3, 16, 24)
        if entry == "ddpm_sample":
            assert tuple(noise.shape) == (3, 2, 3, 16, 24)
    # without custom_shape: the model's own size, as before
    m.sample_log(cond=cond, batch_size=2, ddim=True, ddim_steps=4)
    assert tuple(ctx.calls[-1][1].shape) == (2, 3, 8, 8)
    # ldm's shape= on the DDPM loop
    z = m.sample(cond=cond, batch_size=2, shape=(2, 3, 24, 16), timesteps=2)
    assert tuple(z.shape) == (2, 3, 24, 16) and tuple(ctx.calls[-1][2].shape) == (2, 2, 3, 24, 16)


def test_custom_shape_must_follow_the_unet_down_factor():
    ctx = StubCtx()
    m = _model(ctx)
    cond = torch.zeros(2, 4, 512)
    for bad in ((3, 18, 24), (3, 16, 20), (4, 16, 24), (3, 0, 8), (16, 24)):
        ctx.calls.clear()
        with pytest.raises(ValueError, match="down factor 8"):
            m.sample_log(cond=cond, batch_size=2, ddim=True, ddim_steps=4, custom_shape=bad)
        with pytest.raises(ValueError, match="down factor 8"):
            m.sample_with_query(query=torch.zeros(2, 512), query_embedded=True, ddim=True, ddim_steps=4, custom_shape=bad)
        with pytest.raises(ValueError, match="down factor 8"):
            m.sample_from_rdata(2, ddim=True, ddim_steps=4, custom_shape=bad)
        assert not ctx.calls                                         # refused before anything reaches the library
    with pytest.raises(ValueError, match="down factor 8"):
        m.sample(cond=cond, batch_size=2, shape=(2, 3, 12, 16), timesteps=2)


def test_sample_shard_draws_noise_at_the_custom_shape():
    """Single-process set_distributed(): the starting noise and a DDIM eta > 0 noise stack are drawn at custom_shape, row i from
    parallel.per_sample_noise(seed, [i], shape) -- the row streams that make sharding bit-invariant."""
    from rdm_amd import parallel
    ctx = StubCtx()
    m = _model(ctx)
    m.set_distributed(True)
    shape, n, S = (3, 16, 24), 3, 5
    c = torch.zeros(n, 4, 512)
    torch.manual_seed(11)
    img = m._sample_shard(c, torch.zeros_like(c), 0, n, n, 2.0, dict(ddim=True, ddim_steps=S, eta=0.5, custom_shape=shape))
    torch.manual_seed(11)
    base = parallel.shared_seed("cpu")
    name, x_T, noise = [e for e in ctx.calls if e[0] == "ddim_sample"][-1]
    steps = len(range(0, m.num_timesteps, m.num_timesteps // S))
    assert tuple(x_T.shape) == (n,) + shape and tuple(noise.shape) == (steps, n) + shape
    for i in range(n):
        assert torch.equal(x_T[i], parallel.per_sample_noise(base, [i], shape)[0])
        assert torch.equal(noise[:, i], parallel.per_sample_noise(base + 1, [i], (steps,) + shape)[0])
    assert tuple(img.shape) == (n, 3, 64, 96)                        # decoded and "gathered" (one rank) at the custom size
    # the DDPM loop's noise stack, rows [1, 3) of a batch of 3: global row indices
    ctx.calls.clear()
    torch.manual_seed(12)
    m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, n, 1.0, dict(ddim=False, ddim_steps=None, timesteps=4, custom_shape=shape))
    torch.manual_seed(12)
    base = parallel.shared_seed("cpu")
    name, x_T, noise = [e for e in ctx.calls if e[0] == "ddpm_sample"][-1]
    assert tuple(x_T.shape) == (2,) + shape and tuple(noise.shape) == (4, 2) + shape
    assert torch.equal(x_T[0], parallel.per_sample_noise(base, [1], shape)[0])
    assert torch.equal(noise[:, 1], parallel.per_sample_noise(base + 1, [2], (4,) + shape)[0])
    # and without custom_shape the model's own size, as before
    ctx.calls.clear()
    m._sample_shard(c, torch.zeros_like(c), 0, n, n, 2.0, dict(ddim=True, ddim_steps=S))
    assert tuple([e for e in ctx.calls if e[0] == "ddim_sample"][-1][1].shape) == (n, 3, 8, 8)


def _script():
    import importlib.util
    path = os.path.join(ROOT, "scripts", "rdm_sample.py")
    spec = importlib.util.spec_from_file_location("rdm_sample_native_sizes_cpu", path)
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_rdm_sample_size_flags(capsys):
    mod = _script()
    opt = mod.parse_args([])
    assert opt.height is None and opt.width is None                 # default: the model's own size
    assert mod._sampler_kwargs(opt, None) == {}                     # ... and the calls are the reference's
    opt = mod.parse_args(["--height", "128", "--width", "256"])
    assert (opt.height, opt.width) == (128, 256)
    for bad in (["--width", "200"], ["--height", "100"], ["--height", "0"], ["--width", "-64"], ["--height", "16"]):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2                                    # argparse's parser.error
        assert "multiple of 32" in capsys.readouterr().err
    assert "--height" in mod.__doc__ and "--width" in mod.__doc__   # listed with the script's other additions

    class Model:                                                    # the shipped sizes: VQ-f4 (three levels), 64 x 64 latents, 3 channels
        class vq_cfg:
            n_ch_mult = 3
        image_size, channels = 64, 3
    kw = lambda argv: mod._sampler_kwargs(mod.parse_args(argv), Model)
    assert kw(["--height", "128", "--width", "256"]) == {"custom_shape": (3, 32, 64)}
    assert kw(["--width", "512"]) == {"custom_shape": (3, 64, 128)}                       # the other side keeps the model's own size
    assert kw(["--height", "512", "--plms"]) == {"plms": True, "custom_shape": (3, 128, 64)}
    assert kw(["--width", "256", "--dpm_solver"]) == {"dpm_solver": True, "custom_shape": (3, 64, 64)}
    assert kw(["--plms"]) == {"plms": True}


def test_reference_flag_table_still_satisfied():
    mod = _script()
    with open(os.path.join(ROOT, "tests", "golden", "rdm_sample_flags.json")) as f:
        ref = json.load(f)
    acts = {tuple(a.option_strings): a for a in mod.build_parser()._actions}
    for e in ref:
        a = acts.get(tuple(e["options"]))
        assert a is not None, f"missing flag {e['options']}"
        if e["action"] == "store_true":
            assert a.const is True and a.default is False and a.nargs == 0
        else:
            assert a.type is {"int": int, "float": float, "str": str, "Path": Path}[e["type"]], e
            assert a.default == e["default"] or str(a.default) == str(e["default"]), e
    assert ("--height",) not in {tuple(e["options"]) for e in ref} and ("--height",) in acts and ("--width",) in acts
