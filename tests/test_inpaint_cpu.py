"""DDIM inpainting without a GPU: the blend's restatements against each other, the per-step path of decode(mask=) against sample(mask=)
and where its known-region noise comes from, the routing of inpaint_mask / keep_known from sample_log, sample_with_query's row
cutting, the mask's two forms, the refusals (raised before a library context is touched: the stand-in models have none), the script's
--mask flag, the generator's stream 0 beyond step 0, and the new C ABI symbols."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff

import _inpaint_ref as ref
import _rng_ref as rng_ref
from test_img2img_cpu import _Rec, _Stand
from test_plms_cpu import CondModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACP = odiff.Schedule().alphas_cumprod
torch.set_grad_enabled(False)

DECODE_KEYS_TODAY = {"unconditional_guidance_scale", "unconditional_conditioning", "callback", "img_callback", "eta", "temperature", "noise",
                     "noise_seed", "noise_row0", "log_every_t", "return_intermediates", "intermediates_to_cpu"}


# ---- the restatements
@pytest.mark.parametrize("soft", [False, True])
def test_fp32_evaluation_lies_inside_the_fp64_bound_and_the_fma_form_differs_from_it(soft):
    """What the GPU test asks of the kernel, asked of the numpy fp32 evaluation: inside K(4) 2^-24 A, and the contracted form -- also
    inside, since contraction removes a rounding -- differs from it in some elements."""
    sa, s1m = ref.level_scalars(float(ACP[601]))
    x, x0, z, m = ref.inputs((3, 3, 8, 8), 1, soft, seed=1)
    got = ref.blend_fp32(x, x0, z, m, sa, s1m)
    print("[inpaint] fp32 evaluation: " + ref.check(got, x, x0, z, m, sa, s1m))
    want, tol, _ = ref.blend(x, x0, z, m, sa, s1m)
    miss = ref.blend_fp32(x, x0, z, m, sa, s1m, contracted=True)
    assert (np.abs(miss.astype(np.float64) - want) <= tol).all() and (miss != got).any()
    assert ref.K_BLEND == 6
    if not soft:
        mb = np.broadcast_to(m, x.shape)
        assert np.array_equal(got[mb == 0], x[mb == 0])
        assert np.array_equal(got[mb == 1], (np.float32(sa) * x0 + np.float32(s1m) * z)[mb == 1])


# ---- the per-step path
class _Ctx:
    """What _device_randn asks of a library context, recording"""

    def __init__(self):
        self.calls = []

    def op_randn(self, seed, B, per_row, row0=0, step=0, stream=0):
        self.calls.append((seed, B, per_row, row0, step, stream))
        return torch.from_numpy(rng_ref.normals(seed, row0, B, per_row, step, stream)[0]).float()


def _case():
    g = torch.Generator().manual_seed(2)
    B, S = 2, 7                                                # eight timesteps: total != S
    r = lambda *s: torch.randn(*s, generator=g)
    x_T, x0, c = r(B, 3, 8, 8), r(B, 3, 8, 8) * 0.5, r(B, 2, 8)
    mask = (torch.rand(B, 1, 8, 8, generator=g) > 0.5).float()
    return B, S, x_T, x0, c, torch.zeros_like(c), mask, r(8, B, 3, 8, 8)


def test_decode_with_a_mask_and_a_callback_is_samples_per_step_path():
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    B, S, x_T, x0, c, uc, mask, qn = _case()
    kw = dict(unconditional_guidance_scale=2.0, unconditional_conditioning=uc, callback=lambda i: None)
    z, _ = DDIMSampler(CondModel()).sample(S, B, (3, 8, 8), conditioning=c, x_T=x_T, verbose=False, mask=mask, x0=x0, q_noise=qn, **kw)
    sm = DDIMSampler(CondModel())
    sm.make_schedule(S, verbose=False)
    total = sm.ddim_timesteps.shape[0]
    assert total == 8
    z2 = sm.decode(x_T, c, total, mask=mask, x0=x0, q_noise=qn, **kw)
    assert torch.equal(z, z2)
    assert not torch.equal(z2, sm.decode(x_T, c, total, **kw))
    # a partial decode consumes q_noise from its own step 0 and blends at its own levels: the float64 restatement
    t_start = 5
    z3 = sm.decode(x_T, c, t_start, mask=mask, x0=x0, q_noise=qn[:t_start], **kw)
    ts, a_t = ref.schedule(ACP, S)
    m = CondModel()
    x = x_T.double()
    for i in range(t_start):
        index = t_start - 1 - i
        a = float(a_t[index])
        x = (np.sqrt(a) * x0.double() + np.sqrt(1 - a) * qn[i].double()) * mask.double() + (1 - mask.double()) * x
        tt = torch.full((B,), int(ts[index]), dtype=torch.long)
        e_c, e_u = m.apply_model(x.float(), tt, c).double(), m.apply_model(x.float(), tt, uc).double()
        e = e_u + 2.0 * (e_c - e_u)
        a_prev = float(ACP[0]) if index == 0 else float(a_t[index - 1])
        p0 = (x - np.sqrt(1 - a) * e) / np.sqrt(a)
        x = np.sqrt(a_prev) * p0 + np.sqrt(1 - a_prev) * e
    assert float((z3.double() - x).norm() / x.norm()) <= 1e-5


def test_known_region_noise_of_the_per_step_path():
    """decode(mask=, noise_seed=, callback=): step i's q_sample noise is the library's (stream 0, step i + 1, noise_row0) -- reached through
    _python_loop's own argument; sample(mask=, noise_seed=) keeps drawing it from torch, and asks the library for the start only."""
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    B, S, x_T, x0, c, uc, mask, _ = _case()
    m = CondModel()
    m.ctx = _Ctx()
    sm = DDIMSampler(m)
    sm.make_schedule(S, verbose=False)
    z = sm.decode(x_T, c, 3, mask=mask, x0=x0, noise_seed=5, noise_row0=4, callback=lambda i: None)
    assert m.ctx.calls == [(5, B, 3 * 8 * 8, 4, i + 1, 0) for i in range(3)]
    qn = torch.stack([torch.from_numpy(rng_ref.normals(5, 4, B, 192, i + 1, 0)[0]).float().reshape(B, 3, 8, 8) for i in range(3)])
    assert torch.equal(z, sm.decode(x_T, c, 3, mask=mask, x0=x0, q_noise=qn, callback=lambda i: None))
    m.ctx.calls.clear()
    torch.manual_seed(3)
    a, _ = DDIMSampler(m).sample(S, B, (3, 8, 8), conditioning=c, verbose=False, mask=mask, x0=x0, noise_seed=5)
    assert m.ctx.calls == [(5, B, 192, 0, 0, 0)]                               # the starting latent, nothing else
    torch.manual_seed(4)
    b, _ = DDIMSampler(m).sample(S, B, (3, 8, 8), conditioning=c, verbose=False, mask=mask, x0=x0, noise_seed=5)
    assert not torch.equal(a, b)                                               # torch's generator drew the known region's noise


def test_decode_refusals_are_raised_before_any_context_is_touched():
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    B, S, x_T, x0, c, uc, mask, qn = _case()
    sm = DDIMSampler(CondModel())
    sm.make_schedule(S, verbose=False)
    with pytest.raises(ValueError, match="x0"):
        sm.decode(x_T, c, 3, mask=mask)
    with pytest.raises(ValueError, match="mask"):
        sm.decode(x_T, c, 3, x0=x0)
    with pytest.raises(ValueError, match="mask"):
        sm.decode(x_T, c, 3, q_noise=qn[:3])
    with pytest.raises(ValueError, match="q_noise"):
        sm.decode(x_T, c, 3, mask=mask, x0=x0, q_noise=qn[:3], noise_seed=1)
    for bad in (mask[:, :, :4], mask.expand(-1, 2, -1, -1), torch.ones(3, 1, 8, 8), mask[0]):
        with pytest.raises(ValueError, match="mask must be"):
            sm.decode(x_T, c, 3, mask=bad, x0=x0)
    with pytest.raises(ValueError, match="x0 must have"):
        sm.decode(x_T, c, 3, mask=mask, x0=x0[:1])


# ---- routing
class _RecKeep(_Rec):
    def keep_known(self, x, x0, mask):
        _Rec.calls.append(("keep_known", float(x.flatten()[0]), x0, mask))
        return x + 10


def test_sample_log_routes_inpaint_mask_and_keep_known(monkeypatch):
    from rdm_amd.models.diffusion import ddpm as ddpm_mod
    monkeypatch.setattr(ddpm_mod, "DDIMSampler", _RecKeep)
    f = ddpm_mod.MinimalRETRODiffusion.sample_log
    lat = torch.zeros(2, 3, 8, 8)
    uc = torch.zeros(2, 4, 8)
    mask = (torch.arange(64).reshape(1, 1, 8, 8) % 3 == 0).float()
    common = dict(cond="c", batch_size=2, ddim=True, ddim_steps=7, init_latent=lat, strength=0.5, unconditional_guidance_scale=3.0,
                  unconditional_conditioning=uc, noise_seed=11, noise_row0=4, eta=0.3, log_every_t=2)
    _Rec.calls = []
    f(_Stand(), **common)
    today = list(_Rec.calls)
    assert [c[0] for c in today] == ["make_schedule", "stochastic_encode", "decode"] and set(today[2][3]) == DECODE_KEYS_TODAY
    _Rec.calls = []
    z, inter = f(_Stand(), inpaint_mask=mask, **common)
    ms, se, de, kk = _Rec.calls
    assert (ms, se[:2]) == (today[0], today[1][:2]) and se[2] == today[1][2]
    assert de[:3] == today[2][:3]
    kw = dict(de[3])
    got_mask, got_x0 = kw.pop("mask"), kw.pop("x0")
    assert kw.pop("q_noise") is None and set(kw) == DECODE_KEYS_TODAY
    assert all(kw[k] is today[2][3][k] or kw[k] == today[2][3][k] for k in kw)
    assert got_x0 is lat and tuple(got_mask.shape) == (1, 1, 8, 8) and got_mask.dtype == torch.float32 and torch.equal(got_mask, mask)
    assert kk[0] == "keep_known" and kk[1] == 1.0 and kk[2] is lat and kk[3] is got_mask
    assert torch.equal(z, lat + 1 + 10) and "x_inter" in inter
    # keep_known=False: no final blend; an explicit q_noise stack is cut to the steps run, like the update noise
    _Rec.calls = []
    z, _ = f(_Stand(), inpaint_mask=mask[0, 0], keep_known=False, q_noise=torch.zeros(8, 2, 3, 8, 8), **{**common, "noise_seed": None})
    assert [c[0] for c in _Rec.calls] == ["make_schedule", "stochastic_encode", "decode"] and torch.equal(z, lat + 1)
    assert _Rec.calls[2][3]["q_noise"].shape[0] == 4 and tuple(_Rec.calls[2][3]["mask"].shape) == (1, 1, 8, 8)
    # mask= together with init_latent still raises, with or without inpaint_mask
    for extra in ({}, dict(inpaint_mask=mask)):
        with pytest.raises(ValueError, match="does not take"):
            f(_Stand(), mask=torch.ones(2, 1, 8, 8), **extra, **common)


def test_sample_log_refusals_are_raised_before_any_gpu_work():
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion as M
    lat = torch.zeros(2, 3, 8, 8)
    mask = torch.ones(2, 1, 8, 8)
    run = lambda **kw: M.sample_log(_Stand(), cond=None, batch_size=2, ddim=kw.pop("ddim", True), ddim_steps=6, **kw)
    with pytest.raises(ValueError, match="invert"):
        run(init_latent=lat, strength=0.5, inpaint_mask=mask, invert=True)
    with pytest.raises(ValueError, match="init_image or init_latent"):
        run(inpaint_mask=mask)
    for sampler in ("plms", "dpm_solver", "uni_pc", "dpm_solver_sde"):
        with pytest.raises(ValueError, match="DDIM"):
            run(init_latent=lat, strength=0.5, inpaint_mask=mask, **{sampler: True})
    with pytest.raises(ValueError, match="DDIM"):
        run(init_latent=lat, strength=0.5, inpaint_mask=mask, ddim=False)
    for bad in (mask * 1.01, mask - 1.01, torch.full_like(mask, float("nan"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            run(init_latent=lat, strength=0.5, inpaint_mask=bad)
    for bad in (mask[:, :, :4], torch.ones(3, 1, 8, 8), torch.ones(2, 3, 8, 8), torch.ones(8), torch.ones(1, 1, 1, 8, 8)):
        with pytest.raises(ValueError, match="inpaint_mask"):
            run(init_latent=lat, strength=0.5, inpaint_mask=bad)
    st = _Stand()
    st.vq_cfg = type("V", (), {"n_ch_mult": 3})
    with pytest.raises(ValueError, match="image resolution"):
        M.sample_log(st, cond=None, batch_size=2, ddim=True, ddim_steps=6, init_latent=lat, strength=0.5, inpaint_mask=torch.ones(2, 16, 16))
    # sample_with_query and sample_from_rdata refuse the same before the retrieval (the stand-in has no retriever)
    q = lambda **kw: M.sample_with_query(_Stand(), query=torch.zeros(2, 512), query_embedded=True, ddim=True, ddim_steps=6, **kw)
    r = lambda **kw: M.sample_from_rdata(_Stand(), 2, ddim=True, ddim_steps=6, **kw)
    for call in (q, r):
        with pytest.raises(ValueError, match="init_image or init_latent"):
            call(inpaint_mask=mask)
        with pytest.raises(ValueError, match="invert"):
            call(init_latent=lat, inpaint_mask=mask, invert=True)
        with pytest.raises(ValueError, match="DDIM"):
            call(init_latent=lat, inpaint_mask=mask, uni_pc=True)
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            call(init_latent=lat, inpaint_mask=mask * 2)


def test_mask_forms_and_the_area_average():
    from rdm_amd.models.diffusion.ddpm import inpaint_mask_to_latent
    no_factor = lambda: pytest.fail("a latent-resolution mask asked for the first stage's factor")
    m = torch.rand(2, 1, 4, 6)
    assert torch.equal(inpaint_mask_to_latent(m, (4, 6), no_factor, rows=2), m)
    assert torch.equal(inpaint_mask_to_latent(m[0, 0], (4, 6), no_factor, rows=5), m[:1])
    assert torch.equal(inpaint_mask_to_latent(m[:1].numpy(), (4, 6), no_factor), m[:1])
    # 2 x 2 -> 1: the share of the latent pixel's image area that is kept
    for block, want in (([[1, 0], [1, 1]], 0.75), ([[0, 0], [0, 1]], 0.25), ([[1, 1], [1, 1]], 1.0), ([[0.5, 0.25], [0, 0.25]], 0.25)):
        got = inpaint_mask_to_latent(torch.tensor([block], dtype=torch.float32), (1, 1), lambda: 2)
        assert tuple(got.shape) == (1, 1, 1, 1) and float(got) == want
    big = (torch.rand(3, 8, 12) > 0.5).float()
    got = inpaint_mask_to_latent(big, (2, 3), lambda: 4, rows=3)
    assert tuple(got.shape) == (3, 1, 2, 3) and np.array_equal(got.numpy(), ref.area_average(big.numpy(), 4).astype(np.float32))
    assert float(got[1, 0, 1, 2]) == float(big[1, 4:8, 8:12].mean())
    with pytest.raises(ValueError, match="image resolution"):
        inpaint_mask_to_latent(big, (2, 3), lambda: 2)


def test_a_rank_takes_its_own_rows_of_the_mask():
    st = _Stand()
    st.encode_first_stage = lambda x: pytest.fail("a latent was given: nothing to encode")
    lat = torch.arange(4.).reshape(4, 1, 1, 1).expand(4, 3, 8, 8)
    mask = (torch.arange(4.) / 4).reshape(4, 1, 1, 1).expand(4, 1, 8, 8)
    kw = {}
    st._img2img_kwargs(kw, 4, 1, 3, None, lat, 0.5, False, mask, False)
    assert kw["inpaint_mask"][:, 0, 0, 0].tolist() == [0.25, 0.5] and kw["keep_known"] is False and kw["init_latent"][:, 0, 0, 0].tolist() == [1., 2.]
    kw = {}
    st._img2img_kwargs(kw, 4, 2, 4, None, lat, 0.5, False, mask[3, 0])         # one [h, w] mask: every row's
    assert tuple(kw["inpaint_mask"].shape) == (1, 1, 8, 8) and kw["keep_known"] is True and float(kw["inpaint_mask"][0, 0, 0, 0]) == 0.75
    with pytest.raises(ValueError, match="one row or one per sample"):
        st._img2img_kwargs({}, 4, 1, 3, None, lat, 0.5, False, mask[:3])
    kw = {}
    st._img2img_kwargs(kw, 4, 1, 3, None, lat, 0.5, False)                     # without a mask: today's keywords
    assert set(kw) == {"init_latent", "strength", "invert"}


# ---- the script
def _script():
    spec = importlib.util.spec_from_file_location("rdm_sample_inpaint", os.path.join(ROOT, "scripts", "rdm_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_mask_flag(tmp_path, capsys):
    """--mask parses, needs --init_img, is refused with --invert and the multistep samplers, and arrives as inpaint_mask [1, H, W] at the
    call's size with white = repaint turned into 0 = repaint; without the flag the keyword is absent."""
    from PIL import Image
    mod = _script()
    png, mpng = tmp_path / "init.png", tmp_path / "mask.png"
    Image.fromarray((np.random.default_rng(0).random((16, 16, 3)) * 255).astype(np.uint8)).save(png)
    grey = np.zeros((16, 16), np.uint8)
    grey[:, 8:] = 255
    grey[0, 0] = 51
    Image.fromarray(grey).save(mpng)
    assert mod.parse_args([]).mask is None
    assert "[native]" in next(a.help for a in mod.build_parser()._actions if "--mask" in a.option_strings)
    for bad in (["--mask", str(mpng)], ["--init_img", str(png), "--mask", str(mpng), "--invert"],
                ["--init_img", str(png), "--mask", str(mpng), "--plms"], ["--init_img", str(png), "--mask", str(mpng), "--dpm_solver_sde"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    capsys.readouterr()
    logged = []

    class Model:
        device = torch.device("cpu")
        channels, image_size = 3, 4

        class vq_cfg:
            n_ch_mult = 3

        def get_qids(self, top_m, n, use_weights=False):
            return np.arange(n)

        def sample_from_rdata(self, n, **kw):
            logged.append(kw)
            return {"samples_with_sampled_nns": torch.zeros(n, 3, 16, 16)}

    base = ["-s", str(tmp_path), "-bs", "2", "-n", "1", "--steps", "6", "--init_img", str(png)]
    mod.sample_unconditional(Model(), mod.parse_args(base + ["--mask", str(mpng), "--strength", "0.5"]))
    mod.sample_unconditional(Model(), mod.parse_args(base))
    with_mask, plain = logged
    assert "inpaint_mask" not in plain and "keep_known" not in plain and "keep_known" not in with_mask
    m = with_mask["inpaint_mask"]
    assert tuple(m.shape) == (1, 16, 16) and m.dtype == torch.float32 and with_mask["strength"] == 0.5
    assert float(m[0, 5, 12]) == 0.0 and float(m[0, 5, 3]) == 1.0              # white = repaint = 0; black = keep = 1
    assert abs(float(m[0, 0, 0]) - (1.0 - 51.0 / 255.0)) < 1e-6
    kw = mod._sampler_kwargs(mod.parse_args(base + ["--mask", str(mpng), "--height", "32", "--width", "64"]), Model())
    assert tuple(kw["inpaint_mask"].shape) == (1, 32, 64) and kw["custom_shape"] == (3, 8, 16) and tuple(kw["init_image"].shape) == (1, 32, 64, 3)


def test_reference_flag_table_is_untouched_by_the_mask_flag():
    import json
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "rdm_sample_flags.json")))
    assert '"mask"' not in json.dumps(table) and "--mask" not in json.dumps(table)


# ---- the generator and the C ABI
def test_stream_0_beyond_step_0_is_the_reference_generator():
    """The known region's noise is stream 0 at step i + 1: the host function returns the reference's words there, they differ from step
    0's (the starting latent) and from stream 1's (the update noise) at the same step, and the stream count stays 2."""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    rng = np.random.default_rng(7)
    for _ in range(200):
        seed, row, block = int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))
        step = int(rng.integers(1, 1001))
        got = _lib.rng_words(seed, row, step, 0, block)
        assert np.array_equal(got, rng_ref.block_words(seed, row, step, 0, block)), (seed, row, step, block)
        assert not np.array_equal(got, _lib.rng_words(seed, row, 0, 0, block)) and not np.array_equal(got, _lib.rng_words(seed, row, step, 1, block))
    src = open(os.path.join(ROOT, "retrieval-augmented-diffusion-models_amd", "csrc", "philox.h")).read()
    assert re.search(r"#define\s+RDM_RNG_STREAMS\s+2u", src)


def test_inpaint_symbols_in_header_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdm_hip.h")).read(), flags=re.S)
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    n_args = {"rdm_op_masked_blend": 14, "rdm_ddim_inpaint": 14}
    for name, n in n_args.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib, name)
        assert re.search(r"int\s+" + name + r"\s*\(\s*rdm_ctx\*", src)
    for name in ("rdm_op_masked_blend_seeded", "rdm_ddim_inpaint_seeded"):      # the twins the one rdm_noise argument replaced
        assert not re.search(r"\b" + name + r"\b", src) and name not in _lib.SIGNATURES, name
    assert re.search(r"int\s+rdm_ddim_inpaint\s*\(\s*rdm_ctx\*\s*\w+,\s*const rdm_ddim_args\*\s*\w+,\s*int\s+t_start", src)
    for m in ("ddim_inpaint", "op_masked_blend"):
        assert callable(getattr(_lib.Context, m))
    assert [f[0] for f in _lib.DdimArgs._fields_] == ["S", "batch", "k", "channels", "height", "width", "eta", "temperature",
                                                      "unconditional_guidance_scale", "log_every_t", "T", "alphas_cumprod"]


def test_a_sharded_run_without_device_noise_draws_the_known_regions_noise_row_by_row(monkeypatch):
    """Rows [1, 3) of a batch of 3 through _sample_shard with a mask: q_noise is one torch stream per GLOBAL row (the call's shared seed
    + 2), [n, b, C, H, W] for the n steps the strength runs, like x_T and the update noise; with device_noise nothing is drawn."""
    from rdm_amd import parallel
    from test_device_noise_cpu import StubCtx, _model
    m = _model(StubCtx())
    m.set_distributed(True)
    seen = []
    monkeypatch.setattr(m, "sample_log", lambda **kw: (seen.append(kw), (torch.zeros(2, 3, 8, 8), {}))[1])
    c = torch.zeros(3, 4, 512)
    kw = lambda: dict(ddim=True, ddim_steps=5, init_latent=torch.zeros(2, 3, 8, 8), strength=0.6, invert=False, inpaint_mask=torch.ones(2, 1, 8, 8),
                      keep_known=True)
    torch.manual_seed(5)
    m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, 3, 2.0, kw())
    torch.manual_seed(5)
    base = parallel.shared_seed("cpu")
    got = seen[-1]
    assert torch.equal(got["q_noise"], parallel.per_sample_noise(base + 2, [1, 2], (3, 3, 8, 8)).transpose(0, 1).contiguous())   # n = int(0.6 * 5)
    assert torch.equal(got["x_T"], parallel.per_sample_noise(base, [1, 2], (3, 8, 8))) and got.get("noise") is None
    m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, 3, 2.0, kw(), device_noise=True)
    assert "q_noise" not in seen[-1] and seen[-1]["noise_row0"] == 1
    plain = {k: v for k, v in kw().items() if k not in ("inpaint_mask", "keep_known")}
    m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, 3, 2.0, plain)
    assert "q_noise" not in seen[-1]
