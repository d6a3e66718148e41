"""PLMS sampler (ldm PLMSSampler) on the CPU: accuracy on an analytic case, the per-step path against this file's own restatement of
ldm's p_sample_plms, the reference-style surface and its wiring into MinimalRETRODiffusion.sample_log and scripts/rdm_sample.py, and
the C ABI entry point."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


class GaussianEps:
    """Stand-in model for data ~ N(0, s^2) per element: the exact optimal eps of x_t = sqrt(ab) x0 + sqrt(1 - ab) e is
    sqrt(1 - ab) x_t / (ab s^2 + 1 - ab).  Only what the per-step path reads: num_timesteps, alphas_cumprod, device, apply_model."""

    def __init__(self, s):
        self.s = s
        self.num_timesteps = 1000
        self.device = torch.device("cpu")
        self.alphas_cumprod = torch.as_tensor(odiff.Schedule().alphas_cumprod)

    def apply_model(self, x, t, c):
        ab = self.alphas_cumprod.double()[t].reshape(-1, 1, 1, 1)
        return (torch.sqrt(1 - ab) * x.double() / (ab * self.s ** 2 + 1 - ab)).float()


class CondModel:
    """Stand-in whose output depends on the conditioning row by row (so the guidance combine matters)."""
    num_timesteps = 1000
    device = torch.device("cpu")

    def __init__(self):
        self.alphas_cumprod = torch.as_tensor(odiff.Schedule().alphas_cumprod)

    def apply_model(self, x, t, c):
        ab = self.alphas_cumprod[t].reshape(-1, 1, 1, 1)
        return torch.tanh(0.7 * x) * torch.sqrt(1 - ab) + c.mean(dim=(1, 2)).reshape(-1, 1, 1, 1) * 0.3 + 0.01 * t.float().reshape(-1, 1, 1, 1) / 1000


def _ode_solution(model, x_T, S):
    """For Gaussian data the probability-flow ODE keeps x_t / std(x_t): the exact endpoint of the sampler's trajectory, which starts
    at the largest DDIM timestep and ends at alphas_cumprod[0]."""
    ac = model.alphas_cumprod.double()
    var = lambda a: a * model.s ** 2 + 1 - a
    return x_T.double() * torch.sqrt(var(ac[0]) / var(ac[int(odiff.make_ddim_timesteps(S)[-1])]))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_plms_converges_faster_than_ddim_on_the_gaussian_case(s):
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    from rdm_amd.models.diffusion.plms import PLMSSampler
    m = GaussianEps(s)
    x_T = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(0))
    c = torch.zeros(2, 1, 8)
    err = {}
    for name, cls, S in (("ddim50", DDIMSampler, 50), ("plms25", PLMSSampler, 25), ("plms50", PLMSSampler, 50)):
        z, _ = cls(m).sample(S, 2, (3, 16, 16), conditioning=c, x_T=x_T, verbose=False, callback=lambda i: None)
        err[name] = _rel(z, _ode_solution(m, x_T, S))
    print(f"[plms] s={s}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert err["plms25"] < err["ddim50"]
    assert err["plms50"] <= 0.15 * err["ddim50"]


def _plms_restated(model, S, x_T, c, uc, scale, mask=None, x0=None, q_noise=None, log_every_t=1):
    """ldm PLMSSampler.plms_sampling / p_sample_plms (eta = 0), written out here: guided eps e_u + scale (e_c - e_u); the first step
    averages e_t with the eps at t_next of x_tmp = update(x, e_t); later steps use the Adams-Bashforth combinations of the stored
    e_t; the update always starts from the step's input x."""
    ac = model.alphas_cumprod.float()
    ts = odiff.make_ddim_timesteps(S)
    a_t = ac[ts]
    a_prev = torch.cat([ac[:1], ac[ts[:-1]]])
    s1m = torch.from_numpy(np.sqrt(1. - a_t.numpy()))
    total = len(ts)
    time_range = np.flip(ts)
    b = x_T.shape[0]
    tfull = lambda v: torch.full((b,), int(v), dtype=torch.long)

    def eps(x, t):
        if uc is None or scale == 1.:
            return model.apply_model(x, t, c)
        e_c, e_u = model.apply_model(x, t, c), model.apply_model(x, t, uc)
        return e_u + scale * (e_c - e_u)

    def update(x, e, i):
        x0_ = (x - s1m[i] * e) / a_t[i].sqrt()
        return a_prev[i].sqrt() * x0_ + (1. - a_prev[i]).sqrt() * e, x0_

    x = x_T
    old = []
    inter = {"x_inter": [x_T], "pred_x0": [x_T]}
    n_forwards = 0
    for i, step in enumerate(time_range):
        index = total - i - 1
        t = tfull(step)
        if mask is not None:
            sa = torch.sqrt(model.alphas_cumprod.double()).float()[t].reshape(-1, 1, 1, 1)
            sb = torch.sqrt(1. - model.alphas_cumprod.double()).float()[t].reshape(-1, 1, 1, 1)
            x = (sa * x0 + sb * q_noise[i]) * mask + (1. - mask) * x
        e_t = eps(x, t); n_forwards += 1
        if len(old) == 0:
            x_tmp, _ = update(x, e_t, index)
            e_next = eps(x_tmp, tfull(time_range[min(i + 1, total - 1)])); n_forwards += 1
            e_p = (e_t + e_next) / 2
        elif len(old) == 1:
            e_p = (3 * e_t - old[-1]) / 2
        elif len(old) == 2:
            e_p = (23 * e_t - 16 * old[-1] + 5 * old[-2]) / 12
        else:
            e_p = (55 * e_t - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24
        x, pred_x0 = update(x, e_p, index)
        old.append(e_t)
        if len(old) == 4:
            old.pop(0)
        if index % log_every_t == 0 or index == total - 1:
            inter["x_inter"].append(x)
            inter["pred_x0"].append(pred_x0)
    return x, inter, n_forwards


class _Counting(CondModel):
    def __init__(self):
        super().__init__()
        self.calls = 0

    def apply_model(self, x, t, c):
        self.calls += 1
        return super().apply_model(x, t, c)


@pytest.mark.parametrize("masked", [False, True])
def test_per_step_path_equals_restatement_bitwise(masked):
    """S = 6 (seven timesteps: the Euler step and all three multistep orders), CFG 2.0, with and without an inpainting mask."""
    from rdm_amd.models.diffusion.plms import PLMSSampler
    g = torch.Generator().manual_seed(4)
    B, S = 3, 6
    x_T = torch.randn(B, 3, 8, 8, generator=g)
    c = torch.randn(B, 2, 8, generator=g)
    uc = torch.zeros_like(c)
    kw = {}
    if masked:
        mask = (torch.rand(B, 1, 8, 8, generator=g) > 0.5).float()
        x0 = torch.randn(B, 3, 8, 8, generator=g)
        q_noise = torch.randn(7, B, 3, 8, 8, generator=g)
        kw = dict(mask=mask, x0=x0, q_noise=q_noise)
    m = _Counting()
    seen, seen_img = [], []
    z, inter = PLMSSampler(m).sample(S, B, (3, 8, 8), conditioning=c, x_T=x_T, verbose=False, log_every_t=1,
                                     unconditional_guidance_scale=2.0, unconditional_conditioning=uc,
                                     callback=seen.append, img_callback=lambda x, i: seen_img.append(i), **kw)
    z_ref, inter_ref, n_fwd = _plms_restated(CondModel(), S, x_T, c, uc, 2.0, log_every_t=1, **kw)
    assert torch.equal(z, z_ref)
    assert len(inter["x_inter"]) == len(inter_ref["x_inter"]) == 8 and len(inter["pred_x0"]) == 8
    for a, b in zip(inter["x_inter"] + inter["pred_x0"], inter_ref["x_inter"] + inter_ref["pred_x0"]):
        assert torch.equal(a, b)
    assert seen == list(range(7)) and seen_img == list(range(7))
    assert m.calls == n_fwd == 8                       # total + 1 forwards (each guided forward is one doubled batch)


def test_per_step_path_without_guidance_and_logging_rule():
    from rdm_amd.models.diffusion.plms import PLMSSampler
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(2, 3, 8, 8, generator=g)
    c = torch.randn(2, 2, 8, generator=g)
    z, inter = PLMSSampler(CondModel()).sample(10, 2, (3, 8, 8), conditioning=c, x_T=x_T, verbose=False, log_every_t=4,
                                                callback=lambda i: None)
    z_ref, inter_ref, _ = _plms_restated(CondModel(), 10, x_T, c, None, 1.0, log_every_t=4)
    assert torch.equal(z, z_ref)
    assert len(inter["x_inter"]) == len(inter_ref["x_inter"]) == 1 + 4         # indices 9 (first), 8, 4, 0
    for a, b in zip(inter["pred_x0"], inter_ref["pred_x0"]):
        assert torch.equal(a, b)


def test_surface_errors():
    from rdm_amd.models.diffusion.plms import PLMSSampler
    sm = PLMSSampler(CondModel())
    with pytest.raises(ValueError, match="ddim_eta must be 0 for PLMS"):
        sm.make_schedule(10, ddim_eta=0.3)
    with pytest.raises(ValueError):
        sm.sample(10, 1, (3, 8, 8), conditioning=torch.zeros(1, 2, 8), eta=0.5, verbose=False)
    sm.make_schedule(10)
    with pytest.raises(NotImplementedError):
        sm.plms_sampling(torch.zeros(1, 2, 8), (1, 3, 8, 8), ddim_use_original_steps=True)


def test_sample_log_selects_plms():
    """MinimalRETRODiffusion.sample_log(plms=True) samples with PLMSSampler on S = ddim_steps; without it, DDIM as before."""
    from rdm_amd.models.diffusion import ddpm as ddpm_mod
    used = []

    def recorder(name):
        class Rec:
            def __init__(self, model):
                pass

            def sample(self, S, batch_size, shape, **kw):
                used.append((name, S, batch_size, shape))
                return "z", {}
        return Rec

    class Stand:
        channels, image_size = 3, 8

    orig = ddpm_mod.PLMSSampler, ddpm_mod.DDIMSampler
    ddpm_mod.PLMSSampler, ddpm_mod.DDIMSampler = recorder("plms"), recorder("ddim")
    try:
        f = ddpm_mod.MinimalRETRODiffusion.sample_log
        f(Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=25, plms=True)
        f(Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=25)
        f(Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=25, plms=False)
    finally:
        ddpm_mod.PLMSSampler, ddpm_mod.DDIMSampler = orig
    assert used == [("plms", 25, 2, (3, 8, 8)), ("ddim", 25, 2, (3, 8, 8)), ("ddim", 25, 2, (3, 8, 8))]


def _script():
    path = os.path.join(ROOT, "scripts", "rdm_sample.py")
    spec = importlib.util.spec_from_file_location("rdm_sample_plms", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("caption", ["", "a dog"])
def test_rdm_sample_plms_flag_reaches_sample_log(tmp_path, caption):
    """--plms parses, and both run loops hand plms=True through sample_with_query / sample_from_rdata to sample_log; without the
    flag, plms is absent."""
    from rdm_amd.models.diffusion import ddpm as ddpm_mod
    mod = _script()
    assert mod.parse_args([]).plms is False and mod.parse_args(["--plms"]).plms is True
    logged = []

    class Clip:
        def encode_text(self, tokens):
            return torch.ones(tokens.shape[0], 512)

    class Model:
        device = torch.device("cpu")
        channels, image_size = 3, 4

        class retriever:
            class retriever:
                model = Clip()

        def get_qids(self, top_m, n, use_weights=False):
            return np.arange(n)

        def _sample(self, n, kw):
            logged.append(dict(kw))
            kw = {k: v for k, v in kw.items() if k in ("ddim", "ddim_steps", "plms")}
            z, _ = ddpm_mod.MinimalRETRODiffusion.sample_log(self, cond=None, batch_size=n, **kw)
            return torch.zeros(n, 3, 4, 4) + z

        def sample_with_query(self, **kw):
            return {"query_samples": self._sample(kw["query"].shape[0], kw)}

        def sample_from_rdata(self, n, **kw):
            return {"samples_with_sampled_nns": self._sample(n, kw)}

    seen = []

    class Rec:
        def __init__(self, model, which):
            self.which = which

        def sample(self, S, batch_size, shape, **kw):
            seen.append((self.which, S))
            return torch.tensor(0.5), {}

    orig = ddpm_mod.PLMSSampler, ddpm_mod.DDIMSampler
    ddpm_mod.PLMSSampler, ddpm_mod.DDIMSampler = (lambda m: Rec(m, "plms")), (lambda m: Rec(m, "ddim"))
    try:
        base = ["-s", str(tmp_path), "-bs", "2", "-n", "1", "--steps", "25"] + (["-c", caption] if caption else [])
        run = mod.sample_conditional if caption else mod.sample_unconditional
        run(Model(), mod.parse_args(base + ["--plms"]))
        run(Model(), mod.parse_args(base))
    finally:
        ddpm_mod.PLMSSampler, ddpm_mod.DDIMSampler = orig
    assert logged[0]["plms"] is True and not logged[1].get("plms", False)
    assert seen == [("plms", 25), ("ddim", 25)]


def test_rdm_plms_sample_in_header_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdm_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+rdm_plms_sample\s*\(([^)]*)\)\s*;", src)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args[0].startswith("rdm_ctx*") and args[1].startswith("const rdm_ddim_args*") and len(args) == 8
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    assert hasattr(_lib.lib, "rdm_plms_sample") and "rdm_plms_sample" in _lib.SIGNATURES
