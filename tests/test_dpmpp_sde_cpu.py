"""SDE-DPM-Solver++(2M) on the CPU: the Python coefficient helper against the D-form restatement of tests/_dpmpp_sde_ref.py, the analytic
Gaussian case (the recorded table, the error trend, and that the SDE run forgets its start where the ODE run cannot), the per-step path
against the restatement, the refusals, and the wiring into MinimalRETRODiffusion.sample_log / _sample_shard, scripts/rdm_sample.py and the
C ABI."""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff

import _dpmpp_sde_ref as ref
from rdm_amd.models.diffusion.dpm_solver import DPMSolverSDESampler, DPMSolverSampler, dpmpp_sde_coefficients
from test_device_noise_cpu import StubCtx, _last, _model
from test_plms_cpu import CondModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

ACP = np.ascontiguousarray(odiff.Schedule().alphas_cumprod.numpy(), dtype=np.float32)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- coefficients
@pytest.mark.parametrize("S", [5, 10, 20])
def test_coefficient_helper_equals_the_d_form(S):
    """Every step of the logSNR grid at order 2 with lower_order_final on (a first-order start, second-order steps, a first-order end):
    the flattened c_x, c_0, c_1, c_n of the helper against the D-form applied to unit inputs.  Both are float64: 1e-12 relative."""
    nodes = ref.timesteps(ACP, S, "logSNR")
    n_steps = len(nodes) - 1
    assert n_steps == S
    h_prev, n_second = None, 0
    for j in range(n_steps):
        second = ref.is_second_order(j, n_steps, 2, True)
        n_second += second
        got = dpmpp_sde_coefficients(ACP, nodes[j], nodes[j + 1], h_prev if second else None)
        want = ref.coefficients(ACP, nodes[j], nodes[j + 1], h_prev if second else None)
        alpha_s, sigma_s, lam_s = ref.node(ACP, nodes[j])
        assert got[0] == alpha_s and got[1] == sigma_s
        for name, g, w in zip(("c_x", "c_0", "c_1", "c_n"), got[2:6], want):
            assert abs(g - w) <= 1e-12 * max(abs(w), 1e-3), f"step {j} {name}: {g} vs {w}"
        assert (got[4] != 0.0) == second and got[5] > 0.0 and 0.0 < got[2] < 1.0
        h_prev = got[6]
        assert h_prev == ref.node(ACP, nodes[j + 1])[2] - lam_s
    assert n_second == S - 2


# ---- the analytic Gaussian case, on the reference alone (float64 numpy, 2^20 samples)
N_GAUSS = 1 << 20
EXACT_MEAN, EXACT_STD = 0.29977, 0.50112
TABLE = {5: (5, 0.3550, 0.3554), 10: (10, 0.4849, 0.4863), 20: (20, 0.5088, 0.5089), 50: (48, 0.5027, 0.5031)}     # requested: real steps, std of two seeds


@functools.lru_cache(maxsize=None)
def _gauss(S, seed, sde=True, x_T=None):
    return ref.gaussian_run(ACP, S, N_GAUSS, seed, sde=sde, x_T=x_T)


def test_the_exact_marginal_of_the_gaussian_case():
    mean, std = ref.gaussian_marginal(ACP, 0)
    assert abs(mean - EXACT_MEAN) < 5e-6 and abs(std - EXACT_STD) < 5e-6


@pytest.mark.parametrize("S", sorted(TABLE))
def test_reference_reproduces_the_recorded_gaussian_table(S):
    """Each output std within 5e-3 of the mean of the row's two recorded values (ten times the two seeds' spread and the standard error of a
    std at this sample count); the mean within 1.2e-3 of the exact one at every step count."""
    real, a, b = TABLE[S]
    for seed in (0, 1):
        mean, std, steps = _gauss(S, seed)
        print(f"[dpmpp sde] gaussian S={S} seed {seed}: {steps} steps, mean {mean:.5f}, std {std:.4f} (recorded {a:.4f} / {b:.4f})")
        assert steps == real
        assert abs(std - 0.5 * (a + b)) <= 5e-3
        assert abs(mean - EXACT_MEAN) <= 1.2e-3


def test_gaussian_std_error_falls_with_the_step_count():
    err = {S: abs(0.5 * (_gauss(S, 0)[1] + _gauss(S, 1)[1]) - EXACT_STD) for S in (5, 10, 50)}
    print("[dpmpp sde] |std - exact|: " + ", ".join(f"S={S} {e:.2e}" for S, e in err.items()))
    assert err[5] > err[10] > err[50]


def test_the_sde_run_forgets_its_start_and_the_ode_run_does_not():
    """From x_T = 0 for every sample at 50 requested steps: the SDE run ends at the data's spread, the ODE run (the deterministic solver of
    tests/_dpmpp_ref.py from the same start) at none."""
    mean, std, steps = _gauss(50, 0, True, 0.0)
    _, std_ode, steps_ode = _gauss(50, 0, False, 0.0)
    print(f"[dpmpp sde] from x_T = 0, {steps} steps: sde mean {mean:.5f} std {std:.4f}; ode std {std_ode:.2e}")
    assert steps == steps_ode == 48
    assert abs(std - EXACT_STD) <= 0.01
    assert std_ode < 0.1


# ---- the per-step path against the D-form restatement
def _restated(model, nodes, x_T, c, uc, scale, noise, order, lower_order_final, log_every_t=1):
    def eps(x, t):
        tt = torch.full((x.shape[0],), t, dtype=torch.long)
        if uc is None:
            return model.apply_model(x, tt, c)
        e_c, e_u = model.apply_model(x, tt, c), model.apply_model(x, tt, uc)
        return e_u + scale * (e_c - e_u)
    return ref.sample(eps, nodes, x_T, model.alphas_cumprod.numpy(), noise, order=order, lower_order_final=lower_order_final,
                      log_every_t=log_every_t)


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("lower_order_final", [True, False])
@pytest.mark.parametrize("order", [1, 2])
def test_per_step_path_equals_the_d_form_restatement(order, lower_order_final, guided):
    """S = 6 on the logSNR grid, B = 3, 8 x 8, an explicit noise stack.  As in test_dpmpp_cpu.py the two formulations differ in association
    only, in fp32 over 6 steps whose c_x < 1 damp what came before: rel-L2 1e-6."""
    g = torch.Generator().manual_seed(4)
    B, S = 3, 6
    x_T = torch.randn(B, 3, 8, 8, generator=g)
    c = torch.randn(B, 2, 8, generator=g)
    uc = torch.zeros_like(c) if guided else None
    noise = torch.randn(S, B, 3, 8, 8, generator=g)
    sampler = DPMSolverSDESampler(CondModel())
    nodes = sampler.make_nodes(S).tolist()
    assert nodes == ref.timesteps(ACP, S, "logSNR") and len(nodes) == S + 1
    seen = []
    z, inter = sampler.sample(S, B, (3, 8, 8), conditioning=c, x_T=x_T, verbose=False, log_every_t=1, order=order,
                              unconditional_guidance_scale=2.0 if guided else 1.0, unconditional_conditioning=uc,
                              lower_order_final=lower_order_final, callback=seen.append, noise=noise)
    z_ref, inter_ref, n_fwd = _restated(CondModel(), nodes, x_T, c, uc, 2.0, noise, order, lower_order_final)
    worst = _rel(z, z_ref)
    assert len(inter["x_inter"]) == len(inter_ref["x_inter"]) == S + 1 and len(inter["pred_x0"]) == S + 1
    for a, b in zip(inter["x_inter"][1:] + inter["pred_x0"][1:], inter_ref["x_inter"][1:] + inter_ref["pred_x0"][1:]):
        worst = max(worst, _rel(a, b))
    print(f"[dpmpp sde] per-step path vs D-form (order {order}, lower_order_final {lower_order_final}, guided {guided}): worst rel-L2 {worst:.2e}")
    assert worst <= 1e-6
    assert torch.equal(inter["x_inter"][0], x_T) and torch.equal(z, inter["x_inter"][-1]) and seen == list(range(S)) and n_fwd == S
    # the noise matters, and so does each of the options the case sets
    z_other, _, _ = _restated(CondModel(), nodes, x_T, c, uc, 2.0, torch.zeros_like(noise), order, lower_order_final)
    assert _rel(z, z_other) > 1e-2
    if order == 2:
        z_other, _, _ = _restated(CondModel(), nodes, x_T, c, uc, 2.0, noise, 2, not lower_order_final)
        assert _rel(z, z_other) > 1e-4
        z_other, _, _ = _restated(CondModel(), nodes, x_T, c, uc, 2.0, noise, 1, lower_order_final)
        assert _rel(z, z_other) > 1e-4


def test_per_step_path_under_a_seed_draws_stream_one_at_the_loop_step():
    """noise_seed / noise_row0 on the per-step path: the start is the library's stream 0, step j's z the library's (stream 1, step j), rows
    from noise_row0 -- what the native seeded loop applies."""
    class Ctx:
        calls = []

        def op_randn(self, seed, B, per_row, row0=0, step=0, stream=0):
            self.calls.append(dict(seed=seed, B=B, per_row=per_row, row0=row0, step=step, stream=stream))
            return torch.full((B, per_row), 0.25 * (step + 1) * (1 if stream else -1))

    m = CondModel()
    m.ctx = Ctx()
    S, B = 5, 2
    c = torch.zeros(B, 2, 8)
    z, _ = DPMSolverSDESampler(m).sample(S, B, (3, 8, 8), conditioning=c, verbose=False, callback=lambda j: None, noise_seed=77, noise_row0=5)
    want = [dict(seed=77, B=B, per_row=192, row0=5, step=0, stream=0)] + [dict(seed=77, B=B, per_row=192, row0=5, step=j, stream=1) for j in range(S)]
    assert m.ctx.calls == want
    nodes = ref.timesteps(ACP, S, "logSNR")
    noise = torch.stack([torch.full((B, 3, 8, 8), 0.25 * (j + 1)) for j in range(S)])
    z_ref, _, _ = _restated(CondModel(), nodes, torch.full((B, 3, 8, 8), -0.25), c, None, 1.0, noise, 2, True)
    assert _rel(z, z_ref) <= 1e-6


# ---- refusals
def test_surface_errors():
    sm = DPMSolverSDESampler(CondModel())
    c = torch.zeros(1, 2, 8)
    with pytest.raises(ValueError, match="not scaled by eta"):
        sm.sample(10, 1, (3, 8, 8), conditioning=c, eta=0.5, verbose=False)
    with pytest.raises(ValueError, match="eta"):                       # the ODE solver keeps its own refusal
        DPMSolverSampler(CondModel()).sample(10, 1, (3, 8, 8), conditioning=c, eta=0.5, verbose=False)
    with pytest.raises(ValueError, match="order"):
        sm.sample(10, 1, (3, 8, 8), conditioning=c, order=3, verbose=False)
    with pytest.raises(ValueError):
        sm.sample(10, 1, (3, 8, 8), conditioning=c, unconditional_guidance_scale=0.5, unconditional_conditioning=c, verbose=False)
    with pytest.raises(ValueError, match="one of them"):
        sm.sample(10, 1, (3, 8, 8), conditioning=c, noise=torch.zeros(10, 1, 3, 8, 8), noise_seed=3, verbose=False)
    for bad in (torch.zeros(9, 1, 3, 8, 8), torch.zeros(10, 2, 3, 8, 8), torch.zeros(10, 1, 3, 8), torch.zeros(1, 3, 8, 8)):
        with pytest.raises(ValueError, match="noise stack must be"):
            sm.sample(10, 1, (3, 8, 8), conditioning=c, noise=bad, verbose=False, callback=lambda j: None)
    assert sm.NAME == "SDE-DPM-Solver++"


def _recorder(name, used):
    class Rec:
        def __init__(self, model):
            pass

        def sample(self, S, batch_size, shape, **kw):
            used.append((name, S, batch_size, shape))
            return torch.tensor(0.5), {}
    return Rec


class _Swapped:
    """ddpm.py's five sampler classes replaced by recorders for the duration of a with block."""
    NAMES = {"PLMSSampler": "plms", "DDIMSampler": "ddim", "DPMSolverSampler": "dpmpp", "UniPCSampler": "unipc", "DPMSolverSDESampler": "sde"}

    def __init__(self, used):
        self.used = used

    def __enter__(self):
        from rdm_amd.models.diffusion import ddpm as ddpm_mod
        self.mod = ddpm_mod
        self.orig = {cls: getattr(ddpm_mod, cls) for cls in self.NAMES}
        for cls, name in self.NAMES.items():
            setattr(ddpm_mod, cls, _recorder(name, self.used))
        return ddpm_mod

    def __exit__(self, *exc):
        for cls, v in self.orig.items():
            setattr(self.mod, cls, v)


def test_sample_log_selects_dpm_solver_sde_and_refuses_the_combinations():
    used = []

    class Stand:
        channels, image_size = 3, 8

    with _Swapped(used) as ddpm_mod:
        f = ddpm_mod.MinimalRETRODiffusion.sample_log
        f(Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=20, dpm_solver_sde=True)
        f(Stand(), cond=None, batch_size=2, ddim=False, ddim_steps=20, dpm_solver_sde=True)
        f(Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=20, dpm_solver_sde=False)
        f(Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=20, dpm_solver=True, dpm_solver_sde=False)
        for other in ("plms", "dpm_solver", "uni_pc"):
            with pytest.raises(ValueError, match=f"{other} and dpm_solver_sde select different samplers: give one of them"):
                f(Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=20, dpm_solver_sde=True, **{other: True})
        with pytest.raises(ValueError, match="plms and dpm_solver select different samplers: give one of them"):       # the earlier words first
            f(Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=20, plms=True, dpm_solver=True, dpm_solver_sde=True)
    assert used == [("sde", 20, 2, (3, 8, 8)), ("sde", 20, 2, (3, 8, 8)), ("ddim", 20, 2, (3, 8, 8)), ("dpmpp", 20, 2, (3, 8, 8))]
    assert ddpm_mod.DPMSolverSDESampler is DPMSolverSDESampler


def test_image_to_image_stays_ddim_only():
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion as M
    from test_img2img_cpu import _Stand
    lat = torch.zeros(2, 3, 8, 8)
    for kw in (dict(init_latent=lat, strength=0.5), dict(init_latent=lat, strength=0.5, invert=True), dict(strength=0.5), dict(invert=True)):
        with pytest.raises(ValueError, match="DDIM"):
            M.sample_log(_Stand(), cond=None, batch_size=2, ddim=True, ddim_steps=6, dpm_solver_sde=True, **kw)
    q = lambda **kw: M.sample_with_query(_Stand(), query=torch.zeros(2, 512), query_embedded=True, ddim=True, ddim_steps=6, dpm_solver_sde=True, **kw)
    with pytest.raises(ValueError, match="DDIM"):
        q(init_latent=lat)
    with pytest.raises(ValueError, match="DDIM"):
        q(init_image=torch.zeros(2, 32, 32, 3))


# ---- the script
def _script():
    spec = importlib.util.spec_from_file_location("rdm_sample_dpmpp_sde", os.path.join(ROOT, "scripts", "rdm_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("caption", ["", "a dog"])
def test_rdm_sample_dpm_solver_sde_flag_reaches_sample_log(tmp_path, caption):
    """--dpm_solver_sde parses (alone and with --device_noise), and both run loops hand dpm_solver_sde=True through sample_with_query /
    sample_from_rdata to sample_log; without the flag, the keyword is absent.  --init_img refuses it."""
    mod = _script()
    assert mod.parse_args([]).dpm_solver_sde is False and mod.parse_args(["--dpm_solver_sde"]).dpm_solver_sde is True
    assert "[native]" in next(a.help for a in mod.build_parser()._actions if "--dpm_solver_sde" in a.option_strings)
    assert mod._sampler_kwargs(mod.parse_args(["--dpm_solver_sde", "--device_noise"])) == {"dpm_solver_sde": True, "device_noise": True}
    with pytest.raises(SystemExit):
        mod.parse_args(["--dpm_solver_sde", "--init_img", str(tmp_path)])
    logged, used = [], []

    class Clip:
        def encode_text(self, tokens):
            return torch.ones(tokens.shape[0], 512)

    with _Swapped(used) as ddpm_mod:
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
                kw = {k: v for k, v in kw.items() if k in ("ddim", "ddim_steps", "plms", "dpm_solver", "uni_pc", "dpm_solver_sde")}
                z, _ = ddpm_mod.MinimalRETRODiffusion.sample_log(self, cond=None, batch_size=n, **kw)
                return torch.zeros(n, 3, 4, 4) + z

            def sample_with_query(self, **kw):
                return {"query_samples": self._sample(kw["query"].shape[0], kw)}

            def sample_from_rdata(self, n, **kw):
                return {"samples_with_sampled_nns": self._sample(n, kw)}

        base = ["-s", str(tmp_path), "-bs", "2", "-n", "1", "--steps", "20"] + (["-c", caption] if caption else [])
        run = mod.sample_conditional if caption else mod.sample_unconditional
        run(Model(), mod.parse_args(base + ["--dpm_solver_sde"]))
        run(Model(), mod.parse_args(base))
    assert logged[0]["dpm_solver_sde"] is True and "dpm_solver_sde" not in logged[1] and "dpm_solver" not in logged[0]
    assert used == [("sde", 20, 2, (3, 4, 4)), ("ddim", 20, 2, (3, 4, 4))]


# ---- the C ABI
def test_dpmpp_sde_symbols_in_header_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdm_hip.h")).read(), flags=re.S)
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    n_args = {"rdm_dpmpp_sde_sample": 9, "rdm_op_dpmpp_sde_step": 18}
    for name, n in n_args.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib, name)
    for name in ("rdm_dpmpp_sde_sample_seeded", "rdm_op_dpmpp_sde_step_seeded"):      # the twins the one rdm_noise argument replaced
        assert not re.search(r"\b" + name + r"\b", src) and name not in _lib.SIGNATURES, name
    assert re.search(r"int\s+rdm_dpmpp_sde_sample\s*\(\s*rdm_ctx\*\s*\w+,\s*const rdm_dpmpp_args\*", src)
    assert hasattr(_lib.Context, "dpmpp_sde_sample") and hasattr(_lib.Context, "op_dpmpp_sde_step")
    # rdm_dpmpp_args is the ODE solver's, field for field
    assert [f[0] for f in _lib.DpmppArgs._fields_] == ["batch", "k", "channels", "height", "width", "unconditional_guidance_scale", "order",
                                                        "lower_order_final", "log_every_t", "T", "alphas_cumprod", "n_nodes", "nodes"]


# ---- the shard
class _SdeCtx(StubCtx):
    def dpmpp_sde_sample(self, nodes, x_T, cond, uncond, alphas_cumprod, scale=1.0, order=2, lower_order_final=None, noise=None, log_every_t=100,
                         want_intermediates=False, seed=None, row0=0, shape=None):
        self.calls.append(("dpmpp_sde_sample", dict(nodes=list(nodes), x_T=x_T, noise=noise, seed=seed, row0=row0)))
        return x_T * 0.5, x_T[None], x_T[None]


def test_sample_shard_passes_row0_and_does_not_treat_the_sampler_as_noiseless(monkeypatch):
    """Rows [1, 3) of a batch of 3.  device_noise: the sampler gets noise_seed = the shared seed and noise_row0 = 1 and nothing is drawn
    here; the library sees the seed, row0 = 1 and no stack.  Without it: the start and a [steps, b, C, H, W] stack are drawn row by row, so
    a row does not depend on the sharding either -- the sampler is not among the noiseless ones."""
    from rdm_amd import parallel
    ctx = _SdeCtx()
    m = _model(ctx)
    m.set_distributed(True)
    n, S = 3, 6
    c = torch.zeros(n, 4, 512)
    nodes = ref.timesteps(ACP, S, "logSNR")
    seen = []
    inner = m.sample_log
    monkeypatch.setattr(m, "sample_log", lambda **kw: (seen.append(kw), inner(**kw))[1])

    torch.manual_seed(41)
    m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, n, 2.0, dict(ddim=True, ddim_steps=S, dpm_solver_sde=True))
    torch.manual_seed(41)
    base = parallel.shared_seed("cpu")
    call = _last(ctx, "dpmpp_sde_sample")
    assert [name for name, _ in ctx.calls] == ["dpmpp_sde_sample"] and call["nodes"] == nodes
    assert call["seed"] is None and call["row0"] == 0
    assert torch.equal(call["x_T"], parallel.per_sample_noise(base, [1, 2], (3, 8, 8)))
    assert torch.equal(call["noise"], parallel.per_sample_noise(base + 1, [1, 2], (S, 3, 8, 8)).transpose(0, 1).contiguous())

    def refuse(*a, **k):
        raise AssertionError("per_sample_noise was called under device_noise")
    monkeypatch.setattr(parallel, "per_sample_noise", refuse)
    ctx.calls.clear()
    torch.manual_seed(42)
    img = m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, n, 2.0, dict(ddim=True, ddim_steps=S, dpm_solver_sde=True), device_noise=True)
    torch.manual_seed(42)
    base = parallel.shared_seed("cpu")
    kw = seen[-1]
    assert kw["noise_seed"] == base and kw["noise_row0"] == 1 and kw.get("x_T") is None and kw.get("noise") is None
    assert [name for name, _ in ctx.calls] == ["op_randn", "dpmpp_sde_sample"]
    assert _last(ctx, "op_randn") == dict(seed=base, B=2, per_row=3 * 8 * 8, row0=1, step=0, stream=0)
    call = _last(ctx, "dpmpp_sde_sample")
    assert call["seed"] == base and call["row0"] == 1 and call["noise"] is None
    assert tuple(img.shape) == (2, 3, 32, 32)
