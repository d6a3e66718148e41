"""The native DPM-Solver++ loop (rdm_dpmpp_sample, fused update kernel) on the GPU: the kernel alone per element against float64 and
bit for bit against the SDE step kernel with its noise term switched off, every step of the loop against the D-form restatement of tests/_dpmpp_ref.py in deterministic mode, order 1 against the DDIM loop,
DPMSolverSampler against the D-form loop over the CPU oracle UNet, batch independence in deterministic mode, errors, and the end-to-end
entry."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff
from oracle import unet as ounet

import _dpmpp_ref as ref
from _util import rel_l2, within
from test_gpu_plms import model, tiny  # noqa: F401  (fixtures: the tiny UNet on the session context, the tiny model)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

LATENT_TOL = 2.5e-2          # as test_gpu_surface.py's DDIM latent bound
UPDATE_TOL = 1e-5            # as the DDIM update in test_gpu_emul.py and the PLMS update in test_gpu_plms.py
ACP = odiff.Schedule().alphas_cumprod


_within = functools.partial(within, "dpmpp")


# ---- the kernel alone
def _coefficients(second):
    """fp32 kernel scalars of the step 571 -> 399 (after 709 -> 571) of the S = 10 logSNR grid, from the D-form's quantities."""
    f32 = lambda v: float(np.float32(v))
    alpha_s, sigma_s, lam_s = ref.node(ACP, 571)
    alpha_t, sigma_t, lam_t = ref.node(ACP, 399)
    h, h_prev = lam_t - lam_s, lam_s - ref.node(ACP, 709)[2]
    g = -alpha_t * math.expm1(-h)
    r = h_prev / h
    c_0, c_1 = (g * (1.0 + 1.0 / (2.0 * r)), -g / (2.0 * r)) if second else (g, 0.0)
    return f32(alpha_s), f32(sigma_s), f32(sigma_t / sigma_s), f32(c_0), f32(c_1)


@pytest.mark.parametrize("config", ["guided_second_aliased", "unguided_first_bare", "guided_first_all_outputs"])
@pytest.mark.parametrize("n,offset", [(1027, 0), (4096, 0), (2 * 1024 * 1024 + 4, 0), (2304, 1)],
                         ids=["n1027_scalar_tail", "n4096_vector", "n2Mplus4_second_stride", "n2304_misaligned_scalar"])
def test_step_kernel_per_element_against_fp64(ctx, n, offset, config):
    """|got - ref| <= 16 * 2^-24 * A per element, A the float64 sum of the absolute values of every term entering the element:
    A = |c_x x| + |c_0| (|x| + s1m (|e_u| + scale (|e_c| + |e_u|))) / sa + |c_1 m_prev|; 16 covers the at most 11 fp32 roundings of the
    expression.  n = 2 * 1024 * 1024 + 4 is one float4 group past 2048 blocks x 256 threads: the stride loop runs a second time.
    offset 1: x starts one float past an aligned address, which puts an n % 4 == 0 call on the scalar path."""
    d = ctx.device
    g = torch.Generator(device=d).manual_seed(n + offset)
    cfg = config != "unguided_first_bare"
    second = config == "guided_second_aliased"
    scale = 2.0 if cfg else 1.0
    sa, s1m, c_x, c_0, c_1 = _coefficients(second)
    rnd = lambda m: torch.randn(m, device=d, generator=g)
    x = rnd(n + offset)[offset:]
    assert x.data_ptr() % 16 == 4 * offset and x.is_contiguous()
    eps = rnd(2 * n if cfg else n)
    m_prev = rnd(n) if second else None
    m_prev_in = m_prev.clone() if second else None
    x_out = torch.full((n,), float("nan"), device=d)
    bare = config == "unguided_first_bare"
    x_dup, pred_x0 = (torch.full_like(x_out, float("nan")), torch.full_like(x_out, float("nan"))) if config == "guided_first_all_outputs" else (None, None)
    m_store = None if bare else (m_prev if second else torch.full_like(x_out, float("nan")))
    ctx.op_dpmpp_step(x, eps, m_prev, cfg, scale, sa, s1m, c_x, c_0, c_1, x_out, x_dup=x_dup, m_store=m_store, pred_x0=pred_x0)
    torch.cuda.synchronize()

    X = x.double()
    e_c = eps[:n].double()
    if cfg:
        e_u = eps[n:].double()
        E, EA = e_u + scale * (e_c - e_u), e_u.abs() + scale * (e_c.abs() + e_u.abs())
    else:
        E, EA = e_c, e_c.abs()
    M0 = (X - s1m * E) / sa
    want = c_x * X + c_0 * M0
    A_m = (X.abs() + s1m * EA) / sa
    A = (c_x * X).abs() + abs(c_0) * A_m
    if second:
        want = want + c_1 * m_prev_in.double()
        A = A + (c_1 * m_prev_in.double()).abs()
    u = 16.0 * 2.0 ** -24
    worst = float(((x_out.double() - want).abs() / A).max())
    print(f"[dpmpp] kernel n={n} offset={offset} {config}: worst |got - ref| / A = {worst / 2.0 ** -24:.2f} * 2^-24 (bound 16)")
    assert torch.isfinite(x_out).all()
    assert ((x_out.double() - want).abs() <= u * A).all()
    if m_store is not None:
        assert ((m_store.double() - M0).abs() <= u * A_m).all()
    if x_dup is not None:
        assert torch.equal(x_dup, x_out)
        assert torch.equal(pred_x0, m_store)


@pytest.mark.parametrize("history", ["m_prev_none", "m_prev_given", "m_store_aliases_m_prev"])
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("n", [4096, 1027], ids=["n4096_vector", "n1027_scalar"])
def test_ode_step_is_the_sde_step_without_its_noise_term(ctx, n, cfg, history):
    """The ODE and SDE step kernels are one element function (csrc/sampler_steps.hip: dpmpp_update) with and without the c_n z term:
    op_dpmpp_step must be torch.equal to op_dpmpp_sde_step (stack form) with c_n = 0 and finite normal z, in every output.  xo + 0 z
    can only turn -0 into +0, which torch.equal treats as equal."""
    d = ctx.device
    g = torch.Generator(device=d).manual_seed(7 * n + cfg)
    rnd = lambda m: torch.randn(m, device=d, generator=g)
    second = history != "m_prev_none"
    sa, s1m, c_x, c_0, c_1 = _coefficients(second)
    x, eps, z = rnd(n), rnd(2 * n if cfg else n), rnd(n)
    m_prev_in = rnd(n) if second else None
    got = []
    for sde in (False, True):
        m_prev = m_prev_in.clone() if second else None
        x_out, x_dup, pred_x0, m_new = (torch.full((n,), float("nan"), device=d) for _ in range(4))
        m_store = m_prev if history == "m_store_aliases_m_prev" else m_new
        if sde:
            ctx.op_dpmpp_sde_step(x, eps, m_prev, z, cfg, 2.0 if cfg else 1.0, sa, s1m, c_x, c_0, c_1, 0.0, x_out, x_dup=x_dup, m_store=m_store,
                                  pred_x0=pred_x0)
        else:
            ctx.op_dpmpp_step(x, eps, m_prev, cfg, 2.0 if cfg else 1.0, sa, s1m, c_x, c_0, c_1, x_out, x_dup=x_dup, m_store=m_store,
                              pred_x0=pred_x0)
        torch.cuda.synchronize()
        got.append((x_out, x_dup, m_store, pred_x0))
    assert torch.isfinite(z).all() and all(torch.isfinite(t).all() for t in got[0])
    for name, ode, sde in zip(("x_out", "x_dup", "m_store", "pred_x0"), *got):
        assert torch.equal(ode, sde), name


# ---- the loop, step by step
def _teacher_forced(ctx, nodes, x_T, cond, uncond, scale, order, lower_order_final):
    """Every step rebuilt from the logged x_inter[j-1] (and pred_x0[j-1] = m_{j-1}) with ctx.unet_forward on [x | x], [cond | uncond]
    and the D-form update ON THE GPU (a CPU restatement would feed ulp-level differences of the update into the next forward of this
    synthetic UNet, which amplifies them: see test_gpu_plms.py)."""
    B = x_T.shape[0]
    z, xi, pi = ctx.dpmpp_sample(nodes, x_T, cond, uncond, ACP, scale=scale, order=order, lower_order_final=lower_order_final,
                                 log_every_t=1, want_intermediates=True)
    n_steps = len(nodes) - 1
    assert xi.shape[0] == pi.shape[0] == n_steps
    assert torch.equal(z, xi[-1])

    def eps(x, t):
        tt = torch.full(((2 if uncond is not None else 1) * B,), t, dtype=torch.long, device=x.device)
        if uncond is None:
            return ctx.unet_forward(x, tt, cond)
        out = ctx.unet_forward(torch.cat([x, x]), tt, torch.cat([cond, uncond]))
        return out[B:] + scale * (out[:B] - out[B:])

    worst = [0.0, 0.0]
    h_prev = None
    for j in range(n_steps):
        x = x_T if j == 0 else xi[j - 1]
        second = ref.is_second_order(j, n_steps, order, lower_order_final)
        want_x, want_m, h_prev = ref.step(x, eps(x, int(nodes[j])), pi[j - 1] if j else None, ACP.numpy(), nodes[j], nodes[j + 1], h_prev, second)
        ex, em = rel_l2(xi[j], want_x), rel_l2(pi[j], want_m)
        worst = [max(worst[0], ex), max(worst[1], em)]
        assert ex <= UPDATE_TOL and em <= UPDATE_TOL, f"step {j} (second order {second}): x {ex:.3e}, pred_x0 {em:.3e}"
    return worst


@pytest.mark.parametrize("lower_order_final", [True, False])
@pytest.mark.parametrize("skip_type", ["logSNR", "time_uniform"])
def test_dpmpp_steps_teacher_forced_deterministic(tiny, skip_type, lower_order_final):
    """S = 6 on both grids, CFG 2.0, B = 3 at 16 x 16 (B C H W = 2304: the kernel's vector path), the last step in either order."""
    ctx, _, _ = tiny
    g = torch.Generator().manual_seed(21)
    B = 3
    x_T = torch.randn(B, 3, 16, 16, generator=g).to(ctx.device)
    cond = (torch.randn(B, 4, 512, generator=g) * 0.45).to(ctx.device)
    nodes = ctx.dpmpp_timesteps(6, ACP, skip_type)
    assert nodes.tolist() == ref.timesteps(ACP.numpy(), 6, skip_type)
    ctx.set_deterministic(True)
    try:
        worst = _teacher_forced(ctx, nodes, x_T, cond, torch.zeros_like(cond), 2.0, 2, lower_order_final)
    finally:
        ctx.set_deterministic(False)
    print(f"[dpmpp] {skip_type} lower_order_final={lower_order_final} teacher-forced steps ({len(nodes) - 1}): worst x_inter {worst[0]:.3e}, "
          f"pred_x0 {worst[1]:.3e} (bound {UPDATE_TOL:.0e})")


def test_dpmpp_unguided_single_row_teacher_forced(tiny):
    ctx, _, _ = tiny
    g = torch.Generator().manual_seed(22)
    x_T = torch.randn(1, 3, 16, 16, generator=g).to(ctx.device)
    cond = (torch.randn(1, 4, 512, generator=g) * 0.45).to(ctx.device)
    ctx.set_deterministic(True)
    try:
        worst = _teacher_forced(ctx, ctx.dpmpp_timesteps(6, ACP), x_T, cond, None, 1.0, 2, True)
    finally:
        ctx.set_deterministic(False)
    print(f"[dpmpp] unguided B = 1 teacher-forced steps: worst x_inter {worst[0]:.3e}, pred_x0 {worst[1]:.3e} (bound {UPDATE_TOL:.0e})")


def test_order_one_on_the_time_uniform_grid_is_the_ddim_loop(tiny):
    """Same forward, different association of the update: the first logged x_inter and pred_x0 of the two loops agree to 1e-5 (later
    steps start from different x; the teacher-forced test covers them)."""
    ctx, _, _ = tiny
    g = torch.Generator().manual_seed(23)
    B, S = 3, 6
    x_T = torch.randn(B, 3, 16, 16, generator=g).to(ctx.device)
    cond = (torch.randn(B, 4, 512, generator=g) * 0.45).to(ctx.device)
    uncond = torch.zeros_like(cond)
    ctx.set_deterministic(True)
    try:
        nodes = ctx.dpmpp_timesteps(S, ACP, "time_uniform")
        _, xi, pi = ctx.dpmpp_sample(nodes, x_T, cond, uncond, ACP, scale=2.0, order=1, log_every_t=1, want_intermediates=True)
        _, xd, pd = ctx.ddim_sample(S, x_T, cond, uncond, ACP, eta=0.0, scale=2.0, log_every_t=1, want_intermediates=True)
    finally:
        ctx.set_deterministic(False)
    assert xi.shape == xd.shape and pi.shape == pd.shape and xi.shape[0] == len(nodes) - 1
    _within("order 1 vs DDIM, first x_inter", rel_l2(xi[0], xd[0]), 1e-5)
    _within("order 1 vs DDIM, first pred_x0", rel_l2(pi[0], pd[0]), 1e-5)


# ---- the sampler surface
def test_dpm_solver_sampler_against_oracle_and_per_step_path(model):
    from rdm_amd.models.diffusion.dpm_solver import DPMSolverSampler
    rng = np.random.default_rng(9)
    B, S, scale = 2, 5, 2.0
    x_T = torch.from_numpy(rng.standard_normal((B, 3, 16, 16)).astype(np.float32)).to(model.device)
    cond = torch.from_numpy((rng.standard_normal((B, 4, 512)) * 0.45).astype(np.float32)).to(model.device)
    uc = torch.zeros_like(cond)
    sampler = DPMSolverSampler(model)
    z, inter = sampler.sample(S, B, (3, 16, 16), conditioning=cond, x_T=x_T, log_every_t=2, verbose=False,
                              unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    n_log = 1 + sum(1 for i in range(S) if (S - 1 - i) % 2 == 0 or i == 0)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == n_log and torch.equal(inter["x_inter"][0].cpu(), x_T.cpu())
    c_cpu, u_cpu = cond.cpu(), uc.cpu()

    def eps(x, t):
        out = ounet.unet_forward(model.sd_unet, model.spec, torch.cat([x, x]), torch.full((2 * B,), t, dtype=torch.long), torch.cat([c_cpu, u_cpu]))
        return out[B:] + scale * (out[:B] - out[B:])

    nodes = ref.timesteps(ACP.numpy(), S, "logSNR")
    assert len(nodes) == S + 1
    z_ref, _, _ = ref.sample(eps, nodes, x_T.cpu(), ACP.numpy(), order=2, lower_order_final=True)
    _within("DPMSolverSampler.sample latent vs the oracle D-form loop (5 steps, CFG 2.0)", rel_l2(z, z_ref), LATENT_TOL)
    seen = []
    z2, _ = sampler.sample(S, B, (3, 16, 16), conditioning=cond, x_T=x_T, verbose=False, unconditional_guidance_scale=scale,
                           unconditional_conditioning=uc, callback=seen.append)
    assert seen == list(range(S))
    _within("DPMSolverSampler per-step path vs the native loop", rel_l2(z2, z), 2e-2)


def test_dpmpp_deterministic_rows_do_not_depend_on_the_batch(tiny):
    ctx, _, _ = tiny
    d = ctx.device
    g = torch.Generator(device=d).manual_seed(5)
    x = torch.randn(6, 3, 16, 16, device=d, generator=g)
    c = torch.randn(6, 4, 512, device=d, generator=g) * 0.45
    nodes = ctx.dpmpp_timesteps(5, ACP)
    ctx.set_deterministic(True)
    try:
        z6 = ctx.dpmpp_sample(nodes, x, c, torch.zeros_like(c), ACP, scale=2.0)[0]
        for r in (0, 4):
            z1 = ctx.dpmpp_sample(nodes, x[r:r + 1], c[r:r + 1], torch.zeros_like(c[r:r + 1]), ACP, scale=2.0)[0]
            assert torch.equal(z1, z6[r:r + 1]), f"row {r}: batch 1 and batch 6 differ"
    finally:
        ctx.set_deterministic(False)


def test_dpmpp_errors_leave_the_context_usable(tiny):
    from rdm_amd._lib import RdmError
    ctx, _, _ = tiny
    d = ctx.device
    x = torch.randn(2, 3, 16, 16, device=d)
    c = torch.randn(2, 4, 512, device=d) * 0.45
    uc = torch.zeros_like(c)
    good = [800, 500, 200, 0]
    bad_calls = {
        "a non-decreasing node list": lambda: ctx.dpmpp_sample([800, 500, 500, 0], x, c, None, ACP),
        "an increasing node list": lambda: ctx.dpmpp_sample([0, 200, 500], x, c, None, ACP),
        "a node equal to T": lambda: ctx.dpmpp_sample([1000, 500, 0], x, c, None, ACP),
        "a negative node": lambda: ctx.dpmpp_sample([500, 0, -1], x, c, None, ACP),
        "one node only": lambda: ctx.dpmpp_sample([500], x, c, None, ACP),
        "order 3": lambda: ctx.dpmpp_sample(good, x, c, None, ACP, order=3),
        "scale 0.5": lambda: ctx.dpmpp_sample(good, x, c, uc, ACP, scale=0.5),
        "guidance without uncond": lambda: ctx.dpmpp_sample(good, x, c, None, ACP, scale=2.0),
        "a wrong context width": lambda: ctx.dpmpp_sample(good, x, c[:, :, :256].contiguous(), None, ACP),
        "a batch mismatch": lambda: ctx.dpmpp_sample(good, x, c[:1], None, ACP),
    }
    for what, call in bad_calls.items():
        with pytest.raises(RdmError):
            call()
            pytest.fail(f"{what} was accepted")
        zz, xi, pi = ctx.dpmpp_sample(good, x, c, uc, ACP, scale=2.0, want_intermediates=True)
        torch.cuda.synchronize()
        assert zz.shape == x.shape and torch.isfinite(zz).all(), f"after {what}"
        assert xi.shape == pi.shape == (2,) + tuple(x.shape)          # log_every_t = 100 over 3 steps: the first step and index 0


def test_sample_with_query_dpm_solver_end_to_end(model):
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    rng = np.random.default_rng(32)
    N = 2000
    pool = {"embedding": (rng.standard_normal((N, 512)) * 0.45).astype(np.float16), "img_id": np.arange(N),
            "patch_coords": rng.integers(0, 1200, (N, 4))}
    db = DatasetBuilder(data_pool=pool, k=20, ctx=model.ctx)
    db.train_searcher()
    model.retriever = db
    q = torch.from_numpy((rng.standard_normal((3, 512)) * 0.45).astype(np.float32))
    out = model.sample_with_query(query=q, query_embedded=True, k_nn=4, ddim=True, ddim_steps=4, dpm_solver=True,
                                  unconditional_guidance_scale=2.0, unconditional_retro_guidance_label=0., visualize_nns=False)
    img = out["query_samples"]
    assert img.shape == (3, 3, 64, 64) and torch.isfinite(img).all()
