"""The native UniPC loop (rdm_unipc_sample, fused predict-and-correct kernel) on the GPU: the kernel alone per element against float64,
every step of the loop teacher-forced against the D-form restatement of tests/_unipc_ref.py in deterministic mode, UniPCSampler against
the D-form loop over the CPU oracle UNet, batch independence in deterministic mode, errors, and the end-to-end entry."""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import diffusion as odiff
from oracle import unet as ounet

import _dpmpp_ref as dref
import _unipc_ref as ref
from _util import rel_l2, within
from test_gpu_plms import model, tiny  # noqa: F401  (fixtures: the tiny UNet on the session context, the tiny model)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

LATENT_TOL = 2.5e-2          # as test_gpu_surface.py's DDIM latent bound
UPDATE_TOL = 1e-5            # as the DDIM update in test_gpu_emul.py and the PLMS / DPM-Solver++ updates
ACP = odiff.Schedule().alphas_cumprod
NODES10 = dref.timesteps(ACP.numpy(), 10, "logSNR")


_within = functools.partial(within, "unipc")


# ---- the kernel alone
KERNEL_CONFIGS = {
    # name: (j on the S = 10 logSNR grid, order, variant, guided)
    "first_step_no_correction_no_history": (0, 3, "bh2", True),
    "guided_order3_in_place_m_into_h3": (4, 3, "bh1", True),
    "unguided_order2_all_outputs": (3, 2, "bh2", False),
}


@pytest.mark.parametrize("config", list(KERNEL_CONFIGS))
@pytest.mark.parametrize("n,offset", [(1027, 0), (4096, 0), (2 * 1024 * 1024 + 4, 0), (2304, 1)],
                         ids=["n1027_scalar_tail", "n4096_vector", "n2Mplus4_second_stride", "n2304_misaligned_scalar"])
def test_step_kernel_per_element_against_fp64(ctx, n, offset, config):
    """|got - ref| <= 16 * 2^-24 * A per element, A the float64 sum of the absolute values of every term entering the element:
    A_m = (|u| + sigma (|e_u| + scale (|e_c| + |e_u|))) / alpha, A_xc = |a_x xc_prev| + |a_t| A_m + sum |a_i h_i| (uncorrected: |u|),
    A_un = |b_x| A_xc + |b_0| A_m + sum |b_i h_i|.  fp32 roundings on the longest path (guided, order 3), sums left to right: the guided
    eps 3 (subtract, scale, add), m 3 more (sigma e, subtract, divide) = 6; a_t m 7, + a_x xc_prev 8, + a_1 h1 9, + a_2 h2 10,
    + a_3 h3 11; b_x xc 12, + b_0 m 13, + b_1 h1 14, + b_2 h2 15: 15 roundings, K = 16.  The reference takes the coefficients as the
    fp32 values the kernel receives.  n = 2 * 1024 * 1024 + 4 is one float4 group past 2048 blocks x 256 threads: the stride loop runs a
    second time.  offset 1: u starts one float past an aligned address, which puts an n % 4 == 0 call on the scalar path.
    Near miss: the same bound against a reference with h1 and h2 swapped must fail.  Measured worst: 4.4 * 2^-24."""
    j, order, variant, cfg = KERNEL_CONFIGS[config]
    d = ctx.device
    g = torch.Generator(device=d).manual_seed(n + offset)
    scale = 2.0 if cfg else 1.0
    co = ctx.unipc_coefficients(NODES10, ACP, j, order=order, variant=variant)
    alpha, sigma, a_x, a_t, a_1, a_2, a_3, b_x, b_0, b_1, b_2 = (float(np.float32(v)) for v in co[:11])
    order_c, order_p = int(co[11]), int(co[12])
    assert (order_c, order_p) == {0: (0, 1), 4: (3, 3), 3: (2, 2)}[j]
    nh = max(order_c, order_p - 1)
    rnd = lambda m: torch.randn(m, device=d, generator=g)
    u = rnd(n + offset)[offset:]
    assert u.data_ptr() % 16 == 4 * offset and u.is_contiguous()
    eps = rnd(2 * n if cfg else n)
    xc_prev = rnd(n) if order_c else None
    hist = [rnd(n) for _ in range(nh)] + [None] * (3 - nh)
    u_in, xp_in, hist_in = u.clone(), (xc_prev.clone() if order_c else None), [None if h is None else h.clone() for h in hist]
    nan = lambda: torch.full((n,), float("nan"), device=d)
    x_dup = pred_x0 = None
    if config == "first_step_no_correction_no_history":            # as the loop's first pass: xc and m kept, nothing else
        u_next, xc_out, m_store = nan(), nan(), nan()
    elif config == "guided_order3_in_place_m_into_h3":             # as a later pass: u and xc updated in place, m takes the oldest slot
        u_next, xc_out, m_store, x_dup = u, xc_prev, hist[2], nan()
    else:
        u_next, xc_out, m_store, x_dup, pred_x0 = nan(), nan(), nan(), nan(), nan()
    ctx.op_unipc_step(u, eps, co, cfg, scale, u_next, xc_prev=xc_prev, h1=hist[0], h2=hist[1], h3=hist[2], xc_out=xc_out, x_dup=x_dup,
                      m_store=m_store, pred_x0=pred_x0)
    torch.cuda.synchronize()

    U = u_in.double()
    e_c = eps[:n].double()
    if cfg:
        e_u = eps[n:].double()
        E, EA = e_u + scale * (e_c - e_u), e_u.abs() + scale * (e_c.abs() + e_u.abs())
    else:
        E, EA = e_c, e_c.abs()
    M = (U - sigma * E) / alpha
    A_m = (U.abs() + sigma * EA) / alpha

    def expected(h):
        if order_c:
            xc = a_x * xp_in.double() + a_t * M
            A_xc = (a_x * xp_in.double()).abs() + abs(a_t) * A_m
            for a_i, h_i in zip((a_1, a_2, a_3)[:order_c], h):
                xc, A_xc = xc + a_i * h_i.double(), A_xc + (a_i * h_i.double()).abs()
        else:
            xc, A_xc = U, U.abs()
        un = b_x * xc + b_0 * M
        A_un = abs(b_x) * A_xc + abs(b_0) * A_m
        for b_i, h_i in zip((b_1, b_2)[:order_p - 1], h):
            un, A_un = un + b_i * h_i.double(), A_un + (b_i * h_i.double()).abs()
        return xc, A_xc, un, A_un

    want_xc, A_xc, want_un, A_un = expected(hist_in)
    bound = 16.0 * 2.0 ** -24
    worst = max(float(((u_next.double() - want_un).abs() / A_un).max()), float(((xc_out.double() - want_xc).abs() / A_xc).max()),
                float(((m_store.double() - M).abs() / A_m).max()))
    print(f"[unipc] kernel n={n} offset={offset} {config}: worst |got - ref| / A = {worst / 2.0 ** -24:.2f} * 2^-24 (bound 16)")
    assert torch.isfinite(u_next).all() and torch.isfinite(xc_out).all() and torch.isfinite(m_store).all()
    assert ((u_next.double() - want_un).abs() <= bound * A_un).all()
    assert ((xc_out.double() - want_xc).abs() <= bound * A_xc).all()
    assert ((m_store.double() - M).abs() <= bound * A_m).all()
    if x_dup is not None:
        assert torch.equal(x_dup, u_next)
    if pred_x0 is not None:
        assert torch.equal(pred_x0, m_store)
    if nh >= 2:
        _, _, swapped_un, _ = expected([hist_in[1], hist_in[0]] + hist_in[2:])
        assert not ((u_next.double() - swapped_un).abs() <= bound * A_un).all(), "the bound does not tell h1 from h2"
        if nh < 3:
            assert torch.equal(hist[0], hist_in[0]) and torch.equal(hist[1], hist_in[1])          # inputs are left alone


# ---- the loop, step by step
def _teacher_forced(ctx, nodes, x_T, cond, uncond, scale, **solver):
    """pred_x0[j] against (u_j - sigma eps(u_j)) / alpha with u_j the logged x_inter[j-1] and the forward run on the GPU (a CPU
    forward would feed ulp-level differences into this synthetic UNet, which amplifies them: see test_gpu_plms.py); the corrected chain
    x_j rebuilt in float64 from the logged m's (linear in them, so the UNet amplifies nothing); x_inter[j] against the D-form
    prediction from that chain."""
    B = x_T.shape[0]
    z, xi, pi = ctx.unipc_sample(nodes, x_T, cond, uncond, ACP, scale=scale, log_every_t=1, want_intermediates=True, **solver)
    n = len(nodes) - 1
    assert xi.shape[0] == pi.shape[0] == n
    assert torch.equal(z, xi[-1])
    asl = ref.node_values(ACP.numpy(), nodes)

    def eps(x, t):
        tt = torch.full(((2 if uncond is not None else 1) * B,), t, dtype=torch.long, device=x.device)
        if uncond is None:
            return ctx.unet_forward(x, tt, cond)
        out = ctx.unet_forward(torch.cat([x, x]), tt, torch.cat([cond, uncond]))
        return out[B:] + scale * (out[:B] - out[B:])

    worst = [0.0, 0.0]
    x, ms = x_T.double(), []
    for j in range(n):
        u = x_T if j == 0 else xi[j - 1]
        want_m = (u - asl[j][1] * eps(u, int(nodes[j]))) / asl[j][0]
        m = pi[j].double()
        if solver["corrector"] and j >= 1:
            x = ref.correct(asl, j, ref.step_order(j, n, solver["order"], solver["lower_order_final"]), solver["variant"], x, ms, m)
        else:
            x = u.double()
        ms = [m] + ms[:2]
        want_u = ref.predict(asl, j + 1, ref.step_order(j + 1, n, solver["order"], solver["lower_order_final"]), solver["variant"], x, ms)
        eu, em = rel_l2(xi[j], want_u), rel_l2(pi[j], want_m)
        worst = [max(worst[0], eu), max(worst[1], em)]
        assert eu <= UPDATE_TOL and em <= UPDATE_TOL, f"step {j} ({solver}): x_inter {eu:.3e}, pred_x0 {em:.3e}"
    return worst


@pytest.mark.parametrize("lower_order_final", [True, False])
@pytest.mark.parametrize("skip_type", ["logSNR", "time_uniform"])
def test_unipc_steps_teacher_forced_deterministic(tiny, skip_type, lower_order_final):
    """S = 6 on both grids, CFG 2.0, B = 3 at 16 x 16 (B C H W = 2304: the kernel's vector path); orders 2 and 3, both variants, with
    and without the corrector.  Measured worst: x_inter 6.9e-7, pred_x0 7.6e-8."""
    ctx, _, _ = tiny
    g = torch.Generator().manual_seed(21)
    B = 3
    x_T = torch.randn(B, 3, 16, 16, generator=g).to(ctx.device)
    cond = (torch.randn(B, 4, 512, generator=g) * 0.45).to(ctx.device)
    nodes = ctx.dpmpp_timesteps(6, ACP, skip_type)
    assert nodes.tolist() == dref.timesteps(ACP.numpy(), 6, skip_type)
    ctx.set_deterministic(True)
    try:
        for order, variant, corrector in itertools.product((2, 3), ("bh1", "bh2"), (True, False)):
            worst = _teacher_forced(ctx, nodes, x_T, cond, torch.zeros_like(cond), 2.0, order=order, variant=variant, corrector=corrector,
                                    lower_order_final=lower_order_final)
            print(f"[unipc] {skip_type} order {order} {variant} corrector={corrector} lower_order_final={lower_order_final} teacher-forced "
                  f"steps ({len(nodes) - 1}): worst x_inter {worst[0]:.3e}, pred_x0 {worst[1]:.3e} (bound {UPDATE_TOL:.0e})")
    finally:
        ctx.set_deterministic(False)


def test_unipc_unguided_single_row_teacher_forced(tiny):
    ctx, _, _ = tiny
    g = torch.Generator().manual_seed(22)
    x_T = torch.randn(1, 3, 16, 16, generator=g).to(ctx.device)
    cond = (torch.randn(1, 4, 512, generator=g) * 0.45).to(ctx.device)
    ctx.set_deterministic(True)
    try:
        for order in (2, 3):
            worst = _teacher_forced(ctx, ctx.dpmpp_timesteps(6, ACP), x_T, cond, None, 1.0, order=order, variant="bh2", corrector=True,
                                    lower_order_final=True)
            print(f"[unipc] unguided B = 1 order {order} teacher-forced steps: worst x_inter {worst[0]:.3e}, pred_x0 {worst[1]:.3e} "
                  f"(bound {UPDATE_TOL:.0e})")
    finally:
        ctx.set_deterministic(False)


# ---- the sampler surface
def test_unipc_sampler_against_oracle_and_per_step_path(model):
    """UniPCSampler.sample against the float64-scalar D-form loop over the CPU oracle UNet, 5 steps, CFG 2.0.  Bound: the larger of the
    project's latent bound and twice the distance of DPMSolverSampler to its own oracle loop on the same inputs (both run five bf16
    forwards; the corrector adds one more linear combination of them).  Measured: UniPCSampler 8.8e-3, DPMSolverSampler 9.0e-3, the
    per-step path against the native loop 1.0e-2."""
    from rdm_amd.models.diffusion.dpm_solver import DPMSolverSampler
    from rdm_amd.models.diffusion.uni_pc import UniPCSampler
    rng = np.random.default_rng(9)
    B, S, scale = 2, 5, 2.0
    x_T = torch.from_numpy(rng.standard_normal((B, 3, 16, 16)).astype(np.float32)).to(model.device)
    cond = torch.from_numpy((rng.standard_normal((B, 4, 512)) * 0.45).astype(np.float32)).to(model.device)
    uc = torch.zeros_like(cond)
    kw = dict(conditioning=cond, x_T=x_T, verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    sampler = UniPCSampler(model)
    z, inter = sampler.sample(S, B, (3, 16, 16), log_every_t=2, **kw)
    n_log = 1 + sum(1 for i in range(S) if (S - 1 - i) % 2 == 0 or i == 0)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == n_log and torch.equal(inter["x_inter"][0].cpu(), x_T.cpu())
    assert torch.equal(inter["x_inter"][-1], z)
    c_cpu, u_cpu = cond.cpu(), uc.cpu()

    def eps(x, t):
        out = ounet.unet_forward(model.sd_unet, model.spec, torch.cat([x, x]), torch.full((2 * B,), t, dtype=torch.long), torch.cat([c_cpu, u_cpu]))
        return out[B:] + scale * (out[:B] - out[B:])

    nodes = dref.timesteps(ACP.numpy(), S, "logSNR")
    assert len(nodes) == S + 1
    z_ref, _, n_fwd = ref.sample(eps, nodes, x_T.cpu(), ACP.numpy(), order=2, variant="bh2", corrector=True, lower_order_final=True)
    assert n_fwd == S
    z_d, _ = DPMSolverSampler(model).sample(S, B, (3, 16, 16), **kw)
    z_d_ref, _, _ = dref.sample(eps, nodes, x_T.cpu(), ACP.numpy(), order=2, lower_order_final=True)
    d_dpmpp, d_unipc = rel_l2(z_d, z_d_ref), rel_l2(z, z_ref)
    print(f"[unipc] latent vs oracle loop (5 steps, CFG 2.0): UniPCSampler {d_unipc:.3e}, DPMSolverSampler {d_dpmpp:.3e}")
    _within("UniPCSampler.sample latent vs the oracle D-form loop", d_unipc, max(LATENT_TOL, 2.0 * d_dpmpp))
    seen = []
    z2, _ = sampler.sample(S, B, (3, 16, 16), callback=seen.append, **kw)
    assert seen == list(range(S))
    _within("UniPCSampler per-step path vs the native loop", rel_l2(z2, z), 2e-2)


def test_unipc_deterministic_rows_do_not_depend_on_the_batch(tiny):
    ctx, _, _ = tiny
    d = ctx.device
    g = torch.Generator(device=d).manual_seed(5)
    x = torch.randn(6, 3, 16, 16, device=d, generator=g)
    c = torch.randn(6, 4, 512, device=d, generator=g) * 0.45
    nodes = ctx.dpmpp_timesteps(5, ACP)
    ctx.set_deterministic(True)
    try:
        z6 = ctx.unipc_sample(nodes, x, c, torch.zeros_like(c), ACP, scale=2.0, order=3)[0]
        for r in (0, 4):
            z1 = ctx.unipc_sample(nodes, x[r:r + 1], c[r:r + 1], torch.zeros_like(c[r:r + 1]), ACP, scale=2.0, order=3)[0]
            assert torch.equal(z1, z6[r:r + 1]), f"row {r}: batch 1 and batch 6 differ"
    finally:
        ctx.set_deterministic(False)


def test_unipc_errors_leave_the_context_usable(tiny):
    from rdm_amd._lib import RdmError
    ctx, _, _ = tiny
    d = ctx.device
    x = torch.randn(2, 3, 16, 16, device=d)
    c = torch.randn(2, 4, 512, device=d) * 0.45
    uc = torch.zeros_like(c)
    good = [800, 500, 200, 0]
    bad_calls = {
        "a non-decreasing node list": lambda: ctx.unipc_sample([800, 500, 500, 0], x, c, None, ACP),
        "an increasing node list": lambda: ctx.unipc_sample([0, 200, 500], x, c, None, ACP),
        "a node equal to T": lambda: ctx.unipc_sample([1000, 500, 0], x, c, None, ACP),
        "a negative node": lambda: ctx.unipc_sample([500, 0, -1], x, c, None, ACP),
        "one node only": lambda: ctx.unipc_sample([500], x, c, None, ACP),
        "order 4": lambda: ctx.unipc_sample(good, x, c, None, ACP, order=4),
        "order 0": lambda: ctx.unipc_sample(good, x, c, None, ACP, order=0),
        "an unknown variant": lambda: ctx.unipc_sample(good, x, c, None, ACP, variant="vary_coeff"),
        "scale 0.5": lambda: ctx.unipc_sample(good, x, c, uc, ACP, scale=0.5),
        "guidance without uncond": lambda: ctx.unipc_sample(good, x, c, None, ACP, scale=2.0),
        "a wrong context width": lambda: ctx.unipc_sample(good, x, c[:, :, :256].contiguous(), None, ACP),
        "a batch mismatch": lambda: ctx.unipc_sample(good, x, c[:1], None, ACP),
        "a kernel call whose orders reach a null history slot": lambda: ctx.op_unipc_step(
            x, torch.zeros_like(x), ctx.unipc_coefficients(NODES10, ACP, 4, order=3), False, 1.0, torch.empty_like(x), xc_prev=x, h1=x),
    }
    for what, call in bad_calls.items():
        with pytest.raises(RdmError):
            call()
            pytest.fail(f"{what} was accepted")
        zz, xi, pi = ctx.unipc_sample(good, x, c, uc, ACP, scale=2.0, order=3, want_intermediates=True)
        torch.cuda.synchronize()
        assert zz.shape == x.shape and torch.isfinite(zz).all(), f"after {what}"
        assert xi.shape == pi.shape == (2,) + tuple(x.shape)          # log_every_t = 100 over 3 steps: the first step and index 0


def test_sample_with_query_uni_pc_end_to_end(model):
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    rng = np.random.default_rng(32)
    N = 2000
    pool = {"embedding": (rng.standard_normal((N, 512)) * 0.45).astype(np.float16), "img_id": np.arange(N),
            "patch_coords": rng.integers(0, 1200, (N, 4))}
    db = DatasetBuilder(data_pool=pool, k=20, ctx=model.ctx)
    db.train_searcher()
    model.retriever = db
    q = torch.from_numpy((rng.standard_normal((3, 512)) * 0.45).astype(np.float32))
    out = model.sample_with_query(query=q, query_embedded=True, k_nn=4, ddim=True, ddim_steps=4, uni_pc=True,
                                  unconditional_guidance_scale=2.0, unconditional_retro_guidance_label=0., visualize_nns=False)
    img = out["query_samples"]
    assert img.shape == (3, 3, 64, 64) and torch.isfinite(img).all()
