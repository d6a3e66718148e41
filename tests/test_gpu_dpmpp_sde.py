"""The native SDE-DPM-Solver++ sampler on the GPU: the step kernel alone per element against the float64 restatement and bound of
tests/_dpmpp_sde_ref.py (every size class of tests/_step_ref.py, into sentinel-guarded buffers) with its near misses; the seeded form bit
for bit against the stack form fed rdm_op_randn's output, and its refusals; the two loops (rdm_dpmpp_sde_sample / _seeded) against a loop
rebuilt from rdm_unet_forward_guided and the step op, against each other, across batch splits and seeds; and the end-to-end entry."""
import numpy as np
import pytest
import torch

from oracle import diffusion as odiff

import _dpmpp_sde_ref as ref
import _step_ref as R
from rdm_amd.models.diffusion.dpm_solver import DPMSolverSDESampler, dpmpp_sde_coefficients
from test_gpu_plms import model, tiny  # noqa: F401  (fixtures: the tiny UNet on the session context, the tiny model)
from test_gpu_step_ops import Bufs, _np, _same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ACP = odiff.Schedule().alphas_cumprod
ACP_NP = np.ascontiguousarray(ACP.numpy(), dtype=np.float32)
NODES10 = [999, 916, 821, 709, 571, 399, 212, 76, 19, 4, 0]           # the S = 10 logSNR grid (test_dpmpp_cpu.py records it)
# the two schedule points: a mid-schedule step (second order: after 709 -> 571) and the last step, to node 0 (after 19 -> 4)
POINTS = ((571, 399, 709), (4, 0, 19))
CONFIGS = {       # cfg, m_prev (second order), x_out in place, m_store aliases m_prev, x_dup and pred_x0
    "guided_second_ring_aliased_all_outputs": (True, True, False, True, True),
    "unguided_first_bare": (False, False, False, False, False),
    "guided_first_in_place": (True, False, True, False, False),
    "unguided_second_in_place_all_outputs": (False, True, True, False, True),
}


def _case(n, point, config):
    cfg, second, _, _, _ = CONFIGS[config]
    s, t, before = POINTS[point]
    sc, raw = ref.kernel_scalars(ACP_NP, s, t, before if second else None)
    arr = R.inputs(n, 7000003 * n + 31 * point + list(CONFIGS).index(config), ("x", "eps", "m_prev", "noise"), 2 if cfg else 1)
    if not second:
        arr["m_prev"] = None
    return arr, dict(cfg=cfg, scale=R.SCALE if cfg else 1.0, **sc), raw


def _call(ctx, x, eps, m_prev, noise, sc, x_out, **kw):
    ctx.op_dpmpp_sde_step(x, eps, m_prev, noise, sc["cfg"], sc["scale"], sc["sa"], sc["s1m"], sc["c_x"], sc["c_0"], sc["c_1"], sc["c_n"], x_out, **kw)


# ---- the stack form, element by element
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("n,off,point", R.GRID, ids=R.GRID_IDS)
def test_step_kernel_per_element_against_fp64(ctx, n, off, point, config):
    """dpmpp_sde_step_kernel<4> at offset 0 and n % 4 == 0 (second trip: n / 4 > 2048 * 256), else <1> (second trip: n > 2048 * 256; offset
    1 puts an n % 4 == 0 call there).  x and every output start `off` floats past an aligned address.  Every element of x_out and of m0
    (m_store, pred_x0) within the bound _dpmpp_sde_ref.kernel derives; every near miss outside it on the first MISS_ELEMENTS elements."""
    cfg, second, in_place, ring, outs = CONFIGS[config]
    arr, sc, raw = _case(n, point, config)
    b = Bufs(ctx)
    x, eps, noise = b.put(arr["x"], off, "x"), b.put(arr["eps"], 0, "eps"), b.put(arr["noise"], 0, "noise")
    m_prev = b.put(arr["m_prev"], 0, "m_prev")
    x_out = x if in_place else b.out(n, off, "x_out")
    x_dup = b.out(n, off, "x_dup") if outs else None
    pred_x0 = b.out(n, off, "pred_x0") if outs else None
    m_store = m_prev if ring else (b.out(n, off, "m_store") if config != "unguided_first_bare" else None)
    _call(ctx, x, eps, m_prev, noise, sc, x_out, x_dup=x_dup, m_store=m_store, pred_x0=pred_x0)
    b.check(written=[x_out, m_store])
    got = {"x_out": _np(x_out)}
    if m_store is not None:
        got["m0"] = _np(m_store)
    want = ref.kernel(**arr, **sc)
    lines = []
    for k, g in got.items():
        assert np.isfinite(g).all(), f"{k}: non-finite output"
        q, units = want[k].ratio(g), want[k].units(g, want["A_" + k])
        lines.append(f"{k}: worst |got - ref| / (2^-24 A) = {units:.2f} (K = {want['K_' + k]}), worst error / tolerance {q:.3f}")
        assert q <= 1.0, f"{k}: worst error / tolerance = {q:.3g}"
    m = min(n, R.MISS_ELEMENTS)
    small = R.head(arr, n, m)
    margin = float("inf")
    for miss in ref.misses(cfg, second):
        r = ref.kernel(**small, **ref.missed(sc, raw, miss), swapped=miss == "rows_swapped")
        q = max(r[k].ratio(g[:m]) for k, g in got.items())
        assert q > 1.0, f"near miss '{miss}' is within the bound (ratio {q:.3g})"
        margin = min(margin, q)
    print(f"[dpmpp sde] kernel {config} n={n} offset={off} step {POINTS[point][0]} -> {POINTS[point][1]}: " + "; ".join(lines) +
          f"; closest near miss {margin:.3g}")
    if outs:
        assert _same_bits(x_dup, x_out)
        assert _same_bits(pred_x0, m_store)


# ---- the seeded form
@pytest.mark.parametrize("row0", [0, 5])
@pytest.mark.parametrize("per_row", [192, 4096])
def test_seeded_step_equals_the_stack_step_fed_the_generator(ctx, per_row, row0):
    """B = 3 rows, guided, second order with the ring aliased, x_dup and pred_x0: every output bit for bit."""
    B, seed, step = 3, 0x5EED0123456789AB, 7
    n = B * per_row
    arr, sc, _ = _case(n, 0, "guided_second_ring_aliased_all_outputs")
    d = ctx.device
    up = lambda a: torch.from_numpy(a).to(d)
    z = ctx.op_randn(seed, B, per_row, row0=row0, step=step, stream=1).reshape(-1)
    outs = []
    for seeded in (False, True):
        x, eps, m_prev = up(arr["x"]), up(arr["eps"]), up(arr["m_prev"])
        o = {k: torch.full((n,), float("nan"), device=d) for k in ("x_out", "x_dup", "pred_x0")}
        kw = dict(seed=seed, row0=row0, per_row=per_row, step=step) if seeded else {}
        _call(ctx, x, eps, m_prev, None if seeded else z, sc, o["x_out"], x_dup=o["x_dup"], m_store=m_prev, pred_x0=o["pred_x0"], **kw)
        torch.cuda.synchronize()
        o["m_store"] = m_prev
        outs.append(o)
    for k in outs[0]:
        assert torch.isfinite(outs[0][k]).all() and _same_bits(outs[0][k], outs[1][k]), k
    # the noise is the step's own: another step counter, another row0 or no noise give other bits
    x_other = torch.empty(n, device=d)
    _call(ctx, up(arr["x"]), up(arr["eps"]), up(arr["m_prev"]), None, sc, x_other, seed=seed, row0=row0, per_row=per_row, step=step + 1)
    assert not _same_bits(x_other, outs[0]["x_out"])
    _call(ctx, up(arr["x"]), up(arr["eps"]), up(arr["m_prev"]), None, sc, x_other, seed=seed, row0=row0 + 1, per_row=per_row, step=step)
    assert not _same_bits(x_other, outs[0]["x_out"])


def test_seeded_step_refusals_leave_the_outputs_untouched(ctx):
    from rdm_amd._lib import RdmError
    d = ctx.device
    arr, sc, _ = _case(4 * 190, 0, "unguided_first_bare")
    up = lambda a: torch.from_numpy(a).to(d)
    b = Bufs(ctx)
    x_out = b.out(4 * 190, 0, "x_out")
    with pytest.raises(RdmError, match="multiple of 4"):                  # per_row % 4 != 0 (it divides n)
        _call(ctx, up(arr["x"]), up(arr["eps"]), None, None, sc, x_out, seed=1, per_row=190)
    with pytest.raises(RdmError, match="divides n"):                      # per_row does not divide n
        _call(ctx, up(arr["x"]), up(arr["eps"]), None, None, sc, x_out, seed=1, per_row=192)
    pred = b.out(4 * 190, 1, "pred_x0")                                   # one float past an aligned address
    with pytest.raises(RdmError, match="16-byte aligned"):
        _call(ctx, up(arr["x"]), up(arr["eps"]), None, None, sc, x_out, pred_x0=pred, seed=1, per_row=4 * 190 // 2)
    with pytest.raises(RdmError, match="per_row"):                        # a seeded call with a noise operand
        _call(ctx, up(arr["x"]), up(arr["eps"]), None, up(arr["noise"]), sc, x_out, seed=1, per_row=380)
    with pytest.raises(RdmError):                                         # neither a noise operand nor a seed
        _call(ctx, up(arr["x"]), up(arr["eps"]), None, None, sc, x_out)
    b.check()
    assert bool((x_out.view(torch.int32) == 0x7FC5A5A5).all()) and bool((pred.view(torch.int32) == 0x7FC5A5A5).all())
    _call(ctx, up(arr["x"]), up(arr["eps"]), None, None, sc, x_out, seed=1, per_row=380)
    torch.cuda.synchronize()
    assert torch.isfinite(x_out).all()


# ---- the loops
LATENT = (3, 16, 16)
PER_ROW = 3 * 16 * 16
S_LOOP = 6


class _deterministic:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_deterministic(True)

    def __exit__(self, *exc):
        self.ctx.set_deterministic(False)


def _conds(ctx, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    cond = (torch.randn(B, 4, 512, generator=g) * 0.45).to(ctx.device)
    return cond, torch.zeros_like(cond)


def _stack(ctx, seed, B, steps, row0=0):
    x_T = ctx.op_randn(seed, B, PER_ROW, row0=row0, step=0, stream=0).reshape((B,) + LATENT)
    noise = torch.stack([ctx.op_randn(seed, B, PER_ROW, row0=row0, step=j, stream=1).reshape((B,) + LATENT) for j in range(steps)])
    return x_T, noise


@pytest.fixture(scope="module")
def loops(tiny):
    """One run of each loop, shared by the tests below and left unchanged: six logSNR steps, B = 2, CFG 2.0, seed 77, deterministic mode."""
    ctx, _, _ = tiny
    B, seed = 2, 77
    nodes = ctx.dpmpp_timesteps(S_LOOP, ACP)
    assert nodes.tolist() == ref.timesteps(ACP_NP, S_LOOP, "logSNR") and len(nodes) == S_LOOP + 1
    cond, uncond = _conds(ctx, B)
    kw = dict(scale=2.0, order=2, lower_order_final=True, log_every_t=1, want_intermediates=True)
    with _deterministic(ctx):
        x_T, noise = _stack(ctx, seed, B, S_LOOP)
        stack = ctx.dpmpp_sde_sample(nodes, x_T, cond, uncond, ACP, noise=noise, **kw)
        seeded = ctx.dpmpp_sde_sample(nodes, None, cond, uncond, ACP, seed=seed, shape=LATENT, **kw)
    return dict(ctx=ctx, B=B, seed=seed, nodes=nodes, cond=cond, uncond=uncond, x_T=x_T, noise=noise, stack=stack, seeded=seeded, kw=kw)


def test_stack_loop_equals_the_loop_rebuilt_from_the_guided_forward_and_the_step_op(loops):
    """The Python per-step loop: rdm_unet_forward_guided at nodes[j], then rdm_op_dpmpp_sde_step with the coefficients of the Python
    helper (float64, rounded to fp32 as the library rounds its own), x in place with the second copy, ONE history slot -- x, every logged
    x_inter and every pred_x0 bit for bit."""
    ctx, B, nodes = loops["ctx"], loops["B"], loops["nodes"].tolist()
    z, xi, pi = loops["stack"]
    assert xi.shape[0] == pi.shape[0] == S_LOOP and torch.isfinite(z).all() and _same_bits(z, xi[-1])
    x = loops["x_T"].clone()
    m_slot = torch.empty_like(x)
    pred = torch.empty_like(x)
    h_prev = None
    with _deterministic(ctx):
        for j in range(S_LOOP):
            second = ref.is_second_order(j, S_LOOP, 2, True)
            eps = ctx.unet_forward_guided(x, nodes[j], loops["cond"], loops["uncond"])
            sa, s1m, c_x, c_0, c_1, c_n, h_prev = dpmpp_sde_coefficients(ACP_NP, nodes[j], nodes[j + 1], h_prev if second else None)
            ctx.op_dpmpp_sde_step(x, eps, m_slot if second else None, loops["noise"][j], True, 2.0, sa, s1m, c_x, c_0, c_1, c_n, x,
                                  m_store=m_slot, pred_x0=pred)
            torch.cuda.synchronize()
            assert _same_bits(x, xi[j]), f"step {j} (second order {second}): x differs"
            assert _same_bits(pred, pi[j]) and _same_bits(m_slot, pi[j]), f"step {j}: pred_x0 differs"
    assert _same_bits(x, z)
    with _deterministic(ctx):
        quiet = ctx.dpmpp_sde_sample(loops["nodes"], loops["x_T"], loops["cond"], loops["uncond"], ACP, noise=torch.zeros_like(loops["noise"]),
                                     scale=2.0, order=2, lower_order_final=True)[0]
    assert not _same_bits(quiet, z), "the noise stack has no effect: the comparison would show nothing"


def test_seeded_loop_equals_the_stack_loop_fed_the_generator(loops):
    ctx = loops["ctx"]
    for a, b in zip(loops["stack"], loops["seeded"]):
        assert _same_bits(a, b)
    with _deterministic(ctx):                   # the start given, the step noise generated
        z2 = ctx.dpmpp_sde_sample(loops["nodes"], loops["x_T"], loops["cond"], loops["uncond"], ACP, seed=loops["seed"], **loops["kw"])[0]
        z3, inter = DPMSolverSDESampler(_as_model(ctx)).sample(S_LOOP, loops["B"], LATENT, conditioning=loops["cond"], verbose=False,
                                                               unconditional_guidance_scale=2.0, unconditional_conditioning=loops["uncond"],
                                                               noise_seed=loops["seed"], log_every_t=1)
    assert _same_bits(z2, loops["stack"][0])
    assert _same_bits(z3, loops["stack"][0]) and _same_bits(inter["x_inter"][0], loops["x_T"]) and len(inter["x_inter"]) == S_LOOP + 1


def _as_model(ctx):
    """What DPMSolverSDESampler reads of a model on the native path"""
    class M:
        num_timesteps = ACP.shape[0]
        alphas_cumprod = ACP
        device = ctx.device
    M.ctx = ctx
    return M()


def test_intermediates_follow_the_ddim_logging_rule(loops):
    """log_every_t = 4 over six steps logs loop steps 0, 1 and 5 (index = 5 - j: 5 is the first step, 4 and 0 are multiples of 4)."""
    from rdm_amd import _lib
    ctx = loops["ctx"]
    kw = dict(loops["kw"], log_every_t=4)
    with _deterministic(ctx):
        z, xi, pi = ctx.dpmpp_sde_sample(loops["nodes"], loops["x_T"], loops["cond"], loops["uncond"], ACP, noise=loops["noise"], **kw)
        zs, xis, pis = ctx.dpmpp_sde_sample(loops["nodes"], None, loops["cond"], loops["uncond"], ACP, seed=loops["seed"], shape=LATENT, **kw)
    logged = [j for j in range(S_LOOP) if (S_LOOP - 1 - j) % 4 == 0 or j == 0]
    assert logged == [0, 1, 5] and xi.shape[0] == pi.shape[0] == len(logged) == _lib.lib.rdm_ddim_num_intermediates(S_LOOP, 4)
    _, xi1, pi1 = loops["stack"]
    for k, j in enumerate(logged):
        assert _same_bits(xi[k], xi1[j]) and _same_bits(pi[k], pi1[j]), f"logged entry {k} is not loop step {j}"
    assert _same_bits(z, loops["stack"][0]) and _same_bits(zs, z) and _same_bits(xis, xi) and _same_bits(pis, pi)


def test_seeded_rows_do_not_depend_on_the_sharding(loops):
    """Deterministic mode is batch-invariant and a row's noise is a function of its global index: rows 2..3 of a B = 4 call equal a B = 2
    call with row0 = 2."""
    ctx = loops["ctx"]
    cond, uncond = _conds(ctx, 4, seed=8)
    kw = dict(scale=2.0, seed=91, shape=LATENT)
    with _deterministic(ctx):
        whole = ctx.dpmpp_sde_sample(loops["nodes"], None, cond, uncond, ACP, **kw)[0]
        upper = ctx.dpmpp_sde_sample(loops["nodes"], None, cond[2:], uncond[2:], ACP, row0=2, **kw)[0]
        lower = ctx.dpmpp_sde_sample(loops["nodes"], None, cond[:2], uncond[:2], ACP, row0=0, **kw)[0]
    assert torch.isfinite(whole).all()
    assert _same_bits(whole[2:], upper) and _same_bits(whole[:2], lower) and not _same_bits(upper, lower)


def test_seeds_differ_and_a_seed_repeats(loops):
    ctx = loops["ctx"]
    run = lambda seed: ctx.dpmpp_sde_sample(loops["nodes"], loops["x_T"], loops["cond"], loops["uncond"], ACP, scale=2.0, seed=seed)[0]
    with _deterministic(ctx):
        a, b, c = run(5), run(6), run(5)
    assert torch.isfinite(a).all() and _same_bits(a, c) and not _same_bits(a, b)


def test_loop_refusals_leave_the_context_usable(loops):
    from rdm_amd._lib import RdmError
    ctx = loops["ctx"]
    nodes, x_T, cond, uncond, noise = (loops[k] for k in ("nodes", "x_T", "cond", "uncond", "noise"))
    bad_calls = {
        "a stack and a seed": lambda: ctx.dpmpp_sde_sample(nodes, x_T, cond, uncond, ACP, scale=2.0, noise=noise, seed=1),
        "neither": lambda: ctx.dpmpp_sde_sample(nodes, x_T, cond, uncond, ACP, scale=2.0),
        "a short stack": lambda: ctx.dpmpp_sde_sample(nodes, x_T, cond, uncond, ACP, scale=2.0, noise=noise[:-1]),
        "order 3": lambda: ctx.dpmpp_sde_sample(nodes, x_T, cond, uncond, ACP, scale=2.0, noise=noise, order=3),
        "a non-decreasing node list": lambda: ctx.dpmpp_sde_sample([800, 500, 500, 0], x_T, cond, None, ACP, noise=noise[:3]),
        "guidance without uncond": lambda: ctx.dpmpp_sde_sample(nodes, x_T, cond, None, ACP, scale=2.0, noise=noise),
        "a seeded call without x_T or a shape": lambda: ctx.dpmpp_sde_sample(nodes, None, cond, uncond, ACP, scale=2.0, seed=1),
        "rows past 32 bits": lambda: ctx.dpmpp_sde_sample(nodes, x_T, cond, uncond, ACP, scale=2.0, seed=1, row0=2 ** 32 - 2),
    }
    for what, call in bad_calls.items():
        with pytest.raises(RdmError):
            call()
            pytest.fail(f"{what} was accepted")
    with _deterministic(ctx):
        z = ctx.dpmpp_sde_sample(nodes, x_T, cond, uncond, ACP, noise=noise, scale=2.0, order=2, lower_order_final=True)[0]
    assert _same_bits(z, loops["stack"][0])


# ---- end to end
def test_sample_with_query_dpm_solver_sde_device_noise_end_to_end(model):
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    rng = np.random.default_rng(32)
    N = 2000
    pool = {"embedding": (rng.standard_normal((N, 512)) * 0.45).astype(np.float16), "img_id": np.arange(N),
            "patch_coords": rng.integers(0, 1200, (N, 4))}
    db = DatasetBuilder(data_pool=pool, k=20, ctx=model.ctx)
    db.train_searcher()
    model.retriever = db
    q = torch.from_numpy((rng.standard_normal((3, 512)) * 0.45).astype(np.float32))
    out = model.sample_with_query(query=q, query_embedded=True, k_nn=4, ddim=True, ddim_steps=4, dpm_solver_sde=True, device_noise=True,
                                  unconditional_guidance_scale=2.0, unconditional_retro_guidance_label=0., visualize_nns=False)
    img = out["query_samples"]
    assert img.shape == (3, 3, 64, 64) and torch.isfinite(img).all()
