"""float64 restatements of the DDIM, PLMS and DDPM step kernels (csrc/sampler_steps.hip: ddim_step_kernel, plms_step_kernel<4|1>, ddpm_step_kernel and
the two seeded forms), the per-element bounds they are held to, their near misses and numpy fp32 emulations of the kernel text.

Every restatement takes the kernel's fp32 inputs and fp32 scalars and evaluates the expression in float64.  Beside each value it returns
A, the float64 sum of the absolute values of every term entering the element (for the guided eps |e_u| + scale (|e_c| + |e_u|)), and the
element's tolerance

    tol = K(count) * 2^-24 * A  [+ the allowance of a launch-uniform scalar that loses digits, below]

count: the fp32 roundings on the longest path from an input to the output, in the expression as the kernel text writes it, plus one for
each sqrtf scalar that multiplies or divides the element on that path.  K(count) = ceil(count * 16 / 11): the head-room
test_gpu_dpmpp.py gives its count of 11.  The counts:

    guided eps              e_c - e_u, scale *, e_u +                                                     3   (unguided: 0)
    DDIM pred_x0            guided + s1m *, x -, / sa, sqrtf(a_t)                                         7
    DDIM x_prev             pred_x0 + sap *, sqrtf(a_prev), + dir  [+ nz when there is noise]            10 [11]     K = 15 [16]
                            (dir = dirc e and nz = sigma z T are shorter side paths: guided + 3, and 3)
    PLMS e'                 guided + order 0 / Euler A: 0 | Euler B: 2 | order 1: 3 | order 2: 4 | order 3: 5  (the product with e_t,
                            one sum per further history term, the division)
    PLMS pred_x0            e' + 4                                          PLMS x_out   e' + 7 (guided order 3: 15, K = 22; the
                            s1p = sqrtf(1 - a_prev) side path is e' + 4: its product, two roundings of s1p, the sum)
    PLMS e_store            guided: 3 (K = 5); unguided: a copy
    DDPM x0                 sqrt_recip *, -                                                                2
    DDPM x_prev             x0 + coef1 *, + coef2 x, + nz                                                  5   K = 8

ddim_step_kernel and ddpm_step_kernel allow FMA contraction, which only removes roundings.

Launch-uniform scalars that lose digits are bounded on their own:
  * dirc = sqrtf(1 - a_prev - sigma_t^2): the radicand cancels; its absolute error is at most 3 * 2^-24 * (1 + a_prev + sigma_t^2) (three
    roundings, each of a value no larger than that sum; a contracted product removes one), so
        |dirc_fp32 - dirc_fp64| <= 3 * 2^-24 * (1 + a_prev + sigma_t^2) / (2 dirc) + 2^-24 dirc          (dirc_bound)
    and the element's tolerance grows by that * |e|.
  * sd = expf(0.5 log_var) (0.5 log_var is exact): held to float64 exp within SD_REL, and the element's tolerance grows by
    SD_REL * |sd z temperature|.  The HIP installation documents no accuracy figure for the device expf, so SD_REL is
    max(4 * SD_MEASURED, 4 ulp) with SD_MEASURED the worst relative error measured on an MI355X over the schedule's 1000
    posterior_log_variance_clipped values (test_gpu_step_ops.py measures it again, prints it and asserts SD_REL).

DDPM's clamp is a branch: an element whose float64 x0 lies within its own x0 tolerance of +-1 may take either branch (ddpm()'s
`boundary`); test_step_ops_cpu.py asserts their share stays below 1e-3 and that at least a tenth of x0 lies beyond each of +-1."""
import math

import numpy as np

from oracle import diffusion as odiff

U = 2.0 ** -24
SD_MEASURED = 6.6953e-08         # worst |expf(0.5 lv) - exp(0.5 lv)| / exp(0.5 lv) over the schedule, measured on an MI355X: 0.562 ulp, at t = 995
SD_REL = max(4.0 * SD_MEASURED, 4.0 * 2.0 ** -23)
PLMS_STEP, PLMS_EULER_A, PLMS_EULER_B = 0, 1, 2

SCHED = odiff.Schedule()
ACP = SCHED.alphas_cumprod.numpy().astype(np.float32)

# the (n, offset) grid of the three unseeded kernels: offset = floats past a 16-byte aligned address
SIZES = [(1027, 0), (4096, 0), (2304, 1), (2048 * 256 + 1, 0), (2 * 1024 * 1024 + 4, 0), (2048 * 256 + 1, 1)]
SIZE_IDS = ["n1027_scalar_tail", "n4096_vector", "n2304_misaligned", "n512Kplus1_second_trip", "n2Mplus4_vector_second_trip",
            "n512Kplus1_misaligned_second_trip"]


def K(count):
    return -(-count * 16 // 11)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- schedules: the scalars the loops hand the kernels
def ddim_scalars(S, index, eta):
    """(ts, a_t, a_prev, sigma_t, s1m) of schedule index `index` of the S-step 'uniform' DDIM schedule, fp32 as the loops compute them: the
    alphas read from the fp32 alphas_cumprod, np.sqrt(1 - a_t) in fp32, sigma in float64 from the fp32 alphas and rounded."""
    T = ACP.shape[0]
    ts = np.asarray(list(range(0, T, T // S))) + 1
    a_t = ACP[ts[index]]
    a_prev = ACP[0] if index == 0 else ACP[ts[index - 1]]
    s1m = np.sqrt(np.float32(1.0) - a_t)
    assert s1m.dtype == np.float32
    atd, apd = float(a_t), float(a_prev)
    sigma = np.float32(float(np.float32(eta)) * math.sqrt((1.0 - apd) / (1.0 - atd) * (1.0 - atd / apd)))       # eta: the fp32 field of rdm_ddim_args
    return int(ts[index]), float(a_t), float(a_prev), float(sigma), float(s1m)


def ddim_steps(S):
    T = ACP.shape[0]
    return len(range(0, T, T // S))


def ddpm_scalars(t):
    """(sqrt_recip, sqrt_recipm1, coef1, coef2, log_var) of timestep t: the fp32 posterior arrays of ldm's register_schedule."""
    g = lambda name: float(getattr(SCHED, name)[t])
    return (g("sqrt_recip_alphas_cumprod"), g("sqrt_recipm1_alphas_cumprod"), g("posterior_mean_coef1"), g("posterior_mean_coef2"),
            g("posterior_log_variance_clipped"))


def ddpm_arrays():
    return {k: getattr(SCHED, k).numpy() for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                                   "posterior_mean_coef2", "posterior_log_variance_clipped")}


def dirc_bound(a_prev, sigma_t):
    rad = 1.0 - a_prev - sigma_t * sigma_t
    d = math.sqrt(rad)
    return 3.0 * U * (1.0 + a_prev + sigma_t * sigma_t) / (2.0 * d) + U * d


def dirc_fp32(a_prev, sigma_t, contracted):
    """The kernel's dirc in numpy fp32; contracted: sigma_t * sigma_t fused into the subtraction."""
    one, ap, sg = np.float32(1.0), np.float32(a_prev), np.float32(sigma_t)
    rad = np.float32(float(one - ap) - float(sg) * float(sg)) if contracted else (one - ap) - sg * sg
    return np.sqrt(rad)


# ---- inputs (numpy fp32; the GPU file uploads these very arrays)
def inputs(n, seed, names, eps_rows=1):
    """standard normal fp32 vectors of n elements by name ('eps': eps_rows * n)."""
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal(n * (eps_rows if k == "eps" else 1)).astype(np.float32) for k in names}


def guided(eps, n, cfg, scale, swapped=False):
    """-> (e, A_e) in float64; swapped: the cond and uncond rows exchanged (a near miss)."""
    e_c = f64(eps[:n])
    if not cfg:
        return e_c, np.abs(e_c)
    e_u = f64(eps[n:])
    if swapped:
        e_c, e_u = e_u, e_c
    return e_u + scale * (e_c - e_u), np.abs(e_u) + scale * (np.abs(e_c) + np.abs(e_u))


def _over(err, tol):
    """err / tol per element, 0 where there is no error (an exact copy of an input that is 0 has tolerance 0)"""
    return np.divide(err, tol, out=np.zeros_like(err), where=err > 0)


class Out:
    """One output of a restatement: the float64 value, its tolerance, and for DDPM's boundary elements the other branch."""

    def __init__(self, want, tol, alt=None):
        self.want, self.tol, self.alt = want, tol, alt

    def ratio(self, got):
        """worst |got - want| / tol over the elements (a boundary element takes the better of its two branches)"""
        q = _over(np.abs(f64(got) - self.want), self.tol)
        if self.alt is not None:
            mask, want2, tol2 = self.alt
            q = np.where(mask, np.minimum(q, _over(np.abs(f64(got) - want2), tol2)), q)
        return float(q.max())

    def units(self, got, A):
        """worst |got - want| / (2^-24 A): what the reports print beside K (DDPM's boundary elements, which have two references, left out)"""
        q = _over(np.abs(f64(got) - self.want), U * A)
        return float((q if self.alt is None else np.where(self.alt[0], 0.0, q)).max())


# ---- DDIM
DDIM_MISSES = ("temperature_twice", "temperature_dropped", "sigma_squared", "dirc_without_sigma", "rows_swapped", "alphas_swapped")


def ddim(x, eps, noise, cfg, scale, a_t, a_prev, sigma_t, s1m, temperature, miss=None):
    """-> {"x_prev": Out, "pred_x0": Out, "A_x_prev": A, "A_pred_x0": A, "K_x_prev", "K_pred_x0"}.  noise None: no noise term."""
    X = f64(x); n = X.size
    E, EA = guided(eps, n, cfg, scale, swapped=miss == "rows_swapped")
    at, ap = (a_prev, a_t) if miss == "alphas_swapped" else (a_t, a_prev)
    sa, sap = math.sqrt(at), math.sqrt(ap)
    dirc = math.sqrt(1.0 - ap - (0.0 if miss == "dirc_without_sigma" else sigma_t * sigma_t))
    x0 = (X - s1m * E) / sa
    A0 = (np.abs(X) + s1m * EA) / sa
    xp = sap * x0 + dirc * E
    A = sap * A0 + dirc * EA
    g = 3 if cfg else 0
    count = g + 7
    if noise is not None:
        T = {"temperature_twice": temperature * temperature, "temperature_dropped": 1.0}.get(miss, temperature)
        nz = (sigma_t * sigma_t if miss == "sigma_squared" else sigma_t) * f64(noise) * T
        xp = xp + nz
        A = A + np.abs(nz)
        count += 1
    k_x, k_0 = K(count), K(g + 4)
    tol = k_x * U * A + dirc_bound(a_prev, sigma_t) * np.abs(E)
    return {"x_prev": Out(xp, tol), "pred_x0": Out(x0, k_0 * U * A0), "A_x_prev": A, "A_pred_x0": A0, "K_x_prev": k_x, "K_pred_x0": k_0}


def ddim_misses(cfg, noise, sigma_t, temperature):
    """the near misses that differ from the kernel's formula in this configuration"""
    out = ["alphas_swapped"]
    if cfg:
        out.append("rows_swapped")
    if sigma_t != 0.0:
        out.append("dirc_without_sigma")
        if noise is not None:
            out.append("sigma_squared")
            if temperature != 1.0:
                out += ["temperature_twice", "temperature_dropped"]
    return out


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64"""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def ddim_fp32(x, eps, noise, cfg, scale, a_t, a_prev, sigma_t, s1m, temperature, contracted):
    """ddim_step_kernel's text in numpy fp32 -> (x_prev, pred_x0); contracted: every product that feeds a sum fused into it."""
    f = np.float32
    n = x.size
    sa, sap = np.sqrt(f(a_t)), np.sqrt(f(a_prev))
    dirc = dirc_fp32(a_prev, sigma_t, contracted)
    e = eps[:n]
    if cfg:
        eu = eps[n:]
        e = _fma(f(scale), e - eu, eu) if contracted else eu + f(scale) * (e - eu)
    x0 = (_fma(-f(s1m), e, x) if contracted else x - f(s1m) * e) / sa
    dir_ = dirc * e
    nz = f(sigma_t) * noise * f(temperature) if noise is not None else f(0.0)
    xp = (_fma(sap, x0, dir_) if contracted else sap * x0 + dir_) + nz
    return xp.astype(np.float32), x0.astype(np.float32)


# ---- PLMS
def plms_combine(mode, order, E, EA, e_prev, h, miss=None):
    """e' and its A in float64.  h = (h1, h2, h3) float64 or None beyond the order."""
    if mode == PLMS_EULER_B:
        return (e_prev + E) / 2.0, (np.abs(e_prev) + EA) / 2.0, 2
    if mode == PLMS_EULER_A or order == 0:
        return E, EA, 0
    if miss == "lower_order":
        order -= 1
        if order == 0:
            return E, EA, 0
    ab = [None if v is None else np.abs(v) for v in h]
    if order == 1:
        return (3.0 * E - h[0]) / 2.0, (3.0 * EA + ab[0]) / 2.0, 3
    if order == 2:
        return (23.0 * E - 16.0 * h[0] + 5.0 * h[1]) / 12.0, (23.0 * EA + 16.0 * ab[0] + 5.0 * ab[1]) / 12.0, 4
    c1, c0 = (55.0, 59.0) if miss == "59_55_swapped" else (59.0, 55.0)
    div = 12.0 if miss == "div12_for_24" else 24.0
    return (c0 * E - c1 * h[0] + 37.0 * h[1] - 9.0 * h[2]) / div, (55.0 * EA + 59.0 * ab[0] + 37.0 * ab[1] + 9.0 * ab[2]) / 24.0, 5


def plms(x, eps, cfg, scale, a_t, a_prev, s1m, mode, order, e_prev=None, h1=None, h2=None, h3=None, miss=None):
    """-> {"x_out", "pred_x0", "e_store": Out (e_store None in Euler B), "A_*", "K_*"}"""
    X = f64(x); n = X.size
    E, EA = guided(eps, n, cfg, scale, swapped=miss == "rows_swapped")
    h = [None if v is None else f64(v) for v in (h1, h2, h3)]
    q = None if e_prev is None else f64(e_prev)
    if miss == "euler_b_unguided":
        O, OA, c = (q + f64(eps[:n])) / 2.0, (np.abs(q) + EA) / 2.0, 2
    else:
        O, OA, c = plms_combine(mode, order, E, EA, q, h, miss)
    if miss == "e_t_in_update":
        O = E
    at, ap = (a_prev, a_t) if miss == "alphas_swapped" else (a_t, a_prev)
    sa, sap, s1p = math.sqrt(at), math.sqrt(ap), math.sqrt(1.0 - ap)
    x0 = (X - s1m * O) / sa
    A0 = (np.abs(X) + s1m * OA) / sa
    xo = sap * x0 + s1p * O
    A = sap * A0 + s1p * OA
    g = 3 if cfg else 0
    k_x, k_0, k_e = K(g + c + 7), K(g + c + 4), K(3)
    out = {"x_out": Out(xo, k_x * U * A), "pred_x0": Out(x0, k_0 * U * A0), "A_x_out": A, "A_pred_x0": A0, "K_x_out": k_x, "K_pred_x0": k_0,
           "e_store": None, "A_e_store": EA, "K_e_store": k_e}
    if mode != PLMS_EULER_B:
        out["e_store"] = Out(E, k_e * U * EA)        # unguided: EA = |E| and the kernel copies, so the error is 0
    return out


def plms_misses(cfg, mode, order):
    out = ["alphas_swapped"]
    if cfg:
        out.append("rows_swapped")
    if mode == PLMS_EULER_B:
        out.append("e_t_in_update")
        if cfg:
            out.append("euler_b_unguided")
    if mode == PLMS_STEP and order >= 1:
        out += ["lower_order", "e_t_in_update"]
        if order == 3:
            out += ["59_55_swapped", "div12_for_24"]
    return out


def plms_fp32(x, eps, cfg, scale, a_t, a_prev, s1m, mode, order, e_prev=None, h1=None, h2=None, h3=None):
    """plms_step_kernel's text in numpy fp32 (no contraction) -> (x_out, pred_x0, e_t)"""
    f = np.float32
    n = x.size
    sa, sap, s1p = np.sqrt(f(a_t)), np.sqrt(f(a_prev)), np.sqrt(f(1.0) - f(a_prev))
    e = eps[:n]
    if cfg:
        u = eps[n:]
        e = u + f(scale) * (e - u)
    if mode == PLMS_EULER_B:
        o = (e_prev + e) / f(2.0)
    elif mode == PLMS_EULER_A or order == 0:
        o = e
    elif order == 1:
        o = (f(3.0) * e - h1) / f(2.0)
    elif order == 2:
        o = (f(23.0) * e - f(16.0) * h1 + f(5.0) * h2) / f(12.0)
    else:
        o = (f(55.0) * e - f(59.0) * h1 + f(37.0) * h2 - f(9.0) * h3) / f(24.0)
    x0 = (x - f(s1m) * o) / sa
    xo = sap * x0 + s1p * o
    assert xo.dtype == np.float32 and x0.dtype == np.float32
    return xo, x0, e


# ---- DDPM
def ddpm(x, eps, noise, sr, srm1, c1, c2, log_var, clip, nonzero, temperature, miss=None):
    """-> {"x_prev": Out, "A_x_prev", "K_x_prev", "beyond": (share of x0 > 1, share < -1), "boundary": share of either-branch elements}"""
    X, Ev = f64(x), f64(eps)
    if miss == "coefs_swapped":
        c1, c2 = c2, c1
    x0r = sr * X - srm1 * Ev
    A0 = np.abs(sr * X) + np.abs(srm1 * Ev)
    clamp_x0 = clip and miss not in ("no_clamp", "clamp_mean")
    x0 = np.clip(x0r, -1.0, 1.0) if clamp_x0 else x0r
    clamped = clamp_x0 & (np.abs(x0r) > 1.0)
    lin = c2 * X
    add_noise = bool(nonzero) or miss == "noise_at_zero"
    if add_noise:
        sd = math.exp(log_var if miss == "exp_full" else 0.5 * log_var)
        T = {"temperature_twice": temperature * temperature, "temperature_dropped": 1.0}.get(miss, temperature)
        nz = sd * f64(noise) * T
    else:
        nz = np.zeros_like(X)
    k = K(5)
    sd_allow = SD_REL * np.abs(nz)

    def branch(v0, a0):
        mean = c1 * v0 + lin
        if miss == "clamp_mean":
            mean = np.clip(mean, -1.0, 1.0)
        A = np.abs(c1) * a0 + np.abs(lin) + np.abs(nz)
        return mean + nz, k * U * A + sd_allow, A

    want_u, tol_u, A_u = branch(x0r, A0)
    if not clamp_x0:
        return {"x_prev": Out(want_u, tol_u), "A_x_prev": A_u, "K_x_prev": k, "beyond": (float((x0r > 1).mean()), float((x0r < -1).mean())),
                "boundary": 0.0}
    want_c, tol_c, A_c = branch(np.sign(x0r), np.ones_like(X))
    want = np.where(clamped, want_c, want_u); tol = np.where(clamped, tol_c, tol_u); A = np.where(clamped, A_c, A_u)
    near = np.abs(np.abs(x0r) - 1.0) <= K(2) * U * A0
    alt = (near, np.where(clamped, want_u, want_c), np.where(clamped, tol_u, tol_c))
    return {"x_prev": Out(want, tol, alt), "A_x_prev": A, "K_x_prev": k, "beyond": (float((x0r > 1).mean()), float((x0r < -1).mean())),
            "boundary": float(near.mean())}


def ddpm_misses(noise, clip, nonzero, temperature):
    out = ["coefs_swapped"]
    if clip:
        out += ["no_clamp", "clamp_mean"]
    if nonzero:
        out.append("exp_full")
        if temperature != 1.0:
            out += ["temperature_twice", "temperature_dropped"]
    elif noise is not None:
        out.append("noise_at_zero")
    return out


def ddpm_fp32(x, eps, noise, sr, srm1, c1, c2, log_var, clip, nonzero, temperature, contracted):
    """ddpm_step_kernel's text in numpy fp32 -> x_prev; contracted: each sum takes one of its products fused."""
    f = np.float32
    sd = np.exp(f(0.5) * f(log_var)) if nonzero else f(0.0)
    x0 = _fma(f(sr), x, -(f(srm1) * eps)) if contracted else f(sr) * x - f(srm1) * eps
    if clip:
        x0 = np.minimum(f(1.0), np.maximum(f(-1.0), x0))
    mean = _fma(f(c1), x0, f(c2) * x) if contracted else f(c1) * x0 + f(c2) * x
    out = mean + (sd * noise * f(temperature) if nonzero else f(0.0))
    assert out.dtype == np.float32
    return out


def closest_miss(got_by_output, restate, misses):
    """the smallest worst-ratio over the near misses: restate(miss) -> {name: Out}; every one must exceed 1 on some output"""
    margin = math.inf
    for m in misses:
        r = restate(m)
        q = max(r[k].ratio(g) for k, g in got_by_output.items() if r.get(k) is not None)
        assert q > 1.0, f"near miss '{m}' is within the bound (ratio {q:.3g})"
        margin = min(margin, q)
    return margin


# ---- the cases both test files run: the GPU file uploads these arrays, the CPU file feeds them to the fp32 emulations
# (n, offset, schedule point): the whole size grid at DDIM / PLMS index 5 of S = 10 and DDPM t = 500; the two small sizes again at index 0
# (a_prev = alphas_cumprod[0]: the smallest radicand) and t = 1 (the most negative log_var)
GRID = [(n, off, 0) for n, off in SIZES] + [(1027, 0, 1), (4096, 0, 1)]
GRID_IDS = [s + "_mid" for s in SIZE_IDS] + ["n1027_scalar_tail_edge", "n4096_vector_edge"]
DDIM_POINTS, DDPM_POINTS = (5, 0), (500, 1)
MISS_ELEMENTS = 4096          # near misses are told apart on the first elements of a large case: the formula does not depend on the index

DDIM_CONFIGS = {       # cfg, eta, temperature, noise, x_dup, pred_x0, in place
    "guided_noise_t07_all_outputs": (True, 0.7, 0.7, True, True, True, False),
    "unguided_eta0_bare": (False, 0.0, 1.0, False, False, False, False),
    "guided_eta1_in_place": (True, 1.0, 1.0, True, True, False, True),
}
PLMS_CONFIGS = {       # cfg, mode, order
    "euler_a_guided": (True, PLMS_EULER_A, 0), "euler_b_guided": (True, PLMS_EULER_B, 0), "order0_unguided": (False, PLMS_STEP, 0),
    "order1_guided": (True, PLMS_STEP, 1), "order2_unguided": (False, PLMS_STEP, 2), "order3_guided_ring_aliased": (True, PLMS_STEP, 3),
}
DDPM_CONFIGS = {       # clip, nonzero, temperature, noise operand, in place
    "clip_noise_t07": (True, True, 0.7, True, False),
    "noclip_noise_t1": (False, True, 1.0, True, False),
    "clip_last_step_noise_ignored": (True, False, 0.7, True, False),
    "noclip_last_step_null_noise": (False, False, 1.0, False, False),
    "clip_noise_t1_in_place": (True, True, 1.0, True, True),
}
SCALE = 2.0


def _seed(n, point, config, configs):
    return 1000003 * n + 101 * point + list(configs).index(config)


def ddim_case(n, point, config):
    """-> (arrays {x, eps, noise | None}, scalars {cfg, scale, a_t, a_prev, sigma_t, s1m, temperature})"""
    cfg, eta, temperature, has_noise, _, _, _ = DDIM_CONFIGS[config]
    _, a_t, a_prev, sigma_t, s1m = ddim_scalars(10, DDIM_POINTS[point], eta)
    arr = inputs(n, _seed(n, point, config, DDIM_CONFIGS), ("x", "eps", "noise"), 2 if cfg else 1)
    if not has_noise:
        arr["noise"] = None
    return arr, dict(cfg=cfg, scale=SCALE if cfg else 1.0, a_t=a_t, a_prev=a_prev, sigma_t=sigma_t, s1m=s1m, temperature=temperature)


def plms_case(n, point, config):
    """-> (arrays {x, eps, e_prev, h1, h2, h3 (None where the mode / order does not read them)}, scalars)"""
    cfg, mode, order = PLMS_CONFIGS[config]
    _, a_t, a_prev, _, s1m = ddim_scalars(10, DDIM_POINTS[point], 0.0)
    arr = inputs(n, _seed(n, point, config, PLMS_CONFIGS), ("x", "eps", "e_prev", "h1", "h2", "h3"), 2 if cfg else 1)
    if mode != PLMS_EULER_B:
        arr["e_prev"] = None
    for j in (1, 2, 3):
        if mode != PLMS_STEP or order < j:
            arr[f"h{j}"] = None
    return arr, dict(cfg=cfg, scale=SCALE if cfg else 1.0, a_t=a_t, a_prev=a_prev, s1m=s1m, mode=mode, order=order)


def ddpm_case(n, point, config):
    """-> (arrays {x, eps, noise | None}, scalars)"""
    clip, nonzero, temperature, has_noise, _ = DDPM_CONFIGS[config]
    sr, srm1, c1, c2, log_var = ddpm_scalars(DDPM_POINTS[point])
    arr = inputs(n, _seed(n, point, config, DDPM_CONFIGS), ("x", "eps", "noise"))
    if not has_noise:
        arr["noise"] = None
    return arr, dict(sr=sr, srm1=srm1, c1=c1, c2=c2, log_var=log_var, clip=clip, nonzero=nonzero, temperature=temperature)


def head(arr, n, m):
    """the first m elements of every operand of an n-element case (eps: of both halves)"""
    out = {}
    for k, v in arr.items():
        out[k] = None if v is None else (v[:m] if v.size == n else np.concatenate([v[:m], v[n:n + m]]))
    return out


def check(kind, arr, sc, got, misses):
    """got {output name: numpy fp32} of one case against the restatement `kind` (ddim | plms | ddpm): every output within its tolerance,
    every near miss outside on the first MISS_ELEMENTS elements.  -> (report lines, worst ratio, closest near miss)"""
    fn = {"ddim": ddim, "plms": plms, "ddpm": ddpm}[kind]
    ref = fn(**arr, **sc)
    lines, worst = [], 0.0
    for k, g in got.items():
        assert np.isfinite(g).all(), f"{k}: non-finite output"
        q = ref[k].ratio(g)
        units = ref[k].units(g, ref["A_" + k])
        lines.append(f"{k}: worst |got - ref| / (2^-24 A) = {units:.2f} (K = {ref['K_' + k]}), worst error / tolerance {q:.3f}")
        assert q <= 1.0, f"{k}: worst error / tolerance = {q:.3g}"
        worst = max(worst, q)
    n = arr["x"].size
    m = min(n, MISS_ELEMENTS)
    small = head(arr, n, m)
    margin = closest_miss({k: g[:m] for k, g in got.items()}, lambda miss: fn(**small, **sc, miss=miss), misses)
    return lines, worst, margin
