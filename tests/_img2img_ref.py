"""float64 restatement of DDIM image-to-image as DESIGN.md section 3 defines it: the schedule's levels, the strength -> steps rule, the
forward-process start, the inversion step (in the form the kernel computes and in ldm's), and the three loops over a guided-eps callable
eps(x, t_int) -> e.  The loops run in whatever dtype x and eps carry (float64 for the accuracy figures, fp32 on the GPU for the
step-by-step comparisons); the scalars are python floats taken in float64 from the fp32 alphas_cumprod."""
import math

import numpy as np
import torch


def schedule(acp, S):
    """ldm's 'uniform' DDIM schedule of S steps over the fp32 alphas_cumprod: ascending timesteps ts (len(ts) may exceed S), and as
    float64 arrays a_t[i] = acp[ts[i]], a_prev[i] = acp[0] for i = 0, else acp[ts[i-1]]."""
    acp = np.asarray(acp, dtype=np.float32)
    T = acp.shape[0]
    ts = np.asarray(list(range(0, T, T // S))) + 1
    a_t = acp[ts].astype(np.float64)
    a_prev = np.concatenate([acp[:1], acp[ts[:-1]]]).astype(np.float64)
    return ts, a_t, a_prev


def strength_steps(strength, total):
    return min(total, max(1, int(strength * total)))


def stochastic_encode(x0, z, a):
    """sqrt(a) x0 + sqrt(1 - a) z at the level a."""
    return math.sqrt(a) * x0 + math.sqrt(1.0 - a) * z


def inverse_step(x, e, a_c, a_n):
    """One inversion step from the level a_c up to a_n, in the form the kernel computes.  -> (x_next, pred_x0)"""
    pred_x0 = (x - math.sqrt(1.0 - a_c) * e) / math.sqrt(a_c)
    return math.sqrt(a_n) * pred_x0 + math.sqrt(1.0 - a_n) * e, pred_x0


def inverse_step_ldm(x, e, a_c, a_n):
    """ldm DDIMSampler.encode's form of the same step: xt_weighted + weighted_noise_pred."""
    return math.sqrt(a_n / a_c) * x + math.sqrt(a_n) * (math.sqrt(1.0 / a_n - 1.0) - math.sqrt(1.0 / a_c - 1.0)) * e


def encode_timestep(ts, i, which):
    """The timestep the model sees at inversion step i: 'target' ts[i] (the definition), 'current' the timestep of the level the iterate
    is at (0 for the first step), 'index' ldm's loop index i."""
    return int(ts[i]) if which == "target" else (int(ts[i - 1]) if i else 0) if which == "current" else i


def encode(eps, x0, sched, t_enc, which="target", log_every_t=None):
    """t_enc inversion steps.  -> (x, [iterate after each logged step]); log_every_t None logs nothing."""
    ts, a_t, a_prev = sched
    x, inter = x0, []
    for i in range(t_enc):
        x, _ = inverse_step(x, eps(x, encode_timestep(ts, i, which)), float(a_prev[i]), float(a_t[i]))
        if log_every_t is not None and (i % log_every_t == 0 or i == t_enc - 1):
            inter.append(x)
    return x, inter


def ddim_step(x, e, a_t, a_prev, sigma=0.0, z=None, temperature=1.0):
    """The DDIM step down from the level a_t to a_prev.  -> (x_prev, pred_x0)"""
    pred_x0 = (x - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
    x_prev = math.sqrt(a_prev) * pred_x0 + math.sqrt(1.0 - a_prev - sigma ** 2) * e
    if sigma != 0.0:
        x_prev = x_prev + sigma * z * temperature
    return x_prev, pred_x0


def decode(eps, x, sched, t_start, eta=0.0, noise=None, log_every_t=None):
    """The DDIM loop from level index t_start - 1 down to index 0: t_start steps, noise[i] the i-th step's.  -> (x, x_inter, pred_x0)"""
    ts, a_t, a_prev = sched
    xi, pi = [], []
    for i in range(t_start):
        index = t_start - 1 - i
        at, ap = float(a_t[index]), float(a_prev[index])
        sigma = eta * math.sqrt((1.0 - ap) / (1.0 - at) * (1.0 - at / ap))
        x, p = ddim_step(x, eps(x, int(ts[index])), at, ap, sigma, None if noise is None else noise[i])
        if log_every_t is not None and (index % log_every_t == 0 or index == t_start - 1):
            xi.append(x); pi.append(p)
    return x, xi, pi


def gaussian_eps(acp, s):
    """The exact eps of data ~ N(0, s^2) per element, in float64: sqrt(1 - a) x / (a s^2 + 1 - a)."""
    ac = torch.as_tensor(np.asarray(acp, dtype=np.float32)).double()
    return lambda x, t: torch.sqrt(1 - ac[t]) * x.double() / (ac[t] * s ** 2 + 1 - ac[t])


def round_trip_error(acp, S, which, s=0.5, n=768, seed=0):
    """Relative error of encode -> decode over the whole S-step schedule on the Gaussian case, x0 = s N(0, 1), in float64."""
    x0 = s * torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    sched = schedule(acp, S)
    total = len(sched[0])
    eps = gaussian_eps(acp, s)
    x, _ = encode(eps, x0, sched, total, which)
    back, _, _ = decode(eps, x, sched, total)
    return float((back - x0).norm() / x0.norm())
