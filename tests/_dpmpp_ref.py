"""DPM-Solver++(2M) on integer timesteps, restated for the tests from the formulas (Lu et al. 2022, multistep data prediction), in the
solver's D-form -- not from the library's flattened coefficients c_x, c_0, c_1, so the two formulations check each other.

For a timestep t: a = float64(alphas_cumprod[t]), alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(a / (1 - a)) / 2.  Step j goes from
s = nodes[j] to t = nodes[j+1]:  m_j = (x - sigma_s eps) / alpha_s,  h_j = lambda_t - lambda_s,
D = (1 + 1/(2r)) m_j - (1/(2r)) m_{j-1} with r = h_{j-1} / h_j when order == 2, j >= 1 and not (lower_order_final and j == n - 2), else
D = m_j;  x <- (sigma_t / sigma_s) x - alpha_t expm1(-h_j) D."""
import math

import numpy as np


def node(acp, t):
    """(alpha, sigma, lambda) of timestep t in float64 from the fp32 alphas_cumprod."""
    a = float(np.asarray(acp, dtype=np.float32)[int(t)])
    return math.sqrt(a), math.sqrt(1.0 - a), 0.5 * math.log(a / (1.0 - a))


def timesteps(acp, S, skip_type):
    """The two grids.  time_uniform: DDIM's timesteps (arange(0, T, T // S) + 1) descending, then 0.  logSNR: S + 1 targets uniform in
    lambda from lambda(T - 1) to lambda(0), each rounded to the timestep of nearest lambda (ties to the smaller t: argmin takes the
    first), kept only when strictly below the previous kept one, 0 appended when missing."""
    acp = np.asarray(acp, dtype=np.float32)
    T = acp.shape[0]
    if skip_type == "time_uniform":
        ts = np.asarray(list(range(0, T, T // S))) + 1
        return [int(v) for v in ts[::-1]] + [0]
    a = acp.astype(np.float64)
    lam = 0.5 * np.log(a / (1.0 - a))
    out = []
    for i in range(S + 1):
        target = lam[T - 1] + (lam[0] - lam[T - 1]) * (float(i) / float(S))
        t = int(np.argmin(np.abs(lam - target)))
        if not out or t < out[-1]:
            out.append(t)
    if out[-1] != 0:
        out.append(0)
    return out


def is_second_order(j, n_steps, order, lower_order_final):
    return order == 2 and j >= 1 and not (lower_order_final and j == n_steps - 1)


def step(x, e, m_prev, acp, s, t, h_prev, second):
    """One D-form update on tensors of any dtype / device: -> (x_next, m_j, h_j).  The scalars are float64 Python numbers."""
    alpha_s, sigma_s, lam_s = node(acp, s)
    alpha_t, sigma_t, lam_t = node(acp, t)
    h = lam_t - lam_s
    m = (x - sigma_s * e) / alpha_s
    if second:
        r = h_prev / h
        D = (1.0 + 1.0 / (2.0 * r)) * m - (1.0 / (2.0 * r)) * m_prev
    else:
        D = m
    return (sigma_t / sigma_s) * x - alpha_t * math.expm1(-h) * D, m, h


def sample(eps, nodes, x_T, acp, order=2, lower_order_final=True, log_every_t=100, before_step=None):
    """The loop over a guided-eps callable eps(x, t_int) -> e.  before_step(x, j, t_int) -> x (the inpainting blend) is optional.
    -> (x, {"x_inter": [x_T, ...], "pred_x0": [x_T, ...]}, n_forwards), logged by the DDIM rule with index = n_steps - 1 - j."""
    n_steps = len(nodes) - 1
    x, m_prev, h_prev = x_T, None, None
    inter = {"x_inter": [x_T], "pred_x0": [x_T]}
    n_forwards = 0
    for j in range(n_steps):
        index = n_steps - 1 - j
        s, t = int(nodes[j]), int(nodes[j + 1])
        if before_step is not None:
            x = before_step(x, j, s)
        e = eps(x, s); n_forwards += 1
        second = is_second_order(j, n_steps, order, lower_order_final)
        x, m_prev, h_prev = step(x, e, m_prev, acp, s, t, h_prev, second)
        if index % log_every_t == 0 or index == n_steps - 1:
            inter["x_inter"].append(x)
            inter["pred_x0"].append(m_prev)
    return x, inter, n_forwards
