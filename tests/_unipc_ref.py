"""UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models"), multistep data
prediction on a list of nodes, restated for the tests in float64 from the paper's algorithm, in the solver's D-form with numpy solves
-- not from the library's flattened coefficients, so the two formulations check each other.

A node i carries (alpha_i, sigma_i, lambda_i), lambda = log(alpha / sigma); from a timestep t: a = float64(alphas_cumprod[t]),
alpha = sqrt(a), sigma = sqrt(1 - a).  n steps, n forwards at nodes 0 .. n-1; u_j is the model input at node j (u_0 = x_0 = x_T),
m_j = (u_j - sigma_j eps_j) / alpha_j.  Step s (1-based, ending at node s) at order p:

    h = lambda_s - lambda_{s-1}, hh = -h, phi_1 = expm1(hh), B = hh (bh1) | expm1(hh) (bh2)
    r_i = (lambda_{s-1-i} - lambda_{s-1}) / h  (i = 1 .. p-1),  r_p = 1
    g_1 = phi_1 / hh - 1, g_{i+1} = g_i / hh - 1 / (i+1)!,  b_i = g_i i! / B,  R_{i,k} = r_k^{i-1}
    rho^p (p - 1 values): none | [1/2] | solve(R[1..2, 1..2], b[1..2]);   rho^c (p values): [1/2] | solve(R, b)
    D_i = (m_{s-1-i} - m_{s-1}) / r_i,  base = (sigma_s / sigma_{s-1}) x_{s-1} - alpha_s phi_1 m_{s-1}
    u_s = base - alpha_s B sum_{i<p} rho^p_i D_i
    x_s = base - alpha_s B (sum_{i<p} rho^c_i D_i + rho^c_p (m_s - m_{s-1}))        (m_s from the forward at u_s; corrector off: x_s = u_s)
"""
import math

import numpy as np


def node(acp, t):
    """(alpha, sigma, lambda) of timestep t in float64 from the fp32 alphas_cumprod."""
    a = float(np.asarray(acp, dtype=np.float32)[int(t)])
    return math.sqrt(a), math.sqrt(1.0 - a), 0.5 * math.log(a / (1.0 - a))


def node_values(acp, nodes):
    return [node(acp, t) for t in nodes]


def step_order(s, n, order, lower_order_final):
    p = min(order, s)
    return min(p, n + 1 - s) if lower_order_final else p


def weights(asl, s, p, variant):
    """-> (phi_1, B, r[0 .. p-2], rho_p[0 .. p-2], rho_c[0 .. p-1]) of step s at order p."""
    lam = [v[2] for v in asl]
    h = lam[s] - lam[s - 1]
    hh = -h
    phi1 = math.expm1(hh)
    B = {"bh1": hh, "bh2": math.expm1(hh)}[variant]
    r = [(lam[s - 1 - i] - lam[s - 1]) / h for i in range(1, p)]
    rk = np.asarray(r + [1.0], dtype=np.float64)
    g, b = phi1 / hh - 1.0, []
    for i in range(1, p + 1):
        b.append(g * math.factorial(i) / B)
        g = g / hh - 1.0 / math.factorial(i + 1)
    b = np.asarray(b, dtype=np.float64)
    R = np.stack([rk ** i for i in range(p)])          # R[i, k] = r_k^i (0-based i)
    if p == 1:
        rho_p, rho_c = [], [0.5]
    else:
        rho_c = np.linalg.solve(R, b).tolist()
        if p == 2:
            rho_p = [0.5]                              # the published shortcut, not the solve
        else:
            rho_p = np.linalg.solve(R[:p - 1, :p - 1], b[:p - 1]).tolist()
    return phi1, B, r, rho_p, rho_c


def _base(asl, s, phi1, x_prev, m_hist):
    return (asl[s][1] / asl[s - 1][1]) * x_prev - asl[s][0] * phi1 * m_hist[0]


def predict(asl, s, p, variant, x_prev, m_hist):
    """u_s from x_{s-1} and m_hist = [m_{s-1}, m_{s-2}, ...] (p entries used)."""
    phi1, B, r, rho_p, _ = weights(asl, s, p, variant)
    out = _base(asl, s, phi1, x_prev, m_hist)
    if p > 1:
        acc = 0.0
        for i in range(1, p):
            acc = acc + rho_p[i - 1] * ((m_hist[i] - m_hist[0]) / r[i - 1])
        out = out - asl[s][0] * B * acc
    return out


def correct(asl, s, p, variant, x_prev, m_hist, m_s):
    """x_s from x_{s-1}, m_hist = [m_{s-1}, m_{s-2}, ...] (p entries used) and m_s."""
    phi1, B, r, _, rho_c = weights(asl, s, p, variant)
    acc = rho_c[p - 1] * (m_s - m_hist[0])
    for i in range(1, p):
        acc = acc + rho_c[i - 1] * ((m_hist[i] - m_hist[0]) / r[i - 1])
    return _base(asl, s, phi1, x_prev, m_hist) - asl[s][0] * B * acc


def flat_coefficients(asl, j, order, variant, corrector, lower_order_final):
    """The pass after forward j as 13 numbers (alpha_j, sigma_j, a_x, a_t, a_1, a_2, a_3, b_x, b_0, b_1, b_2, order_c, order_p): each
    coefficient is the D-form update applied to a unit input, the updates being linear."""
    n = len(asl) - 1
    out = [asl[j][0], asl[j][1]]
    pc = step_order(j, n, order, lower_order_final) if (corrector and j >= 1) else 0
    if pc:
        unit = lambda k: [1.0 if i == k else 0.0 for i in range(5)]          # x_{j-1}, m_j, m_{j-1}, m_{j-2}, m_{j-3}
        out += [correct(asl, j, pc, variant, v[0], v[2:], v[1]) for v in map(unit, range(5))]
    else:
        out += [0.0] * 5
    pp = step_order(j + 1, n, order, lower_order_final)
    unit = lambda k: [1.0 if i == k else 0.0 for i in range(4)]              # x_j, m_j, m_{j-1}, m_{j-2}
    out += [predict(asl, j + 1, pp, variant, v[0], v[1:]) for v in map(unit, range(4))]
    return np.asarray(out + [float(pc), float(pp)], dtype=np.float64)


def sample(eps, nodes, x_T, acp, order=2, variant="bh2", corrector=True, lower_order_final=True, log_every_t=100):
    """The loop over a guided-eps callable eps(u, t_int) -> e.
    -> (z, {"x_inter": [x_T, u_1, ...], "pred_x0": [x_T, m_0, ...]}, n_forwards), logged by the DDIM rule with index = n - 1 - j."""
    asl = node_values(acp, nodes)
    n = len(nodes) - 1
    u = x = x_T
    ms = []                                    # m_{j-1}, m_{j-2}, ...
    inter = {"x_inter": [x_T], "pred_x0": [x_T]}
    n_forwards = 0
    for j in range(n):
        index = n - 1 - j
        e = eps(u, int(nodes[j])); n_forwards += 1
        m = (u - asl[j][1] * e) / asl[j][0]
        if corrector and j >= 1:
            x = correct(asl, j, step_order(j, n, order, lower_order_final), variant, x, ms, m)
        else:
            x = u
        ms = [m] + ms[:2]
        u = predict(asl, j + 1, step_order(j + 1, n, order, lower_order_final), variant, x, ms)
        if index % log_every_t == 0 or index == n - 1:
            inter["x_inter"].append(u)
            inter["pred_x0"].append(m)
    return u, inter, n_forwards
