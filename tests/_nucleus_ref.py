"""Float64 restatement of the RARM sampler's nucleus (top-p) rule (include/rdm_hip.h, rdm_rarm_sample_top_p) -- test infrastructure.

Per row of guided, temperature-scaled logits g (the fp32 values the kernel forms, widened to float64):
  1. top-k first, unchanged (oracle.rarm.top_k_logits: values below the k-th largest dropped, ties with it kept): survivors K;
  2. p_i = exp(g_i - max) / sum over K, for i in K: mass relative to the top-k survivors;
  3. M(theta) = sum of p_i over i in K with g_i >= theta; theta* = the largest value present in K with M(theta*) >= top_p;
     the nucleus is { i in K : g_i >= theta* } (crossing token kept, its whole tie group kept, arg-max always kept);
  4. the draw is oracle.rarm.draw over the nucleus.
`top_p` is taken as the fp32 number the library receives.

`variant` names the deliberately WRONG restatements the near-miss tests must tell apart from the right one.
The error bands of the kernel's fp32 sums (u = 2^-24) are derived in tests/test_gpu_rarm_top_p.py and evaluated here."""
import numpy as np
import torch

from oracle import rarm as orarm

U = 2.0 ** -24
NEG = -float("inf")


def guided_logits(lc, lu, scale, temperature):
    """The kernel's logits: (lu + scale * (lc - lu)) * (1 / temperature) in fp32, the multiply-add fused (one rounding)."""
    lc = torch.as_tensor(lc, dtype=torch.float32)
    inv_t = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(temperature), dtype=torch.float32))
    if lu is None:
        return lc * inv_t
    lu = torch.as_tensor(lu, dtype=torch.float32)
    d = (lc - lu).double()                                    # fp32 difference
    s = float(np.float32(scale))
    return (lu.double() + s * d).float() * inv_t              # 24 x 24-bit product is exact in float64: the fused result


def _top_k(g, top_k):
    if top_k is None or top_k <= 0 or top_k >= g.shape[-1]:
        return g.clone()
    return orarm.top_k_logits(g, int(top_k))


def nucleus(g32, top_k, top_p, variant=None):
    """g32 [B, V] fp32 logits -> dict of [B]-shaped float64 / bool tensors:
    keep [B, V] (the nucleus), count, theta (theta*), m_star = M(theta*), m_next = M(next larger present value, 0 if none),
    margin = min(m_star - top_p, top_p - m_next), xk = sum over K of p_i |g_i - max| (for the error band).
    variant: None | 'whole_vocab' | 'strict' | 'cut_tie' | 'p_before_k'."""
    g = torch.as_tensor(g32).double()
    if g.ndim == 1:
        g = g[None]
    B, V = g.shape
    tp = float(np.float32(top_p))
    if variant == "p_before_k":                               # wrong order: nucleus over the whole vocabulary, then top-k of its members
        first = nucleus(g32, None, top_p)
        gk = _top_k(torch.where(first["keep"], g, torch.full_like(g, NEG)), top_k)
        keep = gk > NEG
        return dict(first, keep=keep, count=keep.sum(-1))
    gk = _top_k(g, top_k)
    in_k = gk > NEG
    mx = g.max(-1, keepdim=True).values
    e_all = torch.exp(g - mx)
    e = torch.where(in_k, e_all, torch.zeros_like(g))
    total = (e_all if variant == "whole_vocab" else e).sum(-1, keepdim=True)     # wrong: mass relative to the whole vocabulary
    p = e / total
    sg, order = torch.sort(gk, dim=-1, descending=True, stable=True)
    c = p.gather(-1, order).cumsum(-1)                        # mass of the descending prefix, inclusive
    is_end = torch.cat([sg[:, :-1] != sg[:, 1:], torch.ones((B, 1), dtype=torch.bool)], dim=1)
    # M(sg[j]) = the prefix mass at the END of j's tie group = the nearest group end at or after j (c never decreases)
    at_end = torch.where(is_end, c, torch.full_like(c, float("inf")))
    m_of = torch.flip(torch.cummin(torch.flip(at_end, [1]), dim=1).values, [1])
    reach = (m_of >= tp) & (sg > NEG)
    n_k = in_k.sum(-1)
    jstar = torch.where(reach.any(-1), reach.float().argmax(-1), n_k - 1)       # nothing reaches (whole_vocab variant): all of K
    rows = torch.arange(B)
    theta = sg[rows, jstar]
    m_star = m_of[rows, jstar]
    first_of_group = (sg == theta[:, None]).float().argmax(-1)
    m_next = torch.where(first_of_group > 0, c[rows, (first_of_group - 1).clamp(min=0)], torch.zeros(B, dtype=torch.float64))
    keep = gk >= theta[:, None]
    if variant == "strict":                                   # wrong: the crossing token (group) dropped; the arg-max group stays
        strict = gk > theta[:, None]
        keep = torch.where(strict.any(-1, keepdim=True), strict, keep)
    elif variant == "cut_tie":                                # wrong: a sort-based filter keeps ONE member of the boundary tie group
        tie = gk == theta[:, None]
        first_tie = tie.float().argmax(-1)
        keep = (gk > theta[:, None]) | (torch.arange(V)[None] == first_tie[:, None])
    xk = (p * (g - mx).abs() * in_k).sum(-1)
    return dict(keep=keep, count=keep.sum(-1), theta=theta, m_star=m_star, m_next=m_next,
                margin=torch.minimum(m_star - tp, tp - m_next), xk=xk)


def probs_of(g32, keep):
    g = torch.as_tensor(g32).double()
    if g.ndim == 1:
        g = g[None]
    return torch.softmax(torch.where(keep, g, torch.full_like(g, NEG)), dim=-1)


def draw(g32, keep, u):
    """Tokens [B] of the inverse-CDF draw over the kept set, each draw's distance |u - nearest CDF edge| (total = 1), and
    xn = sum over the kept set of p_i |g_i - max| (for draw_band)."""
    p = probs_of(g32, keep)
    u = torch.as_tensor(u)
    tok = orarm.draw(p, u)
    c = p.cumsum(-1)
    edge = (c / c[:, -1:] - u.double()[:, None]).abs().min(-1).values
    g = torch.as_tensor(g32).double().reshape(p.shape)
    xn = (p * torch.where(keep, (g - g.max(-1, keepdim=True).values).abs(), torch.zeros_like(g))).sum(-1)
    return tok, edge, xn


def mass_band(xk, top_p, depth=26):
    """|M^(theta)/T^ - M(theta)/T| the kernel's fp32 mass search can be off by, per row (derivation: test_gpu_rarm_top_p.py):
    u [(depth + 2) + 3 X] (1 + top_p) + u top_p with X = sum over K of p_i |g_i - max|."""
    return U * ((depth + 2 + 3.0 * xk) * (1.0 + top_p) + top_p)


def draw_band(xn, depth=320):
    """The same for the draw's running sums against u * total: 64-term chunk + 256 partials, serial (depth 320)."""
    return U * (2.0 * (depth + 2 + 3.0 * xn) + 1.0)


def sort_cumsum_keep(g32, top_k, top_p):
    """An independent formulation (the warper order of taming / HF): top-k, softmax, sort descending, drop every token whose
    PRECEDING cumulative mass already reaches top_p.  Equal to `nucleus` wherever no tie sits at the boundary."""
    g = np.asarray(g32, dtype=np.float64)
    out = np.zeros(g.shape, dtype=bool)
    tp = float(np.float32(top_p))
    for r in range(g.shape[0]):
        row = g[r].copy()
        if top_k is not None and 0 < top_k < row.size:
            kth = np.sort(row)[-top_k]
            row[row < kth] = -np.inf
        pr = np.exp(row - row.max()); pr /= pr.sum()
        idx = np.argsort(-row, kind="stable")
        before = np.concatenate([[0.0], np.cumsum(pr[idx])[:-1]])
        out[r, idx[(before < tp) & np.isfinite(row[idx])]] = True
    return out
