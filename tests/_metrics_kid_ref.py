"""Float64 numpy restatements of the count, nearest and cubic-kernel modes of metric_dist_kernel (csrc/metrics.hip) and of
rdm_amd.metrics.density_coverage / kernel_distance, the bounds the GPU tests hold them to, and the seeded inputs those tests share.
tests/test_metrics_kid_cpu.py checks the restatements against brute-force loops and re-checks every condition the inputs are picked for.

Bounds (none measured on the code under test; D2_GAMMA = 5e-7 and its derivation are tests/_metrics_ref.py's).
  d2:       D2_GAMMA (|a|^2 + |b|^2).
  nearest:  a minimum moves by at most the largest change of any of its arguments: per probe, D2_GAMMA (|probe_i|^2 + max_j |ref_j|^2).
  counts:   equal to fp64, on inputs where no pair lies within hit_margin_ok's margin of its radius.
  poly:     a d2 is two norms minus twice the dot product, so the dot product's share of the d2 budget is
            delta = (D2_GAMMA / 2) (|a|^2 + |b|^2)  (the header's "dot product within 2.5e-7 (|a|^2 + |b|^2)").  With v = gamma dot + coef0
            in fp64, a pair's k = v^3 may move by (|v| + gamma delta)^3 - |v|^3; a row sum by the sum of its pairs' bounds plus
            n 2^-52 SUM_j |k_ij| for the fp64 adds (2^-53 relative each, on either side of the comparison).
  KID:      the three terms' bounds combined as the terms are: bxx / (m (m - 1)) + byy / (n (n - 1)) + 2 bxy / (m n).
"""
import numpy as np

import _metrics_ref as R

DOT_GAMMA = R.D2_GAMMA / 2


# ------------------------------------------------------------------------------------------------ counts, nearest, density / coverage
def manifold_counts(probe, ref, ref_radius2, d2=None):
    """count [m] int64: #{ j : d2(probe_i, ref_j) <= ref_radius2[j] }."""
    d2 = R.d2_matrix(probe, ref) if d2 is None else d2
    return (d2 <= np.asarray(ref_radius2, np.float64)[None, :]).sum(1)


def nearest_d2(probe, ref, d2=None):
    d2 = R.d2_matrix(probe, ref) if d2 is None else d2
    return d2.min(1)


def nearest_bound(probe, ref):
    return R.D2_GAMMA * (R.sqnorms(probe) + R.sqnorms(ref).max())


def density_coverage(real, gen, k):
    """Naeem et al. 2020: (SUM over gen rows of the real k-NN balls they lie in / (k n_gen), share of real rows with a gen row in their ball)."""
    r_real = R.knn_radius2(real, k)
    density = float(manifold_counts(gen, real, r_real).sum()) / (k * np.asarray(gen).shape[0])
    coverage = float((nearest_d2(real, gen) <= r_real).mean())
    return density, coverage


def dc_margin_ok(real, gen, k):
    """density_coverage composes kernels as precision_recall does: both comparisons hold a d2 (within its bound) against a radius that is
    itself a kernel result (within radius_bound(real)).  Exact agreement with the restatement follows when every (gen, real) pair keeps the
    margin of R.pr_margin_ok, and every real row keeps |min_j d2_ij - r2_i| above max_j d2 bound + radius_bound.
    -> (ok, smallest coverage gap / its margin)."""
    r2 = R.knn_radius2(real, k)
    rb = R.radius_bound(real)
    d2 = R.d2_matrix(gen, real)
    gap = np.abs(d2 - r2[None, :])
    ok = bool((gap > np.maximum(2 * R.d2_bound_matrix(gen, real), R.d2_bound_matrix(gen, real) + rb)).all())
    cgap = np.abs(nearest_d2(real, gen) - r2)
    cmargin = nearest_bound(real, gen) + rb
    return ok and bool((cgap > cmargin).all()), float((cgap / cmargin).min())


def identical_case():
    """The set the identical-sets test hands in twice (tests/test_metrics_kid_cpu.py checks its neighbour gaps)."""
    return R.feature_rows(150, 64, 9)


# (n, d) -> seed of the count tests' inputs (tests/test_metrics_kid_cpu.py re-checks the conditions they were picked for)
COUNT_SEEDS = {(127, 32): 300, (129, 32): 300, (127, 512): 300, (129, 512): 300, (257, 64): 300}
COUNT_PAIRS = 4 * 130


def counts_case(m, n, d, seed, k=5):
    """-> (probe f32 [m, d], ref f32 [n, d], ref_radius2 f32 [n]): the ref rows' k-NN radii, all scaled by ONE factor such that about
    4 x 130 pairs of the 130-row parent probe set fall inside their ball (a mean count of 4): pair (i, j) is inside from the factor
    d2_ij / r2_j on, and the factor is the midpoint of the widest gap among the ten sorted ratios after the 520th.  Smaller m take the
    first rows of the parent set."""
    ref = R.feature_rows(n, d, seed)
    parent = R.feature_rows(130, d, seed + 1000)
    r2 = R.knn_radius2(ref, k)
    rho = np.sort((R.d2_matrix(parent, ref) / r2[None, :]).ravel())
    i = COUNT_PAIRS + int(np.argmax(np.diff(rho[COUNT_PAIRS:COUNT_PAIRS + 11])))
    return parent[:m].copy(), ref, (0.5 * (rho[i] + rho[i + 1]) * r2).astype(np.float32)


# ------------------------------------------------------------------------------------------------ cubic-kernel row sums, KID
def _dots(a, b):
    return np.asarray(a, np.float64) @ np.asarray(b, np.float64).T


def poly3_rowsums(probe, ref, gamma, coef0, exclude_same_index=False):
    """rowsum [m] in fp64: SUM_j (gamma probe_i . ref_j + coef0)^3, without j == i when exclude_same_index."""
    k = (gamma * _dots(probe, ref) + coef0) ** 3
    if exclude_same_index:
        q = min(k.shape)
        k[np.arange(q), np.arange(q)] = 0.0
    return k.sum(1)


def poly3_pair_bounds(probe, ref, gamma, coef0, exclude_same_index=False):
    """-> (pair bounds [m, n], |k| [m, n]), the excluded pairs at 0 in both."""
    v = np.abs(gamma * _dots(probe, ref) + coef0)
    delta = DOT_GAMMA * (R.sqnorms(probe)[:, None] + R.sqnorms(ref)[None, :])
    pb, k = (v + abs(gamma) * delta) ** 3 - v ** 3, v ** 3
    if exclude_same_index:
        q = min(k.shape)
        pb[np.arange(q), np.arange(q)] = 0.0
        k[np.arange(q), np.arange(q)] = 0.0
    return pb, k


def poly3_bound(probe, ref, gamma, coef0, exclude_same_index=False):
    """bound [m] of a row sum: its pairs' bounds plus n 2^-52 SUM_j |k_ij|."""
    pb, k = poly3_pair_bounds(probe, ref, gamma, coef0, exclude_same_index)
    return pb.sum(1) + k.shape[1] * 2.0 ** -52 * k.sum(1)


def kid_terms(x, y, gamma, coef0):
    """-> ((SUM xx without diagonal, SUM yy without diagonal, SUM xy), their bounds) in fp64."""
    sums = (poly3_rowsums(x, x, gamma, coef0, True).sum(), poly3_rowsums(y, y, gamma, coef0, True).sum(), poly3_rowsums(x, y, gamma, coef0).sum())
    bounds = (poly3_bound(x, x, gamma, coef0, True).sum(), poly3_bound(y, y, gamma, coef0, True).sum(), poly3_bound(x, y, gamma, coef0).sum())
    return sums, bounds


def kid(x, y, gamma=None, coef0=1.0):
    """-> (unbiased MMD^2 of the whole sets, its bound).  gamma=None: 1 / d."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    m, n = x.shape[0], y.shape[0]
    (sxx, syy, sxy), (bxx, byy, bxy) = kid_terms(x, y, gamma, coef0)
    return sxx / (m * (m - 1.0)) + syy / (n * (n - 1.0)) - 2.0 * sxy / (m * n), bxx / (m * (m - 1.0)) + byy / (n * (n - 1.0)) + 2.0 * bxy / (m * n)


def kid_near_misses(x, y, gamma=None, coef0=1.0):
    """What a wrong kernel_distance would return: each must lie outside kid()'s bound."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = x.shape[1]
    gamma = 1.0 / d if gamma is None else gamma
    m, n = x.shape[0], y.shape[0]
    (sxx, syy, sxy), _ = kid_terms(x, y, gamma, coef0)
    dx = ((gamma * (x * x).sum(1) + coef0) ** 3).sum()
    dy = ((gamma * (y * y).sum(1) + coef0) ** 3).sum()
    return {"biased (diagonal kept, / s^2)": (sxx + dx) / (m * m) + (syy + dy) / (n * n) - 2.0 * sxy / (m * n),
            "coef0 = 0": kid(x, y, gamma, 0.0)[0],
            "gamma = 1 / (d + 32)": kid(x, y, gamma * d / (d + 32.0), coef0)[0],
            "cross term once": sxx / (m * (m - 1.0)) + syy / (n * (n - 1.0)) - sxy / (m * n),
            "0": 0.0}


def kid_subsets(x, y, subsets, subset_size, seed, gamma=None, coef0=1.0):
    """kernel_distance's subset draw restated: -> (values [subsets], bounds [subsets])."""
    x, y = np.asarray(x), np.asarray(y)
    s = min(subset_size, x.shape[0], y.shape[0])
    rng = np.random.default_rng(seed)
    vals, bounds = [], []
    for _ in range(subsets):
        ix = rng.choice(x.shape[0], s, replace=False)
        iy = rng.choice(y.shape[0], s, replace=False)
        v, b = kid(x[ix], y[iy], gamma, coef0)
        vals.append(v); bounds.append(b)
    return np.array(vals), np.array(bounds)


def kid_pairs():
    """The four (real, gen) pairs of the KID tests, float32."""
    f = R.feature_rows
    return {"pr_clouds": R.pr_clouds(),
            "257x512": (f(257, 512, 11), (0.9 * f(129, 512, 12) + 0.02).astype(np.float32)),
            "129x32": (f(129, 32, 13), (0.9 * f(127, 32, 14) + 0.05).astype(np.float32)),
            "clip-scaled": ((10 * f(257, 512, 15)).astype(np.float32), (9 * f(200, 512, 16) + 0.1).astype(np.float32))}


def poly_case(m, n, d):
    """Probe and ref of the row-sum tests: two views of ONE seeded set, ref = 0.9 x + 0.02, so the pair of equal row index has a large
    positive dot product (0.9 |x_i|^2 + ...) and leaving it out moves the row sum far beyond its bound whatever gamma and coef0."""
    base = R.feature_rows(max(m, n), d, 500 + m + n + d)
    return base[:m].copy(), (0.9 * base[:n] + 0.02).astype(np.float32)


def group_case(groups=3, m=129, n=127, d=64):
    """-> (probe f32 [G, m, d], ref f32 [G, n, d]): unrelated sets per group."""
    p = np.stack([R.feature_rows(m, d, 600 + g) for g in range(groups)])
    r = np.stack([(0.9 * R.feature_rows(n, d, 700 + g) + 0.03 * g).astype(np.float32) for g in range(groups)])
    return p, r


# ------------------------------------------------------------------------------------------------ the kernel's fp32 chain on the CPU
def chain_dots_f32(a, b):
    """The dot products [m, n] by the chain the header of metrics.hip states: per 32-wide chunk an fp32 fma chain from 0 in the order
    k, k+4, k+1, k+5, k+2, k+6, k+3, k+7 per 8 k, then the chunk sums added in ascending chunk order, in fp32.  An fma is emulated as the
    fp64 a * b + s (the product of two floats is exact in fp64) rounded to fp32: one extra rounding at 2^-53, far below the fp32 one."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = a.shape[1]
    tot = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for c in range(d // 32):
        s = np.zeros_like(tot)
        for q in range(4):
            for u in range(4):
                for k in (c * 32 + q * 8 + u, c * 32 + q * 8 + 4 + u):
                    s = (a[:, k].astype(np.float64)[:, None] * b[:, k].astype(np.float64)[None, :] + s.astype(np.float64)).astype(np.float32)
        tot = (tot + s).astype(np.float32)
    return tot
