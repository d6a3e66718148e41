"""Float64 numpy restatements of the metric kernels (csrc/metrics.hip) and of rdm_amd.metrics, the bounds the GPU tests hold the kernels
to, and the seeded input sets those tests share.  tests/test_metrics_cpu.py checks these restatements against brute-force loops.

Bounds.
  moments:  every entry of SUM_i x_ia x_ib within  n 2^-52 SUM_i |x_ia x_ib|  (a float product is exact in fp64, so only the n adds round,
            2^-53 relative each, on either side of the comparison); the sum vector likewise with |x_ia|.
  d2:       |d2_kernel - d2_fp64| <= D2_GAMMA (|a|^2 + |b|^2),  D2_GAMMA = 5e-7: three fp32 fma chains (two norms, one dot product, ~1.5e-7
            of the sum of their terms' magnitudes each for d <= 1024) and the final adds.
  radius2:  the k-th smallest of n - 1 values moves by at most the largest change of any of them, so a radius is held to D2_GAMMA times
            the largest |a|^2 + |b|^2 of the set, whichever pair the kernel picked.
"""
import numpy as np

D2_GAMMA = 5e-7


# ------------------------------------------------------------------------------------------------ moments
def moments(x):
    """-> (sum [d], outer [d, d]) of x [n, d] in fp64."""
    x = np.asarray(x, np.float64)
    return x.sum(0), x.T @ x


def moments_bound(x, n_roundings=None):
    """-> (bound of sum [d], bound of outer [d, d]); n_roundings: adds that round (default: the row count)."""
    x = np.abs(np.asarray(x, np.float64))
    n = x.shape[0] if n_roundings is None else n_roundings
    return n * 2.0 ** -52 * x.sum(0), n * 2.0 ** -52 * (x.T @ x)


class NumpyStats:
    """mean / unbiased covariance of a whole set at once (numpy.cov): what FeatureStats must reproduce from its running moments."""

    def __init__(self, x):
        self.x = np.asarray(x, np.float64)
        self.n = self.x.shape[0]

    def mean(self):
        return self.x.mean(0)

    def cov(self):
        return np.cov(self.x, rowvar=False)


class GivenStats:
    def __init__(self, mu, sigma):
        self.mu, self.sigma = np.asarray(mu, np.float64), np.asarray(sigma, np.float64)

    def mean(self):
        return self.mu

    def cov(self):
        return self.sigma


# ------------------------------------------------------------------------------------------------ distances
def sqnorms(x):
    x = np.asarray(x, np.float64)
    return (x * x).sum(1)


def d2_matrix(a, b):
    """Squared Euclidean distances [m, n] in fp64, by differences (no cancellation), row block by row block."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(0, a.shape[0], 32):
        diff = a[i:i + 32, None, :] - b[None, :, :]
        out[i:i + 32] = (diff * diff).sum(2)
    return out


def d2_bound_matrix(a, b):
    return D2_GAMMA * (sqnorms(a)[:, None] + sqnorms(b)[None, :])


def knn_radius2(x, k, include_self=False, d2=None):
    """radius2 [n] in fp64: distance^2 to the k-th nearest other row (self left out by INDEX); include_self: the near miss that counts a row
    as its own nearest neighbour."""
    d2 = d2_matrix(x, x) if d2 is None else d2.copy()
    if not include_self:
        d2[np.arange(d2.shape[0]), np.arange(d2.shape[0])] = np.inf
    return np.sort(d2, axis=1)[:, k - 1]


def radius_bound(x):
    """D2_GAMMA (|a|^2 + |b|^2) at the pair of rows with the largest norms."""
    n2 = np.sort(sqnorms(x))
    return D2_GAMMA * (n2[-1] + n2[-2]) if n2.shape[0] > 1 else D2_GAMMA * 2 * n2[-1]


def manifold_hits(probe, ref, ref_radius2, d2=None):
    """hit [m] bool: some j with d2(probe_i, ref_j) <= ref_radius2[j]."""
    d2 = d2_matrix(probe, ref) if d2 is None else d2
    return (d2 <= np.asarray(ref_radius2, np.float64)[None, :]).any(1)


def hit_margin_ok(probe, ref, ref_radius2, d2=None):
    """The condition under which a kernel within the d2 bound must reproduce `manifold_hits` exactly: every pair has
    |d2 - r2_j| > 2 D2_GAMMA (|a|^2 + |b|^2).  -> (all pairs satisfy it, share of pairs that do not)."""
    d2 = d2_matrix(probe, ref) if d2 is None else d2
    gap = np.abs(d2 - np.asarray(ref_radius2, np.float64)[None, :])
    bad = gap <= 2 * d2_bound_matrix(probe, ref)
    return not bool(bad.any()), float(bad.mean())


def precision_recall(real, gen, k):
    """Kynkaanniemi et al.: (share of gen rows in some real row's k-NN ball, share of real rows in some gen row's k-NN ball)."""
    r_real, r_gen = knn_radius2(real, k), knn_radius2(gen, k)
    return float(manifold_hits(gen, real, r_real).mean()), float(manifold_hits(real, gen, r_gen).mean())


# ------------------------------------------------------------------------------------------------ Frechet distance
def frechet_diagonal(mu_a, var_a, mu_b, var_b):
    """Closed form for diagonal covariances: |mu_a - mu_b|^2 + SUM (sqrt a_i - sqrt b_i)^2."""
    mu_a, var_a, mu_b, var_b = (np.asarray(v, np.float64) for v in (mu_a, var_a, mu_b, var_b))
    return float(((mu_a - mu_b) ** 2).sum() + ((np.sqrt(var_a) - np.sqrt(var_b)) ** 2).sum())


def frechet_low_rank(mu_a, fa, mu_b, fb):
    """Frechet distance of N(mu_a, Fa Fa^T) and N(mu_b, Fb Fb^T) from the FACTORS (d x r, r << d): Tr (Sa Sb)^1/2 = SUM of the singular
    values of Fa^T Fb (the non-zero eigenvalues of Sa Sb are those of (Fa^T Fb)(Fa^T Fb)^T), never forming a d x d square root."""
    mu_a, fa, mu_b, fb = (np.asarray(v, np.float64) for v in (mu_a, fa, mu_b, fb))
    cross = np.linalg.svd(fa.T @ fb, compute_uv=False).sum()
    return float(((mu_a - mu_b) ** 2).sum() + (fa * fa).sum() + (fb * fb).sum() - 2.0 * cross)


# ------------------------------------------------------------------------------------------------ the GPU tests' seeded inputs
def feature_rows(n, d, seed, spread=0.5):
    """Rows with norms that differ (a per-row scale in [1 - spread, 1 + spread]) around a common offset, as float32."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) * (1.0 + spread * (2.0 * rng.random((n, 1)) - 1.0)) + 0.25 * rng.standard_normal((1, d))
    return (x / np.sqrt(d)).astype(np.float32)


# (n, d) -> seed of the hit tests' inputs, picked so that NO pair lies inside the margin of hit_margin_ok (tests/test_metrics_cpu.py re-checks)
HIT_SEEDS = {(127, 32): 200, (129, 32): 201, (127, 512): 202, (129, 512): 203}


def hits_case(m, n, d, seed, k=3):
    """-> (probe f32 [m, d], ref f32 [n, d], ref_radius2 f32 [n]): the ref rows' k-NN radii, all scaled by ONE factor such that half of
    the case's 130-row parent probe set hits; smaller m take the first rows of that parent set.  Probe i hits from the factor
    rho_i = min_j d2_ij / r2_j on; the factor is the midpoint of the widest gap among the middle ten of the sorted rho."""
    ref = feature_rows(n, d, seed)
    parent = feature_rows(130, d, seed + 1000)
    r2 = knn_radius2(ref, k)
    rho = np.sort((d2_matrix(parent, ref) / r2[None, :]).min(1))
    i = 60 + int(np.argmax(np.diff(rho[60:71])))
    return parent[:m].copy(), ref, (0.5 * (rho[i] + rho[i + 1]) * r2).astype(np.float32)


PR_SEED = 32          # picked so that pr_margin_ok holds (tests/test_metrics_cpu.py re-checks)


def pr_clouds(seed=PR_SEED, n=300, m=200, d=64):
    """Two Gaussian clouds (real [n, d], gen [m, d], float32): the generated one is shifted and narrower, so neither number is 0 or 1."""
    rng = np.random.default_rng(seed)
    real = rng.standard_normal((n, d)) / np.sqrt(d)
    gen = (0.85 * rng.standard_normal((m, d)) + 0.35 * rng.standard_normal((1, d))) / np.sqrt(d)
    return real.astype(np.float32), gen.astype(np.float32)


def pr_margin_ok(real, gen, k):
    """precision_recall composes two kernels: a hit compares a distance (within the d2 bound) with a RADIUS that is itself a kernel result
    (within radius_bound of its set).  Exact agreement with the fp64 restatement follows when every pair keeps
    |d2 - r2_j| > D2_GAMMA (|a|^2 + |b|^2) + radius_bound(ref set), and the margin of hit_margin_ok (2 D2_GAMMA (|a|^2 + |b|^2)) as well."""
    ok = True
    for probe, ref in ((gen, real), (real, gen)):
        r2 = knn_radius2(ref, k)
        d2 = d2_matrix(probe, ref)
        gap = np.abs(d2 - r2[None, :])
        ok &= bool((gap > np.maximum(2 * d2_bound_matrix(probe, ref), d2_bound_matrix(probe, ref) + radius_bound(ref))).all())
    return ok
