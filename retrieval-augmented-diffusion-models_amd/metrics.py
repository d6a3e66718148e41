"""Quality metrics on feature sets: Frechet distance (Heusel et al. 2017) and improved precision / recall (Kynkaanniemi et al. 2019),
on CLIP ViT-B/32 image features -- what the reference's model zoo reports for its FFHQ checkpoint ("using CLIP as feature extractor
instead of Inception") -- and, for the sets those are weak on, KID (Binkowski et al. 2018: unbiased at any set size) and density /
coverage (Naeem et al. 2020: no saturation at 1, no inflation by outliers).

The work that scales with the set runs in the library (csrc/metrics.hip): fp64 moments, k-NN radii, manifold membership and counts,
nearest distances and cubic-kernel row sums, streamed, nothing of size n x n stored.  What is left is d x d host arithmetic in fp64 numpy: the covariance from the moments and one symmetric
eigendecomposition pair for the Frechet distance.  No scipy.
"""
import numpy as np
import torch


class FeatureStats:
    """Running first and second moments of a stream of feature batches [b, d], held in fp64 on the device of the first batch's
    context.  `update` folds a batch in (Context.op_moments_f64); `mean` and `cov` (unbiased, n - 1) return host fp64 arrays."""

    def __init__(self, d):
        self.d = int(d)
        self.n = 0
        self._sum = None
        self._outer = None

    def update(self, ctx, feats):
        if feats.ndim != 2 or feats.shape[1] != self.d:
            raise ValueError(f"FeatureStats.update: features must be [b, {self.d}], got {tuple(feats.shape)}")
        if feats.shape[0] == 0:
            return self
        if self._sum is None:
            self._sum = torch.zeros((self.d,), device=ctx.device, dtype=torch.float64)
            self._outer = torch.zeros((self.d, self.d), device=ctx.device, dtype=torch.float64)
        ctx.op_moments_f64(feats, self._sum, self._outer)
        self.n += int(feats.shape[0])
        return self

    def _host(self, t):
        return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)

    def mean(self):
        if self.n < 1:
            raise ValueError("FeatureStats.mean: no features yet")
        return self._host(self._sum) / self.n

    def cov(self):
        """(SUM x x^T - n mu mu^T) / (n - 1), symmetrised.  The subtraction cancels when |mu|^2 dwarfs the variances: at fp64 that
        takes a mean ~1e7 standard deviations out, far from any feature extractor's output."""
        if self.n < 2:
            raise ValueError("FeatureStats.cov: the unbiased covariance needs at least two rows")
        mu = self.mean()
        c = (self._host(self._outer) - self.n * np.outer(mu, mu)) / (self.n - 1)
        return 0.5 * (c + c.T)


def _sqrtm_psd(a):
    """Symmetric square root of a symmetric positive semi-definite matrix; eigenvalues below 0 (rounding) are taken as 0."""
    w, v = np.linalg.eigh(a)
    return (v * np.sqrt(np.maximum(w, 0.0))) @ v.T


def frechet_distance(stats_a, stats_b):
    """|mu_a - mu_b|^2 + Tr S_a + Tr S_b - 2 Tr (S_a S_b)^1/2, with Tr (S_a S_b)^1/2 = SUM_i sqrt(max(lambda_i, 0)) over the eigenvalues of
    the symmetric S_a^1/2 S_b S_a^1/2 (similar to S_a S_b): two `eigh` calls, and a singular covariance (fewer rows than dimensions) is
    harmless where a general matrix square root is not.  stats_*: anything with `.mean()` and `.cov()` (FeatureStats).  Host fp64."""
    mu_a, mu_b = np.asarray(stats_a.mean(), np.float64), np.asarray(stats_b.mean(), np.float64)
    s_a, s_b = np.asarray(stats_a.cov(), np.float64), np.asarray(stats_b.cov(), np.float64)
    if mu_a.shape != mu_b.shape or s_a.shape != s_b.shape:
        raise ValueError(f"frechet_distance: the two sets differ in width ({mu_a.shape[0]} and {mu_b.shape[0]})")
    # the symmetric form is not symmetric in (a, b) to rounding; put the argument order out of the result
    def cross(p, q):
        r = _sqrtm_psd(p)
        m = r @ q @ r
        return float(np.sqrt(np.maximum(np.linalg.eigvalsh(0.5 * (m + m.T)), 0.0)).sum())
    tr = 0.5 * (cross(s_a, s_b) + cross(s_b, s_a))
    diff = mu_a - mu_b
    return max(float(diff @ diff + np.trace(s_a) + np.trace(s_b) - 2.0 * tr), 0.0)         # >= 0 but for rounding


def precision_recall(ctx, feats_real, feats_gen, k=3, center=True):
    """Improved precision and recall (Kynkaanniemi et al. 2019): precision = share of generated rows inside the k-NN ball of some real
    row, recall = share of real rows inside the k-NN ball of some generated row.  Two Context.op_knn_radius and two
    Context.op_manifold_hits calls.  -> (precision, recall) as Python floats.

    center: both sets are first shifted by ONE common vector, the fp32 mean of the real set.  Euclidean distances are translation
    invariant, and the kernels' error bound, 5e-7 (|a|^2 + |b|^2), shrinks with the norms: CLIP features share a large common
    component.  The shift itself rounds each coordinate once (fp32); center=False hands the rows to the kernels as given."""
    real = ctx._features("precision_recall", feats_real, "feats_real")
    gen = ctx._features("precision_recall", feats_gen, "feats_gen")
    if real.shape[1] != gen.shape[1]:
        raise ValueError(f"precision_recall: the two sets differ in width ({real.shape[1]} and {gen.shape[1]})")
    if center:
        mu = real.mean(dim=0, keepdim=True)
        real, gen = (real - mu).contiguous(), (gen - mu).contiguous()
    r_real, r_gen = ctx.op_knn_radius(real, k), ctx.op_knn_radius(gen, k)
    precision = int(ctx.op_manifold_hits(gen, real, r_real).sum()) / gen.shape[0]
    recall = int(ctx.op_manifold_hits(real, gen, r_gen).sum()) / real.shape[0]
    return precision, recall


def density_coverage(ctx, feats_real, feats_gen, k=5, center=True):
    """Density and coverage (Naeem et al. 2020).  density = 1 / (k n_gen) SUM over generated rows of the number of real rows' k-NN balls
    the row lies in: it counts where precision ORs, so it does not saturate at 1 (it EXCEEDS 1 where the generated rows crowd the dense
    part of the real set).  coverage = share of real rows whose k-NN ball holds at least one generated row: only the real set's balls
    are used, so a generated outlier cannot inflate it as it inflates recall.  One Context.op_knn_radius, one op_manifold_counts and one
    op_nearest_d2 call.  -> (density, coverage) as Python floats.  center: as in `precision_recall`."""
    real = ctx._features("density_coverage", feats_real, "feats_real")
    gen = ctx._features("density_coverage", feats_gen, "feats_gen")
    if real.shape[1] != gen.shape[1]:
        raise ValueError(f"density_coverage: the two sets differ in width ({real.shape[1]} and {gen.shape[1]})")
    if center:
        mu = real.mean(dim=0, keepdim=True)
        real, gen = (real - mu).contiguous(), (gen - mu).contiguous()
    r_real = ctx.op_knn_radius(real, k)
    density = int(ctx.op_manifold_counts(gen, real, r_real).sum(dtype=torch.int64)) / (k * gen.shape[0])
    coverage = int((ctx.op_nearest_d2(real, gen) <= r_real).sum()) / real.shape[0]
    return density, coverage


KID_GATHER_BYTES = 512 << 20          # most bytes the two gathered subset tensors of one kernel_distance chunk may take together


def kernel_distance(ctx, feats_real, feats_gen, subsets=100, subset_size=1000, seed=0, gamma=None, coef0=1.0):
    """Kernel Inception Distance (Binkowski et al. 2018) on whatever features are given: the unbiased MMD^2 under the kernel
    k(x, y) = (gamma x.y + coef0)^3, gamma=None meaning 1 / d, over `subsets` subsets of s = min(subset_size, n_real, n_gen) rows each.
    -> (mean, population std over the subsets) as Python floats.  Per subset:
        SUM_{i != j} k(x_i, x_j) / (s (s - 1)) + SUM_{i != j} k(y_i, y_j) / (s (s - 1)) - 2 SUM_{i, j} k(x_i, y_j) / s^2.
    Unlike the Frechet distance its expectation does not depend on the row count, so it is the one to read on small sets.

    Subsets: rng = numpy.random.default_rng(seed); for each subset in order rng.choice(n_real, s, replace=False), then
    rng.choice(n_gen, s, replace=False).  The rows are gathered to [G, s, d] in chunks of G subsets, the two gathered tensors of a chunk
    together bounded by KID_GATHER_BYTES = 512 MiB (the default 100 x 1000 x 512 is one chunk of 391 MiB; a single subset is never split),
    and each chunk takes three Context.op_poly3_rowsums calls (XX and YY without the diagonal, XY with it), one block row per subset.
    The row sums (fp64, dot products in fp32) are reduced on the host in fp64.  gamma and coef0 reach the kernel as fp32.

    subsets=0: ONE estimate on the whole sets (n_real and n_gen may differ), std 0.0.  Fewer than two rows a side: ValueError."""
    real = ctx._features("kernel_distance", feats_real, "feats_real")
    gen = ctx._features("kernel_distance", feats_gen, "feats_gen")
    if real.shape[1] != gen.shape[1]:
        raise ValueError(f"kernel_distance: the two sets differ in width ({real.shape[1]} and {gen.shape[1]})")
    (n_real, d), n_gen = real.shape, gen.shape[0]
    gamma = 1.0 / d if gamma is None else float(gamma)
    subsets = int(subsets)
    if subsets < 0:
        raise ValueError(f"kernel_distance: subsets = {subsets}; 0 (the whole sets) or more")

    def estimate(x, y):
        """x [G, m, d], y [G, n, d] -> fp64 numpy [G]"""
        m, n = x.shape[1], y.shape[1]
        xx = ctx.op_poly3_rowsums(x, x, gamma, coef0, exclude_same_index=True).cpu().numpy().sum(axis=1)
        yy = ctx.op_poly3_rowsums(y, y, gamma, coef0, exclude_same_index=True).cpu().numpy().sum(axis=1)
        xy = ctx.op_poly3_rowsums(x, y, gamma, coef0, exclude_same_index=False).cpu().numpy().sum(axis=1)
        return xx / (m * (m - 1.0)) + yy / (n * (n - 1.0)) - 2.0 * xy / (float(m) * n)

    if subsets == 0:
        if min(n_real, n_gen) < 2:
            raise ValueError(f"kernel_distance: n_real = {n_real}, n_gen = {n_gen}; the unbiased estimate needs two rows a side")
        return float(estimate(real[None], gen[None])[0]), 0.0
    s = min(int(subset_size), n_real, n_gen)
    if s < 2:
        raise ValueError(f"kernel_distance: subsets of s = {s} rows (subset_size {subset_size}, n_real {n_real}, n_gen {n_gen}); the unbiased "
                         f"estimate needs two")
    rng = np.random.default_rng(seed)
    idx = [(rng.choice(n_real, s, replace=False), rng.choice(n_gen, s, replace=False)) for _ in range(subsets)]
    per = max(1, KID_GATHER_BYTES // (2 * s * d * 4))
    vals = []
    for lo in range(0, subsets, per):
        chunk = idx[lo:lo + per]
        ix = torch.from_numpy(np.concatenate([c[0] for c in chunk])).to(ctx.device)
        iy = torch.from_numpy(np.concatenate([c[1] for c in chunk])).to(ctx.device)
        vals.append(estimate(real.index_select(0, ix).view(len(chunk), s, d), gen.index_select(0, iy).view(len(chunk), s, d)))
    vals = np.concatenate(vals)
    return float(vals.mean()), float(vals.std())


def clip_features(retriever, images, batch=64, normalize=False):
    """images f32 [B, 3, H, W] in [-1, 1] -> f32 [B, embed_dim] on the retriever's device: the CLIP image tower's pooled, projected
    embedding through ClipImageRetriever.forward (bicubic preprocess fused in), `batch` images at a time.

    The embedding is UN-normalised by default.  That is this project's choice: the reference reports "CLIP as feature extractor instead
    of Inception" for its FFHQ numbers and does not say which it used, so its figures are not comparable to ours digit for digit.
    normalize=True divides each row by its Euclidean norm (the cosine geometry CLIP was trained in)."""
    if images.ndim != 4 or images.shape[1] != 3:
        raise ValueError(f"clip_features: images must be [B, 3, H, W], got {tuple(images.shape)}")
    out = [retriever.forward(images[i:i + batch]) for i in range(0, images.shape[0], max(int(batch), 1))]
    feats = torch.cat(out, dim=0)
    if normalize:
        feats = feats / feats.norm(dim=1, keepdim=True)
    return feats


EVALUATE_EXTRAS = ("kid", "density_coverage")


def evaluate(model, real_images_iter, gen_images_iter, k=3, batch=64, normalize=False, extra=(), kid_subsets=100, kid_subset_size=1000,
             kid_seed=0, dc_k=5):
    """model: a ClipImageRetriever.  The two iterables yield image batches [b, 3, H, W] in [-1, 1] (a single tensor counts as one batch).
    -> {"fid", "precision", "recall", "n_real", "n_gen"}.  The moments are folded in batch by batch; the features themselves ([n, 512]
    f32) are kept on the device for the neighbour searches.

    extra: any of "kid" (adds "kid" and "kid_std": kernel_distance with kid_subsets, kid_subset_size, kid_seed) and "density_coverage"
    (adds "density" and "coverage": density_coverage at k = dc_k).  With the default extra=() the dict has the five keys above."""
    extra = (extra,) if isinstance(extra, str) else tuple(extra)
    unknown = [e for e in extra if e not in EVALUATE_EXTRAS]
    if unknown:
        raise ValueError(f"evaluate: extra holds {unknown}; known: {EVALUATE_EXTRAS}")
    ctx = model.model.ctx
    sets = []
    for it in (real_images_iter, gen_images_iter):
        if isinstance(it, torch.Tensor):
            it = (it,)
        stats, feats = None, []
        for imgs in it:
            f = clip_features(model, imgs, batch=batch, normalize=normalize)
            stats = stats if stats is not None else FeatureStats(f.shape[1])
            stats.update(ctx, f)
            feats.append(f)
        if stats is None:
            raise ValueError("evaluate: an image set is empty")
        sets.append((stats, torch.cat(feats, dim=0)))
    (s_real, f_real), (s_gen, f_gen) = sets
    precision, recall = precision_recall(ctx, f_real, f_gen, k=k)
    res = {"fid": frechet_distance(s_real, s_gen), "precision": precision, "recall": recall, "n_real": s_real.n, "n_gen": s_gen.n}
    if "kid" in extra:
        res["kid"], res["kid_std"] = kernel_distance(ctx, f_real, f_gen, subsets=kid_subsets, subset_size=kid_subset_size, seed=kid_seed)
    if "density_coverage" in extra:
        res["density"], res["coverage"] = density_coverage(ctx, f_real, f_gen, k=dc_k)
    return res
