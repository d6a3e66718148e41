"""Quality metrics on feature sets: Frechet distance (Heusel et al. 2017) and improved precision / recall (Kynkaanniemi et al. 2019),
on CLIP ViT-B/32 image features -- what the reference's model zoo reports for its FFHQ checkpoint ("using CLIP as feature extractor
instead of Inception").

The work that scales with the set runs in the library (csrc/metrics.hip): fp64 moments, k-NN radii and manifold membership, streamed,
nothing of size n x n stored.  What is left is d x d host arithmetic in fp64 numpy: the covariance from the moments and one symmetric
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


def evaluate(model, real_images_iter, gen_images_iter, k=3, batch=64, normalize=False):
    """model: a ClipImageRetriever.  The two iterables yield image batches [b, 3, H, W] in [-1, 1] (a single tensor counts as one batch).
    -> {"fid", "precision", "recall", "n_real", "n_gen"}.  The moments are folded in batch by batch; the features themselves ([n, 512]
    f32) are kept on the device for the two neighbour searches."""
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
    return {"fid": frechet_distance(s_real, s_gen), "precision": precision, "recall": recall, "n_real": s_real.n, "n_gen": s_gen.n}
