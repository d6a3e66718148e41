"""CPU suite of the quality metrics: the host arithmetic of rdm_amd.metrics (Frechet distance, FeatureStats), the fp64 restatements the GPU
tests hold the kernels to (tests/_metrics_ref.py) against brute-force loops, scripts/rdm_eval.py's parser, and the three C-ABI symbols."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("rdm_op_moments_f64", "rdm_op_knn_radius", "rdm_op_manifold_hits")


def _metrics():
    import rdm_amd  # noqa: F401
    from rdm_amd import metrics
    return metrics


# ------------------------------------------------------------------------------------------------ Frechet distance
def _random_stats(d, seed, n=None):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((d, n or 2 * d))
    return R.GivenStats(rng.standard_normal(d), a @ a.T / a.shape[1])


def test_frechet_distance_of_identical_stats_is_zero():
    m = _metrics()
    s = _random_stats(24, 0)
    scale = np.trace(s.cov())
    assert abs(m.frechet_distance(s, s)) <= 1e-9 * scale
    # and of a singular covariance with itself: sqrt amplifies the eigenvalues' rounding (1e-16 |S|^2 -> 1e-8 |S| per null direction)
    lo = _random_stats(24, 1, n=5)
    assert abs(m.frechet_distance(lo, lo)) <= 1e-6 * np.trace(lo.cov())


def test_frechet_distance_diagonal_closed_form():
    m = _metrics()
    rng = np.random.default_rng(2)
    d = 40
    mu_a, mu_b = rng.standard_normal(d), rng.standard_normal(d)
    va, vb = rng.random(d) + 0.1, rng.random(d) * 3 + 0.1
    got = m.frechet_distance(R.GivenStats(mu_a, np.diag(va)), R.GivenStats(mu_b, np.diag(vb)))
    want = R.frechet_diagonal(mu_a, va, mu_b, vb)
    assert abs(got - want) <= 1e-10 * want
    # the same in a rotated basis: no longer diagonal, the same distance
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    rot = m.frechet_distance(R.GivenStats(q @ mu_a, q @ np.diag(va) @ q.T), R.GivenStats(q @ mu_b, q @ np.diag(vb) @ q.T))
    assert abs(rot - want) <= 1e-9 * want


def test_frechet_distance_is_symmetric():
    m = _metrics()
    a, b = _random_stats(32, 3), _random_stats(32, 4)
    ab, ba = m.frechet_distance(a, b), m.frechet_distance(b, a)
    assert ab > 0 and ab == ba


def test_frechet_distance_rank_deficient_covariance():
    """n < d samples of a low-rank Gaussian: the sample covariance F F^T is known by its factor F = Xc^T / sqrt(n - 1), and the distance
    follows from the factors alone (singular values of Fa^T Fb), with no d x d square root."""
    m = _metrics()
    rng = np.random.default_rng(5)
    d, r, n = 64, 6, 20
    xa = rng.standard_normal((n, r)) @ rng.standard_normal((r, d)) + rng.standard_normal(d)
    xb = rng.standard_normal((n, r)) @ rng.standard_normal((r, d)) * 1.5 + rng.standard_normal(d)
    sa, sb = R.NumpyStats(xa), R.NumpyStats(xb)
    assert np.linalg.matrix_rank(sa.cov()) <= r < d
    fa, fb = (xa - xa.mean(0)).T / np.sqrt(n - 1), (xb - xb.mean(0)).T / np.sqrt(n - 1)
    want = R.frechet_low_rank(xa.mean(0), fa, xb.mean(0), fb)
    got = m.frechet_distance(sa, sb)
    assert np.isfinite(got) and abs(got - want) <= 1e-6 * (np.trace(sa.cov()) + np.trace(sb.cov()))
    assert want > 0


# ------------------------------------------------------------------------------------------------ FeatureStats on a fake context
class _NumpyCtx:
    """Context stand-in: op_moments_f64 is the numpy restatement, accumulated in place like the kernel."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = 0

    def op_moments_f64(self, x, sum_, outer):
        assert sum_.dtype == torch.float64 and outer.dtype == torch.float64 and outer.shape == (x.shape[1], x.shape[1])
        s, o = R.moments(x.numpy())
        sum_ += torch.from_numpy(s); outer += torch.from_numpy(o)
        self.calls += 1


def test_feature_stats_chunked_updates_equal_one_update():
    m = _metrics()
    x = torch.from_numpy(R.feature_rows(97, 32, 6))
    whole, parts, ctx = m.FeatureStats(32), m.FeatureStats(32), _NumpyCtx()
    whole.update(ctx, x)
    for lo, hi in ((0, 1), (1, 50), (50, 50), (50, 97)):           # an empty batch in the stream is a no-op
        parts.update(ctx, x[lo:hi])
    assert whole.n == parts.n == 97 and ctx.calls == 4
    assert np.allclose(whole.mean(), parts.mean(), rtol=0, atol=1e-15)
    assert np.allclose(whole.cov(), parts.cov(), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        whole.update(ctx, x[:, :16])
    with pytest.raises(ValueError):
        m.FeatureStats(32).cov()


def test_feature_stats_cov_equals_numpy_cov():
    m = _metrics()
    x = R.feature_rows(60, 64, 7) + 3.0          # a mean well away from 0: the n mu mu^T subtraction has something to cancel
    st = m.FeatureStats(64).update(_NumpyCtx(), torch.from_numpy(x.astype(np.float32)))
    ref = R.NumpyStats(x.astype(np.float32))
    assert st.n == 60
    assert np.abs(st.mean() - ref.mean()).max() <= 1e-14
    assert np.abs(st.cov() - ref.cov()).max() <= 1e-12
    assert np.array_equal(st.cov(), st.cov().T)
    assert abs(m.frechet_distance(st, ref)) <= 1e-6 * np.trace(ref.cov())


# ------------------------------------------------------------------------------------------------ the restatements against loops
def test_reference_restatements_against_brute_force_loops():
    rng = np.random.default_rng(8)
    n, mp, d, k = 12, 7, 5, 3
    x = rng.standard_normal((n, d)); x[9] = x[2]                   # one duplicate pair
    probe = rng.standard_normal((mp, d)) * 1.6
    d2 = np.zeros((n, n)); s = np.zeros(d); outer = np.zeros((d, d))
    for i in range(n):
        for a in range(d):
            s[a] += x[i, a]
            for b in range(d):
                outer[a, b] += x[i, a] * x[i, b]
        for j in range(n):
            for a in range(d):
                d2[i, j] += (x[i, a] - x[j, a]) ** 2
    rs, ro = R.moments(x)
    assert np.allclose(rs, s, rtol=0, atol=1e-13) and np.allclose(ro, outer, rtol=0, atol=1e-13)
    assert np.allclose(R.d2_matrix(x, x), d2, rtol=0, atol=1e-13)
    rad = np.array([sorted(d2[i, j] for j in range(n) if j != i)[k - 1] for i in range(n)])
    assert np.allclose(R.knn_radius2(x, k), rad, rtol=0, atol=1e-13)
    assert R.knn_radius2(x, 1)[2] == 0.0 and R.knn_radius2(x, 1)[9] == 0.0          # the duplicate is a neighbour, self is not
    assert np.allclose(R.knn_radius2(x, k, include_self=True), np.sort(d2, 1)[:, k - 1], rtol=0, atol=1e-13)
    assert (R.knn_radius2(x, 1, include_self=True) == 0).all()
    hits = []
    for i in range(mp):
        hit = False
        for j in range(n):
            hit |= sum((probe[i, a] - x[j, a]) ** 2 for a in range(d)) <= rad[j]
        hits.append(hit)
    assert 0 < sum(hits) < mp
    assert R.manifold_hits(probe, x, rad).tolist() == hits
    p, r = R.precision_recall(x, probe, k)
    assert p == sum(hits) / mp and 0.0 <= r <= 1.0
    assert R.precision_recall(x, x, k) == (1.0, 1.0)


def test_hit_inputs_leave_no_pair_inside_the_margin():
    """The seeded inputs of the GPU hit tests, judged without a GPU: no pair within 2 x the kernel's bound of its radius, about half of the
    probes hit, and the two near misses (radii permuted, one largest radius for all) give another answer."""
    for (n, d), seed in R.HIT_SEEDS.items():
        probe, ref, r2 = R.hits_case(130, n, d, seed)
        d2 = R.d2_matrix(probe, ref)
        ok, share = R.hit_margin_ok(probe, ref, r2, d2)
        assert ok and share == 0.0, (n, d, share)
        hit = R.manifold_hits(probe, ref, r2, d2)
        perm = np.random.default_rng(1).permutation(n)              # the permutation tests/test_gpu_metrics.py uses
        for m in (77, 130):
            assert 0.1 < hit[:m].mean() < 0.9
            assert not np.array_equal(R.manifold_hits(probe, ref, r2[perm], d2)[:m], hit[:m])
            assert not np.array_equal(R.manifold_hits(probe, ref, np.full_like(r2, r2.max()), d2)[:m], hit[:m])
        assert hit.any() and not hit.all()


# ------------------------------------------------------------------------------------------------ script and symbols
def _load_script():
    spec = importlib.util.spec_from_file_location("rdm_eval_script", os.path.join(ROOT, "scripts", "rdm_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rdm_eval_parser(tmp_path, capsys):
    mod = _load_script()
    opt = mod.parse_args(["--real", "a", "--fake", "b", "--synthetic"])
    assert (str(opt.real), str(opt.fake), opt.k, opt.gpu, opt.synthetic, opt.clip_ckpt, opt.normalize) == ("a", "b", 3, 0, True, None, False)
    opt = mod.parse_args(["--real", "a", "--fake", "b", "--clip_ckpt", "w.pt", "--gpu", "2", "--k", "5", "--normalize"])
    assert (str(opt.clip_ckpt), opt.gpu, opt.k, opt.normalize, opt.synthetic) == ("w.pt", 2, 5, True, False)
    for bad in (["--real", "a", "--fake", "b"],                                    # neither weights nor --synthetic
                ["--real", "a", "--synthetic"],                                    # --fake missing
                ["--real", "a", "--fake", "b", "--synthetic", "--k", "0"],
                ["--real", "a", "--fake", "b", "--synthetic", "--k", "9"],
                ["--real", "a", "--fake", "b", "--synthetic", "--gpu", "-1"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    capsys.readouterr()
    # the folder reader: sorted, images only, [-1, 1], a new batch where the size changes
    from PIL import Image
    for name, size, v in (("b.png", (8, 8), 255), ("a.png", (8, 8), 0), ("c.png", (4, 4), 255), ("notes.txt", None, 0)):
        if size is None:
            (tmp_path / name).write_text("x")
        else:
            Image.fromarray(np.full(size + (3,), v, np.uint8)).save(tmp_path / name)
    paths = mod.list_images(tmp_path)
    assert [p.name for p in paths] == ["a.png", "b.png", "c.png"]
    batches = list(mod.image_batches(paths, 8))
    assert [tuple(b.shape) for b in batches] == [(2, 3, 8, 8), (1, 3, 4, 4)]
    assert float(batches[0][0].max()) == -1.0 and float(batches[0][1].min()) == 1.0
    (tmp_path / "empty").mkdir()
    with pytest.raises(SystemExit):
        mod.list_images(tmp_path / "empty")


def test_metric_symbols_in_header_signature_table_and_binding():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    src = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for op, nargs in zip(OPS, (6, 6, 8)):
        assert re.search(r"\bint\s+%s\s*\(" % op, decl), op
        assert len(_lib.SIGNATURES[op][1]) == nargs
        assert hasattr(_lib.lib, op)
    for method in ("op_moments_f64", "op_knn_radius", "op_manifold_hits"):
        assert callable(getattr(_lib.Context, method))
    # each C entry's header comment names the paper formula it implements
    assert "Heusel" in src and "Kynkaanniemi" in src


def test_precision_recall_inputs_keep_the_margin():
    real, gen = R.pr_clouds()
    assert real.shape == (300, 64) and gen.shape == (200, 64)
    assert R.pr_margin_ok(real, gen, 3)
    p, r = R.precision_recall(real, gen, 3)
    assert 0.0 < r < p < 1.0
