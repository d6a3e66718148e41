"""GPU suite of the quality metrics (csrc/metrics.hip through Context.op_moments_f64 / op_knn_radius / op_manifold_hits, and
rdm_amd.metrics on top) against the fp64 restatements of tests/_metrics_ref.py.

Bounds (derived in tests/_metrics_ref.py):
  moments   every entry within n 2^-52 SUM_i |x_ia x_ib| of fp64 numpy.
  radius2   within D2_GAMMA (|a|^2 + |b|^2) = 5e-7 (...) of the fp64 radius, the bound taken at the two largest norms of the set.
            Measured on an MI355X: the largest radius error over all cases below is 1.27e-7 of that figure (n = 257, d = 32, k = 1; each
            case prints its own).  The bound is not tightened: that ratio divides by the LARGEST norms of the set, and per pair the CPU
            emulation of the same fma chains reaches 3.6e-7 (|a|^2 + |b|^2) (d = 32, all 257^2 pairs), 1.4x under the bound.
  hits      equal to the fp64 answer, on inputs whose every pair keeps |d2 - r2_j| > 2 D2_GAMMA (|a|^2 + |b|^2) (asserted first).
The hit rate of a case must lie strictly inside (0.1, 0.9).  One probe (m = 1) has a rate of 0 or 1 whatever the kernel does, so that
case is judged on the 130-row parent set its probe is the first row of (same ref set, same radii), and run once more on a probe the
reference says hits and on one it says misses."""
import numpy as np
import pytest
import torch

from oracle import clip as oclip
from oracle import unet as ounet

import _metrics_ref as R
from _util import spec_to_clip_cfg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------------------------------------ moments
def _moments(ctx, x, chunks=None):
    d = x.shape[1]
    s = torch.zeros((d,), device=ctx.device, dtype=torch.float64)
    o = torch.zeros((d, d), device=ctx.device, dtype=torch.float64)
    lo = 0
    for c in chunks or (x.shape[0],):
        ctx.op_moments_f64(_t(x[lo:lo + c]), s, o)
        lo += c
    assert lo == x.shape[0]
    return s.cpu().numpy(), o.cpu().numpy()


@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_moments_against_fp64(ctx, n, d):
    x = R.feature_rows(n, d, 40 + n)
    rs, ro = R.moments(x)
    bs, bo = R.moments_bound(x)
    s, o = _moments(ctx, x)
    es, eo = np.abs(s - rs), np.abs(o - ro)
    print(f"[metrics] moments n={n} d={d}: sum error / bound {float((es / np.maximum(bs, 1e-300)).max()):.3g}, "
          f"outer error / bound {float((eo / np.maximum(bo, 1e-300)).max()):.3g}")
    assert (es <= bs).all() and (eo <= bo).all()
    assert np.array_equal(o, o.T)                                  # both triangles sum the same products in the same order
    if n >= 3:
        # three uneven chunks: the same bound (each partial sum rounds no more often than the whole)
        a = max(1, n // 7)
        s3, o3 = _moments(ctx, x, (a, n - a - 1, 1))
        assert (np.abs(s3 - rs) <= bs).all() and (np.abs(o3 - ro) <= bo).all()
    # a second call accumulates: the moments of the set taken twice, to that set's bound
    s2 = _t(s).to(ctx.device); o2 = _t(o).to(ctx.device)
    ctx.op_moments_f64(_t(x), s2, o2)
    xx = np.concatenate([x, x])
    (r2s, r2o), (b2s, b2o) = R.moments(xx), R.moments_bound(xx)
    assert (np.abs(s2.cpu().numpy() - r2s) <= b2s).all() and (np.abs(o2.cpu().numpy() - r2o) <= b2o).all()
    assert np.abs(o2.cpu().numpy() - ro).max() > bo.max()          # ... and did not overwrite


# ------------------------------------------------------------------------------------------------ radius
def _radius_rows(n, d, k):
    """Seeded rows with, from n >= 16 on, one exact duplicate pair (rows 3, n - 2) and one row present k + 1 times (rows 5, 6 + i)."""
    x = R.feature_rows(n, d, 7 * n + d)
    dup, rep = [], []
    if n >= 16:
        x[n - 2] = x[3]; dup = [3, n - 2]
        rep = [5] + [6 + i for i in range(k)]
        x[rep[1:]] = x[5]
    return x, dup, rep


RADIUS_CASES = [(n, d, k) for n in (2, 127, 128, 129, 257) for d in (32, 512) for k in (1, 3, 8) if k < n]
_radius_worst = {"ratio": 0.0}


@pytest.mark.parametrize("n,d,k", RADIUS_CASES)
def test_knn_radius_against_fp64(ctx, n, d, k):
    x, dup, rep = _radius_rows(n, d, k)
    got = ctx.op_knn_radius(_t(x), k).cpu().numpy().astype(np.float64)
    d2 = R.d2_matrix(x, x)
    ref = R.knn_radius2(x, k, d2=d2)
    tol = R.radius_bound(x)
    err = np.abs(got - ref)
    n2 = np.sort(R.sqnorms(x))
    ratio = float(err.max() / (n2[-1] + n2[-2]))
    _radius_worst["ratio"] = max(_radius_worst["ratio"], ratio)
    print(f"[metrics] radius n={n} d={d} k={k}: max |r2 - fp64| = {ratio:.3e} (|a|^2 + |b|^2) (bound {R.D2_GAMMA:.1e}); "
          f"worst so far {_radius_worst['ratio']:.3e}")
    assert got.shape == (n,) and (got >= 0).all() and (err <= tol).all()
    if dup and k == 1:
        assert got[dup[0]] == 0.0 and got[dup[1]] == 0.0          # exactly 0: the norms and the dot product are one chain
    if rep:
        assert (got[rep] == 0.0).all()                             # k other copies at distance exactly 0
        assert (ref[rep] == 0.0).all()
    # near misses: each must leave the bound on at least one row
    misses = {"self included": R.knn_radius2(x, k, include_self=True, d2=d2)}
    if k >= 2:
        misses["(k-1)-th neighbour"] = R.knn_radius2(x, k - 1, d2=d2)
    if k + 1 <= n - 1:
        misses["(k+1)-th neighbour"] = R.knn_radius2(x, k + 1, d2=d2)
    for what, wrong in misses.items():
        assert (np.abs(got - wrong) > tol).any(), what


def test_knn_radius_duplicates_at_k1(ctx):
    """Two equal rows in a set without other structure: both radii at k = 1 are exactly 0, and no other row's is."""
    x = R.feature_rows(129, 512, 77)
    x[100] = x[17]
    got = ctx.op_knn_radius(_t(x), 1).cpu().numpy()
    assert got[17] == 0.0 and got[100] == 0.0 and (np.delete(got, [17, 100]) > 0).all()


# ------------------------------------------------------------------------------------------------ hits
@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("n", [127, 129])
@pytest.mark.parametrize("m", [1, 77, 130])
def test_manifold_hits_against_fp64(ctx, m, n, d):
    parent, ref, r2 = R.hits_case(130, n, d, R.HIT_SEEDS[(n, d)])
    d2 = R.d2_matrix(parent, ref)
    ok, share = R.hit_margin_ok(parent, ref, r2, d2)
    assert ok and share == 0.0, f"{share} of the pairs lie inside the margin"
    want = R.manifold_hits(parent, ref, r2, d2)
    rate = want[:max(m, 77)].mean() if m > 1 else want.mean()      # m = 1: judged on the parent set, see the module docstring
    assert 0.1 < rate < 0.9
    got = ctx.op_manifold_hits(_t(parent[:m]), _t(ref), _t(r2)).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (m,) and set(got.tolist()) <= {0, 1}
    assert np.array_equal(got.astype(bool), want[:m])
    if m == 1:
        for i in (int(np.argmax(want)), int(np.argmin(want))):     # one probe that hits, one that misses
            one = ctx.op_manifold_hits(_t(parent[i:i + 1]), _t(ref), _t(r2)).cpu().numpy()
            assert bool(one[0]) == bool(want[i])
        return
    # near misses that must differ
    perm = np.random.default_rng(1).permutation(n)
    assert not np.array_equal(R.manifold_hits(parent, ref, r2[perm], d2)[:m], got.astype(bool)), "radii permuted among the ref rows"
    assert not np.array_equal(R.manifold_hits(parent, ref, np.full_like(r2, r2.max()), d2)[:m], got.astype(bool)), "max radius for all"


# ------------------------------------------------------------------------------------------------ precision / recall
def test_precision_recall_against_fp64(ctx):
    from rdm_amd import metrics
    real, gen = R.pr_clouds()
    assert R.pr_margin_ok(real, gen, 3)
    want = R.precision_recall(real, gen, 3)
    got = metrics.precision_recall(ctx, _t(real), _t(gen), k=3, center=False)
    print(f"[metrics] precision / recall: {got} (fp64 {want})")
    assert got == want and 0 < got[1] < got[0] < 1
    # centred on the real set's fp32 mean (the default): the restatement on the same shifted rows
    rd, gd = _t(real).to(ctx.device), _t(gen).to(ctx.device)
    mu = rd.mean(dim=0, keepdim=True)
    rc, gc = (rd - mu).cpu().numpy(), (gd - mu).cpu().numpy()
    assert R.pr_margin_ok(rc, gc, 3)
    assert metrics.precision_recall(ctx, rd, gd, k=3) == R.precision_recall(rc, gc, 3)


def test_precision_recall_of_identical_sets(ctx):
    from rdm_amd import metrics
    x = _t(R.feature_rows(150, 64, 9))
    assert metrics.precision_recall(ctx, x, x, k=3) == (1.0, 1.0)
    assert metrics.precision_recall(ctx, x, x.clone(), k=1, center=False) == (1.0, 1.0)


# ------------------------------------------------------------------------------------------------ refusals, determinism
def test_refusals_name_the_op_and_leave_the_context_usable(ctx):
    from rdm_amd import _lib
    x32, x48 = torch.zeros(16, 32), torch.zeros(16, 48)
    s48, o48 = (torch.zeros(sh, device=ctx.device, dtype=torch.float64) for sh in ((48,), (48, 48)))
    s32, o32 = (torch.zeros(sh, device=ctx.device, dtype=torch.float64) for sh in ((32,), (32, 32)))
    cases = [
        ("rdm_op_moments_f64", "48", lambda: ctx.op_moments_f64(x48, s48, o48)),
        ("rdm_op_knn_radius", "48", lambda: ctx.op_knn_radius(x48, 3)),
        ("rdm_op_manifold_hits", "48", lambda: ctx.op_manifold_hits(x48, x48, torch.zeros(16))),
        ("rdm_op_knn_radius", "k = 0", lambda: ctx.op_knn_radius(x32, 0)),
        ("rdm_op_knn_radius", "k = 9", lambda: ctx.op_knn_radius(x32, 9)),
        ("rdm_op_knn_radius", "k = 3", lambda: ctx.op_knn_radius(x32[:3], 3)),           # k >= n
        ("rdm_op_knn_radius", "k = 1", lambda: ctx.op_knn_radius(x32[:1], 1)),
        ("rdm_op_knn_radius", "n = 0", lambda: ctx.op_knn_radius(x32[:0], 1)),
        ("rdm_op_moments_f64", "n = 0", lambda: ctx.op_moments_f64(x32[:0], s32, o32)),
        ("rdm_op_manifold_hits", "m = 0", lambda: ctx.op_manifold_hits(x32[:0], x32, torch.zeros(16))),
        ("rdm_op_manifold_hits", "n = 0", lambda: ctx.op_manifold_hits(x32, x32[:0], torch.zeros(0))),
        ("rdm_op_knn_radius", "d = 4128", lambda: ctx.op_knn_radius(torch.zeros(4, 4128), 1)),
    ]
    x = R.feature_rows(40, 32, 3)
    before = ctx.op_knn_radius(_t(x), 3).cpu()
    for op, word, call in cases:
        with pytest.raises(_lib.RdmError) as e:
            call()
        assert op in str(e.value) and word in str(e.value), str(e.value)
        assert torch.equal(ctx.op_knn_radius(_t(x), 3).cpu(), before)
    # the binding's own argument checks
    with pytest.raises(_lib.RdmError):
        ctx.op_moments_f64(x32, torch.zeros(32, device=ctx.device), o32)                 # fp32 accumulator
    with pytest.raises(_lib.RdmError):
        ctx.op_manifold_hits(x32, torch.zeros(16, 64), torch.zeros(16))
    with pytest.raises(_lib.RdmError):
        ctx.op_manifold_hits(x32, x32, torch.zeros(15))
    with pytest.raises(_lib.RdmError):
        ctx.op_knn_radius(torch.zeros(32), 1)


def test_two_runs_are_bitwise_equal(ctx):
    x, p = R.feature_rows(257, 512, 5), R.feature_rows(130, 512, 6)
    r1, r2 = ctx.op_knn_radius(_t(x), 3), ctx.op_knn_radius(_t(x), 3)
    assert torch.equal(r1, r2)
    scaled = r1 * 1.5
    assert torch.equal(ctx.op_manifold_hits(_t(p), _t(x), scaled), ctx.op_manifold_hits(_t(p), _t(x), scaled))
    (s1, o1), (s2, o2) = _moments(ctx, x), _moments(ctx, x)
    assert np.array_equal(s1, s2) and np.array_equal(o1, o2)
    # a pair's value does not depend on n or on the tile and lane its rows land in: rows 50..179 alone, for the rows whose nearest
    # neighbour within the whole set is one of them
    sub = ctx.op_knn_radius(_t(x[50:180]), 1).cpu().numpy()
    d2 = R.d2_matrix(x, x); np.fill_diagonal(d2, np.inf)
    nearest = d2[50:180].argmin(1)
    same = (nearest >= 50) & (nearest < 180)
    assert same.sum() > 10 and np.array_equal(sub[same], ctx.op_knn_radius(_t(x), 1).cpu().numpy()[50:180][same])


# ------------------------------------------------------------------------------------------------ end to end
def test_evaluate_end_to_end_on_a_tiny_clip(ctx):
    from rdm_amd import metrics
    from rdm_amd.modules.retrievers import ClipImageRetriever
    spec = oclip.tiny_clip_spec()
    sd = ounet.synth_state_dict(oclip.clip_param_shapes(spec), seed=3)
    sd["positional_embedding"] = sd["positional_embedding"] * 0.1
    model = ClipImageRetriever(state_dict=sd, ctx=ctx, clip_cfg=spec_to_clip_cfg(spec))
    g = torch.Generator().manual_seed(12)
    a = torch.rand((40, 3, 48, 48), generator=g) * 2 - 1
    b = (torch.rand((40, 3, 48, 48), generator=g) * 2 - 1) * 0.6 + 0.2
    f = metrics.clip_features(model, a, batch=16)
    assert f.shape == (40, spec.embed_dim) and f.dtype == torch.float32 and bool(torch.isfinite(f).all())
    fn = metrics.clip_features(model, a, batch=16, normalize=True)
    assert torch.allclose(fn.norm(dim=1), torch.ones(40, device=fn.device), atol=1e-5)
    res = metrics.evaluate(model, [a[:25], a[25:]], b, k=3)
    print(f"[metrics] evaluate: {res}")
    assert set(res) == {"fid", "precision", "recall", "n_real", "n_gen"} and (res["n_real"], res["n_gen"]) == (40, 40)
    assert all(np.isfinite(res[key]) for key in ("fid", "precision", "recall"))
    assert 0 <= res["precision"] <= 1 and 0 <= res["recall"] <= 1 and res["fid"] >= 0
    st = metrics.FeatureStats(spec.embed_dim).update(ctx, f)
    same = metrics.evaluate(model, a, a, k=3)
    assert abs(same["fid"]) <= 1e-6 * np.trace(st.cov()) and (same["precision"], same["recall"]) == (1.0, 1.0)
