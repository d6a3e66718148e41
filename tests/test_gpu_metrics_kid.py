"""GPU suite of KID and density / coverage: the count, nearest and cubic-kernel modes of metric_dist_kernel (csrc/metrics.hip) through
Context.op_manifold_counts / op_nearest_d2 / op_poly3_rowsums, and rdm_amd.metrics.density_coverage / kernel_distance / evaluate on top,
against the fp64 restatements of tests/_metrics_kid_ref.py.

Bounds (derived in tests/_metrics_kid_ref.py and tests/_metrics_ref.py; tests/test_metrics_kid_cpu.py re-checks the inputs' conditions):
  counts    equal to fp64, on inputs whose every pair keeps |d2 - r2_j| > 2 D2_GAMMA (|a|^2 + |b|^2).
  nearest   within D2_GAMMA (|probe_i|^2 + max_j |ref_j|^2) of the fp64 minimum.
  poly      every row sum within SUM_j [(|v_ij| + gamma delta_ij)^3 - |v_ij|^3] + n 2^-52 SUM_j |k_ij|, delta = 2.5e-7 (|a|^2 + |b|^2).
  KID       the three terms' bounds combined as the terms are.
  density / coverage   equal to fp64 (the inputs keep the composed margins)."""
import numpy as np
import pytest
import torch

from oracle import clip as oclip
from oracle import unet as ounet

import _metrics_kid_ref as K
import _metrics_ref as R
from _util import spec_to_clip_cfg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("n,d", sorted(K.COUNT_SEEDS))
@pytest.mark.parametrize("m", [1, 77, 130])
def test_manifold_counts_against_fp64(ctx, m, n, d):
    parent, ref, r2 = K.counts_case(130, n, d, K.COUNT_SEEDS[(n, d)])
    d2 = R.d2_matrix(parent, ref)
    ok, share = R.hit_margin_ok(parent, ref, r2, d2)
    assert ok and share == 0.0, f"{share} of the pairs lie inside the margin"
    want = K.manifold_counts(parent, ref, r2, d2)
    got = ctx.op_manifold_counts(_t(parent[:m]), _t(ref), _t(r2))
    assert got.dtype == torch.int32 and tuple(got.shape) == (m,)
    got = got.cpu().numpy()
    print(f"[kid] counts m={m} n={n} d={d}: sum {int(got.sum())} (fp64 {int(want[:m].sum())}), max {int(got.max())}")
    assert np.array_equal(got, want[:m])
    hits = ctx.op_manifold_hits(_t(parent[:m]), _t(ref), _t(r2)).cpu().numpy()
    assert np.array_equal(got > 0, hits.astype(bool))
    if m == 1:
        for i in (int(np.argmax(want)), int(np.argmin(want))):     # the fullest probe and an empty one, alone
            one = ctx.op_manifold_counts(_t(parent[i:i + 1]), _t(ref), _t(r2)).cpu().numpy()
            assert int(one[0]) == int(want[i])
        assert want.max() >= 4 and want.min() == 0
        return
    # near misses that must differ
    perm = np.random.default_rng(1).permutation(n)
    assert not np.array_equal(K.manifold_counts(parent, ref, r2[perm], d2)[:m], got), "radii permuted among the ref rows"
    assert not np.array_equal(np.minimum(want[:m], 1), got), "a kernel that ORs"


# ------------------------------------------------------------------------------------------------ nearest
@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 257])
@pytest.mark.parametrize("m", [1, 130])
def test_nearest_d2_against_fp64(ctx, m, n, d):
    ref = R.feature_rows(n, d, 800 + n + d)
    probe = R.feature_rows(m, d, 900 + n + d)
    probe[0] = ref[n // 2]                                          # a probe copied from a ref row
    d2 = R.d2_matrix(probe, ref)
    want, tol = K.nearest_d2(probe, ref, d2), K.nearest_bound(probe, ref)
    got = ctx.op_nearest_d2(_t(probe), _t(ref))
    assert got.dtype == torch.float32 and tuple(got.shape) == (m,)
    got32 = got.cpu().numpy()
    got = got32.astype(np.float64)
    print(f"[kid] nearest m={m} n={n} d={d}: worst error / bound {float((np.abs(got - want) / tol).max()):.3g}")
    assert (got >= 0).all() and (np.abs(got - want) <= tol).all()
    assert got[0] == 0.0 and want[0] == 0.0
    if n >= 2 and m > 1:
        assert (np.abs(got - np.sort(d2, axis=1)[:, 1]) > tol).any(), "the second-smallest distance"
    if m > 1:
        # one constant radius strictly between two distinct kernel outputs: hits with that radius are the nearest mode's comparison
        vals = np.unique(got32)
        r = None
        for i in range(len(vals) // 2, len(vals) - 1):
            mid = np.float32(0.5 * (float(vals[i]) + float(vals[i + 1])))
            if vals[i] < mid < vals[i + 1]:
                r = mid
                break
        assert r is not None
        hits = ctx.op_manifold_hits(_t(probe), _t(ref), torch.full((n,), float(r))).cpu().numpy().astype(bool)
        assert np.array_equal(hits, got32 <= r) and hits.any() and not hits.all()


# ------------------------------------------------------------------------------------------------ cubic-kernel row sums
_poly_worst = {"ratio": 0.0}


@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("m,n", [(1, 1), (2, 2), (127, 129), (128, 128), (129, 127), (257, 130)])
def test_poly3_rowsums_against_fp64(ctx, m, n, d):
    probe, ref = K.poly_case(m, n, d)
    q = min(m, n)
    for gamma in (1.0 / d, 1.0):
        for coef0 in (0.0, 1.0):
            got = {}
            for excl in (0, 1):
                out = ctx.op_poly3_rowsums(_t(probe), _t(ref), gamma, coef0, exclude_same_index=excl)
                assert out.dtype == torch.float64 and tuple(out.shape) == (m,)
                got[excl] = out.cpu().numpy()
                want, tol = K.poly3_rowsums(probe, ref, gamma, coef0, excl), K.poly3_bound(probe, ref, gamma, coef0, excl)
                err = np.abs(got[excl] - want)
                ratio = float((err / np.maximum(tol, 1e-300)).max()) if tol.max() > 0 else 0.0
                _poly_worst["ratio"] = max(_poly_worst["ratio"], ratio)
                print(f"[kid] poly m={m} n={n} d={d} gamma={gamma:.4g} coef0={coef0} excl={excl}: worst error / bound {ratio:.3g} "
                      f"(worst so far {_poly_worst['ratio']:.3g})")
                assert (err <= tol).all()
            tol_both = K.poly3_bound(probe, ref, gamma, coef0, 0) + K.poly3_bound(probe, ref, gamma, coef0, 1)
            assert (np.abs(got[0] - got[1])[:q] > tol_both[:q]).all(), "the excluded pair"
            assert np.array_equal(got[0][q:], got[1][q:])          # rows without a same-index partner: nothing to leave out
            if m == 1 and n == 1:
                assert got[1][0] == 0.0


def test_poly3_rowsums_groups(ctx):
    probe, ref = K.group_case()
    G, m, n = probe.shape[0], probe.shape[1], ref.shape[1]
    for gamma, excl in ((1.0 / 64, 0), (1.0, 1)):
        whole = ctx.op_poly3_rowsums(_t(probe), _t(ref), gamma, 1.0, exclude_same_index=excl)
        assert tuple(whole.shape) == (G, m) and whole.dtype == torch.float64
        whole = whole.cpu().numpy()
        for g in range(G):
            one = ctx.op_poly3_rowsums(_t(probe[g]), _t(ref[g]), gamma, 1.0, exclude_same_index=excl).cpu().numpy()
            assert np.array_equal(whole[g], one)                   # bitwise: a row's sum does not depend on the group count
            tol = K.poly3_bound(probe[g], ref[g], gamma, 1.0, excl)
            assert (np.abs(whole[g] - K.poly3_rowsums(probe[g], ref[g], gamma, 1.0, excl)) <= tol).all()
        # the 3-D binding with one group equals the 2-D one
        assert np.array_equal(ctx.op_poly3_rowsums(_t(probe[:1]), _t(ref[:1]), gamma, 1.0, exclude_same_index=excl).cpu().numpy()[0], whole[0])
        swapped = ctx.op_poly3_rowsums(_t(probe), _t(ref[[1, 0, 2]]), gamma, 1.0, exclude_same_index=excl).cpu().numpy()
        for g in (0, 1):
            tol = K.poly3_bound(probe[g], ref[g], gamma, 1.0, excl) + K.poly3_bound(probe[g], ref[1 - g], gamma, 1.0, excl)
            assert (np.abs(swapped[g] - whole[g]) > tol).any(), "group g saw another group's ref rows"
        assert np.array_equal(swapped[2], whole[2])


# ------------------------------------------------------------------------------------------------ kernel_distance
@pytest.mark.parametrize("name", sorted(K.kid_pairs()))
def test_kernel_distance_against_fp64(ctx, name):
    from rdm_amd import metrics
    x, y = K.kid_pairs()[name]
    xd, yd = _t(x).to(ctx.device), _t(y).to(ctx.device)
    for gamma in (None, 1.0):
        want, tol = K.kid(x, y, gamma)
        got, std = metrics.kernel_distance(ctx, xd, yd, subsets=0, gamma=gamma)
        print(f"[kid] {name} gamma={gamma}: whole-set KID {got:.9g} (fp64 {want:.9g}), error / bound {abs(got - want) / tol:.3g}")
        assert std == 0.0 and abs(got - want) <= tol
        for what, wrong in K.kid_near_misses(x, y, gamma).items():
            assert abs(got - wrong) > tol, what
        vals, bounds = K.kid_subsets(x, y, 7, 100, 3, gamma)
        mean, std = metrics.kernel_distance(ctx, xd, yd, subsets=7, subset_size=100, seed=3, gamma=gamma)
        print(f"[kid] {name} gamma={gamma}: 7 x 100 KID {mean:.9g} +- {std:.3g} (fp64 {vals.mean():.9g} +- {vals.std():.3g})")
        assert abs(mean - vals.mean()) <= bounds.mean() and abs(std - vals.std()) <= 2 * bounds.max()
        assert std > 0


def test_kernel_distance_subsets_clamp_repeat_and_seed(ctx):
    from rdm_amd import metrics
    x, y = K.kid_pairs()["129x32"]
    xd, yd = _t(x).to(ctx.device), _t(y).to(ctx.device)
    vals, bounds = K.kid_subsets(x, y, 5, 1000, 0)                  # 1000 > 127 rows: subsets of 127
    first = metrics.kernel_distance(ctx, xd, yd, subsets=5, subset_size=1000, seed=0)
    assert abs(first[0] - vals.mean()) <= bounds.mean()
    assert first == metrics.kernel_distance(ctx, xd, yd, subsets=5, subset_size=127, seed=0)
    assert first == metrics.kernel_distance(ctx, xd, yd, subsets=5, subset_size=1000, seed=0)          # two runs, bitwise
    other = metrics.kernel_distance(ctx, xd, yd, subsets=5, subset_size=100, seed=1)
    assert other[0] != metrics.kernel_distance(ctx, xd, yd, subsets=5, subset_size=100, seed=0)[0]
    # chunked gathers (a cap that holds two subsets a chunk) give the same numbers
    cap = metrics.KID_GATHER_BYTES
    try:
        metrics.KID_GATHER_BYTES = 2 * 2 * 127 * 32 * 4
        assert metrics.kernel_distance(ctx, xd, yd, subsets=5, subset_size=1000, seed=0) == first
    finally:
        metrics.KID_GATHER_BYTES = cap


# ------------------------------------------------------------------------------------------------ density / coverage
@pytest.mark.parametrize("k", [3, 5])
def test_density_coverage_against_fp64(ctx, k):
    from rdm_amd import metrics
    real, gen = R.pr_clouds()
    assert K.dc_margin_ok(real, gen, k)[0]
    want = K.density_coverage(real, gen, k)
    got = metrics.density_coverage(ctx, _t(real), _t(gen), k=k, center=False)
    print(f"[kid] density / coverage k={k}: {got} (fp64 {want})")
    assert got == want and got[0] > 1.0 and 0.0 < got[1] < 1.0
    # centred on the real set's fp32 mean (the default): the restatement on the same shifted rows
    rd, gd = _t(real).to(ctx.device), _t(gen).to(ctx.device)
    mu = rd.mean(dim=0, keepdim=True)
    rc, gc = (rd - mu).cpu().numpy(), (gd - mu).cpu().numpy()
    assert K.dc_margin_ok(rc, gc, k)[0]
    assert metrics.density_coverage(ctx, rd, gd, k=k) == K.density_coverage(rc, gc, k)


def test_density_coverage_of_identical_sets(ctx):
    from rdm_amd import metrics
    x = K.identical_case()
    want = K.density_coverage(x, x, 3)
    for center in (False, True):
        got = metrics.density_coverage(ctx, _t(x), _t(x).clone(), k=3, center=center)
        assert got[1] == 1.0 and got[0] >= 1.0 and got == want


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_op_and_leave_the_context_usable(ctx):
    from rdm_amd import _lib, metrics
    x32, x48, big = torch.zeros(16, 32), torch.zeros(16, 48), torch.zeros(4, 4128)
    r16 = torch.zeros(16)
    cases = [
        ("rdm_op_manifold_counts", "48", lambda: ctx.op_manifold_counts(x48, x48, r16)),
        ("rdm_op_nearest_d2", "48", lambda: ctx.op_nearest_d2(x48, x48)),
        ("rdm_op_poly3_rowsums", "48", lambda: ctx.op_poly3_rowsums(x48, x48, 1.0)),
        ("rdm_op_manifold_counts", "4128", lambda: ctx.op_manifold_counts(big, big, torch.zeros(4))),
        ("rdm_op_nearest_d2", "4128", lambda: ctx.op_nearest_d2(big, big)),
        ("rdm_op_poly3_rowsums", "4128", lambda: ctx.op_poly3_rowsums(big, big, 1.0)),
        ("rdm_op_manifold_counts", "m = 0", lambda: ctx.op_manifold_counts(x32[:0], x32, r16)),
        ("rdm_op_manifold_counts", "n = 0", lambda: ctx.op_manifold_counts(x32, x32[:0], torch.zeros(0))),
        ("rdm_op_nearest_d2", "m = 0", lambda: ctx.op_nearest_d2(x32[:0], x32)),
        ("rdm_op_nearest_d2", "n = 0", lambda: ctx.op_nearest_d2(x32, x32[:0])),
        ("rdm_op_poly3_rowsums", "m = 0", lambda: ctx.op_poly3_rowsums(x32[:0], x32, 1.0)),
        ("rdm_op_poly3_rowsums", "n = 0", lambda: ctx.op_poly3_rowsums(x32, x32[:0], 1.0)),
        ("rdm_op_poly3_rowsums", "groups = 0", lambda: ctx.op_poly3_rowsums(torch.zeros(0, 16, 32), torch.zeros(0, 16, 32), 1.0)),
        # the binding's own argument checks
        ("op_manifold_counts", "[16]", lambda: ctx.op_manifold_counts(x32, x32, torch.zeros(15))),
        ("op_manifold_counts", "(16, 64)", lambda: ctx.op_manifold_counts(x32, torch.zeros(16, 64), r16)),
        ("op_nearest_d2", "(16, 64)", lambda: ctx.op_nearest_d2(x32, torch.zeros(16, 64))),
        ("op_poly3_rowsums", "3 groups", lambda: ctx.op_poly3_rowsums(torch.zeros(3, 16, 32), torch.zeros(2, 16, 32), 1.0)),
        ("op_poly3_rowsums", "float64", lambda: ctx.op_poly3_rowsums(x32, x32, 1.0, out=torch.zeros(16, device=ctx.device))),
        ("op_poly3_rowsums", "(16,)", lambda: ctx.op_poly3_rowsums(x32, x32, 1.0, out=torch.zeros(15, device=ctx.device, dtype=torch.float64))),
        ("op_poly3_rowsums", "(16, 32)", lambda: ctx.op_poly3_rowsums(torch.zeros(1, 16, 32), x32, 1.0)),
    ]
    x = R.feature_rows(40, 32, 3)
    before = ctx.op_knn_radius(_t(x), 3).cpu()
    for op, word, call in cases:
        with pytest.raises(_lib.RdmError) as e:
            call()
        assert op in str(e.value) and word in str(e.value), str(e.value)
        assert torch.equal(ctx.op_knn_radius(_t(x), 3).cpu(), before)
    for bad, word in ((lambda: metrics.kernel_distance(ctx, x32[:1], x32), "s = 1"),
                      (lambda: metrics.kernel_distance(ctx, x32, x32[:1], subsets=0), "n_gen = 1"),
                      (lambda: metrics.kernel_distance(ctx, x32, torch.zeros(16, 64)), "32 and 64")):
        with pytest.raises(ValueError) as e:
            bad()
        assert "kernel_distance" in str(e.value) and word in str(e.value), str(e.value)
        assert torch.equal(ctx.op_knn_radius(_t(x), 3).cpu(), before)


# ------------------------------------------------------------------------------------------------ end to end
def test_evaluate_extras_on_a_tiny_clip(ctx):
    from rdm_amd import metrics
    from rdm_amd.modules.retrievers import ClipImageRetriever
    spec = oclip.tiny_clip_spec()
    sd = ounet.synth_state_dict(oclip.clip_param_shapes(spec), seed=3)
    sd["positional_embedding"] = sd["positional_embedding"] * 0.1
    model = ClipImageRetriever(state_dict=sd, ctx=ctx, clip_cfg=spec_to_clip_cfg(spec))
    g = torch.Generator().manual_seed(12)
    a = torch.rand((40, 3, 48, 48), generator=g) * 2 - 1
    b = (torch.rand((40, 3, 48, 48), generator=g) * 2 - 1) * 0.6 + 0.2
    old = metrics.evaluate(model, [a[:25], a[25:]], b, k=3)
    assert set(old) == {"fid", "precision", "recall", "n_real", "n_gen"}
    assert metrics.evaluate(model, [a[:25], a[25:]], b, k=3, extra=()) == old
    res = metrics.evaluate(model, [a[:25], a[25:]], b, k=3, extra=("kid", "density_coverage"), kid_subsets=4, kid_subset_size=30, kid_seed=1, dc_k=5)
    print(f"[kid] evaluate: {res}")
    assert set(res) == set(old) | {"kid", "kid_std", "density", "coverage"}
    assert all(res[key] == old[key] for key in old)
    assert all(np.isfinite(res[key]) for key in ("kid", "kid_std", "density", "coverage"))
    assert 0 <= res["coverage"] <= 1 and res["density"] >= 0 and res["kid_std"] >= 0
    assert set(metrics.evaluate(model, a, b, extra=("kid",))) == set(old) | {"kid", "kid_std"}
    with pytest.raises(ValueError):
        metrics.evaluate(model, a, b, extra=("rbf",))
