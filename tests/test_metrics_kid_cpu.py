"""CPU suite of KID and density / coverage: the fp64 restatements of tests/_metrics_kid_ref.py against brute-force loops, every condition
the GPU tests' seeded inputs were picked for, the CPU emulation of the kernel's fp32 dot-product chain against the dot bound, the new flags
of scripts/rdm_eval.py, and the three C-ABI symbols."""
import importlib.util
import os
import re

import numpy as np
import pytest

import _metrics_kid_ref as K
import _metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"rdm_op_manifold_counts": 8, "rdm_op_nearest_d2": 7, "rdm_op_poly3_rowsums": 11}


# ------------------------------------------------------------------------------------------------ the restatements against loops
def test_restatements_against_brute_force_loops():
    rng = np.random.default_rng(21)
    n, m, d, k = 11, 7, 5, 3
    x = rng.standard_normal((n, d))
    y = rng.standard_normal((m, d)) * 0.8 + 0.3
    r2 = R.knn_radius2(x, k)
    d2 = [[sum((y[i, a] - x[j, a]) ** 2 for a in range(d)) for j in range(n)] for i in range(m)]
    counts = [sum(d2[i][j] <= r2[j] for j in range(n)) for i in range(m)]
    assert K.manifold_counts(y, x, r2).tolist() == counts and max(counts) >= 2
    assert np.array_equal(K.manifold_counts(y, x, r2) > 0, R.manifold_hits(y, x, r2))
    assert np.allclose(K.nearest_d2(y, x), [min(row) for row in d2], rtol=0, atol=1e-13)
    dens, cov = K.density_coverage(x, y, k)
    assert dens == sum(counts) / (k * m)
    assert cov == sum(min(d2[i][j] for i in range(m)) <= r2[j] for j in range(n)) / n
    # identical sets: every row lies in its own ball and in those of the k rows it is a k-NN of at least ... so density >= 1, coverage 1
    dens_same, cov_same = K.density_coverage(x, x, k)
    assert cov_same == 1.0 and dens_same >= 1.0

    gamma, coef0 = 0.37, 0.8
    for excl in (False, True):
        rows = [sum((gamma * sum(y[i, a] * x[j, a] for a in range(d)) + coef0) ** 3 for j in range(n) if not (excl and i == j)) for i in range(m)]
        assert np.allclose(K.poly3_rowsums(y, x, gamma, coef0, excl), rows, rtol=1e-13, atol=0)
    kern = lambda a, b: (gamma * float(a @ b) + coef0) ** 3
    xx = sum(kern(x[i], x[j]) for i in range(n) for j in range(n) if i != j) / (n * (n - 1))
    yy = sum(kern(y[i], y[j]) for i in range(m) for j in range(m) if i != j) / (m * (m - 1))
    xy = sum(kern(x[i], y[j]) for i in range(n) for j in range(m)) / (n * m)
    val, bound = K.kid(x, y, gamma, coef0)
    assert abs(val - (xx + yy - 2 * xy)) <= 1e-12 and 0 < bound < 1e-4 * abs(val)
    biased = (sum(kern(x[i], x[j]) for i in range(n) for j in range(n)) / n ** 2 + sum(kern(y[i], y[j]) for i in range(m) for j in range(m)) / m ** 2 - 2 * xy)
    assert abs(K.kid_near_misses(x, y, gamma, coef0)["biased (diagonal kept, / s^2)"] - biased) <= 1e-12
    # the default gamma is 1 / d; the subset restatement draws x first, then y, per subset
    assert K.kid(x, y)[0] == K.kid(x, y, 1.0 / d, 1.0)[0]
    vals, _ = K.kid_subsets(x, y, 3, 4, 9)
    rng2 = np.random.default_rng(9)
    for v in vals:
        ix = rng2.choice(n, 4, replace=False); iy = rng2.choice(m, 4, replace=False)
        assert v == K.kid(x[ix], y[iy])[0]
    assert K.kid_subsets(x, y, 2, 100, 9)[0][0] == K.kid_subsets(x, y, 2, m, 9)[0][0]          # subset_size clamps to the smaller set


# ------------------------------------------------------------------------------------------------ the inputs' conditions
def test_count_inputs_meet_their_conditions():
    assert set(K.COUNT_SEEDS) == {(127, 32), (129, 32), (127, 512), (129, 512), (257, 64)}
    for (n, d), seed in K.COUNT_SEEDS.items():
        probe, ref, r2 = K.counts_case(130, n, d, seed)
        d2 = R.d2_matrix(probe, ref)
        ok, share = R.hit_margin_ok(probe, ref, r2, d2)
        assert ok and share == 0.0, (n, d, share)
        cnt = K.manifold_counts(probe, ref, r2, d2)
        print(f"[kid] counts n={n} d={d}: mean {cnt.mean():.2f}, max {cnt.max()}, share >= 2 {np.mean(cnt >= 2):.2f}, share 0 {np.mean(cnt == 0):.2f}")
        assert 520 < cnt.sum() <= 530
        perm = np.random.default_rng(1).permutation(n)              # the permutation tests/test_gpu_metrics_kid.py uses
        for m in (77, 130):
            assert np.mean(cnt[:m] >= 2) >= 0.15 and np.mean(cnt[:m] == 0) >= 0.15 and cnt[:m].max() >= 4
            assert not np.array_equal(K.manifold_counts(probe, ref, r2[perm], d2)[:m], cnt[:m])
            assert not np.array_equal(np.minimum(cnt[:m], 1), cnt[:m])


def test_density_coverage_inputs_keep_the_margin():
    real, gen = R.pr_clouds()
    for k, want_cov, want_dens in ((3, 0.85, 2.545), (5, 0.92, 2.529)):
        assert R.pr_margin_ok(real, gen, k)
        ok, closest = K.dc_margin_ok(real, gen, k)
        dens, cov = K.density_coverage(real, gen, k)
        print(f"[kid] density / coverage k={k}: {dens:.4f} / {cov:.4f}, closest coverage gap {closest:.0f} margins")
        assert ok and closest >= 260
        assert abs(cov - want_cov) < 0.005 and abs(dens - want_dens) < 0.0005
    # identical sets: a row's k-th neighbour sits ON its ball (the same pair, the same value, in the kernels bit for bit), so no margin holds
    # there; the count of a ball is k + 1 in fp64 and on the kernel alike when its k-th and (k + 1)-th neighbours are more than two d2
    # bounds apart.  Density is then (k + 1) / k
    x, k = K.identical_case(), 3
    d2 = R.d2_matrix(x, x); np.fill_diagonal(d2, np.inf)
    d2.sort(axis=1)
    assert ((d2[:, k] - d2[:, k - 1]) > 2 * R.radius_bound(x)).all()
    assert K.density_coverage(x, x, k) == ((k + 1) / k, 1.0)


def test_kid_inputs_and_near_misses():
    worst, ratios = np.inf, []
    for name, (x, y) in K.kid_pairs().items():
        for gamma in (None, 1.0):
            val, bound = K.kid(x, y, gamma)
            ratios.append(bound / abs(val))
            assert 1e-3 < val < 4e3, (name, gamma, val)
            for what, wrong in K.kid_near_misses(x, y, gamma).items():
                worst = min(worst, abs(wrong - val) / bound)
                assert abs(wrong - val) > bound, (name, gamma, what)
    print(f"[kid] bound / KID from {min(ratios):.2e} to {max(ratios):.2e}; the closest near miss lies {worst:.3g} bounds away")
    assert 5e-6 < min(ratios) and max(ratios) < 2e-5 and worst >= 1.4e3
    # the subset runs of the GPU test: every set holds the 100 rows a subset takes
    assert all(min(x.shape[0], y.shape[0]) >= 100 for x, y in K.kid_pairs().values())


def test_poly_and_group_inputs():
    for m, n in ((1, 1), (2, 2), (127, 129), (128, 128), (129, 127), (257, 130)):
        for d in (32, 512):
            p, r = K.poly_case(m, n, d)
            assert p.shape == (m, d) and r.shape == (n, d)
            for gamma in (1.0 / d, 1.0):
                for coef0 in (0.0, 1.0):
                    q = min(m, n)
                    diff = (K.poly3_rowsums(p, r, gamma, coef0) - K.poly3_rowsums(p, r, gamma, coef0, True))[:q]
                    both = (K.poly3_bound(p, r, gamma, coef0) + K.poly3_bound(p, r, gamma, coef0, True))[:q]
                    assert (np.abs(diff) > 4 * both).all(), (m, n, d, gamma, coef0)          # the excluded pair is visible on every such row
    p, r = K.group_case()
    assert p.shape == (3, 129, 64) and r.shape == (3, 127, 64)
    for gamma in (1.0 / 64, 1.0):
        a, b = K.poly3_rowsums(p[0], r[0], gamma, 1.0), K.poly3_rowsums(p[0], r[1], gamma, 1.0)
        assert (np.abs(a - b) > 4 * (K.poly3_bound(p[0], r[0], gamma, 1.0) + K.poly3_bound(p[0], r[1], gamma, 1.0))).any()


# ------------------------------------------------------------------------------------------------ the fp32 chain, emulated
def test_fp32_chain_emulation_stays_inside_the_dot_bound():
    worst = 0.0
    groups = K.group_case()
    cases = [K.poly_case(129, 127, 32), K.poly_case(129, 127, 512), (groups[0][0], groups[1][0])] + list(K.kid_pairs().values())
    for p, r in cases:
        p, r = p[:130], r[:130]
        got = K.chain_dots_f32(p, r).astype(np.float64)
        bound = K.DOT_GAMMA * (R.sqnorms(p)[:, None] + R.sqnorms(r)[None, :])
        ratio = float((np.abs(got - K._dots(p, r)) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0
        # a row against itself: the chain gives the same value whichever side the row is on
        assert np.array_equal(K.chain_dots_f32(p[:5], p[:5]), K.chain_dots_f32(p[:5], p[:5]).T)
    print(f"[kid] fp32 chain emulation: worst |dot - fp64| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ script and symbols
def _load_script():
    spec = importlib.util.spec_from_file_location("rdm_eval_script_kid", os.path.join(ROOT, "scripts", "rdm_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rdm_eval_parser_new_flags(capsys):
    mod = _load_script()
    base = ["--real", "a", "--fake", "b", "--synthetic"]
    opt = mod.parse_args(base)
    assert (opt.kid, opt.kid_subsets, opt.kid_subset_size, opt.kid_seed, opt.density_coverage, opt.dc_k) == (False, 100, 1000, 0, False, 5)
    assert mod.extras(opt) == ()
    opt = mod.parse_args(base + ["--kid", "--kid_subsets", "10", "--kid_subset_size", "50", "--kid_seed", "4", "--density_coverage", "--dc_k", "8"])
    assert (opt.kid, opt.kid_subsets, opt.kid_subset_size, opt.kid_seed, opt.density_coverage, opt.dc_k) == (True, 10, 50, 4, True, 8)
    assert mod.extras(opt) == ("kid", "density_coverage")
    assert mod.extras(mod.parse_args(base + ["--density_coverage"])) == ("density_coverage",)
    for bad in (base + ["--dc_k", "0"], base + ["--dc_k", "9"], base + ["--kid_subsets", "-1"], base + ["--kid_subset_size", "1"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    capsys.readouterr()


def test_new_symbols_in_header_signature_table_and_library():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    src = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for op, nargs in OPS.items():
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % op, decl)
        assert found, f"{op} is not declared in include/rdm_hip.h"
        assert len(found.group(1).split(",")) == nargs, op
        assert len(_lib.SIGNATURES[op][1]) == nargs, op
        assert hasattr(_lib.lib, op), f"{op} is not exported by the built library"
    for method in ("op_manifold_counts", "op_nearest_d2", "op_poly3_rowsums"):
        assert callable(getattr(_lib.Context, method))
    from rdm_amd import metrics
    assert callable(metrics.density_coverage) and callable(metrics.kernel_distance)
    # each C entry's header comment names the paper whose formula it serves
    assert "Naeem" in src and "Binkowski" in src
