"""CPU suite of the retrieval search's premises: the input builders of tests/_knn_ref.py have the property each exists for (asserted
inside the builder, in the fp64 reference), and rdm_knn_select -- the one statement of the scan path and of the certificate's eps, which
the search itself launches from -- follows the documented rule and gives an eps no smaller than the derived bound."""
import numpy as np
import pytest

from oracle import retrieval as oret

import _knn_ref as kr


def test_eps_bound_terms():
    """The numbers the derivation comments in csrc/knn.hip quote."""
    assert kr.eps_terms("d512", 512) == {"hi_word": 2.0 ** -11, "accumulation": 512 * 2.0 ** -23}
    assert abs(kr.eps_bound("bulk", 512) - 5.49e-4) < 1e-6 and abs(kr.eps_bound("generic", 512) - 1.23e-4) < 1e-6
    assert kr.eps_bound("generic", 4096) > 9.7e-4 and kr.eps_bound("d512", 512) == kr.eps_bound("bulk", 512)
    for path in kr.PATHS:
        assert all(kr.eps_bound(path, d) < kr.eps_bound(path, d + 64) for d in range(64, 4096, 64))


def test_recorded_measurements_lie_inside_the_derived_bounds():
    for (path, dim), (err_exact, err_path, margin) in kr.MEASURED.items():
        assert err_exact <= kr.eps_bound(path, dim) and err_path <= kr.accumulation_bound(path, dim) and margin > 0


@pytest.mark.parametrize("dim", [256, 512, 4096])
def test_hi_word_worst_case_builder(dim):
    db, q = kr.hi_word_worst_case(300, dim)
    qn, dbn = oret.normalize_queries(q), kr.oracle_dbn(db)
    ex = kr.exact_scores(qn, dbn)
    # the worst case sits inside the derived bound of the hi-word paths and OUTSIDE what the library assumed before (2.4e-4 + accumulation)
    worst = np.abs(ex - kr.path_scores("d512", qn, dbn)).max()
    assert 4.6e-4 <= worst <= kr.eps_bound("d512", dim)
    # the hi + lo reference repairs it, and the answer is the matched row
    assert np.abs(ex - kr.path_scores("generic", qn, dbn)).max() <= kr.eps_terms("generic", dim)["lo_tail"]
    assert kr.topk(dbn, qn, 1)[0][:, 0].tolist() == [0, 1]


@pytest.mark.parametrize("dim,n", [(512, 4097), (64, 4097), (256, 769)])
def test_overflow_builder(dim, n):
    for stride in kr.OVERFLOW_STRIDES:
        if (kr.OVERFLOW_TOP - 1) * stride + 256 >= n:
            continue
        db, q, planted = kr.overflow_case(n, dim, 1, stride)
        ref_i, _ = kr.topk(kr.oracle_dbn(db), oret.normalize_queries(q), 28)
        assert ref_i[0].tolist() == [256 + stride * j for j in range(28)] == planted[:28].tolist()
        assert set(range(256, 512)) <= set(planted.tolist())


@pytest.mark.parametrize("n", [600, 4097, 769])
def test_tie_flood_builder(n):
    db, q, rows = kr.tie_flood_case(n, 64)
    assert len(rows) == 600 if n == 4097 else len(rows) > 250          # a small database holds fewer; still hundreds
    for k in (1, 4, 28):
        ref_i, ref_s = kr.topk(kr.oracle_dbn(db), oret.normalize_queries(q), k)
        assert ref_i[0].tolist() == rows[:k].tolist() and (ref_s[0] == ref_s[0, 0]).all()


def test_all_negative_builder():
    db, q = kr.all_negative_case(4097, 512)
    assert db.shape == (4097, 512)
    with pytest.raises(AssertionError):
        kr.all_negative_case(4096, 512)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("dim", [64, 192, 512, 4096])
def test_normalisation_reference_brackets_the_oracle(dim, dtype):
    """The oracle's own normalised rows (fp32 quotient of the numpy-order norm) lie inside the bracket the kernel is held to, and the
    bracket is one bit pattern nearly everywhere."""
    for n in (1, 3, 4, 5):
        x = kr.normalisation_edges(n, dim, dtype)
        lo, hi = kr.norm_rows64(x)
        got = kr.oracle_dbn(x).view(np.uint16)
        assert ((got == lo) | (got == hi)).all()
        assert (lo != hi).mean() <= 2e-2
        if n > 1:
            assert not got[n - 1].any()
    xq = kr.normalisation_edges(5, dim, np.float32)[:1]          # the oracle's normalised queries against fp64: QN_REL
    q64 = kr.norm_queries64(xq)
    assert (np.abs(oret.normalize_queries(xq) - q64) <= kr.QN_REL * np.abs(q64)).all()


def test_split_hi_lo():
    rng = np.random.default_rng(0)
    qn = oret.normalize_queries(rng.standard_normal((4, 512)).astype(np.float32))
    hi, lo = kr.split_hi_lo(qn)
    resid = qn.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)
    assert (np.abs(resid) <= np.maximum(2.0 ** -25, kr.U16 * kr.U16 * np.abs(qn))).all()


DIMS = list(range(64, 4097, 64))
BS = (1, 64, 65, 127, 128, 512, 513)
KS = (1, 4, 5, 28)
NS = (1, 255, 3840, 3841, 10 ** 6)


def test_knn_select_rule_and_eps():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    seen = set()
    for dim in DIMS:
        for n in NS:
            for b in BS:
                for k in KS:
                    if k > n:
                        with pytest.raises(_lib.RdmError):
                            _lib.knn_select(n, dim, b, k)
                        continue
                    f = _lib.knn_select(n, dim, b, k)
                    path = kr.expected_path(n, dim, b)
                    assert f["path"] == path, (n, dim, b, k, f)
                    assert f["queries_per_launch"] == (512 if path == "bulk" else 64)
                    assert f["ksel"] == 8 and f["rescored"] == (16 if k <= 4 else 64) and f["rescored"] >= k
                    assert f["lists_per_block"] == (4 if path == "bulk" else 8)
                    assert f["eps"] >= kr.eps_bound(path, dim), (path, dim, f["eps"], kr.eps_bound(path, dim))
                    assert f["eps"] <= 1.01 * kr.eps_bound(path, dim) + 2e-6          # derived, not padded: the fallback rate follows it
                    seen.add(path)
    assert seen == set(kr.PATHS)
    for bad in ((0, 512, 1, 1), (10, 100, 1, 1), (10, 4160, 1, 1), (100, 512, 0, 1), (100, 512, 1, 0), (100, 512, 1, 29), (2 ** 32, 512, 1, 1)):
        with pytest.raises(_lib.RdmError):
            _lib.knn_select(*bad)
