"""The retrieval search (csrc/knn.hip) stage by stage on the device, against the float64 references and derived bounds of
tests/_knn_ref.py.  rdm_op_knn_stages runs the launches rdm_knn runs and copies out the prepared queries, every lane list of the scan,
and the merge's certificate before the exact fallback; rdm_db_rows gives the normalised rows.

What is held, per scan path (generic hi + lo, dim-512 hi word, bulk hi word) and at the sizes where each takes another turn (one row, a
tile less / exactly / plus one row, a last tile of one row, the third tile of a block, one to four query groups):
  1  normalised rows and prepared queries, bit for bit where the definition fixes the bits;
  2  the certificate's premise: every candidate score within eps_bound(path, dim) of the exact score, and within the accumulation term
     alone of the path's own exact-arithmetic score (a scan that lost the lo word or a K slice falls outside that);
  3  list invariants and completeness;  4  the certificate's arithmetic;  5  random data certifies (the margin is printed and recorded);
  6  inputs that MUST fall back -- overflowed lanes, hundreds of ties, the hi-word worst case -- return the oracle's answer.
Figures are printed before they are asserted; tests/_knn_ref.py MEASURED records them."""
import numpy as np
import pytest
import torch

from oracle import retrieval as oret

import _knn_ref as kr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


# ---------------------------------------------------------------------------------------------------------------- helpers
def _np(t):
    return t.detach().cpu().numpy()


def _stages(ctx, q, k):
    st = ctx.knn_stages(torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)), k)
    torch.cuda.synchronize()
    out = {name: (_np(v) if isinstance(v, torch.Tensor) else v) for name, v in st.items()}
    for name in ("idx", "cand_i", "tau_idx"):
        out[name] = out[name].view(np.uint32)
    return out


def _dbn(ctx, n):
    d = ctx.db_rows(0, n)
    torch.cuda.synchronize()
    return _np(d)


def _check_prepared(st, q):
    """Case 1, queries: qn against float64 and against the definition, hi / lo split of the device's own qn, padding rows."""
    b, dim = q.shape
    qn, qh, ql = st["qn"], st["qh"], st["ql"]
    assert qn.shape[0] in (64, 128, 256, 384, 512) and qn.shape[0] >= b
    q64 = kr.norm_queries64(q)
    rel = np.abs(qn[:b] - q64).max() / max(np.abs(q64).max(), 1e-30)
    assert (np.abs(qn[:b] - q64) <= kr.QN_REL * np.abs(q64)).all(), rel
    ref = oret.normalize_queries(q)                                   # the definition: fp32 quotient by the fp32 norm
    same = (qn[:b].view(np.uint32) == ref.view(np.uint32)).all(axis=1)
    # a row may differ from numpy's only through the fp32 norm (another summation order): then the whole row is q / neighbouring norm
    for r in np.nonzero(~same)[0]:
        n32 = np.sqrt((q[r].astype(np.float64) ** 2).sum()).astype(np.float32)
        assert any(np.array_equal(qn[r], q[r] / m) for m in (np.nextafter(n32, np.float32(0)), np.nextafter(n32, np.float32(np.inf)))), r
    assert same.mean() >= 0.9
    hi, lo = kr.split_hi_lo(qn)
    assert np.array_equal(qh.view(np.uint16), hi.view(np.uint16)) and np.array_equal(ql.view(np.uint16), lo.view(np.uint16))
    for a in (qn.view(np.uint32), qh.view(np.uint16), ql.view(np.uint16)):
        assert not a[b:].any()


def _check_rows(ctx, x):
    """Case 1, rows: inside the bracket of _knn_ref.norm_rows64 (one bit pattern nearly everywhere), zero rows -> zeros."""
    got = _dbn(ctx, x.shape[0]).view(np.uint16)
    lo, hi = kr.norm_rows64(x)
    assert ((got == lo) | (got == hi)).all(), int((~((got == lo) | (got == hi))).sum())
    zero = ~np.asarray(x).astype(np.float32).any(axis=1)
    assert not got[zero].any()
    return got


def _merge_model(cs, ci, R):
    """The merge's candidate selection for one query, from its lists: thread t keeps the best 8 of the entries c = t (mod 256); the best R
    of what the threads keep are re-scored.  -> (indices of the re-scored prefix, theta the merge must report)."""
    fs, fi = cs.reshape(-1), ci.reshape(-1)
    valid = fi != kr.EMPTY
    pad = (-len(fs)) % 256
    s2 = np.concatenate([fs, np.full(pad, -np.inf, np.float32)]).reshape(-1, 256)
    i2 = np.concatenate([fi, np.full(pad, kr.EMPTY, np.uint32)]).reshape(-1, 256)
    order = np.lexsort((i2, -s2), axis=0)[:8]                                  # per thread: (score desc, index asc)
    ks, ki = np.take_along_axis(s2, order, 0).reshape(-1), np.take_along_axis(i2, order, 0).reshape(-1)
    o = np.lexsort((ki, -ks))
    pref = ki[o][:R]
    pref = pref[pref != kr.EMPTY]
    outside = valid & ~np.isin(fi, pref)
    full = ci[:, -1] != kr.EMPTY
    theta = np.float32(-np.inf)
    if outside.any():
        theta = max(theta, fs[outside].max())
    if full.any():
        theta = max(theta, cs[full, -1].max())
    return pref, theta, (fs[outside].max() if outside.any() else np.float32(-np.inf))


def _check_search(ctx, db, q, k, must_certify, want_path=None):
    """Cases 1 (queries), 2, 3, 4 and the final answer for one query group; -> figures."""
    n, dim = db.shape
    b = q.shape[0]
    st = _stages(ctx, q, k)
    path = st["path"]
    assert want_path is None or path == want_path, path
    assert path == kr.expected_path(n, dim, b)
    _check_prepared(st, q)
    dbn = _dbn(ctx, n)
    qn = st["qn"][:b]
    exact = kr.exact_scores(qn, dbn)
    pref_scores = kr.path_scores(path, qn, dbn)
    eps_b, acc_b, eps_lib = kr.eps_bound(path, dim), kr.accumulation_bound(path, dim), float(st["eps"])
    assert eps_lib >= eps_b
    R = st["rescored"]
    fig = {"err_exact": 0.0, "err_path": 0.0, "margin": np.inf, "flags": int(st["flag"].sum()), "path": path, "st": st}
    rows = np.arange(n)
    for j in range(b):
        cs, ci = st["cand_s"][j], st["cand_i"][j]
        valid = ci != kr.EMPTY
        # 3: invariants
        assert (ci[valid] < n).all()
        assert len(np.unique(ci[valid])) == valid.sum()
        assert (valid[:, :-1] >= valid[:, 1:]).all()                                      # empty slots trail ...
        assert np.isneginf(cs[~valid]).all() and not np.isinf(cs[valid]).any()            # ... and are exactly (-inf, 0xffffffff)
        both = valid[:, :-1] & valid[:, 1:]
        a, c = cs[:, :-1], cs[:, 1:]
        assert ((a > c) | ((a == c) & (ci[:, :-1] < ci[:, 1:])))[both].all()
        # 2: the certificate's premise
        e1 = np.abs(cs[valid].astype(np.float64) - exact[j, ci[valid]])
        e2 = np.abs(cs[valid].astype(np.float64) - pref_scores[j, ci[valid]])
        if valid.any():
            fig["err_exact"], fig["err_path"] = max(fig["err_exact"], e1.max()), max(fig["err_path"], e2.max())
        # 3: completeness -- a row in no list was dropped by a FULL list, whose tail bounds its approximate score
        absent = np.setdiff1d(rows, ci[valid])
        full = valid[:, -1]
        if len(absent):
            assert full.any(), (j, len(absent))
            assert exact[j, absent].max() <= cs[full, -1].max() + eps_b, (j, exact[j, absent].max(), cs[full, -1].max())
        # 4: the certificate's arithmetic
        pref, theta, best_outside = _merge_model(cs, ci, R)
        ex = exact[j, pref]
        o = np.lexsort((pref, -ex))
        tau = ex[o][k - 1]
        assert abs(st["tau"][j] - tau) <= 1e-12, (j, st["tau"][j], tau)
        assert abs(exact[j, st["tau_idx"][j]] - tau) <= 1e-12 and st["tau_idx"][j] in pref
        assert st["theta"][j] >= best_outside
        assert st["theta"][j] == theta, (j, st["theta"][j], theta)
        assert bool(st["flag"][j]) == (float(st["theta"][j]) + eps_lib >= st["tau"][j]), j
        fig["margin"] = min(fig["margin"], float(st["tau"][j]) - float(st["theta"][j]) - eps_lib)
    print(f"[knn stages] {path} dim {dim} n {n} b {b} k {k}: max |s - exact| {fig['err_exact']:.3e} (bound {eps_b:.3e}), "
          f"max |s - path ref| {fig['err_path']:.3e} (bound {acc_b:.3e}), min(tau - theta - eps) {fig['margin']:.3e}, flagged {fig['flags']}")
    assert fig["err_exact"] <= eps_b
    assert fig["err_path"] <= acc_b
    if must_certify:
        assert fig["flags"] == 0, fig["margin"]
    # the final answer is the oracle's
    ref_i, ref_s = oret.exact_topk(kr.oracle_dbn(db), oret.normalize_queries(q), k)
    assert np.array_equal(st["idx"], ref_i), f"top-k indices differ in {(st['idx'] != ref_i).sum()} places"
    assert np.abs(st["score"] - ref_s).max() <= 1e-6
    return fig


def _random(n, dim, b, seed):
    rng = np.random.default_rng(seed)
    return kr.background(rng, n, dim), (rng.standard_normal((b, dim)) * 0.45).astype(np.float32)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------- 1: preparation
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("dim", [64, 192, 512, 4096])
def test_normalised_rows_and_gather(ctx, dim, dtype):
    for n in (1, 3, 4, 5):
        x = kr.normalisation_edges(n, dim, dtype)
        ctx.db_load(x)
        _check_rows(ctx, x)
        idx = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=ctx.device)
        emb = _np(ctx.db_gather(idx, dim))
        assert np.array_equal(emb, x[::-1].astype(np.float32))                 # bit-equal to the input, fp32 pools included
    # a search over the fp32 pool runs the same checks as every other database (k = 1: three real rows and the zero row)
    x = kr.normalisation_edges(5, dim, dtype)
    ctx.db_load(x)
    q = x[:2].astype(np.float32) * 3.0
    _check_search(ctx, x, q, 1, must_certify=False)


def test_zero_norm_query_is_refused(ctx):
    """A query of norm zero has no direction (oracle/retrieval.py divides by the norm): the search refuses it by name."""
    from rdm_amd import _lib
    db, q = _random(300, 512, 5, 1)
    ctx.db_load(db)
    q[3] = 0.0
    with pytest.raises(_lib.RdmError, match="query 3 has zero norm"):
        ctx.knn(torch.from_numpy(q), 4)
    q2 = np.concatenate([_random(1, 512, 70, 2)[1], np.zeros((1, 512), np.float32)])
    with pytest.raises(_lib.RdmError, match="query 70 has zero norm"):
        ctx.knn(torch.from_numpy(q2), 4)
    idx, _ = ctx.knn(torch.from_numpy(q2[:70]), 4)                                  # the context stays usable
    torch.cuda.synchronize()
    assert np.array_equal(_np(idx).view(np.uint32), oret.exact_topk(oret.normalize_db(db), oret.normalize_queries(q2[:70]), 4)[0])


# ---------------------------------------------------------------------------------------------------------------- 2-5: random data
ONLINE_N = (1, 255, 256, 257, 4097)
ONLINE = [(dim, n, (1, 63, 64)[(i + j) % 3]) for i, dim in enumerate((64, 256, 4096, 512)) for j, n in enumerate(ONLINE_N)]


@pytest.mark.parametrize("dim,n,b", ONLINE, ids=[f"d{d}_n{n}_b{b}" for d, n, b in ONLINE])
def test_online_scan_stages(ctx, dim, n, b):
    db, q = _random(n, dim, b, 1000 + dim + n)
    ctx.db_load(db)
    _check_search(ctx, db, q, min(4, n), must_certify=True, want_path="d512" if dim == 512 else "generic")
    if n == 4097 and dim in (256, 512):                        # the 64-candidate prefix (k > 4)
        _check_search(ctx, db, q[:7], 28, must_certify=True)


def test_generic_scan_third_tile_ring_wrap(ctx):
    """dim 256 at (2 CUs + 1) tiles, the last of one row: block 0 walks three tiles (both LDS ring slots reused across tiles)."""
    n = (2 * _cus() + 1) * 256 - 255
    db, q = _random(n, 256, 64, 5)
    db[n - 1] = (q[9] * 0.7).astype(np.float16)               # the one row of the last tile is query 9's best match
    ctx.db_load(db)
    fig = _check_search(ctx, db, q, 4, must_certify=True, want_path="generic")
    assert fig["st"]["idx"][9, 0] == n - 1


BULK = [(dim, n, b) for dim in (512, 64) for n in (3841, 4096, 4097) for b in (128, 129, 512)]


@pytest.mark.parametrize("dim,n,b", BULK, ids=[f"d{d}_n{n}_b{b}" for d, n, b in BULK])
def test_bulk_scan_stages(ctx, dim, n, b):
    db, q = _random(n, dim, b, 2000 + dim + n + b)
    ctx.db_load(db)
    _check_search(ctx, db, q, 4, must_certify=True, want_path="bulk")
    if n == 4097 and b == 129 and dim == 512:
        _check_search(ctx, db, q, 28, must_certify=True, want_path="bulk")


@pytest.mark.parametrize("dim,n,b", [(512, 4097, 65), (256, 4097, 65), (512, 4097, 513), (64, 3841, 513)])
def test_second_group_reuses_scratch(ctx, dim, n, b):
    """b = 65 (a second online group) and b = 513 (a second bulk launch) through rdm_knn itself: the second group's prepared queries,
    lists and certificate overwrite the first's."""
    db, q = _random(n, dim, b, 3000 + dim + b)
    db[n - 1] = (q[b - 1] * 0.5).astype(np.float16)           # the last query's best match is the last row (ragged tile)
    ctx.db_load(db)
    idx, sc = ctx.knn(torch.from_numpy(q), 4)
    torch.cuda.synchronize()
    assert ctx.knn_last_fallback() == 0
    ref_i, ref_s = oret.exact_topk(oret.normalize_db(db), oret.normalize_queries(q), 4)
    assert np.array_equal(_np(idx).view(np.uint32), ref_i) and ref_i[b - 1, 0] == n - 1
    assert np.abs(_np(sc) - ref_s).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- 2 + 6: hi-word worst case
@pytest.mark.parametrize("path,dim,n,b", [("generic", 256, 4097, 2), ("generic", 4096, 257, 2), ("d512", 512, 4097, 2), ("bulk", 512, 4097, 128)])
def test_hi_word_worst_case(ctx, path, dim, n, b):
    """The 247-hot queries against fp16(q^): the hi-word scans must show ~4.7e-4 (inside eps_bound, outside the 2.4e-4 once assumed); the
    hi + lo scan must NOT -- its lo words are all fp16 subnormals, so a flushing MFMA would show the same 4.7e-4 there."""
    db, q2 = kr.hi_word_worst_case(n, dim)
    q = np.concatenate([q2, _random(1, dim, b - 2, 7)[1]]) if b > 2 else q2
    ctx.db_load(db)
    fig = _check_search(ctx, db, q, 4, must_certify=False, want_path=path)
    st = fig["st"]
    assert st["idx"][0, 0] == 0 and st["idx"][1, 0] == 1
    if path != "generic":
        assert fig["err_exact"] >= 4.6e-4                       # the input does what it was built for
    # generic: _check_search held every score to the accumulation term of the hi + lo reference (6.1e-5 at dim 256): a scan whose MFMA
    # flushed the subnormal lo words would sit 4.7e-4 from it.  (At dim 4096 the accumulation term alone is wider than that.)


# ---------------------------------------------------------------------------------------------------------------- 3: ragged tail
@pytest.mark.parametrize("dim,b", [(512, 3), (256, 3), (512, 128), (64, 130)])
def test_all_negative_ragged_tail(ctx, dim, b):
    """Every real score is negative and the last tile holds one row: a zero-padded row that is scored (0) would win everywhere."""
    n = 4097
    db, q1 = kr.all_negative_case(n, dim)
    q = q1 * np.linspace(0.5, 2.0, b, dtype=np.float32)[:, None]
    ctx.db_load(db)
    fig = _check_search(ctx, db, q, 4, must_certify=False)
    assert (fig["st"]["score"] < 0).all() and (fig["st"]["cand_s"][:b][fig["st"]["cand_i"][:b] != kr.EMPTY] < 0).all()


# ---------------------------------------------------------------------------------------------------------------- 6: must fall back
@pytest.mark.parametrize("path,dim,b", [("generic", 256, 3), ("d512", 512, 3), ("bulk", 512, 128), ("bulk", 64, 128)])
def test_overflow_strides_fall_back(ctx, path, dim, b):
    """The best 28 rows at five strides inside / from one planted tile: some stride fills a lane's list with rows the answer needs (a
    full list whose tail reaches tau - eps), the certificate must flag it, and the answer is the oracle's for every stride."""
    n, k = 4097, 28
    overflowed = flagged = 0
    tiles = (1,) if path != "bulk" else (1, 12)                 # bulk: a tile of two different walkers
    for tile in tiles:
        for stride in kr.OVERFLOW_STRIDES:
            db, q1, planted = kr.overflow_case(n, dim, tile, stride)
            q = q1 * np.linspace(0.5, 2.0, b, dtype=np.float32)[:, None]
            ctx.db_load(db)
            fig = _check_search(ctx, db, q, k, must_certify=False, want_path=path)
            st = fig["st"]
            assert st["idx"][0].tolist() == planted[:k].tolist()
            cs, ci = st["cand_s"][0], st["cand_i"][0]
            full = ci[:, -1] != kr.EMPTY
            hit = bool((cs[full, -1] >= st["tau"][0] - st["eps"]).any())
            print(f"[knn overflow] {path} dim {dim} tile {tile} stride {stride}: overflowed lane {hit}, flag {int(st['flag'][0])}")
            assert not hit or st["flag"][0] == 1
            overflowed += hit
            flagged += int(st["flag"][0])
        assert overflowed >= 1 and flagged >= 1                 # at most four of the five strides may certify
        overflowed = flagged = 0


@pytest.mark.parametrize("path,dim,n,b", [("generic", 256, 4097, 2), ("d512", 512, 4097, 2), ("bulk", 512, 4097, 128), ("bulk", 64, 3841, 128)])
def test_tie_flood(ctx, path, dim, n, b):
    """600 bit-identical rows, two tiles packed with them: the answer is the k lowest indices with bit-equal scores.  The ascending
    insertion of the hi-word scans keeps the lower index on a tie only if its rows arrive in ascending order."""
    db, q1, rows = kr.tie_flood_case(n, dim)
    q = np.concatenate([q1, _random(1, dim, b - 1, 11)[1]])
    ctx.db_load(db)
    for k in (1, 4, 28):
        fig = _check_search(ctx, db, q, k, must_certify=False, want_path=path)
        st = fig["st"]
        assert st["idx"][0].tolist() == rows[:k].tolist()
        assert (st["score"][0].view(np.uint32) == st["score"][0].view(np.uint32)[0]).all()
        assert st["flag"][0] == 1 and ctx.knn_last_fallback() == 1
