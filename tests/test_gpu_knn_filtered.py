"""Filtered retrieval (rdm_knn_filtered, csrc/knn.hip) on the device: the exact top-k over the rows a per-query bitmap allows.

The reference of every case is the oracle on the allowed rows alone, oret.exact_topk(kr.oracle_dbn(db)[allowed], qn, k) with the indices
mapped back through np.flatnonzero(allowed): indices equal, scores within 1e-6 (the bound test_gpu_knn_stages._check_search uses).  The
shapes are the smallest ones of the stage tests, one per scan path and per second query group.  What is held:
  1  random masks (densities 1/2, 1/64, exactly k rows; one shared mask and one mask per query) on every path, k = 4 and 20;
  2  an all-ones mask (tail bits included) gives rdm_knn's answer bit for bit;
  3  every in-tile bit position: 256 one-row masks, the rows over the first, the last full and the ragged last tile;
  4  the best rows disallowed: none of them in any candidate list;
  5  the exact fallback under a mask (tie flood, overflowed lanes): flagged, and still no disallowed row;
  6  short subsets: 0, 1 and k - 1 allowed rows end in (0xffffffff, -inf);
  7  rdm_op_row_mask / rdm_op_row_mask_count against the host packer;  8  refusals leave the context usable;
  9  the Python surface: sample_with_query(db_subset=) against a model whose database holds the subset's rows only, per-sample subsets,
     the ValueError of a subset smaller than k, and the row-sharded searcher on two ranks against the unsharded filtered search."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import retrieval as oret, unet as ounet, vqdecoder as ovq

import _knn_ref as kr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NO_ROW = 0xffffffff
# (path, dim, n, b): the stage tests' smallest shape per path, and the two second-group shapes
SHAPES = [("generic", 256, 4097, 2), ("generic", 4096, 257, 2), ("d512", 512, 4097, 2), ("bulk", 512, 4097, 128), ("bulk", 64, 3841, 128),
          ("d512", 512, 4097, 65), ("bulk", 512, 4097, 513)]
SHAPE_IDS = [f"{p}_d{d}_n{n}_b{b}" for p, d, n, b in SHAPES]
PATH_SHAPES = [("generic", 256, 4097, 2), ("d512", 512, 4097, 2), ("bulk", 512, 4097, 128)]


def _np(t):
    return t.detach().cpu().numpy()


def _random(n, dim, b, seed):
    rng = np.random.default_rng(seed)
    return kr.background(rng, n, dim), (rng.standard_normal((b, dim)) * 0.45).astype(np.float32)


def _masks_tensor(ctx, allowed):
    """bool [m, n] -> int64 [m, words] on the device, through the host packer."""
    from rdm_amd import _lib
    return torch.from_numpy(np.stack([_lib.pack_row_mask(a) for a in np.atleast_2d(allowed)])).to(ctx.device)


def _reference(dbn, q, k, allowed, ids):
    """The oracle on each mask's allowed rows; a mask with fewer than k rows: its rows, then (NO_ROW, -inf)."""
    qn = oret.normalize_queries(q)
    b = q.shape[0]
    ref_i = np.full((b, k), NO_ROW, np.uint32)
    ref_s = np.full((b, k), -np.inf, np.float32)
    allowed = np.atleast_2d(allowed)
    for m in np.unique(ids):
        qs = np.flatnonzero(ids == m)
        rows = np.flatnonzero(allowed[m])
        if not len(rows):
            continue
        i, s = oret.exact_topk(dbn[allowed[m]], qn[qs], k)
        ref_i[qs, :i.shape[1]] = rows[i].astype(np.uint32)
        ref_s[qs, :s.shape[1]] = s
    return ref_i, ref_s


def _check_answer(idx, sc, ref_i, ref_s, allowed, ids, what=""):
    idx, sc = _np(idx).view(np.uint32), _np(sc)
    allowed = np.atleast_2d(allowed)
    real = idx != NO_ROW
    for j in range(idx.shape[0]):
        assert allowed[ids[j]][idx[j][real[j]]].all(), f"{what}: query {j} got a row its mask disallows"
    assert np.array_equal(idx, ref_i), f"{what}: top-k indices differ in {(idx != ref_i).sum()} places"
    assert np.array_equal(np.isneginf(sc), ~real)
    err = np.abs(sc[real] - ref_s[real]).max() if real.any() else 0.0
    print(f"[knn filtered] {what}: max |score - oracle| {err:.3e} (bound 1e-6)")
    assert err <= 1e-6


def _search(ctx, q, k, allow, ids):
    idx, sc = ctx.knn(torch.from_numpy(q), k, allow=allow, mask_of_query=ids)
    torch.cuda.synchronize()
    return idx, sc


# ---------------------------------------------------------------------------------------------------------------- 1: random masks
@pytest.mark.parametrize("k", [4, 20])
@pytest.mark.parametrize("path,dim,n,b", SHAPES, ids=SHAPE_IDS)
def test_random_masks(ctx, path, dim, n, b, k):
    from rdm_amd import _lib
    db, q = _random(n, dim, b, 4000 + dim + n + b)
    ctx.db_load(db)
    assert _lib.knn_select(n, dim, b, k)["path"] == path
    dbn = kr.oracle_dbn(db)
    rng = np.random.default_rng(b + k)
    for density in ("1/2", "1/64", "k rows"):
        for shared in (True, False):
            m = 1 if shared else b
            if density == "k rows":
                allowed = np.zeros((m, n), bool)
                for j in range(m):
                    allowed[j, rng.choice(n, k, replace=False)] = True
            else:
                allowed = rng.random((m, n)) < (0.5 if density == "1/2" else 1.0 / 64)
            # mask ids follow the queries across the 64- and 512-query launches: query j names mask j (shared: none given)
            ids = np.zeros(b, np.int64) if shared else np.arange(b)
            idx, sc = _search(ctx, q, k, _masks_tensor(ctx, allowed), None if shared else ids)
            ref_i, ref_s = _reference(dbn, q, k, allowed, ids)
            _check_answer(idx, sc, ref_i, ref_s, allowed, ids, f"{path} dim {dim} n {n} b {b} k {k} density {density} {'shared' if shared else 'per query'}")
            if density == "k rows":
                assert (_np(idx).view(np.uint32) != NO_ROW).all()


# ---------------------------------------------------------------------------------------------------------------- 2: all ones
@pytest.mark.parametrize("dim,b", [(512, 3), (256, 3), (512, 128), (64, 130)])
def test_all_ones_mask_is_the_plain_search(ctx, dim, b):
    """Every real score is negative and the last tile holds one row: were the bits beyond n honoured, a zero row (score 0) would win."""
    from rdm_amd import _lib
    n = 4097
    db, q1 = kr.all_negative_case(n, dim)
    q = q1 * np.linspace(0.5, 2.0, b, dtype=np.float32)[:, None]
    ctx.db_load(db)
    allow = torch.full((1, _lib.knn_mask_words(n)), -1, dtype=torch.int64, device=ctx.device)       # all ones, the words beyond n too
    for k in (4, 20):
        i0, s0 = ctx.knn(torch.from_numpy(q), k)
        i1, s1 = ctx.knn(torch.from_numpy(q), k, allow=allow)
        torch.cuda.synchronize()
        assert np.array_equal(_np(i0), _np(i1))
        assert np.array_equal(_np(s0).view(np.uint32), _np(s1).view(np.uint32))
        assert (_np(s1) < 0).all()


# ---------------------------------------------------------------------------------------------------------------- 3: every bit position
@pytest.mark.parametrize("path,dim", [("bulk", 512), ("d512", 512), ("generic", 256)])
def test_every_bit_position(ctx, path, dim):
    """k = 1, 256 queries, each with a mask of ONE row: position p of tile p % 16 (the first tile .. the last full one), position 0 in the
    ragged last tile (row n - 1).  The lane-to-row-to-bit mapping of each kernel: the answer must be that row."""
    from rdm_amd import _lib
    n = 4097
    db, q = _random(n, dim, 256, 77 + dim)
    ctx.db_load(db)
    rows = np.array([n - 1] + [(p % 16) * 256 + p for p in range(1, 256)])
    assert sorted(rows % 256) == list(range(256)) and {0, 15, 16} <= set(rows // 256)
    allowed = np.zeros((256, n), bool)
    allowed[np.arange(256), rows] = True
    allow = _masks_tensor(ctx, allowed)
    dbn = kr.oracle_dbn(db)
    groups = [slice(0, 256)] if path == "bulk" else [slice(g, g + 64) for g in range(0, 256, 64)]
    for g in groups:
        assert _lib.knn_select(n, dim, g.stop - g.start, 1)["path"] == path
        ids = np.arange(g.start, g.stop)
        idx, sc = _search(ctx, q[g], 1, allow, ids)
        got = _np(idx).view(np.uint32)[:, 0]
        assert np.array_equal(got, rows[g]), np.flatnonzero(got != rows[g])
        ref_i, ref_s = _reference(dbn, q[g], 1, allowed, ids)
        _check_answer(idx, sc, ref_i, ref_s, allowed, ids, f"{path} bit positions {g.start}..{g.stop - 1}")


# ---------------------------------------------------------------------------------------------------------------- 4: best rows disallowed
def _stages(ctx, q, k, allow, ids):
    st = ctx.knn_stages(torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)), k, allow=allow, mask_of_query=ids)
    torch.cuda.synchronize()
    out = {name: (_np(v) if isinstance(v, torch.Tensor) else v) for name, v in st.items()}
    for name in ("idx", "cand_i", "tau_idx"):
        out[name] = out[name].view(np.uint32)
    return out


def _check_lists(st, b, n, allowed, ids):
    """The list invariants of test_gpu_knn_stages._check_search, and: no candidate of a query is a row its mask disallows."""
    allowed = np.atleast_2d(allowed)
    for j in range(b):
        cs, ci = st["cand_s"][j], st["cand_i"][j]
        valid = ci != kr.EMPTY
        assert (ci[valid] < n).all()
        assert allowed[ids[j]][ci[valid]].all(), f"query {j}: a disallowed row in a candidate list"
        assert len(np.unique(ci[valid])) == valid.sum()
        assert (valid[:, :-1] >= valid[:, 1:]).all()
        assert np.isneginf(cs[~valid]).all() and not np.isinf(cs[valid]).any()
        both = valid[:, :-1] & valid[:, 1:]
        a, c = cs[:, :-1], cs[:, 1:]
        assert ((a > c) | ((a == c) & (ci[:, :-1] < ci[:, 1:])))[both].all()


@pytest.mark.parametrize("path,dim,n,b", PATH_SHAPES, ids=[s[0] for s in PATH_SHAPES])
def test_best_rows_disallowed(ctx, path, dim, n, b):
    """64 near-copies (cosine > 0.99) of each of two base queries at random rows -- every query is a scaled base query --, all
    disallowed by the query's mask together with a random half of the background."""
    rng = np.random.default_rng(9 + dim)
    db = kr.background(rng, n, dim)
    base = (rng.standard_normal((2, dim)) * 0.45).astype(np.float32)
    planted = rng.choice(n, 128, replace=False).reshape(2, 64)
    assert len(set(planted.reshape(-1) // 256)) >= 12 and len(set(planted.reshape(-1) % 64)) >= 48      # over tiles and lanes
    for j in range(2):
        db[planted[j]] = (base[j][None] * rng.uniform(0.5, 1.5, (64, 1)) + 0.03 * rng.standard_normal((64, dim))).astype(np.float16)
    q = base[np.arange(b) % 2] * np.linspace(0.5, 2.0, b, dtype=np.float32)[:, None]
    ids = np.arange(b) % 2
    dbn = kr.oracle_dbn(db)
    cos = kr.exact_scores(oret.normalize_queries(base), dbn)
    assert min(cos[0, planted[0]].min(), cos[1, planted[1]].min()) > 0.99
    allowed = rng.random((2, n)) < 0.5
    for j in range(2):
        allowed[j, planted[j]] = False
    ctx.db_load(db)
    allow = _masks_tensor(ctx, allowed)
    for k in (4, 20):
        st = _stages(ctx, q, k, allow, ids)
        assert st["path"] == path
        _check_lists(st, b, n, allowed, ids)
        ref_i, ref_s = _reference(dbn, q, k, allowed, ids)
        assert np.array_equal(st["idx"], ref_i) and np.abs(st["score"] - ref_s).max() <= 1e-6
        assert not np.isin(st["idx"], planted.reshape(-1)).any() and st["score"].max() < 0.9


# ---------------------------------------------------------------------------------------------------------------- 5: fallback under a mask
@pytest.mark.parametrize("path,dim,n,b", [("generic", 256, 4097, 2), ("d512", 512, 4097, 2), ("bulk", 512, 4097, 128), ("bulk", 64, 3841, 128)])
def test_fallback_under_a_mask(ctx, path, dim, n, b):
    """Tie flood with every second tied row disallowed, and overflowed lanes with ladder rows removed: where the merge flags, the exact
    pass answers -- it must test the bit before it scores a row.  The tie flood must flag on every path."""
    db, q1, ties = kr.tie_flood_case(n, dim)
    q = np.concatenate([q1, _random(1, dim, b - 1, 11)[1]])
    allowed = np.ones(n, bool)
    allowed[ties[1::2]] = False
    ctx.db_load(db)
    allow = _masks_tensor(ctx, allowed)
    ids = np.zeros(b, np.int64)
    dbn = kr.oracle_dbn(db)
    flagged = 0
    for k in (4, 28):
        st = _stages(ctx, q, k, allow, None)
        assert st["path"] == path
        _check_lists(st, b, n, allowed, ids)
        ref_i, ref_s = _reference(dbn, q, k, allowed, ids)
        assert np.array_equal(st["idx"], ref_i) and np.abs(st["score"] - ref_s).max() <= 1e-6
        assert st["idx"][0].tolist() == ties[0::2][:k].tolist()
        assert st["flag"][0] == 1 and ctx.knn_last_fallback() == 1
        flagged += int(st["flag"][0])
    assert flagged >= 1
    if n == 4097:
        k, stride = 28, 8
        db, q1, planted = kr.overflow_case(n, dim, 1, stride)
        q = q1 * np.linspace(0.5, 2.0, b, dtype=np.float32)[:, None]
        allowed = np.ones(n, bool)
        allowed[planted[:60:3]] = False                          # every third rung of the ladder's top
        ctx.db_load(db)
        st = _stages(ctx, q, k, _masks_tensor(ctx, allowed), None)
        _check_lists(st, b, n, allowed, ids)
        ref_i, ref_s = _reference(kr.oracle_dbn(db), q, k, allowed, ids)
        print(f"[knn filtered] overflow {path} dim {dim} stride {stride}: flag {int(st['flag'][0])}, fallback {ctx.knn_last_fallback()}")
        assert np.array_equal(st["idx"], ref_i) and np.abs(st["score"] - ref_s).max() <= 1e-6
        assert st["idx"][0].tolist() == [r for r in planted.tolist() if allowed[r]][:k]


# ---------------------------------------------------------------------------------------------------------------- 6: short subsets
@pytest.mark.parametrize("k", [4, 20])
@pytest.mark.parametrize("path,dim,n,b", [("generic", 256, 4097, 8), ("d512", 512, 4097, 8), ("bulk", 512, 4097, 128)], ids=["generic", "d512", "bulk"])
def test_short_subsets(ctx, path, dim, n, b, k):
    from rdm_amd import _lib
    db, q = _random(n, dim, b, 600 + dim + b)
    ctx.db_load(db)
    assert _lib.knn_select(n, dim, b, k)["path"] == path
    rng = np.random.default_rng(k)
    allowed = np.zeros((4, n), bool)
    counts = (0, 1, k - 1, n)
    for m, c in enumerate(counts):
        allowed[m, rng.choice(n, c, replace=False)] = True
    ids = np.arange(b) % 4
    idx, sc = _search(ctx, q, k, _masks_tensor(ctx, allowed), ids)           # the call succeeds
    ref_i, ref_s = _reference(kr.oracle_dbn(db), q, k, allowed, ids)
    _check_answer(idx, sc, ref_i, ref_s, allowed, ids, f"{path} short subsets k {k}")
    got_i, got_s = _np(idx).view(np.uint32), _np(sc)
    for j in range(b):
        c = min(counts[ids[j]], k)
        assert (got_i[j, :c] != NO_ROW).all() and (got_i[j, c:] == NO_ROW).all() and np.isneginf(got_s[j, c:]).all()
    assert np.array_equal(ctx.row_mask_count(_masks_tensor(ctx, allowed)), counts)


# ---------------------------------------------------------------------------------------------------------------- 7: mask builder
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_row_mask_and_count(ctx, n):
    from rdm_amd import _lib
    ctx.db_load(_random(n, 64, 1, n)[0])
    rng = np.random.default_rng(n)
    rows = rng.integers(0, n, size=max(1, n // 3))
    rows = np.concatenate([rows, rows[: len(rows) // 2], [n - 1, 0]])          # duplicates, the first and the last row
    want = np.zeros(n, bool)
    want[rows] = True
    for invert in (False, True):
        exp = _lib.pack_row_mask(~want if invert else want)
        for given in (rows, torch.from_numpy(rows).to(ctx.device), want, torch.from_numpy(want)):
            bits = ctx.row_mask(given, invert=invert)
            torch.cuda.synchronize()
            assert bits.dtype == torch.int64 and bits.shape == (_lib.knn_mask_words(n),)
            assert np.array_equal(_np(bits), exp)
    assert np.array_equal(_np(ctx.row_mask(np.zeros(0, np.int64))), _lib.pack_row_mask(np.zeros(n, bool)))
    both = torch.stack([ctx.row_mask(rows), ctx.row_mask(rows, invert=True), torch.full_like(ctx.row_mask(rows), -1)])
    assert ctx.row_mask_count(both).tolist() == [int(want.sum()), n - int(want.sum()), n]        # bits at or beyond n do not count
    for bad in ([n], [-1], [0, n + 70000]):
        with pytest.raises(_lib.RdmError, match="outside"):
            ctx.row_mask(np.array(bad))
    assert np.array_equal(_np(ctx.row_mask(rows)), _lib.pack_row_mask(want))        # and the context stays usable


# ---------------------------------------------------------------------------------------------------------------- 8: refusals
def test_refusals_leave_the_context_usable(ctx):
    from rdm_amd import _lib
    n, dim, b, k = 4097, 512, 5, 4
    db, q = _random(n, dim, b, 31)
    ctx.db_load(db)
    ref_i = oret.exact_topk(oret.normalize_db(db), oret.normalize_queries(q), k)[0]
    qt = torch.from_numpy(q).to(ctx.device)
    allow = torch.full((2, _lib.knn_mask_words(n)), -1, dtype=torch.int64, device=ctx.device)
    idx = torch.empty((b, k), device=ctx.device, dtype=torch.int32)
    sc = torch.empty((b, k), device=ctx.device, dtype=torch.float32)

    def still_fine():
        got, _ = ctx.knn(qt, k)
        torch.cuda.synchronize()
        assert np.array_equal(_np(got).view(np.uint32), ref_i)

    def err():
        return _lib.lib.rdm_last_error(ctx._h).decode()

    def raw(allow_ptr, n_masks, ids):
        ids_p = None if ids is None else np.asarray(ids, np.int32).ctypes.data_as(C.c_void_p)
        return _lib.lib.rdm_knn_filtered(ctx._h, qt.data_ptr(), b, k, allow_ptr, n_masks, ids_p, idx.data_ptr(), sc.data_ptr())

    assert raw(None, 1, None) != 0 and "null mask" in err()
    still_fine()
    assert raw(allow.data_ptr(), 0, None) != 0 and "n_masks" in err()
    still_fine()
    assert raw(allow.data_ptr(), 2, [0, 1, 0, 2, 0]) != 0 and "query 3 names mask 2" in err()
    still_fine()
    assert raw(allow.data_ptr(), 2, [0, -1, 0, 1, 0]) != 0 and "query 1 names mask -1" in err()
    still_fine()
    with pytest.raises(_lib.RdmError, match="query 3 names mask 2"):
        ctx.knn(qt, k, allow=allow, mask_of_query=[0, 1, 0, 2, 0])
    with pytest.raises(_lib.RdmError, match="mask_of_query needs allow"):
        ctx.knn(qt, k, mask_of_query=[0] * b)
    with pytest.raises(_lib.RdmError, match="allow must be"):
        ctx.knn(qt, k, allow=allow[:, :-1])
    q0 = q.copy()
    q0[2] = 0.0
    with pytest.raises(_lib.RdmError, match="query 2 has zero norm"):
        ctx.knn(torch.from_numpy(q0), k, allow=allow, mask_of_query=[0, 1, 0, 1, 0])
    still_fine()
    got, _ = ctx.knn(qt, k, allow=allow, mask_of_query=[0, 1, 0, 1, 0])               # and a filtered search after the refusals
    torch.cuda.synchronize()
    assert np.array_equal(_np(got).view(np.uint32), ref_i)


# ---------------------------------------------------------------------------------------------------------------- 9: surface
def _tiny_model(ctx):
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    spec, vspec = ounet.tiny_spec(), ovq.tiny_vq_spec()
    unet = dict(in_channels=spec.in_channels, out_channels=spec.out_channels, model_channels=spec.model_channels,
                num_res_blocks=spec.num_res_blocks, attention_resolutions=spec.attention_resolutions, channel_mult=spec.channel_mult,
                num_head_channels=spec.num_head_channels, context_dim=spec.context_dim)
    fs = {"params": {"embed_dim": 3, "n_embed": vspec.n_embed, "ddconfig": {"z_channels": 3, "ch": vspec.ch, "ch_mult": vspec.ch_mult,
                                                                          "num_res_blocks": vspec.num_res_blocks, "resolution": vspec.resolution}}}
    m = MinimalRETRODiffusion(unet_config={"params": unet}, first_stage_config=fs, k_nn=4, image_size=16, ctx=ctx)
    m.load_unet_state_dict(ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234))
    m.load_first_stage_state_dict(ounet.synth_state_dict(ovq.vq_param_shapes(vspec), seed=5))
    return m


def _surface_pool(n=5003):
    rng = np.random.default_rng(57)
    pool = {"embedding": (rng.standard_normal((n, 512)) * 0.45).astype(np.float16), "img_id": np.arange(n) * 3,
            "patch_coords": rng.integers(0, 1200, (n, 4))}
    subsets = {"style": np.sort(rng.choice(n, 700, replace=False)), "low": np.arange(40, 900, 3),       # "low": inside the first of two shards
               "tiny": np.array([5, 4000, 77])}
    qs = (rng.standard_normal((4, 512)) * 0.45).astype(np.float32)
    return pool, subsets, qs


def test_sampling_from_a_subset(ctx):
    """sample_with_query(db_subset=S) == a model whose database holds S's rows only (deterministic mode, same x_T, same k), bit for bit;
    a list of per-sample subsets gives each sample what it gets alone; a subset smaller than k is a ValueError."""
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    was = ctx.deterministic
    ctx.set_deterministic(True)
    try:
        m = _tiny_model(ctx)
        pool, subsets, qs = _surface_pool()
        rng = np.random.default_rng(3)
        x_T = torch.from_numpy(rng.standard_normal((4, 3, 16, 16)).astype(np.float32))
        kw = dict(query_embedded=True, k_nn=4, ddim=True, ddim_steps=4, unconditional_guidance_scale=2.0, unconditional_retro_guidance_label=0.)
        db = DatasetBuilder(data_pool=pool, k=4, ctx=ctx)
        for name, rows in subsets.items():
            db.define_subset(name, rows)                                  # before train_searcher: built there
        db.train_searcher()
        assert db.subsets() == {"style": 700, "low": len(subsets["low"]), "tiny": 3}
        m.retriever = db
        full = m.sample_with_query(query=torch.from_numpy(qs), x_T=x_T, **kw)["query_samples"]
        got = {name: m.sample_with_query(query=torch.from_numpy(qs), x_T=x_T, db_subset=name, **kw)["query_samples"] for name in ("style", "low")}
        nn = db.search_k_nearest(qs, k=4, query_embedded=True, subset="style")
        assert np.isin(nn["nns"], subsets["style"]).all()
        mixed_names = ["style", None, "low", "style"]
        mixed = m.sample_with_query(query=torch.from_numpy(qs), x_T=x_T, db_subset=mixed_names, **kw)["query_samples"]
        for j, name in enumerate(mixed_names):
            alone = m.sample_with_query(query=torch.from_numpy(qs[j:j + 1]), x_T=x_T[j:j + 1], db_subset=name, **kw)["query_samples"]
            assert torch.equal(mixed[j:j + 1], alone), (j, name)
            assert torch.equal(mixed[j], (full if name is None else got[name])[j])
        with pytest.raises(ValueError, match=r"subset 'tiny' allows 3 rows, fewer than k = 4"):
            db.search_k_nearest(qs, k=4, query_embedded=True, subset="tiny")
        with pytest.raises(ValueError, match="tiny"):
            m.sample_with_query(query=torch.from_numpy(qs), x_T=x_T, db_subset=[None, "tiny", None, None], **kw)
        assert db.search_k_nearest(qs, k=3, query_embedded=True, subset="tiny")["nns"].shape == (4, 3)
        with pytest.raises(KeyError):
            db.search_k_nearest(qs, k=4, query_embedded=True, subset="nope")
        # sample_from_rdata: the pseudo-queries are database rows as before, only their neighbours come from the subset
        rkw = dict(qids=np.array([1, 2, 3, 4]), x_T=x_T, k_nn=4, ddim=True, ddim_steps=4, unconditional_guidance_scale=2.0,
                   unconditional_retro_guidance_label=0.)
        rd = m.sample_from_rdata(4, db_subset="style", **rkw)["samples_with_sampled_nns"]
        nn_rd = db.search_k_nearest(pool["embedding"][rkw["qids"]], k=4, query_embedded=True, subset="style")
        assert np.isin(nn_rd["nns"], subsets["style"]).all()
        given = torch.from_numpy(np.asarray(nn_rd["embeddings"])).to(m.device).to(torch.float)
        assert torch.equal(rd, m.sample_from_rdata(4, nn_embeddings=given, **rkw)["samples_with_sampled_nns"])
        assert not torch.equal(rd, m.sample_from_rdata(4, **rkw)["samples_with_sampled_nns"])
        for name in ("style", "low"):                                     # the database of S's rows only
            only = DatasetBuilder(data_pool={key: v[subsets[name]] for key, v in pool.items()}, k=4, ctx=ctx)
            only.train_searcher()
            m.retriever = only
            ref = m.sample_with_query(query=torch.from_numpy(qs), x_T=x_T, **kw)["query_samples"]
            assert torch.equal(got[name], ref), name
            assert not torch.equal(got[name], full)
        db.train_searcher()                                               # the session context gets the whole pool back; the masks are rebuilt
        assert np.array_equal(db.search_k_nearest(qs, k=4, query_embedded=True, subset="style")["nns"], nn["nns"])
    finally:
        ctx.set_deterministic(was)


def _sharded_filter_worker(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from rdm_amd import _lib, parallel
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    r, local = parallel.init_distributed("gloo")
    ctx = _lib.Context(local)
    pool, subsets, qs = _surface_pool()
    db = DatasetBuilder(data_pool=pool, k=20, ctx=ctx).shard_rows(True)
    db.train_searcher()
    for name, rows in subsets.items():
        db.define_subset(name, rows)
    out = [db.search_k_nearest(qs, k=20, query_embedded=True, subset=s) for s in ("style", "low", ["style", None, "low", "style"])]
    short = db.searcher.search_batched(qs, final_num_neighbors=20, allow=db._subsets["tiny"]["mask"][None])
    rows = ctx.db_size()
    torch.cuda.synchronize(); ctx.close()
    if r == 0:
        q.put(([(o["nns"], o["distances"]) for o in out], short, rows))
    parallel.shutdown()


def test_row_sharded_filtered_search(ctx):
    """Two ranks on the one GPU (gloo), the database rows halved: every rank passes its own local masks, the pad-and-merge takes the
    library's 0xffffffff entries as "no row".  Equal to the unsharded filtered search and to the oracle; "low" lies in rank 0's rows."""
    import torch.multiprocessing as mp
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_sharded_filter_worker, args=(r, 2, 29694, q)) for r in range(2)]
    for p in procs: p.start()
    got, short, rows = q.get(timeout=600)
    for p in procs: p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs)
    pool, subsets, qs = _surface_pool()
    n = len(pool["embedding"])
    assert rows == (n + 1) // 2 and subsets["low"].max() < rows
    db = DatasetBuilder(data_pool=pool, k=20, ctx=ctx)
    db.train_searcher()
    for name, r in subsets.items():
        db.define_subset(name, r)
    dbn = kr.oracle_dbn(pool["embedding"])
    member = {name: np.isin(np.arange(n), r) for name, r in subsets.items()}
    for (nns, dist), s in zip(got, ("style", "low", ["style", None, "low", "style"])):
        one = db.search_k_nearest(qs, k=20, query_embedded=True, subset=s)
        assert np.array_equal(nns, one["nns"]) and np.array_equal(dist, one["distances"])
        names = [s] * 4 if isinstance(s, str) else s
        for j, name in enumerate(names):
            allowed = member[name] if name is not None else np.ones(n, bool)
            ref_i, ref_s = _reference(dbn, qs[j:j + 1], 20, allowed, np.zeros(1, np.int64))
            assert np.array_equal(nns[j:j + 1], ref_i) and np.abs(dist[j:j + 1] - ref_s).max() <= 1e-6
    ref_i, ref_s = _reference(dbn, qs, 20, member["tiny"], np.zeros(4, np.int64))         # three rows over two shards, then "no row"
    assert np.array_equal(short[0], ref_i) and np.isneginf(short[1][:, 3:]).all() and np.abs(short[1][:, :3] - ref_s[:, :3]).max() <= 1e-6


def test_rdm_sample_script_db_subset(tmp_path):
    """scripts/rdm_sample.py --db_subset: an index file and the inverted boolean file of its complement name the same subset and give the
    same PNGs, other PNGs than the whole database gives, and every retrieved neighbour is a row of the subset."""
    import importlib.util
    import os
    from PIL import Image
    spec = importlib.util.spec_from_file_location("rdm_sample_db_subset", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                      "scripts", "rdm_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = 20000
    rows = np.sort(np.random.default_rng(8).choice(n, 300, replace=False))
    np.save(tmp_path / "rows.npy", rows)
    np.save(tmp_path / "others.npy", ~np.isin(np.arange(n), rows))
    base = ["--synthetic", "--synthetic_db_rows", str(n), "--gpu", "0", "-bs", "2", "-n", "1", "--steps", "4", "--seed", "3", "-c", "a painting of a fox"]
    runs = {"whole": [], "rows": ["--db_subset", str(tmp_path / "rows.npy")],
            "others inverted": ["--db_subset", str(tmp_path / "others.npy"), "--db_subset_invert"]}
    model, px = None, {}
    for name, extra in runs.items():
        out = tmp_path / name.replace(" ", "_")
        out.mkdir()
        opt = mod.parse_args(base + extra + ["-s", str(out)])
        if model is None:
            model = mod.load_model(opt)
        model.retriever._subsets.clear()                                 # a fresh process defines the subset of its own command line
        mod.sample_conditional(model, opt)
        px[name] = [np.asarray(Image.open(f)) for f in sorted(out.iterdir())]
        assert len(px[name]) == 2
    assert model.retriever.subsets() == {mod.DB_SUBSET_NAME: 300}
    assert all(np.array_equal(a, b) for a, b in zip(px["rows"], px["others inverted"]))
    assert not np.array_equal(px["rows"][0], px["whole"][0])
    from rdm_amd.modules.custom_clip.tokenizer import tokenize
    q = model.retriever.retriever.model.encode_text(torch.from_numpy(tokenize(["a painting of a fox"] * 2))).cpu()
    nn = model.retriever.search_k_nearest(q, k=4, query_embedded=True, subset=mod.DB_SUBSET_NAME)
    assert np.isin(nn["nns"], rows).all()
    model.ctx.close()
