"""The neighbour bias without a GPU: the C ABI's new symbols and their arities, the references of tests/_nnbias_ref.py held to their own
bounds by an fp32 stand-in (and told apart from every near miss), the biased oracle restatement against the plain oracle on the kept
neighbours alone, and the host logic -- nn_counts / nn_weights -> bias, tiling, the rank cut, short subsets, every refusal, the script's
two flags."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from oracle import unet as ounet

import _fwd_ref as R
import _nnbias_ref as N
from _train_ref import check, standin
from _util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")
torch.set_grad_enabled(False)
torch.set_num_threads(min(16, torch.get_num_threads()))


# ------------------------------------------------------------------------------------------------ the C ABI
def _declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdm_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/rdm_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,arity", [("rdm_set_neighbour_bias", 4), ("rdm_get_neighbour_bias", 3), ("rdm_op_xattn_fused_biased", 20),
                                        ("rdm_op_small_attention_biased", 16)])
def test_new_symbols_are_declared_exported_and_bound(name, arity):
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    assert len(_declared(name)) == arity
    assert hasattr(_lib.lib, name), f"librdm_hip.so does not export {name}"
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == arity


def test_biased_entries_extend_the_old_ones_and_the_old_ones_keep_their_signatures():
    from rdm_amd import _lib
    assert len(_declared("rdm_op_xattn_fused")) == 16 and len(_declared("rdm_op_xattn_fused_ln3")) == 17 and len(_declared("rdm_op_small_attention")) == 15
    assert _declared("rdm_op_small_attention_biased")[:15] == _declared("rdm_op_small_attention")
    assert "key_bias" in _declared("rdm_op_small_attention_biased")[-1] and "key_bias" in _declared("rdm_op_xattn_fused_biased")[-1]
    assert _lib.SIGNATURES["rdm_op_small_attention_biased"][1][:15] == _lib.SIGNATURES["rdm_op_small_attention"][1]


def test_sampler_argument_structs_keep_their_layout():
    """The bias does not travel in rdm_ddim_args: the struct of the header and the binding's are what they were."""
    from rdm_amd import _lib
    src = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    body = re.search(r"typedef struct\s*(?:rdm_ddim_args)?\s*\{(.*?)\}\s*rdm_ddim_args\s*;", src, flags=re.S).group(1)
    assert "bias" not in body
    names = [f[0] for f in _lib.DdimArgs._fields_]
    assert not any("bias" in n for n in names)
    assert names[:5] == ["batch", "k", "channels", "height", "width"] or {"batch", "k", "channels", "height", "width"} <= set(names)


# ------------------------------------------------------------------------------------------------ the references hold their own bounds
_FUSED = [(2, 32, 2, 4, ("finite", "first")), (2, 32, 2, 4, ("one", "finite")), (2, 96, 6, 2, ("finite", "first")),
          (2, 96, 6, 2, ("one", "finite")), (2, 32, 30, 4, ("finite", "first")), (2, 32, 30, 4, ("one", "finite"))]


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("B,n,heads,k,patterns", _FUSED, ids=[f"n{c[1]}-h{c[2]}-k{c[3]}-{'+'.join(c[4])}" for c in _FUSED])
def test_fused_reference_bound_and_near_misses(B, n, heads, k, patterns, ln):
    inp = N.XattnFusedBiased.make(B, n, heads, k, patterns, ln=ln)
    worst, margin = check(N.XattnFusedBiased, inp, standin(N.XattnFusedBiased, inp, lambda *a: True))
    print(f"fp32 stand-in: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    P = N.XattnFusedBiased.probs(inp, torch.float64)
    if "one" in patterns:                        # all but one masked: probabilities exactly 1 and 0
        b0 = patterns.index("one")
        assert set(P[b0].unique().tolist()) == {0.0, 1.0}


_SMALL = [dict(B=2, nq=16, nkv=3, H=4, D=32, masked=[[0], [1, 2]]), dict(B=2, nq=50, nkv=16, H=6, D=32, masked=[[0, 5, 15], []]),
          dict(B=2, nq=40, nkv=300, H=2, D=32, masked=[[0, 100, 254, 255, 256, 257, 299], list(range(256, 300))])]


@pytest.mark.parametrize("kw", _SMALL, ids=["k3-first-masked", "k16-odd-queries", "k300-two-chunks"])
def test_small_attention_reference_bound_and_near_misses(kw):
    inp = N.SmallAttentionBiased.make(**kw)
    worst, margin = check(N.SmallAttentionBiased, inp, standin(N.SmallAttentionBiased, inp, lambda *a: True))
    print(f"fp32 stand-in: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def test_zero_bias_references_are_the_unbiased_ones():
    inp = N.XattnFusedBiased.make(2, 32, 2, 4, ("zero", "zero"))
    assert torch.equal(N.XattnFusedBiased.ref(inp, torch.float64)["out"], R.XattnFused.ref(inp, torch.float64)["out"])
    si = N.SmallAttentionBiased.make(B=2, nq=8, nkv=5, H=2, D=32, masked=[[], []])
    si["key_bias"] = torch.zeros(2, 5)
    assert torch.equal(N.SmallAttentionBiased.ref(si, torch.float64)["out"], R.SmallAttention.ref(si, torch.float64)["out"])


# ------------------------------------------------------------------------------------------------ the oracle restatement
def test_biased_oracle_is_the_plain_oracle_on_the_kept_neighbours(monkeypatch):
    """Row [0, 0, -inf, -inf] at k = 4 against the same sample at k = 2 (measured <= 2.1e-6 relative L2: held to 1e-5); and a zero bias is
    the plain oracle bit for bit."""
    spec = ounet.tiny_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234)
    g = torch.Generator().manual_seed(3)
    x, t, c = torch.randn(2, 3, 16, 16, generator=g), torch.tensor([500, 37]), torch.randn(2, 4, 512, generator=g)
    plain4 = ounet.unet_forward(sd, spec, x, t, c)
    plain2 = ounet.unet_forward(sd, spec, x, t, c[:, :2].contiguous())
    with monkeypatch.context() as mp:
        mp.setattr(ounet, "cross_attention", N.biased_cross_attention([[0.0, 0.0, NEG, NEG]] * 2))
        masked = ounet.unet_forward(sd, spec, x, t, c)
    with monkeypatch.context() as mp:
        mp.setattr(ounet, "cross_attention", N.biased_cross_attention(torch.zeros(2, 4)))
        zero = ounet.unet_forward(sd, spec, x, t, c)
    e = rel_l2(masked, plain2)
    print(f"biased oracle at k = 4, two masked, vs plain oracle at k = 2: {e:.3e}; vs plain at k = 4: {rel_l2(masked, plain4):.3e}")
    assert e <= 1e-5
    assert rel_l2(masked, plain4) > 0.1
    assert torch.equal(zero, plain4)
    assert ounet.cross_attention.__module__ == "oracle.unet"       # the replacement is gone


# ------------------------------------------------------------------------------------------------ host logic
def test_counts_and_weights_become_the_bias():
    from rdm_amd.util import neighbour_bias_from
    assert neighbour_bias_from(3, 4) is None
    b = neighbour_bias_from(2, 4, nn_counts=[4, 1])
    assert torch.equal(b, torch.tensor([[0.0, 0, 0, 0], [0.0, NEG, NEG, NEG]]))
    assert torch.equal(neighbour_bias_from(3, 4, nn_counts=2), torch.tensor([[0.0, 0, NEG, NEG]] * 3))
    w = neighbour_bias_from(2, 4, nn_weights=[[4, 1, 1, 0.25], [1, 0, 2, 0]])
    assert torch.allclose(w[0], torch.log(torch.tensor([4.0, 1, 1, 0.25]))) and w[1].tolist() == [0.0, NEG, pytest.approx(np.log(2.0)), NEG]
    assert torch.equal(neighbour_bias_from(2, 3, nn_weights=[1.0, 2.0, 0.0]), torch.log(torch.tensor([[1.0, 2.0, 0.0]] * 2)))
    both = neighbour_bias_from(1, 4, nn_counts=[3], nn_weights=[[2.0, 1, 1, 5]])
    assert both[0, 3] == NEG and both[0, 0] == pytest.approx(np.log(2.0))
    # tiling under n_reps: like torch.cat([retro_cond] * n_reps, dim=1)
    t = neighbour_bias_from(2, 4, nn_counts=[4, 1], n_reps=3)
    assert tuple(t.shape) == (2, 12) and torch.equal(t, torch.cat([b] * 3, dim=1))
    assert b.dtype == torch.float32 and b.is_contiguous()


@pytest.mark.parametrize("kw,word", [(dict(nn_counts=[4, 0]), "lie in"), (dict(nn_counts=[5, 1]), "lie in"), (dict(nn_counts=[1, 2, 3]), "one per sample"),
                                     (dict(nn_counts=[1.5, 2]), "one per sample"), (dict(nn_weights=[[1, 1, 1, 1]]), "must be"),
                                     (dict(nn_weights=[[1, -1, 1, 1]] * 2), "non-negative"), (dict(nn_weights=[[1, float("nan"), 1, 1]] * 2), "finite"),
                                     (dict(nn_weights=[[1, float("inf"), 1, 1]] * 2), "finite"), (dict(nn_weights=[[1, 1, 1, 1], [0, 0, 0, 0]]), "no finite entry"),
                                     (dict(nn_counts=[2, 2], nn_weights=[[1, 1, 1, 1], [0, 0, 1, 1]]), "no finite entry")])
def test_counts_and_weights_refusals(kw, word):
    from rdm_amd.util import neighbour_bias_from
    with pytest.raises(ValueError, match=word):
        neighbour_bias_from(2, 4, **kw)


@pytest.mark.parametrize("bias,word", [([[0.0, float("nan")]], "NaN"), ([[0.0, float("inf")]], "inf"), ([[0.0, 0.0], [NEG, NEG]], "no finite entry"),
                                       ([0.0, 1.0], "must be"), ([[0.0, 0.0, 0.0]], "must be")])
def test_bias_refusals_of_the_python_surface(bias, word):
    from rdm_amd.util import check_neighbour_bias
    with pytest.raises(ValueError, match=word):
        check_neighbour_bias(bias, None if np.ndim(bias) != 2 or len(bias[0]) != 3 else 1, 2)
    ok = check_neighbour_bias([[0.0, NEG], [1.0, -2.0]], 2, 2)
    assert ok.dtype == torch.float32 and ok.tolist() == [[0.0, NEG], [1.0, -2.0]]


class _FakeCtx:
    """records what the sampling methods set on the native context"""
    def __init__(self):
        self.log, self.bias = [], None

    def neighbour_bias(self, bias):
        import contextlib

        @contextlib.contextmanager
        def cm():
            self.bias = bias
            self.log.append(("set", None if bias is None else bias.clone()))
            try:
                yield
            finally:
                self.bias = None
                self.log.append(("clear", None))
        return cm()


def test_sampling_methods_set_the_bias_around_the_call_and_clear_it():
    from rdm_amd.util import takes_neighbour_bias

    class S:
        def __init__(self):
            self.ctx = _FakeCtx()

        @takes_neighbour_bias(lambda s: s.ctx)
        def sample(self, a, fail=False):
            assert (self.ctx.bias is not None) == bool(a)
            if fail:
                raise RuntimeError("boom")
            return a

    s = S()
    assert s.sample(0) == 0 and s.ctx.log == []                        # without a bias the context is not touched
    assert s.sample(1, neighbour_bias=[[0.0, NEG]]) == 1
    assert [e[0] for e in s.ctx.log] == ["set", "clear"] and s.ctx.log[0][1].tolist() == [[0.0, NEG]]
    with pytest.raises(RuntimeError):
        s.sample(1, fail=True, neighbour_bias=[[0.0, 0.0]])
    assert s.ctx.log[-1][0] == "clear" and s.ctx.bias is None
    with pytest.raises(ValueError, match="no finite entry"):
        s.sample(1, neighbour_bias=[[NEG, NEG]])
    from rdm_amd.models.diffusion import ddim, ddpm, dpm_solver, plms, uni_pc
    import inspect
    for fn in (ddim.DDIMSampler.sample, ddim.DDIMSampler.decode, ddim.DDIMSampler.encode, plms.PLMSSampler.sample, dpm_solver.DPMSolverSampler.sample,
               dpm_solver.DPMSolverSDESampler.sample, uni_pc.UniPCSampler.sample, ddpm.MinimalRETRODiffusion.sample_log,
               ddpm.MinimalRETRODiffusion.sample, ddpm.MinimalRETRODiffusion.p_sample_loop):
        assert "neighbour_bias" in inspect.signature(fn, follow_wrapped=False).parameters, fn.__qualname__


# ---- the model surface on a stand-in retriever and a stand-in sample_log
def _surface_model(k_nn=4, rows=40, distributed=None):
    from rdm_amd import _lib
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    rng = np.random.default_rng(0)
    pool = {"embedding": rng.standard_normal((rows, 16)).astype(np.float32), "img_id": np.arange(rows), "patch_coords": np.zeros((rows, 4), np.int64)}
    db = DatasetBuilder(data_pool=pool, k=k_nn)

    class Searcher:
        """exact search over the allowed rows; NO_ROW where a subset runs out (what the library returns)"""
        row0, sharded, n_local = 0, False, rows

        def search_batched(self, q, final_num_neighbors=None, allow=None, mask_of_query=None):
            sc = np.asarray(q, np.float32) @ pool["embedding"].T
            k = final_num_neighbors
            idx = np.full((len(sc), k), _lib.NO_ROW, dtype=np.uint32)
            dist = np.full((len(sc), k), -np.inf, dtype=np.float32)
            for b in range(len(sc)):
                ok = np.arange(rows) if allow is None or allow[mask_of_query[b]] is None else allow[mask_of_query[b]]
                order = ok[np.argsort(-sc[b, ok], kind="stable")][:k]
                idx[b, : len(order)] = order; dist[b, : len(order)] = sc[b, order]
            return idx, dist
    db.searcher = Searcher()
    db._subset_filter = lambda subset, b: ([None if nm is None else db._subsets[nm]["rows"] for nm in ([subset] * b if subset is None or isinstance(subset, str) else subset)],
                                           np.arange(b), [subset] * b if subset is None or isinstance(subset, str) else list(subset))
    db._subsets = {"two": {"rows": np.array([3, 7]), "mask": None}, "none": {"rows": np.array([], dtype=np.int64), "mask": None},
                   "many": {"rows": np.arange(10, 30), "mask": None}}
    m = MinimalRETRODiffusion.__new__(MinimalRETRODiffusion)
    m.retriever, m.k_nn, m.device, m.distributed = db, k_nn, torch.device("cpu"), distributed is not None
    m.retrieval_encoder = lambda t: t
    m._sync_retriever_sharding = lambda: None
    m._latent_shape = lambda cs: (3, 8, 8)
    m.get_unconditional_conditioning = lambda shape, **kw: torch.zeros(shape)
    m.decode_first_stage = lambda z: z
    if distributed is not None:
        m._shard = lambda n: distributed
        m.shard_db = False
    calls = []

    def sample_log(cond, batch_size, **kw):
        calls.append(dict(kw, cond=cond, batch_size=batch_size))
        return torch.zeros(batch_size, 3, 8, 8), None
    m.sample_log = sample_log
    m._sample_shard = lambda c, cu, lo, hi, n, scale, kw, dn=False: sample_log(c, hi - lo, **kw)[0]
    return m, db, pool, calls


def test_short_ok_fills_zero_embeddings_and_counts():
    from rdm_amd import _lib
    m, db, pool, _ = _surface_model()
    q = np.random.default_rng(1).standard_normal((3, 16)).astype(np.float32)
    with pytest.raises(ValueError, match="fewer than k = 4"):
        db.search_k_nearest(q, k=4, query_embedded=True, subset="two")
    out = db.search_k_nearest(q, k=4, query_embedded=True, subset=["two", None, "many"], short_ok=True)
    assert out["counts"].tolist() == [2, 4, 4]
    assert (out["nns"][0, 2:] == _lib.NO_ROW).all() and set(out["nns"][0, :2].tolist()) == {3, 7}
    assert (out["embeddings"][0, 2:] == 0).all() and np.array_equal(out["embeddings"][0, :2], pool["embedding"][out["nns"][0, :2]])
    assert np.array_equal(out["embeddings"][1], pool["embedding"][out["nns"][1]])
    with pytest.raises(ValueError, match="no row at all"):
        db.search_k_nearest(q, k=4, query_embedded=True, subset="none", short_ok=True)
    with pytest.raises(ValueError):
        db.search_subset(q, 4, "none")
    full = db.search_k_nearest(q, k=4, query_embedded=True, subset="many")
    assert "counts" not in full                                       # the default's result is what it was


def test_sample_with_query_passes_the_bias_to_sample_log():
    m, db, pool, calls = _surface_model()
    q = torch.from_numpy(np.random.default_rng(2).standard_normal((3, 16)).astype(np.float32))
    m.sample_with_query(q, query_embedded=True, ddim=True, ddim_steps=2)
    assert "neighbour_bias" not in calls[-1]
    m.sample_with_query(q, query_embedded=True, nn_counts=[4, 2, 1], ddim=True, ddim_steps=2)
    assert calls[-1]["neighbour_bias"].tolist() == [[0.0] * 4, [0.0, 0.0, NEG, NEG], [0.0, NEG, NEG, NEG]]
    m.sample_with_query(q, query_embedded=True, nn_counts=2, n_reps=2, ddim=True, ddim_steps=2)
    assert tuple(calls[-1]["cond"].shape) == (3, 8, 16) and calls[-1]["neighbour_bias"].tolist() == [[0.0, 0.0, NEG, NEG] * 2] * 3
    # a short subset: the query, then the two rows that exist; "mask" masks the fourth place, the default raises
    with pytest.raises(ValueError, match="fewer than k = 4"):
        m.sample_with_query(q, query_embedded=True, db_subset="two", ddim=True, ddim_steps=2)
    m.sample_with_query(q, query_embedded=True, db_subset="two", short_subsets="mask", ddim=True, ddim_steps=2)
    assert calls[-1]["neighbour_bias"].tolist() == [[0.0, 0.0, 0.0, NEG]] * 3 and bool((calls[-1]["cond"][:, 3] == 0).all())
    m.sample_with_query(q, query_embedded=True, db_subset="two", short_subsets="mask", omit_query=True, nn_weights=[2.0, 1.0, 1.0, 1.0], ddim=True, ddim_steps=2)
    assert calls[-1]["neighbour_bias"][0].tolist() == [pytest.approx(np.log(2.0)), 0.0, NEG, NEG]
    m.sample_with_query(q, query_embedded=True, db_subset="many", short_subsets="mask", ddim=True, ddim_steps=2)
    assert "neighbour_bias" not in calls[-1]                            # nothing is short: nothing is masked
    with pytest.raises(ValueError, match="no row at all"):
        m.sample_with_query(q, query_embedded=True, db_subset="none", short_subsets="mask", ddim=True, ddim_steps=2)
    with pytest.raises(ValueError, match="example_maps"):
        m.sample_with_query(q, query_embedded=True, nn_counts=2, example_maps=torch.zeros(3, 16), ddim=True, ddim_steps=2)
    with pytest.raises(ValueError, match="short_subsets"):
        m.sample_with_query(q, query_embedded=True, short_subsets="drop", ddim=True, ddim_steps=2)
    with pytest.raises(ValueError, match="lie in"):
        m.sample_with_query(q, query_embedded=True, nn_counts=[4, 2, 5], ddim=True, ddim_steps=2)


def test_the_rank_cut_takes_its_rows_of_the_bias():
    m, db, pool, calls = _surface_model(distributed=(1, 3))
    q = torch.from_numpy(np.random.default_rng(2).standard_normal((4, 16)).astype(np.float32))
    m.sample_with_query(q, query_embedded=True, nn_counts=[4, 3, 2, 1], ddim=True, ddim_steps=2)
    assert calls[-1]["batch_size"] == 2 and calls[-1]["neighbour_bias"].tolist() == [[0.0, 0.0, 0.0, NEG], [0.0, 0.0, NEG, NEG]]
    m.sample_with_query(q, query_embedded=True, db_subset=[None, "two", None, "two"], short_subsets="mask", ddim=True, ddim_steps=2)
    assert calls[-1]["neighbour_bias"].tolist() == [[0.0, 0.0, 0.0, NEG], [0.0, 0.0, 0.0, 0.0]]


def test_sample_from_rdata_counts_and_short_subsets():
    m, db, pool, calls = _surface_model()
    m.get_qids = lambda memsize, N, qids=None, use_weights=False, verbose=False: np.arange(N)
    m.sample_from_rdata(2, nn_counts=[3, 1], ddim=True, ddim_steps=2)
    assert calls[-1]["neighbour_bias"].tolist() == [[0.0, 0.0, 0.0, NEG], [0.0, NEG, NEG, NEG]]
    with pytest.raises(ValueError, match="fewer than k = 4"):
        m.sample_from_rdata(2, db_subset="two", ddim=True, ddim_steps=2)
    m.sample_from_rdata(2, db_subset="two", short_subsets="mask", ddim=True, ddim_steps=2)
    assert calls[-1]["neighbour_bias"].tolist() == [[0.0, 0.0, NEG, NEG]] * 2 and bool((calls[-1]["cond"][:, 2:] == 0).all())
    m.sample_from_rdata(2, ddim=True, ddim_steps=2)
    assert "neighbour_bias" not in calls[-1]


# ------------------------------------------------------------------------------------------------ scripts/rdm_sample.py
def _script():
    spec = importlib.util.spec_from_file_location("rdm_sample_native_bias", os.path.join(ROOT, "scripts", "rdm_sample.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_the_two_flags_parse_and_the_reference_table_still_matches():
    import json
    from pathlib import Path
    mod = _script()
    opt = mod.parse_args([])
    assert opt.nn_counts is None and opt.short_subsets == "error"
    assert mod.parse_args(["--nn_counts", "3"]).nn_counts == 3
    assert mod.parse_args(["--nn_counts", "4,2,1,1"]).nn_counts == [4, 2, 1, 1]
    assert mod.parse_args(["-bs", "2", "--nn_counts", "4,1", "--db_subset", "x.npy", "--short_subsets", "mask"]).short_subsets == "mask"
    for bad in (["--nn_counts", "4,2"], ["--nn_counts", "5"], ["--nn_counts", "0"], ["--nn_counts", "a"], ["--short_subsets", "mask"],
                ["--db_subset", "x.npy", "--short_subsets", "drop"], ["--only_caption", "--nn_counts", "2"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    kw = mod._sampler_kwargs(mod.parse_args(["--nn_counts", "2"]))
    assert kw == {"nn_counts": 2}
    assert mod._sampler_kwargs(mod.parse_args([])) == {}
    with open(os.path.join(ROOT, "tests", "golden", "rdm_sample_flags.json")) as f:
        ref = json.load(f)
    acts = {tuple(a.option_strings): a for a in mod.build_parser()._actions}
    for e in ref:
        a = acts.get(tuple(e["options"]))
        assert a is not None, f"missing flag {e['options']}"
        if e["action"] == "store_true":
            assert a.const is True and a.default is False and a.nargs == 0
        else:
            assert a.type is {"int": int, "float": float, "str": str, "Path": Path}[e["type"]], e
            assert a.default == e["default"] or str(a.default) == str(e["default"]), e
    assert ("--nn_counts",) not in {tuple(e["options"]) for e in ref} and ("--nn_counts",) in acts and ("--short_subsets",) in acts
