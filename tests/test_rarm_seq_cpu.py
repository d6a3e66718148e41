"""CPU suite of the RARM whole-sequence pass: fp32 restatements of the causal d_head-64 attention and the token-NLL kernel held to the
bounds tests/test_gpu_rarm_seq.py holds the HIP kernels to (tests/_rarm_seq_ref.py), what the LatentImageRETRO mirror computes and hands
down to the context for forward / shared_step / compute_loss / validation_step / nll / training_step, how `prefill` travels from sample,
sampling_util and log_images to rarm_sample, the script's --prefill and --score flags, and the argument errors of the Python layer."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rarm_seq_ref as S
from _train_ref import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(16, torch.get_num_threads()))


# ------------------------------------------------------------------------------------------------ the kernels' references
@pytest.mark.parametrize("shape", S.CAUSAL_SHAPES, ids=["x".join(map(str, s)) for s in S.CAUSAL_SHAPES])
def test_causal_attention_restatement_within_bound_and_near_misses_outside(shape):
    inp = S.CausalAttention.make(*shape)
    worst, margin = check(S.CausalAttention, inp, S.CausalAttention.standin(inp))
    print(f"causal attention {shape}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


@pytest.mark.parametrize("shape", S.NLL_SHAPES, ids=["x".join(map(str, s)) for s in S.NLL_SHAPES])
def test_nll_restatement_within_bound_and_near_miss_outside(shape):
    inp = S.Nll.make(*shape)
    assert int(inp["targets"].min()) == 0 and int(inp["targets"].max()) == shape[1] - 1
    worst, margin = check(S.Nll, inp, S.Nll.standin(inp))
    print(f"nll {shape}: worst error / bound {worst:.3g}, near miss {margin:.3g}")


def test_signatures_declare_the_new_entries():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    for name in ("rdm_rarm_forward_seq", "rdm_rarm_nll", "rdm_rarm_sample_prefill", "rdm_op_causal_attention_d64", "rdm_op_rarm_nll"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name


# ------------------------------------------------------------------------------------------------ the mirror against a fake context
V = 512


class _FakeCtx:
    """Stands in for _lib.Context: deterministic pseudo-logits from the tokens, and a record of every call."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def vq_encode_indices(self, x, return_quant=False):
        b = x.shape[0]
        idx = (torch.arange(b * 4).reshape(b, 4) * 37 + 11) % V
        return torch.zeros((b, 64, 2, 2)), idx

    def _logits(self, tokens, context):
        g = torch.Generator().manual_seed(int(tokens.sum()) % 1000 + int(context.abs().sum() * 10) % 7)
        return torch.randn(tokens.shape + (V,), generator=g)

    def rarm_forward_seq(self, tokens, context):
        self.calls.append(("rarm_forward_seq", tokens.clone(), context.clone()))
        return self._logits(tokens, context)

    def rarm_nll(self, tokens, targets, context):
        self.calls.append(("rarm_nll", tokens.clone(), targets.clone(), context.clone()))
        lg = self._logits(tokens, context)
        return F.cross_entropy(lg.reshape(-1, V), targets.reshape(-1), reduction="none").reshape(targets.shape)

    def rarm_sample(self, cond_tokens, context, steps, uniforms, **kw):
        self.calls.append(("rarm_sample", dict(kw, steps=steps, tc=cond_tokens.shape[1])))
        return torch.zeros((cond_tokens.shape[0], steps), dtype=torch.long)

    def vq_decode_indices(self, idx):
        return torch.zeros((idx.shape[0], 3, 8, 8))


def _mirror(p_mask_max=0.):
    import rdm_amd  # noqa: F401
    from rdm_amd.models.autoregression.transformer import LatentImageRETRO
    fake = _FakeCtx()
    m = LatentImageRETRO({"params": dict(in_channels=514, out_channels=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64)},
                         None, mask_token=512, sos_token=513, ctx=fake, p_mask_max=p_mask_max)
    return m, fake


def _batch(n=3):
    g = torch.Generator().manual_seed(3)
    return {"image": torch.rand((n, 8, 8, 3), generator=g) * 2 - 1, "nn_embeddings": torch.randn((n, 4, 512), generator=g)}


def test_forward_feeds_sos_and_all_but_the_last_code():
    m, fake = _mirror()
    b = _batch()
    x, c = m.get_xc(b)
    r = m.get_r(b)
    logits, target = m.forward(x, c, r)
    _, z = fake.vq_encode_indices(x)
    name, tokens, context = fake.calls[-1]
    assert name == "rarm_forward_seq"
    assert torch.equal(tokens, torch.cat([torch.full((3, 1), 513), z], 1)[:, :-1])
    assert torch.equal(context, r) and torch.equal(target, z)
    assert logits.shape == (3, 4, V) and torch.equal(logits, fake._logits(tokens, context))            # logits[:, cond_len - 1:] with one sos token
    l2, t2 = m(x, c, r)
    assert torch.equal(l2, logits) and torch.equal(t2, target)


def test_shared_step_draws_the_mask_probability_from_numpy():
    m, fake = _mirror(p_mask_max=0.8)
    b = _batch()
    np.random.seed(12)
    want_p = np.random.uniform(0., 0.8)
    np.random.seed(12)
    assert m.get_mask_prob() == want_p
    np.random.seed(12); torch.manual_seed(5)
    logits, target = m.shared_step(b, 0)
    torch.manual_seed(5)
    want_r = m.get_r(b, p_mask=want_p)
    assert int((want_r == 512).sum()) > 0                                                              # the mask did something
    assert torch.equal(fake.calls[-1][2], want_r)
    # p_mask_max = 0: no masking at all
    m0, fake0 = _mirror()
    m0.shared_step(b, 0)
    assert torch.equal(fake0.calls[-1][2], b["nn_embeddings"])


@pytest.mark.parametrize("split", ["val", "train"])
def test_compute_loss_is_cross_entropy_under_the_split_key(split):
    m, _ = _mirror()
    g = torch.Generator().manual_seed(1)
    logits = torch.randn((3, 4, V), generator=g); targets = torch.randint(0, V, (3, 4), generator=g)
    loss, log = m.compute_loss(logits, targets, split=split)
    assert list(log) == [f"{split}/loss"]
    assert torch.equal(loss, F.cross_entropy(logits.reshape(-1, V), targets.reshape(-1))) and torch.equal(log[f"{split}/loss"], loss)


def test_validation_step_is_the_mean_of_rarm_nll():
    m, fake = _mirror()
    b = _batch()
    out = m.validation_step(b, 0)
    assert list(out) == ["val/loss"]
    names = [c[0] for c in fake.calls]
    assert names == ["rarm_nll"]                                                                       # no logits tensor on this path
    _, tokens, targets, context = fake.calls[-1]
    _, z = fake.vq_encode_indices(b["image"])
    assert torch.equal(targets, z) and torch.equal(tokens, torch.cat([torch.full((3, 1), 513), z], 1)[:, :-1])
    want, _ = m.compute_loss(*m.forward(*m.get_xc(b), m.get_r(b)), split="val")
    assert abs(float(out["val/loss"]) - float(want)) <= 1e-5
    per_token = m.nll(m.get_xc(b)[0], m.get_r(b))
    assert per_token.shape == (3, 4) and abs(float(per_token.mean()) - float(want)) <= 1e-5


def test_training_step_names_the_missing_backward():
    m, _ = _mirror()
    with pytest.raises(NotImplementedError, match="backward"):
        m.training_step(_batch(), 0)


# ------------------------------------------------------------------------------------------------ prefill plumbing
def _util_args(n=2, steps=4, kept=2):
    return dict(steps=steps, z_start=torch.zeros((n, kept), dtype=torch.long), r=torch.zeros((n, 1, 512)),
                c=torch.full((n, 1), 513, dtype=torch.long), temperature=1.0, top_k=50, zshape=(n, 64, 2, 2))


def test_prefill_reaches_rarm_sample_from_sample_and_sampling_util():
    m, fake = _mirror()
    a = _util_args()
    m.sample(a["z_start"], a["r"], a["c"], steps=4, sample=True, top_k=50, prefill=True)
    assert fake.calls[-1] == ("rarm_sample", dict(temperature=1.0, top_k=50, guidance_scale=1.0, prefill=True, steps=4, tc=3))
    m.sampling_util(prefill=True, **a)
    assert fake.calls[-1][1]["prefill"] is True
    # the default, None and False are the call made before the option existed: no such keyword
    for kw in ({}, {"prefill": None}, {"prefill": False}):
        m.sampling_util(**a, **kw)
        assert "prefill" not in fake.calls[-1][1]
    out = m.sample_from_rdata(2, nn_embeddings=torch.zeros(2, 1, 512), code_side_len=2, z_dimensionality=64, top_k=10, prefill=True)
    assert fake.calls[-1][1]["prefill"] is True and "samples_with_sampled_nns" in out


def test_prefill_reaches_rarm_sample_from_log_images():
    m, fake = _mirror()
    m.log_images(_batch(), N=2, top_k=50, p_sample=False, prefill=True)
    samples = [c[1] for c in fake.calls if c[0] == "rarm_sample"]
    assert [s["tc"] for s in samples] == [1, 3] and all(s["prefill"] is True for s in samples)         # samples_full, samples_half (sos + 2 of 4 codes)
    m.log_images(_batch(), N=2, top_k=50, p_sample=False)
    assert all("prefill" not in c[1] for c in fake.calls[-2:])


def _script():
    spec = importlib.util.spec_from_file_location("rarm_sample_native_seq_cpu", os.path.join(ROOT, "scripts", "rarm_sample.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_script_parses_and_documents_prefill_and_score():
    mod = _script()
    d = mod.parse_args([])
    assert d.prefill is False and d.score is None
    o = mod.parse_args(["--prefill", "--complete_from", "a.png", "--score", "imgs"])
    assert o.prefill is True and str(o.score) == "imgs"
    assert "--prefill" in mod.__doc__ and "--score" in mod.__doc__
    helps = {a.dest: a.help for a in mod.build_parser()._actions}
    assert helps["prefill"].startswith("[native]") and helps["score"].startswith("[native]")


# ------------------------------------------------------------------------------------------------ argument errors of the Python layer
def _bare_context(sequence_length=24):
    """A Context without a device or a library handle: enough of one to reach every check that comes before the library call."""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    c = object.__new__(_lib.Context)
    c.device = torch.device("cpu")
    c.rarm_cfg = _lib.make_rarm_cfg(in_channels=1002, out_channels=1000, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=sequence_length)
    c._h = None
    return c, _lib


def test_whole_sequence_entries_refuse_bad_arguments():
    c, _lib = _bare_context()
    tok = torch.zeros((2, 12), dtype=torch.long)
    cx = torch.zeros((2, 4, 512))
    for call in (lambda **k: c.rarm_forward_seq(k.get("tokens", tok), k.get("context", cx)),
                 lambda **k: c.rarm_nll(k.get("tokens", tok), k.get("targets", tok), k.get("context", cx))):
        with pytest.raises(_lib.RdmError, match="sequence_length"):
            call(tokens=torch.zeros((2, 25), dtype=torch.long), targets=torch.zeros((2, 25), dtype=torch.long))
        with pytest.raises(_lib.RdmError, match="128 neighbours"):
            call(context=torch.zeros((2, 129, 512)))
        with pytest.raises(_lib.RdmError, match="tokens must lie in"):
            call(tokens=torch.full((2, 12), 1002, dtype=torch.long))
        with pytest.raises(_lib.RdmError, match="neighbours must be"):
            call(context=torch.zeros((3, 4, 512)))
    with pytest.raises(_lib.RdmError, match="targets must lie in"):
        c.rarm_nll(tok, torch.full((2, 12), 1000, dtype=torch.long), cx)                               # vocab_out = 1000: 1000 and 1001 are input-only ids
    with pytest.raises(_lib.RdmError, match="targets must lie in"):
        c.rarm_nll(tok, torch.full((2, 12), -1, dtype=torch.long), cx)
    with pytest.raises(_lib.RdmError, match="targets must be"):
        c.rarm_nll(tok, torch.zeros((2, 11), dtype=torch.long), cx)
    c.rarm_cfg = None
    with pytest.raises(_lib.RdmError, match="not loaded"):
        c.rarm_forward_seq(tok, cx)
    with pytest.raises(_lib.RdmError, match="not loaded"):
        c.rarm_nll(tok, tok, cx)


def test_prefill_refuses_bad_arguments():
    c, _lib = _bare_context()
    cx = torch.zeros((2, 4, 512))
    with pytest.raises(_lib.RdmError, match="sequence_length"):
        c.rarm_sample(torch.zeros((2, 13), dtype=torch.long), cx, 13, torch.zeros((13, 2)), prefill=True)     # 13 + 13 - 1 = 25 > 24
    with pytest.raises(_lib.RdmError, match="128 neighbours"):
        c.rarm_sample(torch.zeros((2, 3), dtype=torch.long), torch.zeros((2, 129, 512)), 4, torch.zeros((4, 2)), prefill=True)
    with pytest.raises(_lib.RdmError, match="top_p"):
        c.rarm_sample(torch.zeros((2, 3), dtype=torch.long), cx, 4, torch.zeros((4, 2)), prefill=True, top_p=0.0)


def test_op_entries_refuse_bad_arguments():
    c, _lib = _bare_context()
    with pytest.raises(_lib.RdmError, match="targets must lie in"):
        c.op_rarm_nll(torch.zeros((4, 10)), torch.tensor([0, 1, 2, 10]))
    with pytest.raises(_lib.RdmError, match="even V"):
        c.op_rarm_nll(torch.zeros((4, 11)), torch.zeros(4, dtype=torch.long))
    qkv = torch.zeros((1, 1025, 3 * 64), dtype=torch.bfloat16)
    with pytest.raises(_lib.RdmError, match="n <= 1024"):
        c.op_causal_attention_d64(qkv, 1, 0.125)
    qkv = torch.zeros((2, 8, 3 * 64), dtype=torch.bfloat16)
    with pytest.raises(_lib.RdmError, match="come together"):
        c.op_causal_attention_d64(qkv, 1, 0.125, kcache=torch.zeros((2, 1, 8, 64), dtype=torch.bfloat16))
    with pytest.raises(_lib.RdmError, match="caches must be"):
        c.op_causal_attention_d64(qkv, 1, 0.125, kcache=torch.zeros((2, 1, 7, 64), dtype=torch.bfloat16), vcache=torch.zeros((2, 1, 7, 64), dtype=torch.bfloat16))
