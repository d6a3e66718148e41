"""CPU suite of the RARM sampler's nucleus (top-p) option: the float64 restatement of its definition (tests/_nucleus_ref.py)
against an independent sort-and-cumsum formulation, what the LatentImageRETRO mirror hands down to the context, the script's flag,
and the argument check of the Python layer.  (The kernel itself: tests/test_gpu_rarm_top_p.py.)"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _nucleus_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_agrees_with_sort_and_cumsum_where_no_tie_sits_at_the_boundary():
    """Random logits (continuous: no ties), with and without top-k, three nucleus masses: the threshold form (largest present value
    whose mass at-or-above reaches top_p) and the sorted-prefix form (keep a token while the mass BEFORE it is below top_p) keep the
    same set on every row; the set holds the arg-max, its mass reaches top_p and the mass without its smallest member does not."""
    rng = np.random.default_rng(5)
    for sigma, top_k in ((3.0, 64), (6.0, 256), (2.0, None)):
        g = torch.from_numpy((rng.standard_normal((48, 2048)) * sigma).astype(np.float32))
        for top_p in (0.5, 0.9, 0.95):
            r = nr.nucleus(g, top_k, top_p)
            assert torch.equal(r["keep"], torch.from_numpy(nr.sort_cumsum_keep(g, top_k, top_p))), (sigma, top_k, top_p)
            assert bool(r["keep"][torch.arange(48), g.argmax(-1)].all())
            assert bool((r["m_star"] >= np.float32(top_p)).all()) and bool((r["m_next"] < np.float32(top_p)).all())
            if top_k is not None:
                assert int(r["count"].max()) <= top_k
    # top-k survivors only: with top_p just below 1 the nucleus is all of K but its smallest members
    g = torch.from_numpy((rng.standard_normal((4, 512)) * 1.0).astype(np.float32))
    assert int(nr.nucleus(g, 16, 0.999999)["count"].max()) <= 16


def test_restatement_keeps_a_planted_boundary_tie_group_whole():
    """Masses 0.4, 0.25, 0.25, 0.1 with the two 0.25 tokens bit-equal and top_p = 0.6: the crossing token is one of the tied pair, so
    BOTH are kept (3 tokens, mass 0.9); the sort-based form cuts the pair (2 tokens); at 0.3 only the arg-max, at 0.95 all four."""
    p = np.array([0.1, 0.25, 0.4, 0.25])
    g = torch.full((1, 64), -30.0)
    g[0, [7, 20, 33, 50]] = torch.from_numpy(np.log(p).astype(np.float32))
    assert g[0, 20] == g[0, 50]
    r = nr.nucleus(g, None, 0.6)
    assert sorted(r["keep"][0].nonzero().flatten().tolist()) == [20, 33, 50] and int(r["count"]) == 3
    assert abs(float(r["m_star"]) - 0.9) < 1e-6 and abs(float(r["m_next"]) - 0.4) < 1e-6
    assert int(nr.sort_cumsum_keep(g, None, 0.6).sum()) == 2
    assert int(nr.nucleus(g, None, 0.6, variant="cut_tie")["count"]) == 2
    assert int(nr.nucleus(g, None, 0.6, variant="strict")["count"]) == 1
    assert int(nr.nucleus(g, None, 0.3)["count"]) == 1 and int(nr.nucleus(g, None, 0.95)["count"]) == 4
    # the mass is relative to the top-k survivors: top_k = 3 leaves 0.4 / 0.25 / 0.25 (0.444 / 0.278 / 0.278 of their own mass), so
    # top_p = 0.7 crosses inside the tied pair and keeps all three
    assert int(nr.nucleus(g, 3, 0.7)["count"]) == 3
    assert int(nr.nucleus(g, 1, 0.9)["count"]) == 1           # top-k first: one survivor holds all the mass


class _MockCtx:
    """Records what LatentImageRETRO passes down."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def rarm_sample(self, cond_tokens, context, steps, uniforms, **kw):
        self.calls.append(dict(kw, steps=steps, b=cond_tokens.shape[0]))
        return torch.zeros((cond_tokens.shape[0], steps), dtype=torch.long)

    def vq_decode_indices(self, idx):
        return torch.zeros((idx.shape[0], 3, 8, 8))


def _mirror():
    import rdm_amd  # noqa: F401
    from rdm_amd.models.autoregression.transformer import LatentImageRETRO
    mock = _MockCtx()
    m = LatentImageRETRO({"params": dict(in_channels=514, out_channels=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64)},
                         None, mask_token=512, sos_token=513, ctx=mock)
    return m, mock


def _util_args(n=2, steps=4):
    return dict(steps=steps, z_start=torch.zeros((n, 0), dtype=torch.long), r=torch.zeros((n, 1, 512)),
                c=torch.full((n, 1), 513, dtype=torch.long), temperature=1.0, top_k=50, zshape=(n, 64, 2, 2))


def test_sampling_util_passes_top_p_down():
    """`sampling_util(top_p=0.9)` reaches ctx.rarm_sample with top_p == 0.9 (the reference, and this mirror before the option was
    built, stop at `assert top_p==1., 'not yet implemented'`, rdm/models/autoregression/transformer.py:280)."""
    m, mock = _mirror()
    img = m.sampling_util(top_p=0.9, **_util_args())
    assert img.shape == (2, 3, 8, 8)
    assert len(mock.calls) == 1 and mock.calls[0]["top_p"] == 0.9 and mock.calls[0]["top_k"] == 50
    out = m.sample_from_rdata(2, nn_embeddings=torch.zeros(2, 1, 512), code_side_len=2, z_dimensionality=64, top_k=10, top_p=0.5)
    assert mock.calls[-1]["top_p"] == 0.5 and mock.calls[-1]["top_k"] == 10 and "samples_with_sampled_nns" in out


def test_top_p_one_and_none_are_todays_call():
    m, mock = _mirror()
    m.sampling_util(**_util_args())
    m.sampling_util(top_p=1.0, **_util_args())
    m.sampling_util(top_p=None, **_util_args())
    a = _util_args()
    m.sample(a["z_start"], a["r"], a["c"], steps=4, sample=True, top_k=50)
    want = dict(temperature=1.0, top_k=50, guidance_scale=1.0, steps=4, b=2)
    assert mock.calls == [want] * 4, mock.calls                # no top_p keyword at all: exactly the call made before the option existed


def test_arg_max_ignores_top_p():
    m, mock = _mirror()
    a = _util_args()
    m.sample(a["z_start"], a["r"], a["c"], steps=4, sample=False, top_k=50, top_p=0.3)
    assert mock.calls == [dict(temperature=1.0, top_k=1, guidance_scale=1.0, steps=4, b=2)]


@pytest.mark.parametrize("bad", [0.0, -0.1, 1.5, float("nan")])
def test_out_of_range_top_p_raises_naming_it(bad):
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    m, mock = _mirror()
    a = _util_args()
    with pytest.raises(_lib.RdmError, match="top_p"):
        m.sample(a["z_start"], a["r"], a["c"], steps=4, sample=True, top_k=50, top_p=bad)
    with pytest.raises(_lib.RdmError, match="top_p"):
        m.sampling_util(top_p=bad, **_util_args())
    assert mock.calls == []
    # the context's own entry points refuse it before they touch anything (no context, no device needed to get there)
    with pytest.raises(_lib.RdmError, match="rarm_sample: top_p"):
        _lib.Context.rarm_sample(None, None, None, 4, None, top_p=bad)
    with pytest.raises(_lib.RdmError, match="op_rarm_sampler: top_p"):
        _lib.Context.op_rarm_sampler(None, None, None, top_p=bad)
    assert _lib.check_top_p("x", None) is None and _lib.check_top_p("x", 1.0) is None and _lib.check_top_p("x", 1) is None
    assert _lib.check_top_p("x", 0.9) == 0.9 and math.isclose(_lib.check_top_p("x", np.float32(0.5)), 0.5)


def test_script_lists_top_p_with_default_one():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rarm_sample.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--top_p" in r.stdout and "--top_k" in r.stdout
    line = " ".join(r.stdout.split())
    assert "default: 1.0" in line[line.rindex("--top_p TOP_P"):line.rindex("--temperature TEMPERATURE")]     # the option's own help entry
    import importlib.util
    spec = importlib.util.spec_from_file_location("rarm_sample_native_cpu", os.path.join(ROOT, "scripts", "rarm_sample.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert mod.parse_args([]).top_p == 1.0 and mod.parse_args(["--top_p", "0.9"]).top_p == 0.9
    assert "--top_p" in mod.__doc__
