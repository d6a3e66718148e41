"""CPU check of the decode-step references (tests/_decode_ref.py) that tests/test_gpu_decode_ops.py holds the HIP kernels to: an fp32 torch
restatement of each op stands in for the kernel, must pass every per-element bound and fall outside it against every near miss.  The
host-only selector (rdm_linear_rows_select, the function the library's own dispatch asks) is enumerated over the decode step's shapes:
every form it can route to must have a case, and every case must reach the form it names.  The wrappers' argument refusals run against a
Context without a device."""
import pytest
import torch

import _decode_ref as R
from _train_ref import check, standin

torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.mark.parametrize("entry", R.CASES, ids=[R.case_id(e) for e in R.CASES])
def test_fp32_restatement_within_bound_and_near_misses_outside(entry):
    case, kw, path = entry
    inp = case.make(**kw)
    worst, margin = check(case, inp, standin(case, inp, R.bf16_out))
    print(f"{path}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def _select(kw):
    from rdm_amd import _lib
    return _lib.linear_rows_select(kw["M"], kw["N"], kw["K"], kw.get("act", R.ACT_NONE), kw.get("ln", False), kw.get("det", False))


def test_every_form_of_the_selector_has_a_case():
    """modes x LayerNorm operand or not x K in {256, 768, 3072} x N in {256, 768, 2304} plain, {1024, 6144} GEGLU x M in 1 .. 4096"""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    forms = set()
    for det in (False, True):
        for ln in (False, True):
            for K in (256, 768, 3072):
                for N, act in ((256, R.ACT_NONE), (768, R.ACT_NONE), (2304, R.ACT_NONE), (1024, R.ACT_GEGLU), (6144, R.ACT_GEGLU)):
                    for M in range(1, 4097):
                        forms.add(_lib.linear_rows_select(M, N, K, act, ln, det))
    cased = {e[1]["form"] for e in R.LINEAR_ROWS} | {("refused",)}
    assert forms == cased, f"forms without a case: {sorted(forms - cased)}; cases no shape of the grid reaches: {sorted(cased - forms)}"
    assert len(forms) == 33


def test_every_case_reaches_the_form_it_names():
    import rdm_amd  # noqa: F401
    for case, kw, path in R.LINEAR_ROWS:
        assert _select(kw) == kw["form"], (path, _select(kw))
        if kw["form"][0] == "sgemm":
            assert (kw["form"][5], kw["form"][6]) == (kw.get("ln", False), kw.get("act") == R.ACT_GEGLU)
    for kw in R.LINEAR_ROWS_REFUSED:
        assert _select(dict(kw, ln=True)) == ("refused",)
    # every form has a case whose M is ragged against its tile (the last tile clamps its rows to M - 1 and must not store them)
    ragged = {kw["form"] for _, kw, _ in R.LINEAR_ROWS if kw["M"] % R.LinearRows.tile_rows({"form": kw["form"]}) != 0}
    assert ragged == {kw["form"] for _, kw, _ in R.LINEAR_ROWS}
    # both modes write the fp32 residual stream in place; the mid-size kernel does too
    assert {kw.get("det", False) for _, kw, _ in R.LINEAR_ROWS if kw.get("res")} == {False, True}
    assert any(kw["form"] == ("mgemm",) and kw.get("res") for _, kw, _ in R.LINEAR_ROWS)


def test_selector_follows_the_mode_not_the_batch():
    """deterministic mode: the four-wave K split at every row count (no eight-wave, folded or mid-size form), one (U, NW) per (N, K, act)"""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    for N, K, act in ((768, 768, R.ACT_NONE), (2304, 768, R.ACT_NONE), (768, 3072, R.ACT_NONE), (6144, 768, R.ACT_GEGLU)):
        split = {_lib.linear_rows_select(M, N, K, act, False, True)[3:5] for M in range(1, 4097)}
        kinds = {_lib.linear_rows_select(M, N, K, act, False, True)[0] for M in range(1, 4097)}
        assert kinds == {"sgemm"} and {nw for _, nw in split} == {4}, (N, K, act, kinds, split)
    with pytest.raises(_lib.RdmError):
        _lib.linear_rows_select(0, 256, 256)


def test_case_ids_name_every_launch_path():
    paths = " | ".join(e[2] for e in R.CASES)
    for kernel in ("sgemm<4, 6, 3, NW8>", "sgemm<4, 4, 3, NW8>", "sgemm<4, 2, 6, NW8>", "sgemm<2, 2, 6, LN, NW4>", "sgemm<2, 4, GEGLU, 6, LN, NW4>", "mgemm", "tiled",
                   "in place on the residual", "deterministic", "small_var", "rarm_decode_attention_kernel<4>: self, append at 1023", "cross, row-major, 33 keys",
                   "rarm_fewkey_attention_kernel: 5 keys", "rarm_xattn_decode_kernel: C 1024, 16 heads x 8", "rarm_embed_kernel", "rarm_embed_seq_kernel"):
        assert kernel in paths, kernel
    assert {e[0].name for e in R.CASES} == {"linear_rows", "decode_attention", "xattn_decode", "embed"}


def test_one_pass_variance_with_a_coarse_sum_falls_outside_the_bound():
    """The LayerNorm operand is held to a two-pass bound: a variance taken as E[x^2] - mean^2 from sums carried in bf16-coarse precision (a
    one-pass form gone wrong) must fail it on the offset rows."""
    entry = next(e for e in R.LINEAR_ROWS if e[1].get("ln") and e[1].get("offset") and not e[1].get("small_var") and e[1]["M"] > 1)
    inp = R.LinearRows.make(**entry[1])
    x = inp["x"]
    mean = x.mean(1, keepdim=True)
    var = (R.bfr((x * x).mean(1, keepdim=True)) - R.bfr(mean * mean)).clamp(min=0)
    xn = (x - mean) / torch.sqrt(var + inp["eps"]) * inp["gamma"] + inp["beta"]
    out = inp["buf16"].clone()
    out[:inp["M"]] = R.bfr(xn @ inp["w"].t() + inp["b"])
    with pytest.raises(AssertionError, match="worst error / bound"):
        check(R.LinearRows, inp, {"out": out})


def _bare_context():
    """A Context without a device or a library handle: enough of one to reach every check that comes before the library call."""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    c = object.__new__(_lib.Context)
    c.device = torch.device("cpu")
    c._h = None
    return c, _lib


def test_linear_rows_refuses_bad_arguments():
    c, _lib = _bare_context()
    BF = torch.bfloat16
    w, a, x = torch.zeros((256, 256), dtype=BF), torch.zeros((4, 256), dtype=BF), torch.zeros((4, 256))
    g = torch.zeros(256)
    with pytest.raises(_lib.RdmError, match="exactly one of"):
        c.op_linear_rows(w)
    with pytest.raises(_lib.RdmError, match="exactly one of"):
        c.op_linear_rows(w, a=a, ln=(x, g, g))
    with pytest.raises(_lib.RdmError, match="operand"):
        c.op_linear_rows(w, a=a.float())
    with pytest.raises(_lib.RdmError, match="operand"):
        c.op_linear_rows(w, a=a, rows=5)
    with pytest.raises(_lib.RdmError, match="no residual"):
        c.op_linear_rows(w, ln=(x, g, g), res_f32=torch.zeros((4, 256)))
    with pytest.raises(_lib.RdmError, match="gamma and beta"):
        c.op_linear_rows(w, ln=(x, g, g[:8]))
    with pytest.raises(_lib.RdmError, match="out_f32 must be"):
        c.op_linear_rows(w, a=a, out_f32=torch.zeros((3, 256)))
    with pytest.raises(_lib.RdmError, match="out_bf16 must be"):
        c.op_linear_rows(w, a=a, act=_lib.ACT_GEGLU, out_bf16=torch.zeros((4, 256), dtype=BF))
    with pytest.raises(_lib.RdmError, match="bias must be"):
        c.op_linear_rows(w, a=a, bias=torch.zeros(255))


def test_decode_attention_refuses_bad_arguments():
    c, _lib = _bare_context()
    BF = torch.bfloat16
    qkv = torch.zeros((2, 3 * 128), dtype=BF)
    q, kn, vn = qkv[:, :128], qkv[:, 128:256], qkv[:, 256:]
    kc, vc = torch.zeros((2, 2, 16, 64), dtype=BF), torch.zeros((2, 2, 16, 64), dtype=BF)
    with pytest.raises(_lib.RdmError, match="come together"):
        c.op_rarm_decode_attention(q, kc, vc, 2, 0.125, pos=0, k_new=kn)
    with pytest.raises(_lib.RdmError, match="0 <= pos < 16"):
        c.op_rarm_decode_attention(q, kc, vc, 2, 0.125, pos=16, k_new=kn, v_new=vn)
    with pytest.raises(_lib.RdmError, match="0 <= pos < 16"):
        c.op_rarm_decode_attention(q, kc, vc, 2, 0.125, pos=-1, k_new=kn, v_new=vn)
    big = torch.zeros((2, 2, 1025, 64), dtype=BF)
    with pytest.raises(_lib.RdmError, match="nkv <= min\\(1024"):
        c.op_rarm_decode_attention(q, big, big, 2, 0.125, pos=0, k_new=kn, v_new=vn)
    with pytest.raises(_lib.RdmError, match="nkv <= min\\(1024"):
        c.op_rarm_decode_attention(q, kc, vc, 2, 0.125, nkv=17)
    with pytest.raises(_lib.RdmError, match="head-major cache"):
        c.op_rarm_decode_attention(q, torch.zeros((2, 3, 16, 64), dtype=BF), torch.zeros((2, 3, 16, 64), dtype=BF), 2, 0.125)
    with pytest.raises(_lib.RdmError, match="row-major cache"):
        c.op_rarm_decode_attention(q, torch.zeros((2, 4, 64), dtype=BF), torch.zeros((2, 4, 64), dtype=BF), 2, 0.125)
    with pytest.raises(_lib.RdmError, match="one shape"):
        c.op_rarm_decode_attention(q, kc, vc[:, :, :8], 2, 0.125)
    with pytest.raises(_lib.RdmError, match="q must be"):
        c.op_rarm_decode_attention(q, kc, vc, 3, 0.125)
    with pytest.raises(_lib.RdmError, match="q's row stride"):
        c.op_rarm_decode_attention(q, kc, vc, 2, 0.125, pos=0, k_new=torch.zeros((2, 128), dtype=BF), v_new=torch.zeros((2, 128), dtype=BF))


def test_xattn_decode_and_embed_refuse_bad_arguments():
    c, _lib = _bare_context()
    BF = torch.bfloat16
    x, v = torch.zeros((4, 192)), torch.zeros(192)
    G = torch.zeros((2, 16, 192), dtype=BF)
    with pytest.raises(_lib.RdmError, match="heads \\* k <= min"):
        c.op_rarm_xattn_decode(x, (v, v), G, G, v, heads=3, k=6)
    with pytest.raises(_lib.RdmError, match="G and UT must be"):
        c.op_rarm_xattn_decode(x, (v, v), torch.zeros((5, 16, 192), dtype=BF), torch.zeros((5, 16, 192), dtype=BF), v, heads=3, k=4)
    with pytest.raises(_lib.RdmError, match="G and UT must be"):
        c.op_rarm_xattn_decode(x, (v, v), G, G[:, :8], v, heads=3, k=4)
    with pytest.raises(_lib.RdmError, match="f32 \\[192\\]"):
        c.op_rarm_xattn_decode(x, (v, v[:8]), G, G, v, heads=3, k=4)
    with pytest.raises(_lib.RdmError, match="f32 \\[192\\]"):
        c.op_rarm_xattn_decode(x, (v, v), G, G, v, heads=3, k=4, ln3=(v, v.double()))
    with pytest.raises(_lib.RdmError, match="multiple of 8"):
        c.op_rarm_xattn_decode(torch.zeros((4, 1032)), (torch.zeros(1032),) * 2, torch.zeros((2, 16, 1032), dtype=BF), torch.zeros((2, 16, 1032), dtype=BF),
                               torch.zeros(1032), heads=3, k=4)
    with pytest.raises(_lib.RdmError, match="x must be"):
        c.op_rarm_xattn_decode(x.to(BF), (v, v), G, G, v, heads=3, k=4)
    emb, pos_t, tok = torch.zeros((10, 8)), torch.zeros((4, 8)), torch.zeros(3, dtype=torch.long)
    with pytest.raises(_lib.RdmError, match="exactly one of"):
        c.op_rarm_embed(tok, emb, pos_t)
    with pytest.raises(_lib.RdmError, match="0 <= pos < 4"):
        c.op_rarm_embed(tok, emb, pos_t, pos=4)
    with pytest.raises(_lib.RdmError, match="1 <= t <= 4"):
        c.op_rarm_embed(torch.zeros((2, 8), dtype=torch.long), emb, pos_t, t=5)
    with pytest.raises(_lib.RdmError, match="tok_ld >= t"):
        c.op_rarm_embed(torch.zeros((2, 3), dtype=torch.long), emb, pos_t, t=4)
    with pytest.raises(_lib.RdmError, match="int64 tokens"):
        c.op_rarm_embed(tok.int(), emb, pos_t, pos=0)
