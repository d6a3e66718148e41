"""The RARM decode step's kernels (the skinny GEMM in every instantiation the dispatch routes to, the mid-size GEMM in place on the fp32
residual stream, the K/V-cache attention in both kernels, the one-launch cross-attention, the token embedding) called one at a time
through the C ABI and held to a float64 CPU restatement of the same operation, element by element (tests/_decode_ref.py states each
bound and near miss).  Every case also shows that its bound discriminates: the kernel output must fall outside the bound against each
near-miss reference.  These kernels sum in fixed orders: every call is repeated once and must agree bitwise."""
import pytest
import torch

import _decode_ref as R
from _train_ref import check

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
torch.set_num_threads(min(16, torch.get_num_threads()))


class _Mode:
    """the context in deterministic (or fast) mode for the length of a block"""

    def __init__(self, ctx, det):
        self.ctx, self.det = ctx, det

    def __enter__(self):
        self.was = self.ctx.deterministic
        self.ctx.set_deterministic(self.det)

    def __exit__(self, *exc):
        self.ctx.set_deterministic(self.was)


def _linear_rows(ctx, inp):
    from rdm_amd.packing import _geglu_perm
    d = ctx.device
    w, bias = inp["w"], inp["b"]
    if inp["act"] == R.ACT_GEGLU:
        perm = _geglu_perm(w.shape[0])
        w = w[perm]; bias = None if bias is None else bias[perm]
    ob = inp["buf16"].to(d, BF).contiguous() if inp["outs"] in ("bf16", "both") else None
    of = inp["buf32"].to(d).contiguous() if inp["outs"] in ("f32", "both") else None
    kw = dict(bias=None if bias is None else bias.to(d), res_f32=of if inp["res"] else None, out_bf16=ob, out_f32=of, act=inp["act"], rows=inp["M"])
    if inp["ln"]:
        kw["ln"] = (inp["x"].to(d).contiguous(), inp["gamma"].to(d), inp["beta"].to(d))
    else:
        kw["a"] = inp["a"].to(d, BF).contiguous()
    with _Mode(ctx, inp["det"]):
        ctx.op_linear_rows(w.to(d, BF).contiguous(), **kw)
    out = {}
    if ob is not None:
        out["out"] = ob
    if of is not None:
        out["out32"] = of
    return out


def _decode_attention(ctx, inp):
    """-> outputs, and the cache tensors after the call with what they must hold"""
    d = ctx.device
    B, H = inp["B"], inp["H"]
    C = H * R.D
    if inp["mode"] == "self":
        qkv = inp["qkv"].to(d, BF).contiguous()
        kc, vc = (c.to(d, BF).contiguous() for c in inp["caches"])
        out = ctx.op_rarm_decode_attention(qkv[:, :C], kc, vc, H, inp["scale"], pos=inp["t"], k_new=qkv[:, C:2 * C], v_new=qkv[:, 2 * C:])
        want = [c.to(BF).clone() for c in inp["caches"]]
        for wnt, new in zip(want, R.DecodeAttention.new_rows(inp, torch.float32)):
            wnt[:, :, inp["t"]] = new.to(BF)
        return {"out": out}, [(kc, want[0]), (vc, want[1])]
    buf = inp["caches"][0].to(d, BF).contiguous()
    out = ctx.op_rarm_decode_attention(inp["q"].to(d, BF).contiguous(), buf[:, :, 2 * C:3 * C], buf[:, :, 3 * C:4 * C], H, inp["scale"], nkv=inp["n"])
    return {"out": out}, [(buf, inp["caches"][0].to(BF))]


def _xattn_decode(ctx, inp):
    d = ctx.device
    f = lambda t: t.to(d).contiguous()
    x = f(inp["x"])
    l3 = ctx.op_rarm_xattn_decode(x, (f(inp["gamma"]), f(inp["beta"])), inp["G"].to(d, BF).contiguous(), inp["UT"].to(d, BF).contiguous(), f(inp["bias"]),
                                  inp["heads"], inp["k"], ln3=(f(inp["gamma3"]), f(inp["beta3"])) if inp["ln3"] else None, eps=inp["eps"])
    return {"x": x, "ln3": l3} if inp["ln3"] else {"x": x}


def _embed(ctx, inp):
    d = ctx.device
    tok, emb, pos_t = inp["tokens"].to(d).contiguous(), inp["emb"].to(d).contiguous(), inp["pos_t"].to(d).contiguous()
    if inp["pos"] is not None:
        return {"x": ctx.op_rarm_embed(tok, emb, pos_t, pos=inp["pos"])}
    return {"x": ctx.op_rarm_embed(tok, emb, pos_t, t=inp["t"], seq0=inp["seq0"], n_seq=inp["n_seq"])}


def _run(ctx, case, inp):
    """-> (outputs, [(tensor, what it must equal bitwise)])"""
    if case is R.LinearRows:
        return _linear_rows(ctx, inp), []
    if case is R.DecodeAttention:
        return _decode_attention(ctx, inp)
    if case is R.XattnDecode:
        return _xattn_decode(ctx, inp), []
    if case is R.Embed:
        return _embed(ctx, inp), []
    raise AssertionError(case.name)


@pytest.mark.parametrize("entry", R.CASES, ids=[R.case_id(e) for e in R.CASES])
def test_decode_op_matches_fp64_restatement(ctx, entry):
    from rdm_amd import _lib
    case, kw, path = entry
    inp = case.make(**kw)
    if case is R.LinearRows:
        assert _lib.linear_rows_select(kw["M"], kw["N"], kw["K"], inp["act"], inp["ln"], inp["det"]) == inp["form"], path
    out, exact = _run(ctx, case, inp)
    torch.cuda.synchronize()
    host = {k: v.float().cpu() for k, v in out.items()}
    worst, margin = check(case, inp, host)
    print(f"{path}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    for got, want in exact:                                # the caches: row t is the new row, every other element what it was
        assert torch.equal(got.cpu(), want), f"{path}: the cache differs from its contents before the call plus the new row"
    if case is R.LinearRows:                               # the rows of the buffers beyond M, bit for bit
        for k, buf in (("out", inp["buf16"].to(BF)), ("out32", inp["buf32"])):
            if k in out:
                assert torch.equal(out[k][inp["M"]:].cpu(), buf[inp["M"]:]), f"{path}: {k} was written beyond row M"
    again, _ = _run(ctx, case, inp)
    for k in out:
        assert torch.equal(out[k], again[k]), f"{path}: two calls differ (fixed summation order expected)"


def test_layernorm_form_is_refused_not_replaced(ctx):
    """where the LayerNorm-in-kernel form declines a shape the entry fails with its own code and message and writes nothing"""
    from rdm_amd import _lib
    d = ctx.device
    for kw in R.LINEAR_ROWS_REFUSED:
        M, N, K = kw["M"], kw["N"], kw["K"]
        x, g = torch.randn((M, K), device=d), torch.ones(K, device=d)
        w = torch.randn((N, K), device=d).to(BF)
        out = torch.full((M, N), 3.0, device=d, dtype=BF)
        with _Mode(ctx, kw["det"]):
            rc = _lib.lib.rdm_op_linear_rows(ctx._h, None, _lib._ptr(x), _lib._ptr(g), _lib._ptr(g), _lib._ptr(w), None, None, _lib._ptr(out), None, M, N, K, kw["act"])
        torch.cuda.synchronize()
        assert rc == -5 and b"LayerNorm-in-kernel" in _lib.lib.rdm_last_error(ctx._h), (rc, _lib.lib.rdm_last_error(ctx._h))
        assert bool((out == 3.0).all())


@pytest.mark.parametrize("kind", ["plain", "geglu", "ln"])
def test_deterministic_rows_do_not_follow_the_batch(ctx, kind):
    """deterministic mode: row r of an M = 400 call equals, bitwise, row r of an M = 16 call (one K split and one summation order at every
    row count: the tile may change, a row's arithmetic may not)"""
    from rdm_amd.packing import _geglu_perm
    d = ctx.device
    g = torch.Generator().manual_seed(7)
    K, N = 768, 1024 if kind == "geglu" else 768
    act = R.ACT_GEGLU if kind == "geglu" else R.ACT_NONE
    w = torch.randn(N, K, generator=g) * 2 / K ** 0.5
    bias = 0.5 * torch.randn(N, generator=g)
    if kind == "geglu":
        perm = _geglu_perm(N)
        w, bias = w[perm], bias[perm]
    w, bias = w.to(d, BF).contiguous(), bias.to(d)
    a = torch.randn(400, K, generator=g)
    res = torch.randn(400, N, generator=g).to(d)
    gam, bet = (1 + 0.3 * torch.randn(K, generator=g)).to(d), (0.3 * torch.randn(K, generator=g)).to(d)

    def call(M):
        if kind == "ln":
            return ctx.op_linear_rows(w, ln=((a[:M] + 5.0).to(d).contiguous(), gam, bet), bias=bias)[0]
        if kind == "geglu":
            return ctx.op_linear_rows(w, a=a[:M].to(d, BF).contiguous(), bias=bias, act=act)[0]
        x = res[:M].clone()
        return ctx.op_linear_rows(w, a=a[:M].to(d, BF).contiguous(), bias=bias, res_f32=x, out_f32=x)[1]

    with _Mode(ctx, True):
        big, small = call(400), call(16)
    torch.cuda.synchronize()
    assert torch.equal(big[:16], small), f"{kind}: a row's bits follow the batch in deterministic mode"
    assert bool(torch.isfinite(big).all()) and float(big.float().abs().max()) > 0


def _seq_inputs(steps, B=2, H=3, L=48, seed=23):
    g = torch.Generator().manual_seed(seed)
    qkv = R.bfr(torch.randn(steps, B, 3 * H * R.D, generator=g) * 1.5)
    K0, V0 = (R.bfr(torch.randn(B, H, L, R.D, generator=g) * 1.5) for _ in range(2))
    return qkv, K0, V0


def test_decode_attention_over_a_growing_cache(ctx):
    """positions 0 .. 40 in sequence on one cache: every step against the reference built from the history, and the final cache bitwise
    the new rows in rows 0 .. 40 and its first contents beyond"""
    d = ctx.device
    B, H, steps = 2, 3, 41
    C = H * R.D
    qkv, K, V = _seq_inputs(steps)
    kc, vc = K.to(d, BF).contiguous(), V.to(d, BF).contiguous()
    K, V = K.clone(), V.clone()
    worst, margin = 0.0, float("inf")
    for t in range(steps):
        row = qkv[t].to(d, BF).contiguous()
        out = ctx.op_rarm_decode_attention(row[:, :C], kc, vc, H, R.D ** -0.5, pos=t, k_new=row[:, C:2 * C], v_new=row[:, 2 * C:])
        w, m = check(R.DecodeAttention, R.DecodeAttention.from_state(qkv[t], K, V, t), {"out": out.float().cpu()})
        worst, margin = max(worst, w), min(margin, m)
        K[:, :, t] = qkv[t][:, C:2 * C].reshape(B, H, R.D)
        V[:, :, t] = qkv[t][:, 2 * C:].reshape(B, H, R.D)
    print(f"rarm_decode_attention_kernel<4> over 41 steps: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    assert torch.equal(kc.cpu(), K.to(BF)) and torch.equal(vc.cpu(), V.to(BF))


def test_decode_step_reads_the_cache_the_sequence_kernel_wrote(ctx):
    """rdm_op_causal_attention_d64 fills the caches for 40 tokens, then one decode step at pos = 40: the two kernels agree on the layout"""
    d = ctx.device
    B, H, n = 2, 3, 40
    C = H * R.D
    qkv, K, V = _seq_inputs(n + 1, seed=29)
    kc, vc = K.to(d, BF).contiguous(), V.to(d, BF).contiguous()
    ctx.op_causal_attention_d64(qkv[:n].transpose(0, 1).to(d, BF).contiguous(), H, R.D ** -0.5, kcache=kc, vcache=vc)
    row = qkv[n].to(d, BF).contiguous()
    out = ctx.op_rarm_decode_attention(row[:, :C], kc, vc, H, R.D ** -0.5, pos=n, k_new=row[:, C:2 * C], v_new=row[:, 2 * C:])
    K, V = K.clone(), V.clone()
    K[:, :, :n] = qkv[:n, :, C:2 * C].reshape(n, B, H, R.D).permute(1, 2, 0, 3)
    V[:, :, :n] = qkv[:n, :, 2 * C:].reshape(n, B, H, R.D).permute(1, 2, 0, 3)
    worst, margin = check(R.DecodeAttention, R.DecodeAttention.from_state(qkv[n], K, V, n), {"out": out.float().cpu()})
    print(f"decode step on causal_d64_kernel's cache: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")
    K[:, :, n] = qkv[n][:, C:2 * C].reshape(B, H, R.D)
    V[:, :, n] = qkv[n][:, 2 * C:].reshape(B, H, R.D)
    assert torch.equal(kc.cpu(), K.to(BF)) and torch.equal(vc.cpu(), V.to(BF))


def test_c_abi_refuses_bad_arguments_and_writes_nothing(ctx):
    from rdm_amd import _lib
    d, L, P = ctx.device, _lib.lib, _lib._ptr
    err = lambda: L.rdm_last_error(ctx._h)
    H, C = 2, 128
    qkv = torch.randn((2, 3 * C), device=d).to(BF)
    raw = lambda t, off=0: t.data_ptr() + 2 * off
    kc, vc = torch.full((2, H, 16, 64), 2.0, device=d, dtype=BF), torch.full((2, H, 16, 64), 2.0, device=d, dtype=BF)
    out = torch.full((2, C), 3.0, device=d, dtype=BF)
    base = dict(q=raw(qkv), ldq=3 * C, kn=raw(qkv, C), vn=raw(qkv, 2 * C), kc=raw(kc), vc=raw(vc), bs=H * 16 * 64, rs=64, hs=16 * 64, nkv=16, pos=3, out=raw(out), ldo=C)

    def attn(**over):
        a = dict(base, **over)
        return L.rdm_op_rarm_decode_attention(ctx._h, a["q"], a["ldq"], a["kn"], a["vn"], a["kc"], a["vc"], a["bs"], a["rs"], a["hs"], a["nkv"], a["pos"], 0.125,
                                              a["out"], a["ldo"], H, 2)

    for over, word in ((dict(nkv=1025), b"nkv"), (dict(pos=16), b"pos"), (dict(pos=-1), b"pos"), (dict(q=None), b"null"), (dict(kc=None), b"null"),
                       (dict(out=None), b"null"), (dict(vn=None), b"come together"), (dict(kn=None), b"come together"), (dict(ldq=3 * C + 4), b"stride"),
                       (dict(rs=60), b"stride"), (dict(q=raw(qkv, 4)), b"aligned"), (dict(kn=None, vn=None, pos=-2), b"pos")):
        assert attn(**over) != 0 and word in err(), (over, err())
    x = torch.full((4, 192), 1.5, device=d); v = torch.ones(192, device=d)
    G = torch.ones((2, 16, 192), device=d, dtype=BF)
    l3 = torch.full((4, 192), 3.0, device=d, dtype=BF)

    def xattn(x_=x, G_=G, Bc=2, C_=192, NP=16, heads=3, k=4, g3=v, b3=v, o3=l3):
        return L.rdm_op_rarm_xattn_decode(ctx._h, P(x_), P(v), P(v), 1e-5, P(G_), P(G_), P(v), 4, Bc, C_, NP, heads, k, P(g3), P(b3), P(o3))

    for over, word in ((dict(x_=None), b"null"), (dict(G_=None), b"null"), (dict(Bc=5), b"bad shape"), (dict(k=6), b"bad shape"), (dict(heads=33, k=4, NP=256), b"bad shape"),
                       (dict(C_=196), b"bad shape"), (dict(k=0), b"bad shape"), (dict(g3=None), b"come together"), (dict(o3=None), b"come together")):
        assert xattn(**over) != 0 and word in err(), (over, err())
    emb, pos_t, tok = torch.ones((10, 8), device=d), torch.ones((4, 8), device=d), torch.zeros((2, 4), dtype=torch.long, device=d)
    xo = torch.full((8, 8), 3.0, device=d)

    def embed(tokens=tok, tok_ld=4, tok_rows=2, seq0=0, rows=8, t=4, Lp=4, pos=-1):
        return L.rdm_op_rarm_embed(ctx._h, P(tokens), tok_ld, tok_rows, seq0, P(emb), P(pos_t), P(xo), rows, t, 8, 10, Lp, pos)

    for over, word in ((dict(tokens=None), b"null"), (dict(t=5), b"bad shape"), (dict(pos=4), b"bad shape"), (dict(pos=1), b"t = 1"), (dict(tok_ld=3), b"tok_ld"),
                       (dict(rows=7), b"whole sequences"), (dict(rows=0), b"bad shape"), (dict(tok_rows=0), b"tok_rows")):
        assert embed(**over) != 0 and word in err(), (over, err())
    a = torch.zeros((4, 256), device=d, dtype=BF); w = torch.zeros((256, 256), device=d, dtype=BF); o = torch.full((4, 256), 3.0, device=d, dtype=BF)
    for args, word in (((None, None, None, None, P(w), None, None, P(o), None, 4, 256, 256, 0), b"exactly one"), ((P(a), None, None, None, None, None, None, P(o), None, 4, 256, 256, 0), b"exactly one"),
                       ((P(a), None, None, None, P(w), None, None, None, None, 4, 256, 256, 0), b"output"), ((P(a), None, None, None, P(w), None, None, P(o), None, 0, 256, 256, 0), b"bad shape"),
                       ((P(a), None, None, None, P(w), None, None, P(o), None, 4, 256, 252, 0), b"bad shape"), ((P(a), None, None, None, P(w), None, None, P(o), None, 4, 255, 256, 1), b"bad shape"),
                       ((P(a), None, None, None, P(w), None, None, P(o), None, 4, 256, 256, 7), b"bad shape")):
        assert L.rdm_op_linear_rows(ctx._h, *args) != 0 and word in err(), (args, err())
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((kc == 2.0).all()) and bool((vc == 2.0).all()) and bool((x == 1.5).all()) and bool((l3 == 3.0).all())
    assert bool((xo == 3.0).all()) and bool((o == 3.0).all())
