"""Float64 restatements of the RARM decode step's kernels (csrc/sgemm.hip and mgemm.hip as rarm_step calls them, rarm.hip's cache
attention in both kernels, the one-launch cross-attention, the token embedding), their per-element error bounds and their near misses.
Shared by tests/test_gpu_decode_ops.py (the HIP kernels through rdm_op_linear_rows / rdm_op_rarm_*) and tests/test_decode_ops_cpu.py
(an fp32 torch restatement standing in for the kernels).  Same CASE contract as tests/_train_ref.py and tests/_fwd_ref.py: `make(**shape)`,
`ref(inp, dt)`, `bound(inp, ref)` -> per output (r, a), `misses(inp)`; `check()` asserts |out - ref| <= r |ref| + a element by element
and that the output falls outside the bound against every near miss.

Bound conventions as in _fwd_ref.py (u = 2^-24): r = 2^-8 for a bf16 output, 0 for an fp32 one; a = c u S, S the fp64 sum of the absolute
terms of the element, c the chain of dependent fp32 roundings of the launch geometry; a bf16 MFMA counts one rounding per product.  Per op:
  * sgemm_kernel<MA, NB, GEGLU, U, LN, NW>: a wave sums its K / NW share (c = K / NW), the NW partial tiles meet in LDS (at most NW adds,
    the fold of waves 4..7 into 0..3 included), bias and residual one add each: c = K / NW + NW + 2;
  * mgemm_kernel: one accumulator over all of K, bias, residual: c = K + 2;  the tiled kernels: _fwd_ref.Linear's (K + 8) and 2^-16 |b|;
  * the LayerNorm operand (LN = true) is held to a TWO-PASS LayerNorm (tests/_fwd_ref.LayerNorm's e_xh with d = K / 16 + 6: a lane's
    K / 16 elements, two lane exchanges, four wave sums) rounded to bf16 (2^-9 |xn|) and then multiplied: no cancellation term for a
    one-pass variance exists in it;
  * __expf / reciprocal: 2^-21 (2 + 2 |argument|) relative, as _fwd_ref._act_bound.
No bound is scaled by a whole-tensor maximum and no element is excluded: the rows of an output buffer beyond M are part of the output and
are held to their initial contents exactly (r = a = 0 there)."""
import math

import torch

from _fwd_ref import ACT_GEGLU, ACT_NONE, ACT_SILU, _act, _act_bound, _geglu_bound, _gelu
from _train_ref import BF, F64, U, bfr, row_offsets

PAD = 64                                      # rows of an output buffer beyond M: the largest tile is 64 rows
HUGE = 3.3895313892515355e38                  # the largest finite bf16
D = 64                                        # d_head of the decode attention


def _rows_bound(M, rows, r, a):
    """(r, a) over a [rows, N] buffer: the bound on rows < M, exact equality beyond"""
    live = (torch.arange(rows) < M).double()[:, None]
    return r * live.expand_as(a), a * live


# ============================================================================================================ linear, one row per sequence
class LinearRows:
    """rdm_op_linear_rows: out[M, No] = act(A w^T + b) (+ res), A = bf16 rows or LayerNorm(x f32; gamma, beta, 1e-5) formed in the kernel;
    outputs `out` (bf16) and / or `out32` (fp32; with `res` it IS the residual buffer: in place), each [M + PAD, No] with the rows beyond M
    holding what they held before.  `form` is the launch the selector reports: ("sgemm", MA, NB, U, NW, LN, GEGLU), ("mgemm",), ("tiled",).
    Near misses: the last 32-wide k-step of every wave's K share dropped (mgemm / tiled: the last 64-wide slice); the K shares of waves
    4..7 dropped (NW = 8); the residual added twice, and not at all; row M - 1 written to the rows of the ragged last tile beyond M; GEGLU
    value and gate swapped, the two 16-wide halves of a strip's 32 outputs exchanged; LayerNorm statistics over the first wave's K share
    only, of the neighbouring row, gamma / beta shifted by a K quarter."""
    name = "linear_rows"
    exact = False

    @staticmethod
    def make(M, N, K, form, act=ACT_NONE, ln=False, det=False, out="bf16", res=False, bias=True, offset=False, small_var=False, seed=131):
        g = torch.Generator().manual_seed(seed)
        No = N // 2 if act == ACT_GEGLU else N
        inp = {"M": M, "form": tuple(form), "act": act, "ln": ln, "det": det, "outs": out, "eps": 1e-5,
               "w": bfr(torch.randn(N, K, generator=g) * 2 / math.sqrt(K)), "b": 0.5 * torch.randn(N, generator=g) if bias else None}
        if ln:
            spread = 0.004 if small_var else 1.0
            off = row_offsets(M, seed + 1, 10.0, 30.0) * spread if offset else 0.3 * torch.randn(M, generator=g)
            # every K quarter (a wave's share) has its own spread and mean: statistics over one share are not the row's
            prof = lambda v: torch.tensor(v).repeat_interleave(K // 4)
            inp["x"] = ((torch.randn(M, K, generator=g) * prof([0.5, 1.0, 1.5, 1.0]) + prof([-0.5, 0.5, 0.25, -0.25])) * spread * (0.5 + torch.rand(M, 1, generator=g))
                        + off[:, None])
            inp["gamma"], inp["beta"] = 1 + 0.3 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
        else:
            inp["a"] = bfr(torch.randn(M, K, generator=g))
        # the buffers as they are before the call: the residual stream (its rows beyond M ordinary values), or a fill the kernel must leave
        inp["buf32"] = torch.randn(M + PAD, No, generator=g) if res else torch.full((M + PAD, No), -7.25)
        inp["buf16"] = torch.full((M + PAD, No), 5.5)
        inp["res"] = res
        return inp

    @staticmethod
    def tile_rows(inp):
        f = inp["form"]
        return 16 * f[1] if f[0] == "sgemm" else 64 if f[0] == "mgemm" else 128

    @staticmethod
    def operand(inp, dt, stats_k=None, shift=False, gshift=0):
        if not inp["ln"]:
            return inp["a"].to(dt)
        x = inp["x"].to(dt)
        xs = x if stats_k is None else x[:, :stats_k]
        mu = xs.mean(1, keepdim=True)
        rstd = 1 / torch.sqrt(((xs - mu) ** 2).mean(1, keepdim=True) + inp["eps"])
        if shift:
            mu, rstd = mu.roll(-1, 0), rstd.roll(-1, 0)
        return (x - mu) * rstd * inp["gamma"].to(dt).roll(gshift) + inp["beta"].to(dt).roll(gshift)

    @staticmethod
    def pre(inp, dt, kmask=None, absval=False, **kw):
        a, w = LinearRows.operand(inp, dt, **kw), inp["w"].to(dt)
        if absval:
            a, w = a.abs(), w.abs()
        if kmask is not None:
            a = a * kmask.to(dt)
        y = a @ w.t()
        if inp["b"] is not None:
            y = y + (inp["b"].to(dt).abs() if absval else inp["b"].to(dt))
        return y

    @staticmethod
    def ref(inp, dt, res_times=1, swap=False, halves=False, spill=False, **kw):
        M, act = inp["M"], inp["act"]
        y = LinearRows.pre(inp, dt, **kw)
        if act == ACT_GEGLU:
            F2 = y.shape[1] // 2
            xv, gt = (y[:, F2:], y[:, :F2]) if swap else (y[:, :F2], y[:, F2:])
            y = xv * _gelu(gt)
            if halves:
                y = y[:, torch.arange(F2) ^ 16]
        else:
            y = _act(y, act)
        if inp["res"]:
            y = y + res_times * inp["buf32"][:M].to(dt)
        out = {}
        for key, buf in (("out", inp["buf16"]), ("out32", inp["buf32"])):
            if (key == "out") == (inp["outs"] == "bf16") or inp["outs"] == "both":
                full = buf.to(dt).clone()
                full[:M] = y
                if spill:                                    # the clamped row M - 1 stored to the rows of its tile beyond M
                    full[M: -(-M // LinearRows.tile_rows(inp)) * LinearRows.tile_rows(inp)] = y[M - 1]
                out[key] = full
        return out

    @staticmethod
    def chain(inp):
        f, K = inp["form"], inp["w"].shape[1]
        return K // f[4] + f[4] + 2 if f[0] == "sgemm" else K + 2 if f[0] == "mgemm" else K + 8

    @staticmethod
    def bound(inp, ref):
        M, K, act = inp["M"], inp["w"].shape[1], inp["act"]
        c = LinearRows.chain(inp)
        S = LinearRows.pre(inp, F64, absval=True)
        e = c * U * S
        if inp["form"][0] == "tiled" and inp["b"] is not None:
            e = e + 2.0 ** -16 * inp["b"].double().abs()
        if inp["ln"]:
            x = inp["x"].double()
            d = K // 16 + 6
            mu = x.mean(1, keepdim=True)
            rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + inp["eps"])
            xh = (x - mu) * rstd
            gam, bet = inp["gamma"].double(), inp["beta"].double()
            e_xh = U * (d * x.abs().mean(1, keepdim=True) * rstd + (d + 8) * xh.abs())
            xn = gam * xh + bet
            e_xn = gam.abs() * e_xh + 2 * U * ((gam * xh).abs() + bet.abs()) + 2.0 ** -9 * xn.abs()
            e = e + e_xn @ inp["w"].double().abs().t()
        y = LinearRows.pre(inp, F64)
        if act == ACT_GEGLU:
            F2 = y.shape[1] // 2
            a = _geglu_bound(y[:, :F2], y[:, F2:], e[:, :F2], e[:, F2:])
        else:
            a = _act_bound(y, e, act)
        if inp["res"]:
            a = a + c * U * inp["buf32"][:M].double().abs()
        a = torch.cat([a, torch.zeros(PAD, a.shape[1], dtype=F64)])
        return {k: _rows_bound(M, M + PAD, BF if k == "out" else 0.0, a) for k in ref}

    @staticmethod
    def misses(inp):
        f, M, K = inp["form"], inp["M"], inp["w"].shape[1]
        k = torch.arange(K)
        if f[0] == "sgemm":
            kq = K // f[4]
            m = [("last k-step of every wave's K share dropped", LinearRows.ref(inp, F64, kmask=(k % kq) < kq - 32))]
            if f[4] == 8:
                m.append(("K shares of waves 4..7 dropped", LinearRows.ref(inp, F64, kmask=k < K // 2)))
        else:
            m = [("last 64-wide K slice dropped", LinearRows.ref(inp, F64, kmask=k < K - 64))]
        if inp["res"]:
            m += [("residual added twice", LinearRows.ref(inp, F64, res_times=2)), ("residual not added", LinearRows.ref(inp, F64, res_times=0))]
        if M % LinearRows.tile_rows(inp):
            m.append(("row M - 1 stored beyond M", LinearRows.ref(inp, F64, spill=True)))
        if inp["act"] == ACT_GEGLU:
            m += [("value and gate swapped", LinearRows.ref(inp, F64, swap=True)), ("halves of a strip exchanged", LinearRows.ref(inp, F64, halves=True))]
        if inp["ln"]:
            m += [("LayerNorm statistics over one wave's K share", LinearRows.ref(inp, F64, stats_k=K // 4)),
                  ("LayerNorm statistics of the next row", LinearRows.ref(inp, F64, shift=True)),
                  ("gamma / beta shifted by a K quarter", LinearRows.ref(inp, F64, gshift=K // 4))]
        return m


# ============================================================================================================ decode attention (K/V cache)
class DecodeAttention:
    """rdm_op_rarm_decode_attention at d_head 64.  mode "self": q | k_new | v_new columns of one fused bf16 row per sequence, head-major
    caches [B, H, L, 64]; k_new / v_new go to cache row t and rows 0..t are attended (row t from the projection output).  mode "cross":
    the executor's row-major neighbour buffer [B, cap, kv_total] (K and V column blocks of one layer, row_stride = kv_total, heads side by
    side), rows 0..nkv-1 attended -- by rarm_decode_attention_kernel<4>, or at batch >= 128 and nkv <= 8 by rarm_fewkey_attention_kernel.
    Cache rows beyond the attended range hold +-HUGE (the largest finite bf16): attended, they would dominate; row t holds an ordinary stale
    value before the call.  Arithmetic: s_j = sum of 8 products and 3 lane exchanges of (q scale) k (12 u sum |q k| scale); p_j = __expf(s_j
    - max) / l, l a sum of <= 13 adds; out = sum p_j v_j over <= 40 adds, one division, bf16.  rho_j = e_sj + max e_s + the __expf terms of
    numerator and denominator + 16 u;  a = sum_j p_j |v_j| (rho_j + 40 u), r = 2^-8.
    Near misses: row t not attended; the stale cache row t used for K, for V; one row past the range attended (on a copy where that row is
    ordinary); row j = 128 (the first of a wave's second chunk) dropped; the scale applied twice; the heads read with the other layout's
    strides; few-key kernel: the dead lanes j >= nkv counted as keys of score zero."""
    name = "decode_attention"
    exact = False

    @staticmethod
    def make(mode, B, H, t=None, L=None, nkv=None, seed=151):
        g = torch.Generator().manual_seed(seed)
        C = H * D
        sign = lambda shape: torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
        inp = {"mode": mode, "B": B, "H": H, "scale": D ** -0.5, "fewkey": mode == "cross" and B >= 128 and nkv <= 8}
        if mode == "self":
            inp["qkv"] = bfr(torch.randn(B, 3 * C, generator=g) * 1.5)
            ordinary = [bfr(torch.randn(B, H, L, D, generator=g) * 1.5) for _ in range(2)]     # rows < t: the history; row t: stale; beyond: for the near misses
            inp["t"], inp["L"], inp["n"] = t, L, t + 1
        else:
            cap, ld = nkv + 2, 4 * C                         # two layers' K | V column blocks; this call is layer 1's
            ordinary = [bfr(torch.randn(B, cap, ld, generator=g) * 1.5)]
            inp["q"] = bfr(torch.randn(B, C, generator=g) * 1.5)
            inp["n"], inp["cap"], inp["ld"] = nkv, cap, ld
        inp["ordinary"] = ordinary
        caches = []
        for o in ordinary:
            c = o.clone()
            if mode == "self":
                c[:, :, t + 1:] = HUGE * sign(c[:, :, t + 1:].shape)
            else:
                c[:, nkv:] = HUGE * sign(c[:, nkv:].shape)
            caches.append(c)
        inp["caches"] = caches
        return inp

    @staticmethod
    def from_state(qkv, K, V, t):
        """a self-mode case on a cache as it stands (no HUGE rows: every row ordinary): qkv [B, 3 H 64], K, V [B, H, L, 64] before the call"""
        B, H, L = K.shape[:3]
        return {"mode": "self", "B": B, "H": H, "scale": D ** -0.5, "fewkey": False, "qkv": qkv, "t": t, "L": L, "n": t + 1,
                "ordinary": [K, V], "caches": [K, V]}

    @staticmethod
    def operands(inp, dt, full=False):
        """(q [B,H,64], K, V [B,H,rows,64]) before the call; full: from the all-ordinary copy (every row of the buffer)"""
        B, H = inp["B"], inp["H"]
        C = H * D
        src = inp["ordinary"] if full else inp["caches"]
        if inp["mode"] == "self":
            return inp["qkv"][:, :C].reshape(B, H, D).to(dt), src[0].to(dt), src[1].to(dt)
        kv = src[0].to(dt)
        K = kv[:, :, 2 * C:3 * C].reshape(B, -1, H, D).transpose(1, 2)
        V = kv[:, :, 3 * C:4 * C].reshape(B, -1, H, D).transpose(1, 2)
        return inp["q"].reshape(B, H, D).to(dt), K, V

    @staticmethod
    def new_rows(inp, dt):
        B, H = inp["B"], inp["H"]
        C = H * D
        return inp["qkv"][:, C:2 * C].reshape(B, H, D).to(dt), inp["qkv"][:, 2 * C:].reshape(B, H, D).to(dt)

    @staticmethod
    def attend(q, K, V, scale, zero_keys=0):
        s = torch.einsum("bhd,bhjd->bhj", q, K) * scale
        if zero_keys:
            s = torch.cat([s, torch.zeros(s.shape[:2] + (zero_keys,), dtype=s.dtype)], 2)
            V = torch.cat([V, torch.zeros(V.shape[:2] + (zero_keys, D), dtype=V.dtype)], 2)
        p = torch.softmax(s, 2)
        return torch.einsum("bhj,bhjd->bhd", p, V).reshape(q.shape[0], -1), s, p

    @staticmethod
    def rows(inp, dt, stale_k=False, stale_v=False, full=False):
        """the attended K, V rows [B,H,n,64]"""
        q, K, V = DecodeAttention.operands(inp, dt, full)
        n = inp["n"]
        K, V = K[:, :, :n].clone(), V[:, :, :n].clone()
        if inp["mode"] == "self":
            kn, vn = DecodeAttention.new_rows(inp, dt)
            if not stale_k:
                K[:, :, n - 1] = kn
            if not stale_v:
                V[:, :, n - 1] = vn
        return q, K, V

    @staticmethod
    def ref(inp, dt, scale=None, drop=None, past=False, other_layout=False, zero_keys=0, **kw):
        q, K, V = DecodeAttention.rows(inp, dt, **kw)
        n = inp["n"]
        if past:                                              # one more row, ordinary on the copy
            _, Kf, Vf = DecodeAttention.operands(inp, dt, full=True)
            K, V = torch.cat([K, Kf[:, :, n:n + 1]], 2), torch.cat([V, Vf[:, :, n:n + 1]], 2)
        if other_layout:
            K, V = DecodeAttention.misread(inp, dt, K, 0), DecodeAttention.misread(inp, dt, V, 1)
        if drop is not None:
            keep = [j for j in range(K.shape[2]) if j != drop]
            K, V = K[:, :, keep], V[:, :, keep]
        return {"out": DecodeAttention.attend(q, K, V, inp["scale"] if scale is None else scale, zero_keys)[0]}

    @staticmethod
    def misread(inp, dt, X, which):
        """the attended rows as the OTHER layout's strides would address them in the same memory (all-ordinary copy, new row in place)"""
        B, H, n = inp["B"], inp["H"], inp["n"]
        C = H * D
        if inp["mode"] == "self":                            # head-major memory read as rows of H heads side by side
            mem = inp["ordinary"][which].to(dt).clone()
            mem[:, :, n - 1] = X[:, :, n - 1]
            return mem.reshape(B, -1)[:, :n * C].reshape(B, n, H, D).transpose(1, 2)
        mem = inp["ordinary"][0].to(dt).reshape(B, -1)[:, (2 + which) * C:]      # from the K (V) block's first element: head-major from there
        return mem[:, :H * n * D].reshape(B, H, n, D)

    @staticmethod
    def bound(inp, ref):
        q, K, V = DecodeAttention.rows(inp, F64)
        _, s, p = DecodeAttention.attend(q, K, V, inp["scale"])
        e_s = 12 * U * torch.einsum("bhd,bhjd->bhj", q.abs(), K.abs()) * inp["scale"]
        m = s.max(2, keepdim=True).values
        ex = 2.0 ** -21 * (2 + 2 * (s - m).abs())
        rho = e_s + e_s.max(2, keepdim=True).values + ex + (p * ex).sum(2, keepdim=True) + 16 * U
        a = torch.einsum("bhj,bhjd->bhd", p * (rho + 40 * U), V.abs()).reshape(q.shape[0], -1)
        return {"out": (BF, a)}

    @staticmethod
    def misses(inp):
        n = inp["n"]
        m = [("scale applied twice", DecodeAttention.ref(inp, F64, scale=inp["scale"] ** 2)),
             ("heads read with the other layout's strides", DecodeAttention.ref(inp, F64, other_layout=True))]
        if inp["mode"] == "self":
            if n > 1:
                m.append(("row t not attended", DecodeAttention.ref(inp, F64, drop=n - 1)))
            m += [("stale cache row t used for K", DecodeAttention.ref(inp, F64, stale_k=True)),
                  ("stale cache row t used for V", DecodeAttention.ref(inp, F64, stale_v=True))]
            if n < inp["L"]:
                m.append(("one row past the range attended", DecodeAttention.ref(inp, F64, past=True)))
        else:
            m.append(("one row past the range attended", DecodeAttention.ref(inp, F64, past=True)))
        if n > 128:
            m.append(("row 128 dropped", DecodeAttention.ref(inp, F64, drop=128)))
        if inp["fewkey"] and n < 8:
            m.append(("dead lanes counted as zero keys", DecodeAttention.ref(inp, F64, zero_keys=8 - n)))
        return m


# ============================================================================================================ one-launch cross-attention
class XattnDecode:
    """rdm_op_rarm_xattn_decode: x[b] += softmax_per_head(LN(x[b]) G[b]^T) UT[b] + bias for b < Bc, x[b] += bias beyond (fp32, in place),
    and ln3 = LayerNorm(the finished row) as bf16.  Two-pass LayerNorm over one channel per thread (sum: 6 lane exchanges + 16 wave sums,
    d = 22), rounded to bf16; a score = 16 products per lane + 6 exchanges (22); softmax over the head's k columns (k + 3 adds, __expf
    twice); the output = 32 rows per group + 4 groups + bias + x (38).  ln3: LayerNorm's own arithmetic on the kernel's fp32 row plus the
    propagated error of that row: |g| rstd (e_c + mean e + |xh_c| mean |xh e|).
    Near misses: one softmax over all heads * k columns; groups of k + 1; the LayerNorm statistics of the next row; a b >= Bc row given
    row b - Bc's attention; the bias left off the zero-neighbour rows; norm3 of the row before the update; row group 3 of 4 dropped."""
    name = "xattn_decode"
    exact = False

    @staticmethod
    def make(C, heads, k, B2, Bc, ln3=True, NP=128, seed=171):
        g = torch.Generator().manual_seed(seed)
        # neighbouring rows differ in the sign of their mean and threefold in spread: statistics of the wrong row cannot pass
        alt = torch.arange(B2) % 2
        x = torch.randn(B2, C, generator=g) * (0.5 + alt)[:, None] + (row_offsets(B2, seed + 1, 3.0, 10.0).abs() * (1 - 2 * alt))[:, None]
        vec = lambda s, o=0.0: o + s * torch.randn(C, generator=g)
        inp = {"x": x, "gamma": vec(0.3, 1.0), "beta": vec(0.3), "eps": 1e-5, "heads": heads, "k": k, "Bc": Bc, "NP": NP, "bias": vec(0.5),
               "G": bfr(torch.randn(Bc, NP, C, generator=g) * 2 / math.sqrt(C)), "UT": bfr(torch.randn(Bc, NP, C, generator=g)), "ln3": ln3}
        if ln3:
            inp["gamma3"], inp["beta3"] = vec(0.3, 1.0), vec(0.3)
        return inp

    @staticmethod
    def ln(x, g, b, eps, shift=False):
        mu = x.mean(1, keepdim=True)
        rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
        if shift:
            mu, rstd = mu.roll(-1, 0), rstd.roll(-1, 0)
        return (x - mu) * rstd * g + b

    @staticmethod
    def attn(inp, dt, group=None, shift=False, drop_group=False):
        """(the attention rows [Bc, C], scores, probabilities) of the first Bc sequences"""
        Bc, nrow = inp["Bc"], inp["heads"] * inp["k"]
        xn = XattnDecode.ln(inp["x"][:Bc].to(dt), inp["gamma"].to(dt), inp["beta"].to(dt), inp["eps"], shift)
        sc = torch.einsum("bjc,bc->bj", inp["G"][:, :nrow].to(dt), xn)
        gidx = torch.arange(nrow) // (inp["k"] if group is None else group)
        p = torch.zeros_like(sc)
        for gi in gidx.unique():
            sel = gidx == gi
            p[:, sel] = torch.softmax(sc[:, sel], 1)
        if drop_group:
            p = p * (torch.arange(nrow) % 4 != 3).to(dt)
        return torch.einsum("bj,bjc->bc", p, inp["UT"][:, :nrow].to(dt)), sc, p, xn

    @staticmethod
    def ref(inp, dt, wrap=False, no_bias_tail=False, ln3_before=False, **kw):
        x, Bc = inp["x"].to(dt), inp["Bc"]
        B2 = x.shape[0]
        o = XattnDecode.attn(inp, dt, **kw)[0]
        add = torch.zeros_like(x)
        add[:Bc] = o
        if wrap and B2 > Bc:
            add[Bc:] = o[(torch.arange(Bc, B2) - Bc) % Bc]
        bias = inp["bias"].to(dt).expand_as(x).clone()
        if no_bias_tail:
            bias[Bc:] = 0
        y = x + (bias + add)
        out = {"x": y}
        if inp["ln3"]:
            out["ln3"] = XattnDecode.ln(x if ln3_before else y, inp["gamma3"].to(dt), inp["beta3"].to(dt), inp["eps"])
        return out

    @staticmethod
    def bound(inp, ref):
        x, Bc, k = inp["x"].double(), inp["Bc"], inp["k"]
        C = x.shape[1]
        nrow = inp["heads"] * k
        e_x = 3 * U * (x.abs() + inp["bias"].double().abs())
        if Bc:
            o, sc, p, xn = XattnDecode.attn(inp, F64)
            xb = x[:Bc]
            mu = xb.mean(1, keepdim=True)
            rstd = 1 / torch.sqrt(((xb - mu) ** 2).mean(1, keepdim=True) + inp["eps"])
            xh = (xb - mu) * rstd
            gam, bet = inp["gamma"].double(), inp["beta"].double()
            e_xh = U * (22 * xb.abs().mean(1, keepdim=True) * rstd + 30 * xh.abs())
            e_xn = gam.abs() * e_xh + 2 * U * ((gam * xh).abs() + bet.abs()) + 2.0 ** -9 * xn.abs()
            Ga, Ua = inp["G"][:, :nrow].double().abs(), inp["UT"][:, :nrow].double().abs()
            e_s = torch.einsum("bjc,bc->bj", Ga, e_xn) + 22 * U * torch.einsum("bjc,bc->bj", Ga, xn.abs())
            hs = lambda t: t.reshape(Bc, inp["heads"], k)
            m = hs(sc).max(2, keepdim=True).values
            ex = 2.0 ** -21 * (2 + 2 * (hs(sc) - m).abs())
            rho = hs(e_s) + hs(e_s).max(2, keepdim=True).values + ex + (hs(p) * ex).sum(2, keepdim=True) + (k + 5) * U
            e_o = torch.einsum("bj,bjc->bc", p * (rho.reshape(Bc, nrow) + 38 * U), Ua)
            e_x[:Bc] = e_x[:Bc] + e_o + 3 * U * o.abs()
        out = {"x": (0.0, e_x)}
        if inp["ln3"]:
            y = ref["x"].double()
            mu = y.mean(1, keepdim=True)
            rstd = 1 / torch.sqrt(((y - mu) ** 2).mean(1, keepdim=True) + inp["eps"])
            yh = (y - mu) * rstd
            g3, b3 = inp["gamma3"].double(), inp["beta3"].double()
            e_yh = U * (22 * y.abs().mean(1, keepdim=True) * rstd + 30 * yh.abs()) + rstd * (e_x + e_x.mean(1, keepdim=True) + yh.abs() * (yh.abs() * e_x).mean(1, keepdim=True))
            out["ln3"] = (BF, g3.abs() * e_yh + 2 * U * ((g3 * yh).abs() + b3.abs()))
        return out

    @staticmethod
    def misses(inp):
        m = [("one softmax over all heads * k columns", XattnDecode.ref(inp, F64, group=inp["heads"] * inp["k"])),
             ("softmax groups of k + 1", XattnDecode.ref(inp, F64, group=inp["k"] + 1)),
             ("LayerNorm statistics of the next row", XattnDecode.ref(inp, F64, shift=True)),
             ("a b >= Bc row given row b - Bc's attention", XattnDecode.ref(inp, F64, wrap=True)),
             ("bias left off the zero-neighbour rows", XattnDecode.ref(inp, F64, no_bias_tail=True)),
             ("row group 3 of 4 dropped", XattnDecode.ref(inp, F64, drop_group=True))]
        if inp["ln3"]:
            m.append(("norm3 of the row before the update", XattnDecode.ref(inp, F64, ln3_before=True)))
        return m


# ============================================================================================================ token embedding
class Embed:
    """rdm_op_rarm_embed: x[r] = emb[token(r)] + pos_t[position(r)], one fp32 add: bitwise.  Decode form (pos): token(r) = tokens[r];
    sequence form (t): row r = position r % t of sequence r / t, tokens row (seq0 + r / t) % tok_rows.  Ids outside [0, vocab) read row 0.
    Near misses: ids taken modulo vocab instead; the token row clamped instead of wrapped; the position one further on."""
    name = "embed"
    exact = True

    @staticmethod
    def make(C, vocab, L, B=None, pos=None, tok_rows=None, tok_ld=None, t=None, seq0=0, n_seq=None, seed=191):
        g = torch.Generator().manual_seed(seed)
        inp = {"emb": torch.randn(vocab, C, generator=g), "pos_t": torch.randn(L, C, generator=g), "pos": pos, "t": t, "seq0": seq0, "n_seq": n_seq}
        shape = (B,) if pos is not None else (tok_rows, tok_ld)
        tok = torch.randint(0, vocab, shape, generator=g)
        flat = tok.reshape(-1)
        flat[0], flat[-1] = -1, vocab                       # out of range on both sides -> row 0
        if flat.numel() > 4:
            flat[2], flat[3] = vocab + 5, -(2 ** 40)
        inp["tokens"] = tok
        return inp

    @staticmethod
    def ref(inp, dt, modulo=False, clamp_row=False, pos_shift=0):
        emb, pos_t, tok = inp["emb"], inp["pos_t"], inp["tokens"]
        vocab, L = emb.shape[0], pos_t.shape[0]
        if inp["pos"] is not None:
            ids, ps = tok, torch.full_like(tok, (inp["pos"] + pos_shift) % L)
        else:
            t, rows = inp["t"], tok.shape[0]
            s = torch.arange(inp["n_seq"] if inp["n_seq"] is not None else rows)
            r = (inp["seq0"] + s).clamp(max=rows - 1) if clamp_row else (inp["seq0"] + s) % rows
            ids = tok[r, :t].reshape(-1)
            ps = ((torch.arange(t) + pos_shift) % L).repeat(len(s))
        ids = ids % vocab if modulo else torch.where((ids < 0) | (ids >= vocab), torch.zeros_like(ids), ids)
        return {"x": (emb[ids] + pos_t[ps]).to(dt)}         # one fp32 add, whatever dt carries it

    @staticmethod
    def bound(inp, ref):
        raise AssertionError("exact")

    @staticmethod
    def misses(inp):
        m = [("ids modulo vocab", Embed.ref(inp, F64, modulo=True)), ("position one further on", Embed.ref(inp, F64, pos_shift=1))]
        if inp["pos"] is None:
            m.append(("token row clamped, not wrapped", Embed.ref(inp, F64, clamp_row=True)))
        return m


# ============================================================================================================ the parametrisations
def bf16_out(case, inp, key):
    """does the kernel write this output as bf16 (the stand-in rounds it the same way)"""
    return key in ("out", "ln3") and case is not Embed


def _lr(form, M, N, K, **kw):
    name = "sgemm<%d, %d, %s%d, %sNW%d>" % (form[1], form[2], "GEGLU, " if form[6] else "", form[3], "LN, " if form[5] else "", form[4]) if form[0] == "sgemm" else form[0]
    tags = [name, "deterministic" if kw.get("det") else "fast", kw.get("out", "bf16") + (" in place on the residual" if kw.get("res") else "")]
    tags += [t for t in ("offset", "small_var") if kw.get(t)]
    return (LinearRows, dict(M=M, N=N, K=K, form=form, **kw), ", ".join(tags))


G_, S_ = ACT_GEGLU, ACT_SILU
# one case per form the selector returns over the grid (modes x K in {256, 768, 3072} x N in {256, 768, 2304} plain, {1024, 6144} GEGLU x
# M in 1..4096), at the smallest M N K that reaches it with M ragged against the tile (tests/test_decode_ops_cpu.py enumerates the grid
# and asserts both the set and every case's own form); the decode step's plain projections write the fp32 residual stream in place
LINEAR_ROWS = [
    _lr(("sgemm", 1, 1, 2, 4, False, False), 1, 256, 256, out="f32", res=True),
    _lr(("sgemm", 1, 2, 2, 4, False, False), 33, 2304, 256),
    _lr(("sgemm", 2, 2, 2, 4, False, False), 65, 2304, 256, out="f32", res=True),
    _lr(("sgemm", 4, 2, 2, 4, False, False), 129, 2304, 256, act=S_),
    _lr(("sgemm", 4, 4, 2, 4, False, False), 257, 2304, 256, out="f32", res=True),
    _lr(("sgemm", 1, 1, 6, 4, False, False), 1, 256, 768, out="both"),
    _lr(("sgemm", 1, 2, 6, 4, False, False), 33, 2304, 768, out="f32", res=True),
    _lr(("sgemm", 2, 2, 6, 4, False, False), 65, 2304, 768, out="f32", bias=False),
    _lr(("sgemm", 4, 2, 6, 4, False, False), 481, 768, 768, det=True, out="f32", res=True),
    _lr(("sgemm", 4, 4, 3, 4, False, False), 257, 2304, 768),
    _lr(("sgemm", 4, 2, 3, 8, False, False), 481, 768, 768, out="f32", res=True),
    _lr(("sgemm", 4, 4, 3, 8, False, False), 897, 768, 768, out="f32", res=True),
    _lr(("sgemm", 4, 6, 3, 8, False, False), 449, 2304, 768),
    _lr(("sgemm", 4, 2, 6, 8, False, False), 481, 768, 3072, out="f32", res=True),
    _lr(("sgemm", 1, 2, 2, 4, False, True), 1, 1024, 256, act=G_),
    _lr(("sgemm", 2, 2, 2, 4, False, True), 17, 6144, 256, act=G_),
    _lr(("sgemm", 1, 4, 2, 4, False, True), 33, 6144, 256, act=G_),
    _lr(("sgemm", 2, 4, 2, 4, False, True), 49, 6144, 256, act=G_),
    _lr(("sgemm", 4, 4, 2, 4, False, True), 97, 6144, 256, act=G_),
    _lr(("sgemm", 1, 2, 6, 4, False, True), 1, 1024, 768, act=G_),
    _lr(("sgemm", 2, 2, 6, 4, False, True), 17, 6144, 768, act=G_),
    _lr(("sgemm", 1, 4, 6, 4, False, True), 33, 6144, 768, act=G_),
    _lr(("sgemm", 2, 4, 6, 4, False, True), 49, 6144, 768, act=G_),
    _lr(("sgemm", 4, 4, 6, 4, False, True), 97, 6144, 768, act=G_),
    _lr(("sgemm", 1, 1, 6, 4, True, False), 1, 256, 768, ln=True, offset=True),
    _lr(("sgemm", 1, 2, 6, 4, True, False), 97, 768, 768, ln=True, offset=True),
    _lr(("sgemm", 1, 2, 6, 4, True, False), 97, 768, 768, ln=True, offset=True, small_var=True),
    _lr(("sgemm", 2, 2, 6, 4, True, False), 241, 768, 768, ln=True, det=True, offset=True),
    _lr(("sgemm", 2, 2, 6, 4, True, False), 241, 768, 768, ln=True, det=True, small_var=True),
    _lr(("sgemm", 1, 2, 6, 4, True, True), 1, 1024, 768, ln=True, act=G_, offset=True),
    _lr(("sgemm", 1, 4, 6, 4, True, True), 17, 6144, 768, ln=True, act=G_, offset=True, small_var=True),
    _lr(("sgemm", 2, 4, 6, 4, True, True), 49, 6144, 768, ln=True, act=G_, offset=True),
    _lr(("sgemm", 2, 4, 6, 4, True, True), 49, 6144, 768, ln=True, act=G_),
    _lr(("mgemm",), 1537, 256, 256),
    _lr(("mgemm",), 1600, 256, 768, out="f32", res=True),
    _lr(("tiled",), 193, 1024, 256, act=G_),
]
# the shapes the LayerNorm-in-kernel form declines (rdm_op_linear_rows fails with its own code, the executor runs LayerNorm + linear)
LINEAR_ROWS_REFUSED = [dict(M=1, N=256, K=256, act=ACT_NONE, det=False), dict(M=193, N=768, K=768, act=ACT_NONE, det=False)]

_SELF_T = (0, 1, 7, 8, 31, 32, 33, 127, 128, 129, 255, 1023)
DECODE_ATTENTION = ([(DecodeAttention, dict(mode="self", B=2, H=3, t=t, L=1024), f"rarm_decode_attention_kernel<4>: self, append at {t}, {-(-(t + 1) // 32)} chunks") for t in _SELF_T]
                    + [(DecodeAttention, dict(mode="cross", B=2, H=3, nkv=n), f"rarm_decode_attention_kernel<4>: cross, row-major, {n} keys") for n in (1, 3, 8, 9, 33)]
                    + [(DecodeAttention, dict(mode="cross", B=128, H=5, nkv=n), f"rarm_fewkey_attention_kernel: {n} keys, 5 heads on 4 waves") for n in (1, 5, 8)])

XATTN_DECODE = [(XattnDecode, dict(C=C, heads=h, k=k, B2=B2, Bc=Bc, ln3=ln3), f"rarm_xattn_decode_kernel: C {C}, {h} heads x {k}, {Bc} of {B2} rows with neighbours{', norm3' if ln3 else ''}")
                for (C, h, k), (B2, Bc), ln3 in (((768, 12, 8), (6, 3), True), ((768, 12, 8), (2, 2), False), ((768, 12, 1), (6, 3), True), ((768, 12, 5), (6, 3), False),
                                                 ((768, 12, 5), (2, 2), True), ((1024, 16, 8), (6, 3), True), ((1024, 16, 8), (2, 2), False), ((192, 3, 4), (6, 3), True),
                                                 ((192, 3, 4), (2, 2), False))]

EMBED = [(Embed, dict(C=768, vocab=50, L=16, B=7, pos=0), "rarm_embed_kernel: position 0"),
         (Embed, dict(C=200, vocab=50, L=16, B=3, pos=15), "rarm_embed_kernel: C % 256 != 0, last position"),
         (Embed, dict(C=768, vocab=50, L=16, tok_rows=3, tok_ld=12, t=9, seq0=2, n_seq=5), "rarm_embed_seq_kernel: token rows wrap, pitch > t"),
         (Embed, dict(C=72, vocab=9, L=4, tok_rows=2, tok_ld=4, t=4), "rarm_embed_seq_kernel: t = L")]

CASES = LINEAR_ROWS + DECODE_ATTENTION + XATTN_DECODE + EMBED


def case_id(entry):
    case, kw, _ = entry
    short = lambda v: "x".join(str(int(e)) if isinstance(e, bool) else str(e) for e in v) if isinstance(v, tuple) else v
    return case.name + "-" + "-".join(f"{k}{short(v)}" for k, v in kw.items())
