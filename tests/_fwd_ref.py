"""Float64 restatements of the inference forward ops (linear / lin4 / sgemm / mgemm, the LayerNorm-folded projection, conv3x3 on every
launch path, the stem conv, GroupNorm, LayerNorm, flash and small attention, the fused cross-attention, the head conv and its VALU
fallback), their per-element error bounds and their near misses.  Shared by tests/test_gpu_forward_ops.py (the HIP kernels through the C ABI) and
tests/test_forward_ops_cpu.py (an fp32 torch restatement standing in for the kernels).  Same CASE contract as tests/_train_ref.py:
`make(**shape)`, `ref(inp, dt)`, `bound(inp, ref)` -> per output (r, a), `misses(inp)`; `check()` asserts |out - ref| <= r |ref| + a
element by element and that the output falls outside the bound against every near miss.

Bound conventions (u = 2^-24): r = 2^-8 for a bf16 output, 0 for an fp32 output; a = c u S with S the fp64 sum of the absolute values
of the terms of the element and c the chain of the launch geometry, stated per op.  The bf16 MFMAs are taken as one fp32 rounding per
product, accumulated in k order (c = K for a K-long dot product; a K-split part and its finisher add at most 3 more).  Every rounding
a kernel adds by design has its own term:
  * bias / time-embedding start values carried as bf16 (hi, lo) pairs (lin4, halo4): 2^-16 |b|;
  * the phase-upsample conv's pre-summed 2 x 2 weights stored as bf16: 2^-9 sum |x| |w| over the original taps;
  * the LayerNorm-folded weights bf16(gamma o W): 2^-9 rstd sum |x - mu| |gamma w|;
  * the attention probabilities rounded to bf16 before the PV MFMA (flash, fused cross-attention): 2^-8 P;
  * the head conv's activations rounded to bf16 and its fp32 weights carried as bf16 hi + lo: 2^-9 |act| and 2^-16 |w|.
No bound is scaled by a whole-tensor maximum."""
import math

import torch
import torch.nn.functional as F

from _train_ref import BF, F64, U, _cdiv, bfr, rand, row_offsets

NCU = 256                                     # MI355X compute units: the launchers' K-split and tile decisions read the device's count
ACT_NONE, ACT_GEGLU, ACT_QUICKGELU, ACT_SILU = 0, 1, 2, 3
HILO = 2.0 ** -16                             # fp32 value carried as a bf16 (hi, lo) pair


def _gelu(g, tanh=False):
    if tanh:
        return 0.5 * g * (1 + torch.tanh(math.sqrt(2 / math.pi) * (g + 0.044715 * g ** 3)))
    return 0.5 * g * (1 + torch.erf(g / math.sqrt(2)))


def _act(y, act):
    if act == ACT_SILU:
        return y * torch.sigmoid(y)
    if act == ACT_QUICKGELU:
        return y * torch.sigmoid(1.702 * y)
    return y


def _act_bound(y, e_y, act):
    """error of act(y) given an error e_y of y: |act'| <= 1.1 for SiLU / QuickGELU, plus __expf / rcp (2^-21 (2 + 2|y|) relative)"""
    if act in (ACT_SILU, ACT_QUICKGELU):
        return 1.1 * e_y + 2.0 ** -21 * (2 + 2 * y.abs()) * _act(y, act).abs()
    return e_y


def _geglu_bound(xv, g, e_x, e_g):
    """h = x gelu(g): gelu' <= 1.13, the kernel's erf polynomial u |g| (8 + g^2) / 2 (tests/_train_ref.Geglu)"""
    return _gelu(g).abs() * e_x + 1.13 * xv.abs() * e_g + U * xv.abs() * (g.abs() * (8 + g * g) / 2 + 2 * _gelu(g).abs())


# ============================================================================================================ launch geometry (host)
def lin4_wm(M, N):
    if N % 384 == 0 and M % 128 == 0:
        return 1
    if N % 192 == 0 and M % 256 == 0:
        return 2
    return 0


def linear_path(M, N, K, act=ACT_NONE, alpha=1.0, f32=False, res=False, rows=None, mgemm=False):
    """the kernel rdm_op_linear / rdm_op_linear_rowvec launches for this call (dispatch.hip Ops::linear, lin4_supported, launch_igemm)"""
    if M <= 128 and alpha == 1.0 and rows is None and K % 256 == 0 and (N % 64 == 0 if act == ACT_GEGLU else N % 32 == 0):
        return "sgemm"
    if mgemm:
        assert M >= 64 and alpha == 1.0 and rows is None and act != ACT_GEGLU
        return "mgemm"
    wm = lin4_wm(M, N)
    ok = wm and K % 64 == 0 and alpha == 1.0 and not f32 and act in (ACT_NONE, ACT_GEGLU) and not (act == ACT_GEGLU and res) and N <= 8192
    if ok and rows is not None:
        ok = rows % (128 * wm) == 0 and 2 * rows >= M
    if ok and (M // (128 * wm)) * (N // (384 if wm == 1 else 192)) >= 128:
        return f"lin4<{'GEGLU' if act == ACT_GEGLU else 'plain'}, WM{wm}{', rowvec' if rows else ''}>"
    wide = N % 192 == 0
    tall = _cdiv(M, 256) * _cdiv(N, 192 if wide else 128) >= 256 and M > 128
    if act == ACT_GEGLU:
        if tall and N % 256 == 0 and _cdiv(M, 256) * (N // 256) >= 256:
            return "igemm<256, 256, GEGLU>"
        return "igemm<256, 128, GEGLU>" if tall else "igemm<128, 128, GEGLU>"
    resk = res and not f32 and alpha == 1.0 and act == ACT_NONE and N % (192 if wide else 128) == 0
    return f"igemm<{256 if tall else 128}, {192 if wide else 128}{', res_k' if resk else ''}>"


def conv3x3_kernel(B, H, W, C, N, stride, rowvec):
    """conv3x3_kernel (conv_halo.hip) for a conv whose OUTPUT is H x W: the halo4 form that takes it, or None: the implicit GEMM"""
    HW = H * W
    if stride != 1 or (B * HW) % 256 or C % 64 or (rowvec and HW % 32):
        return None
    if W > 64:
        if W % 64 or H % 4 or max(H, W) > 4096 or (N % 192 and N % 128):
            return None
        return f"halo4<{3 if N % 192 == 0 else 2}, STRIP>"
    if W < 4 or 256 % W or (N % 192 and N % 128):
        return None
    if (HW % 256 or H % (256 // W)) if HW >= 256 else 256 % HW:
        return None
    RS = 256 // W if HW >= 256 else H                  # halo4_geom (common.h)
    HPW, NROW = W + 2, 256 // (RS * W) * (RS + 2)
    HBYTES = (NROW * (HPW * 144 + (224 if W <= 16 else 0)) + 255) & ~255
    if HBYTES > 66560 or NROW * ((HPW + 7) >> 3) > 84 or NROW * HPW > 400:
        return None
    return f"halo4<{3 if N % 192 == 0 else 2}>"


def conv_ksplit(B, H, W, C, N):
    bn = 192 if N % 192 == 0 else 128
    tiles = (B * H * W // 256) * (N // bn)
    if tiles * 4 > NCU * 3:
        return 1
    best, bestc = 1, 1.0
    for S in (2, 3):
        if C // 64 < 2 * S:
            continue
        c = _cdiv(tiles * S, NCU) / S * (1.0 + 0.06 * (S - 1))
        if c < bestc - 0.08:
            best, bestc = S, c
    return best


def conv_path(B, H, W, C, N, stride=1, ups=0, dual=False, rowvec=False, res=False):
    """(kernel, K-split planes) rdm_op_conv3x3 launches (dispatch.hip Ops::conv3, conv_halo.hip launch_conv3x3); H, W: the input"""
    Ho, Wo = (2 * H, 2 * W) if ups else ((H // 2, W // 2) if stride == 2 else (H, W))
    if ups and not dual and C % 64 == 0 and N % 8 == 0 and not rowvec and not res and stride == 1:
        return "igemm phase2", 1
    kernel = conv3x3_kernel(B, Ho, Wo, C, N, stride, rowvec)
    if kernel is None:
        return ("igemm ups" if ups else "igemm conv"), 1
    return kernel, (1 if "STRIP" in kernel else conv_ksplit(B, Ho, Wo, C, N))


def gn_onepass_plan(HW, C):
    """(slice groups, threads, NV) of gn_onepass_kernel (norm.hip gn_onepass_plan) or None: the two-pass gn_stats + gn_apply"""
    cg = C // 32
    if HW > 1024 or HW < 1:
        return None
    want = HW * C / 4
    best = None
    for g in range(1, 33):
        if 32 % g or (g * cg) % 8 or g * cg * 2 < 96:
            continue
        VS = g * cg // 8
        t_ok = n_ok = 0
        for t in (256, 512, 1024):
            if VS > t:
                continue
            R = t // VS; n = _cdiv(HW, R)
            if n <= (16 if t == 1024 else 32):
                t_ok, n_ok = t, n
                break
        if not t_ok:
            continue
        d = abs(g * cg * HW - want)
        if best is None or d < best[0]:
            best = (d, g, t_ok, 4 if n_ok <= 4 else 8 if n_ok <= 8 else 16 if n_ok <= 16 else 32)
    return None if best is None else best[1:]


# ============================================================================================================ linear
class Linear:
    """y = act(alpha a w^T + b (+ rowvec[row // rows]) (+ res)), bf16 operands, fp32 accumulation.  e_y = (K + 8) u S + 2^-16 (|b| +
    |rowvec|) with S = sum_k |alpha a_k w_k| + |b| + |rowvec| + |res| (a K-long chain of product roundings, the epilogue adds; the start
    values' (hi, lo) carriage).  SiLU / QuickGELU / GEGLU: propagated as _act_bound / _geglu_bound.  r = 2^-8 (bf16 out) or 0.  Near
    misses: the last 64-wide K slice (16 k of a one-slice K) dropped; alpha applied twice; a bias-only epilogue where the residual belongs; the row-group split one
    tile (128 rows) off; tanh GELU; value and gate swapped; SiLU and QuickGELU exchanged.
    res_f32 (the CLIP towers' x += proj(h), rdm_op_linear_res_f32): the residual is fp32, NOT rounded to bf16, and is added to the finished
    fp32 y in one rounding: e = e_y (the fp32-output model, the residual not in S) + u (|res| + |y|), r = 0.  Its near misses: the
    residual dropped; the residual of row m + 1; the bias dropped."""
    name = "linear"
    exact = False

    @staticmethod
    def make(M, N, K, act=ACT_NONE, bias=True, res=False, f32=False, alpha=1.0, rows=None, mgemm=False, seed=31, res_f32=False):
        g = torch.Generator().manual_seed(seed)
        inp = {"a": bfr(torch.randn(M, K, generator=g)), "w": bfr(torch.randn(N, K, generator=g) * 2 / math.sqrt(K)), "act": act, "f32": f32,
               "alpha": alpha, "rows": rows, "mgemm": mgemm, "b": 0.5 * torch.randn(N, generator=g) if bias else None,
               "res": bfr(torch.randn(M, N // 2 if act == ACT_GEGLU else N, generator=g)) if res else None, "res_f32": res_f32}
        if res_f32:                                          # an fp32 residual stream: full mantissas, a few times the projection's size
            assert f32 and not res and act != ACT_GEGLU and rows is None and alpha == 1.0
            inp["res"] = 3.0 * torch.randn(M, N, generator=g)
        if rows is not None:
            inp["rv"] = torch.randn(_cdiv(M, rows), N, generator=g)
        return inp

    @staticmethod
    def pre(inp, dt, kcut=None, alpha=None, rows=None, absval=False, no_bias=False):
        a, w = inp["a"].to(dt), inp["w"].to(dt)
        if absval:
            a, w = a.abs(), w.abs()
        if kcut:
            a, w = a[:, :kcut], w[:, :kcut]
        al = inp["alpha"] if alpha is None else alpha
        y = (abs(al) if absval else al) * (a @ w.t())
        if inp["b"] is not None and not no_bias:
            y = y + (inp["b"].to(dt).abs() if absval else inp["b"].to(dt))
        if "rv" in inp:
            rv = inp["rv"].to(dt).abs() if absval else inp["rv"].to(dt)
            y = y + rv.repeat_interleave(inp["rows"] if rows is None else rows, 0)[: y.shape[0]]
        return y

    @staticmethod
    def ref(inp, dt, kcut=None, alpha=None, rows=None, no_res=False, act=None, tanh=False, swap=False, no_bias=False, res_shift=False):
        y = Linear.pre(inp, dt, kcut, alpha, rows, no_bias=no_bias)
        act = inp["act"] if act is None else act
        if inp.get("res_f32"):                               # added to the finished (activated) fp32 value
            y = _act(y, act)
            return {"out": y if no_res else y + (inp["res"].roll(-1, 0) if res_shift else inp["res"]).to(dt)}
        if act == ACT_GEGLU:
            F2 = y.shape[1] // 2
            xv, gt = (y[:, F2:], y[:, :F2]) if swap else (y[:, :F2], y[:, F2:])
            return {"out": xv * _gelu(gt, tanh)}
        if inp["res"] is not None and not no_res:
            y = y + inp["res"].to(dt)
        return {"out": _act(y, act)}

    @staticmethod
    def bound(inp, ref):
        K = inp["a"].shape[1]
        S = Linear.pre(inp, F64, absval=True)
        carried = torch.zeros_like(S)
        if inp["b"] is not None:
            carried = carried + inp["b"].double().abs()
        if "rv" in inp:
            carried = carried + inp["rv"].double().abs().repeat_interleave(inp["rows"], 0)[: S.shape[0]]
        if inp["res"] is not None and not inp.get("res_f32"):
            S = S + inp["res"].double().abs()
        e = (K + 8) * U * S + HILO * carried
        r = 0.0 if inp["f32"] else BF
        y = Linear.pre(inp, F64)
        if inp.get("res_f32"):
            z = _act(y, inp["act"])
            return {"out": (r, _act_bound(y, e, inp["act"]) + U * (inp["res"].double().abs() + z.abs()))}
        if inp["act"] == ACT_GEGLU:
            F2 = y.shape[1] // 2
            return {"out": (r, _geglu_bound(y[:, :F2], y[:, F2:], e[:, :F2], e[:, F2:]))}
        if inp["res"] is not None:
            y = y + inp["res"].double()
        return {"out": (r, _act_bound(y, e, inp["act"]))}

    @staticmethod
    def misses(inp):
        K = inp["a"].shape[1]
        m = [("last K slice dropped", Linear.ref(inp, F64, kcut=K - 64))] if K >= 128 else [("last 16 k dropped", Linear.ref(inp, F64, kcut=K - 16))]
        if inp["alpha"] != 1.0:
            m.append(("alpha applied twice", Linear.ref(inp, F64, alpha=inp["alpha"] ** 2)))
        if inp["res"] is not None:
            m.append(("bias-only epilogue (residual dropped)", Linear.ref(inp, F64, no_res=True)))
        if inp.get("res_f32"):
            m.append(("residual of row m + 1", Linear.ref(inp, F64, res_shift=True)))
            if inp["b"] is not None:
                m.append(("bias dropped", Linear.ref(inp, F64, no_bias=True)))
        if inp["rows"] is not None:
            m.append(("row-group split one tile off", Linear.ref(inp, F64, rows=inp["rows"] + 128)))
        if inp["act"] == ACT_GEGLU:
            m += [("tanh GELU", Linear.ref(inp, F64, tanh=True)), ("value and gate swapped", Linear.ref(inp, F64, swap=True))]
        if inp["act"] in (ACT_SILU, ACT_QUICKGELU):
            m.append(("SiLU <-> QuickGELU", Linear.ref(inp, F64, act=ACT_SILU + ACT_QUICKGELU - inp["act"])))
        return m


class LinearLN:
    """act(LayerNorm(x; gamma, beta, eps) W^T + b) through lin4 <.., LN>, which forms rstd (x (gamma o W)'^T - mu s) + b' per row:
    the GEMM runs on the RAW rows against g' = bf16(gamma o W), s = sum_k g'_k, b' = b + sum_k beta_k w_k, and the row statistics are
    one-pass fp32 sums of x and x^2 over 8 lanes (K / 8 elements each) and 3 DPP levels, var = E[x^2] - mean^2.  Error model:
      e_acc = (K + 2) u sum |x| |g'|;   e_mu = c_s u mean|x|, c_s = K / 8 + 3;   e_s = (K / 64 + 7) u sum |g'|;
      rstd relative e_r = (c_s u mean(x^2) + 2 |mu| e_mu + 2 u (mean(x^2) + mu^2)) / (2 (var + eps)) + 4 u   (the one-pass variance);
      the rounding of gamma o W: 2^-9 rstd sum |x - mu| |gamma w|;   b': (K / 64 + 7) u (sum |beta w| + |b|);
      a = rstd (e_acc + |s| e_mu + |mu| e_s + u (|mu s| + |z|)) + e_r rstd |z| + (rounding of gamma o W) + e_b' + 2 u |y|, z = acc - mu s.
    GEGLU propagates as in Linear.  Near misses: eps 1e-6 (rows of small variance), the statistics of the next row, value and gate swapped,
    the bias dropped."""
    name = "linear_ln"
    exact = False

    @staticmethod
    def make(M, N, K, act=ACT_NONE, bias=True, offset=False, small_var=False, seed=41):
        g = torch.Generator().manual_seed(seed)
        spread = 0.004 if small_var else 1.0
        off = row_offsets(M, seed + 1, 10.0, 30.0) * spread if offset else 0.3 * torch.randn(M, generator=g)
        x = bfr(torch.randn(M, K, generator=g) * spread * (0.5 + torch.rand(M, 1, generator=g)) + off[:, None])
        return {"x": x, "w": bfr(torch.randn(N, K, generator=g) * 2 / math.sqrt(K)), "gamma": 1 + 0.3 * torch.randn(K, generator=g),
                "beta": 0.3 * torch.randn(K, generator=g), "b": 0.5 * torch.randn(N, generator=g) if bias else None, "act": act, "eps": 1e-5,
                "small_var": small_var, "offset": offset}

    @staticmethod
    def ref(inp, dt, eps=None, shift=False, no_bias=False, swap=False):
        x = inp["x"].to(dt)
        mu = x.mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True)
        rstd = 1 / torch.sqrt(var + (inp["eps"] if eps is None else eps))
        if shift:
            mu, rstd = mu.roll(-1, 0), rstd.roll(-1, 0)
        y = ((x - mu) * rstd * inp["gamma"].to(dt) + inp["beta"].to(dt)) @ inp["w"].to(dt).t()
        if inp["b"] is not None and not no_bias:
            y = y + inp["b"].to(dt)
        if inp["act"] == ACT_GEGLU:
            F2 = y.shape[1] // 2
            xv, gt = (y[:, F2:], y[:, :F2]) if swap else (y[:, :F2], y[:, F2:])
            return {"out": xv * _gelu(gt)}
        return {"out": y}

    @staticmethod
    def bound(inp, ref):
        x, w, gam, bet = inp["x"].double(), inp["w"].double(), inp["gamma"].double(), inp["beta"].double()
        K = x.shape[1]
        gw = gam[None, :] * w
        gq = bfr(gw.float()).double()
        mu = x.mean(1, keepdim=True); ex2 = (x * x).mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True); rstd = 1 / torch.sqrt(var + inp["eps"])
        c_s = K // 8 + 3
        e_acc = (K + 2) * U * (x.abs() @ gq.abs().t())
        e_mu = c_s * U * x.abs().mean(1, keepdim=True)
        s = gq.sum(1)[None, :]
        e_s = (K // 64 + 7) * U * gq.abs().sum(1)[None, :]
        e_r = (c_s * U * ex2 + 2 * mu.abs() * e_mu + 2 * U * (ex2 + mu * mu)) / (2 * (var + inp["eps"])) + 4 * U
        z = x @ gq.t() - mu * s
        b_abs = (bet.abs()[None, :] @ w.abs().t())
        bp = bet[None, :] @ w.t()
        if inp["b"] is not None:
            b_abs = b_abs + inp["b"].double().abs(); bp = bp + inp["b"].double()
        y = rstd * z + bp
        e = (rstd * (e_acc + s.abs() * e_mu + mu.abs() * e_s + U * ((mu * s).abs() + z.abs())) + e_r * rstd * z.abs()
             + 2.0 ** -9 * rstd * ((x - mu).abs() @ gw.abs().t()) + (K // 64 + 7) * U * b_abs + 2 * U * y.abs())
        if inp["act"] == ACT_GEGLU:
            F2 = y.shape[1] // 2
            return {"out": (BF, _geglu_bound(y[:, :F2], y[:, F2:], e[:, :F2], e[:, F2:]))}
        return {"out": (BF, e)}

    @staticmethod
    def misses(inp):
        m = [("statistics of the next row", LinearLN.ref(inp, F64, shift=True))]
        if inp["small_var"]:
            m.append(("eps 1e-6", LinearLN.ref(inp, F64, eps=1e-6)))
        if inp["act"] == ACT_GEGLU:
            # (tanh GELU is Linear's near miss: it moves an output by ~1e-3 relative, below this bound's 2^-9 sum over the rounded
            # gamma o W products)
            m.append(("value and gate swapped", LinearLN.ref(inp, F64, swap=True)))
        if inp["b"] is not None:
            m.append(("bias dropped", LinearLN.ref(inp, F64, no_bias=True)))
        return m


# ============================================================================================================ conv3x3
class Conv3x3:
    """3x3 conv (pad 1; stride 1 or 2; fused nearest-2x upsample) of [x0 | x1] (bf16 NHWC) with W [N, C, 3, 3] (bf16) + bias (+ a per-sample
    time-embedding row of pitch rowvec_ld >= N) (+ bf16 residual) -> bf16.  K = 9 C products in a k-ordered chain (K-split: each plane a
    chain of its slices, then the finisher's <= 3 adds of fp32 planes); a = (K + 8) u S + 2^-16 (|b| + |t|) (start values as (hi, lo)
    pairs); the phase-upsample igemm adds 2^-9 sum |x| |w| (its pre-summed 2 x 2 weights are stored as bf16).  Inputs: x carries a
    positive offset and the weights of the K-split parts have means of opposite sign, so each partial plane is large while their sum is
    small (a plane rounded to bf16 is seen) and every 64-channel slice carries weight.  Near misses: the K-split planes rounded to bf16;
    the last 64-channel slice of tap (2, 2) dropped; the taps flipped; the neighbouring sample's rows instead of the zero padding (and, on
    strips, zero padding at the 64-column strip edges instead of the neighbouring strip's pixels); the time-embedding row of sample b + 1;
    the bias missing on the last 8 channels; bilinear instead of nearest upsample; the residual dropped.
    asym = 1 (rdm_op_conv3x3_down, IgemmParams::asym): the first-stage encoder's Downsample, conv2d(pad(x, (0, 1, 0, 1)), w, stride 2) without
    further padding -- the window of output (oy, ox) starts AT input (2 oy, 2 ox), zero beyond the last row and column; bound and launch
    geometry are those of the stride-2 generic conv.  Its near misses: the symmetric padding-1 stride-2 conv (window origin one up and
    left); the zero row / column on the other side, pad (1, 0, 1, 0); the conv without its bias."""
    name = "conv3x3"
    exact = False

    @staticmethod
    def make(B, H, W, C0, N, C1=0, stride=1, ups=0, rowvec=False, ld_pad=0, res=False, seed=51, asym=0):
        g = torch.Generator().manual_seed(seed)
        C = C0 + C1
        assert not asym or (stride == 2 and not (ups or C1 or rowvec or res) and H % 2 == 0 and W % 2 == 0)
        kind, S = conv_path(B, H, W, C, N, stride, ups, C1 > 0, rowvec, res)
        x = bfr(torch.randn(B, H, W, C, generator=g) + 1.5)
        mean = torch.zeros(C)
        if S > 1:                                            # slice split of the planes: part s holds slices [s n / S, (s + 1) n / S)
            ns = C // 64
            bounds = [(s * ns // S * 64, (s + 1) * ns // S * 64) for s in range(S)]
            for lo, hi in bounds[:-1]:
                mean[lo:hi] = 1.0
            lo, hi = bounds[-1]
            mean[lo:hi] = -(bounds[-1][0]) / (hi - lo)
        w = bfr((torch.randn(N, C, 3, 3, generator=g) + 0.5 * mean[None, :, None, None]) / math.sqrt(9 * C))
        Ho, Wo = (2 * H, 2 * W) if ups else ((H // 2, W // 2) if stride == 2 else (H, W))
        inp = {"x": x, "C0": C0, "w": w, "b": 0.5 * torch.randn(N, generator=g), "stride": stride, "ups": ups, "S": S, "kind": kind, "asym": asym}
        if rowvec:
            inp["t"] = torch.randn(B, N + ld_pad, generator=g)
        if res:
            inp["res"] = bfr(torch.randn(B, Ho, Wo, N, generator=g))
        return inp

    @staticmethod
    def conv(inp, dt, x=None, w=None, mode="nearest", stack=False, strips=False, pad=(0, 1, 0, 1)):
        x = (inp["x"] if x is None else x).to(dt).permute(0, 3, 1, 2)
        w = (inp["w"] if w is None else w).to(dt)
        if inp.get("asym") and pad is not None:                 # pad None: the symmetric conv below
            return F.conv2d(F.pad(x, pad), w, stride=2).permute(0, 2, 3, 1)
        if inp["ups"]:
            x = F.interpolate(x, scale_factor=2, mode=mode, **({} if mode == "nearest" else {"align_corners": False}))
        if stack:                                            # the samples stacked vertically: each one's top / bottom pad row is its neighbour
            B, C, H, W = x.shape
            y = F.conv2d(x.permute(1, 0, 2, 3).reshape(1, C, B * H, W), w, padding=1)
            return y.reshape(-1, B, H, W).permute(1, 2, 3, 0)
        if strips:                                           # every 64-column strip zero-padded on its own
            return torch.cat([F.conv2d(x[..., s:s + 64], w, padding=1) for s in range(0, x.shape[3], 64)], 3).permute(0, 2, 3, 1)
        return F.conv2d(x, w, stride=inp["stride"], padding=1).permute(0, 2, 3, 1)

    @staticmethod
    def epilogue(inp, dt, y, shift_t=False, bias_cut=False, no_res=False, no_bias=False):
        b = inp["b"].to(dt).clone()
        if bias_cut:
            b[-8:] = 0
        if no_bias:
            b[:] = 0
        y = y + b
        if "t" in inp:
            t = inp["t"].to(dt)[:, : y.shape[3]]
            y = y + (t.roll(-1, 0) if shift_t else t)[:, None, None, :]
        if "res" in inp and not no_res:
            y = y + inp["res"].to(dt)
        return y

    @staticmethod
    def ref(inp, dt, **kw):
        return {"out": Conv3x3.epilogue(inp, dt, Conv3x3.conv(inp, dt), **kw)}

    @staticmethod
    def partials_bf16(inp):
        """the K-split planes rounded to bf16 before the finisher's sum"""
        S, C = inp["S"], inp["x"].shape[3]
        ns = C // 64
        y = 0
        for s in range(S):
            lo, hi = s * ns // S * 64, (s + 1) * ns // S * 64
            y = y + bfr(Conv3x3.conv(inp, F64, x=inp["x"][..., lo:hi], w=inp["w"][:, lo:hi]).float()).double()
        return Conv3x3.epilogue(inp, F64, y)

    @staticmethod
    def bound(inp, ref):
        C = inp["x"].shape[3]
        S = Conv3x3.conv(inp, F64, x=inp["x"].abs(), w=inp["w"].abs())
        carried = inp["b"].double().abs()[None, None, None, :].expand_as(S)
        if "t" in inp:
            carried = carried + inp["t"].double().abs()[:, None, None, : S.shape[3]]
        tot = S + carried + (inp["res"].double().abs() if "res" in inp else 0)
        a = (9 * C + 8) * U * tot + HILO * carried
        if inp["kind"] == "igemm phase2":
            a = a + 2.0 ** -9 * S
        return {"out": (BF, a)}

    @staticmethod
    def misses(inp):
        C = inp["x"].shape[3]
        w = inp["w"].clone(); w[:, C - 64:, 2, 2] = 0
        m = [("last 64-channel slice of tap (2, 2) dropped", {"out": Conv3x3.epilogue(inp, F64, Conv3x3.conv(inp, F64, w=w))}),
             ("taps flipped", {"out": Conv3x3.epilogue(inp, F64, Conv3x3.conv(inp, F64, w=inp["w"].flip(2, 3)))}),
             ("bias missing on the last 8 channels", Conv3x3.ref(inp, F64, bias_cut=True))]
        if inp.get("asym"):
            m += [("symmetric padding 1 (window origin one up and left)", {"out": Conv3x3.epilogue(inp, F64, Conv3x3.conv(inp, F64, pad=None))}),
                  ("zero row and column on the wrong side: pad (1, 0, 1, 0)", {"out": Conv3x3.epilogue(inp, F64, Conv3x3.conv(inp, F64, pad=(1, 0, 1, 0)))}),
                  ("bias dropped", Conv3x3.ref(inp, F64, no_bias=True))]
        if inp["stride"] == 1 and inp["x"].shape[0] > 1:
            m.append(("neighbouring sample instead of zero padding", {"out": Conv3x3.epilogue(inp, F64, Conv3x3.conv(inp, F64, stack=True))}))
        Wo = inp["x"].shape[2] * (2 if inp["ups"] else 1)
        if inp["stride"] == 1 and Wo > 64:
            m.append(("strip edges zero-padded", {"out": Conv3x3.epilogue(inp, F64, Conv3x3.conv(inp, F64, strips=True))}))
        if inp["S"] > 1:
            m.append(("K-split planes rounded to bf16", {"out": Conv3x3.partials_bf16(inp)}))
        if "t" in inp:
            m.append(("time-embedding row of sample b + 1", Conv3x3.ref(inp, F64, shift_t=True)))
        if inp["ups"]:
            m.append(("bilinear upsample", {"out": Conv3x3.epilogue(inp, F64, Conv3x3.conv(inp, F64, mode="bilinear"))}))
        if "res" in inp:
            m.append(("residual dropped", Conv3x3.ref(inp, F64, no_res=True)))
        return m


# ============================================================================================================ normalisation
def _group_inputs(B, HW, C, offset, small_var, g, seed):
    spread = 0.004 if small_var else 1.0
    off = (row_offsets(B * 32, seed + 1) * spread if offset else 0.3 * torch.randn(B * 32, generator=g)).reshape(B, 1, 32, 1)
    x = torch.randn(B, HW, 32, C // 32, generator=g) * spread * (0.5 + torch.rand(B, 1, 32, 1, generator=g)) + off
    return bfr(x.reshape(B, HW, C))


def gn_stats_chain(B, HW, C):
    """the fp32 chain of a group sum (x or x^2): one-pass kernel: a thread's NV pixels, the R pixel lanes, the group's channels;
    gn_stats: a thread's pixel rows of its chunk, the R lanes, the channels (the chunks are added in double)"""
    cg = C // 32
    plan = gn_onepass_plan(HW, C)
    if plan:
        gpb, T, NV = plan
        R = T // (gpb * cg // 8)
        return NV + R + cg + 2
    R = max(1, 256 // (C // 8)); nchunk = min(32, max(1, HW // 64))
    return _cdiv(_cdiv(HW, nchunk), R) + R + cg + 2


def _gn_xh_error(x, mean, rstd, var, c_s):
    """GroupNormBwd's model of the one-pass statistics: var off by c_s u mean(x^2), i.e. k = 4 + c_s mean(x^2) / (2 var)"""
    return U * (c_s * x.abs().mean((1, 3), keepdim=True) * rstd + 2 * (x.abs() + mean.abs()) * rstd
                + (4 + c_s * (x * x).mean((1, 3), keepdim=True) / (2 * var)) * ((x - mean) * rstd).abs())


class GroupNorm:
    """GroupNorm(32) (+ SiLU) of [x0 | x1] (bf16 [B, HW, C]) -> bf16 (rdm_op_groupnorm: gn_onepass_kernel or gn_stats + gn_apply).
    Statistics: fp32 sums of x and x^2 (a chain of c_s = gn_stats_chain roundings) finished in double as E[x^2] - mean^2 -- modelled as
    GroupNormBwd does for the same statistics: e_xh = u (c_s mean|x| rstd + 2 (|x| + |mean|) rstd + (4 + c_s mean(x^2) / (2 var)) |xh|).
    The apply pass forms x (rstd gamma) + (beta - mean rstd gamma): e_z = |gamma| e_xh + 3 u (|x| + |mean|) rstd |gamma| + 2 u |beta|;
    SiLU: _act_bound.  r = 2^-8.  Inputs: every (sample, group) has its own offset and scale (offsets 30-100x the spread in the offset
    cases).  Near misses: eps 1e-6 (small-variance groups); the statistics of the next group; of sample b + 1; SiLU dropped / added;
    unbiased variance (tiny groups)."""
    name = "groupnorm"
    exact = False

    @staticmethod
    def make(B, HW, C0, C1=0, silu=1, offset=False, small_var=False, seed=61):
        g = torch.Generator().manual_seed(seed)
        C = C0 + C1
        return {"x": _group_inputs(B, HW, C, offset, small_var, g, seed), "C0": C0, "gamma": 1 + 0.3 * torch.randn(C, generator=g),
                "beta": 0.3 * torch.randn(C, generator=g), "eps": 1e-5, "silu": silu, "small_var": small_var}

    @staticmethod
    def stats(x, eps, unbiased=False):
        mean = x.mean((1, 3), keepdim=True)
        n = x.shape[1] * x.shape[3]
        var = ((x - mean) ** 2).sum((1, 3), keepdim=True) / (n - 1 if unbiased else n)
        return mean, var, 1 / torch.sqrt(var + eps)

    @staticmethod
    def ref(inp, dt, eps=None, shift=None, silu=None, unbiased=False):
        x = inp["x"].to(dt)
        B, HW, C = x.shape
        xg = x.reshape(B, HW, 32, C // 32)
        mean, _, rstd = GroupNorm.stats(xg, inp["eps"] if eps is None else eps, unbiased)
        if shift == "group":
            mean, rstd = mean.roll(-1, 2), rstd.roll(-1, 2)
        if shift == "sample":
            mean, rstd = mean.roll(-1, 0), rstd.roll(-1, 0)
        z = ((xg - mean) * rstd).reshape(B, HW, C) * inp["gamma"].to(dt) + inp["beta"].to(dt)
        return {"out": _act(z, ACT_SILU) if (inp["silu"] if silu is None else silu) else z}

    @staticmethod
    def bound(inp, ref):
        x = inp["x"].double()
        B, HW, C = x.shape
        xg = x.reshape(B, HW, 32, C // 32)
        mean, var, rstd = GroupNorm.stats(xg, inp["eps"])
        gam, bet = inp["gamma"].double(), inp["beta"].double()
        e_xh = _gn_xh_error(xg, mean, rstd, var, gn_stats_chain(B, HW, C)).reshape(B, HW, C)
        e_z = gam.abs() * e_xh + 3 * U * ((xg.abs() + mean.abs()) * rstd).reshape(B, HW, C) * gam.abs() + 2 * U * bet.abs()
        z = GroupNorm.ref(inp, F64, silu=0)["out"]
        return {"out": (BF, _act_bound(z, e_z, ACT_SILU if inp["silu"] else ACT_NONE))}

    @staticmethod
    def misses(inp):
        m = [("statistics of the next group", GroupNorm.ref(inp, F64, shift="group")), ("SiLU dropped" if inp["silu"] else "SiLU added",
             GroupNorm.ref(inp, F64, silu=1 - inp["silu"]))]
        if inp["x"].shape[0] > 1:
            m.append(("statistics of sample b + 1", GroupNorm.ref(inp, F64, shift="sample")))
        if inp["small_var"]:
            m.append(("eps 1e-6", GroupNorm.ref(inp, F64, eps=1e-6)))
        if inp["x"].shape[1] * inp["x"].shape[2] // 32 <= 16:
            m.append(("unbiased variance", GroupNorm.ref(inp, F64, unbiased=True)))
        return m


class LayerNorm:
    """LayerNorm over C -> bf16 (rdm_op_layernorm: layernorm_bf16x8_kernel for bf16 rows with C % 8 == 0, C <= 1024, else the fp32- /
    bf16-input layernorm_kernel), exact two-pass variance.  e_xh = u (d mean|x| rstd + (d + 8) |xh|), d = ceil(C / 64) + 14 (the chain of
    a row sum: a lane's elements, 6 shuffle levels); a = |gamma| e_xh + 2 u (|gamma xh| + |beta|), r = 2^-8.  Near misses: eps 1e-6
    (small-variance rows), the statistics of the next row, unbiased variance (C = 16).
    out_f32 (rdm_op_layernorm_f32, the image tower's ln_pre: fp32 rows in, fp32 rows out): the same a with r = 0 -- no output rounding
    term -- and one more near miss, the output rounded to bf16, which a bound this tight tells from the fp32 output."""
    name = "layernorm"
    exact = False

    @staticmethod
    def make(M, C, f32=False, offset=False, small_var=False, seed=71, x=None, gamma=None, beta=None, out_f32=False):
        g = torch.Generator().manual_seed(seed)
        if x is None:
            spread = 0.004 if small_var else 1.0
            off = row_offsets(M, seed + 1) * spread if offset else 0.3 * torch.randn(M, generator=g)
            x = torch.randn(M, C, generator=g) * spread * (0.5 + torch.rand(M, 1, generator=g)) + off[:, None]
            x = x if f32 else bfr(x)
        return {"x": x, "f32": f32, "gamma": 1 + 0.3 * torch.randn(C, generator=g) if gamma is None else gamma,
                "beta": 0.3 * torch.randn(C, generator=g) if beta is None else beta, "eps": 1e-5, "small_var": small_var, "out_f32": out_f32}

    @staticmethod
    def stats(x, eps, unbiased=False):
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).sum(1, keepdim=True) / (x.shape[1] - 1 if unbiased else x.shape[1])
        return mean, 1 / torch.sqrt(var + eps)

    @staticmethod
    def ref(inp, dt, eps=None, shift=False, unbiased=False):
        x = inp["x"].to(dt)
        mean, rstd = LayerNorm.stats(x, inp["eps"] if eps is None else eps, unbiased)
        if shift:
            mean, rstd = mean.roll(-1, 0), rstd.roll(-1, 0)
        return {"out": (x - mean) * rstd * inp["gamma"].to(dt) + inp["beta"].to(dt)}

    @staticmethod
    def bound(inp, ref):
        x = inp["x"].double()
        d = _cdiv(x.shape[1], 64) + 14
        mean, rstd = LayerNorm.stats(x, inp["eps"])
        xh = (x - mean) * rstd
        gam, bet = inp["gamma"].double(), inp["beta"].double()
        e_xh = U * (d * x.abs().mean(1, keepdim=True) * rstd + (d + 8) * xh.abs())
        return {"out": (0.0 if inp.get("out_f32") else BF, gam.abs() * e_xh + 2 * U * ((gam * xh).abs() + bet.abs()))}

    @staticmethod
    def misses(inp):
        m = [("statistics of the next row", LayerNorm.ref(inp, F64, shift=True))]
        if inp.get("out_f32"):
            m.append(("output rounded to bf16", {"out": bfr(LayerNorm.ref(inp, F64)["out"].float()).double()}))
        if inp["small_var"]:
            m.append(("eps 1e-6", LayerNorm.ref(inp, F64, eps=1e-6)))
        if inp["x"].shape[1] <= 16:
            m.append(("unbiased variance", LayerNorm.ref(inp, F64, unbiased=True)))
        return m


# ============================================================================================================ attention
def _heads(t, H, D):
    B, n, _ = t.shape
    return t[..., : H * D].reshape(B, n, H, D).permute(0, 2, 1, 3)


def _unheads(t):
    B, H, n, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, H * D)


def _attn(q, k, v, H, D, scale):
    s = _heads(q, H, D) @ _heads(k, H, D).transpose(-1, -2) * scale
    return _unheads(torch.softmax(s, -1) @ _heads(v, H, D))


def _attn_bound(q, k, v, H, D, scale, pb, causal=False):
    """e_P = P (b + 2^-22 (4 + scale |S|) + 2 D u scale sum|q k| + m u) (b = 2^-8 when P is rounded to bf16 for the PV MFMA);
    a = e_P |v| + (m + 4) u P |v| + 4 u |o| (the PV chain, the normaliser), r = 2^-8"""
    qh, kh, vh = (_heads(t.double(), H, D) for t in (q, k, v))
    m = kh.shape[2]
    S = qh @ kh.transpose(-1, -2)
    s = S * scale
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), float("-inf"))
    P = torch.softmax(s, -1)
    e_P = P * ((BF if pb else 0.0) + 2.0 ** -22 * (4 + scale * S.abs()) + 2 * D * U * scale * (qh.abs() @ kh.abs().transpose(-1, -2)) + m * U)
    o = P @ vh
    return _unheads(e_P @ vh.abs() + (m + 4) * U * (P @ vh.abs()) + 4 * U * o.abs())


class SelfAttention:
    """flash self-attention, d_head 32, scale 32^-0.5 (rdm_op_self_attention: V^T given -> flash_d32_lds_kernel<false> when n % 64 == 0,
    flash_d32_kernel otherwise; rdm_op_self_attention_qkv: token-major V -> flash_d32_lds_kernel<true>).  P is rounded to bf16 before the
    PV MFMA (b = 2^-8 in _attn_bound).  Near misses: the scale applied twice; the head order reversed; k and v swapped."""
    name = "self_attention"
    exact = False
    SCALE = 32 ** -0.5

    @staticmethod
    def make(B, n, H, mode="vt", seed=81):
        g = torch.Generator().manual_seed(seed)
        q, k, v = (bfr(torch.randn(B, n, H * 32, generator=g) * s) for s in (1.0, 2.0, 1.0))
        return {"q": q, "k": k, "v": v, "H": H, "mode": mode}

    @staticmethod
    def ref(inp, dt, scale=None, swap=False, reverse=False):
        k, v = (inp["v"], inp["k"]) if swap else (inp["k"], inp["v"])
        o = _attn(inp["q"].to(dt), k.to(dt), v.to(dt), inp["H"], 32, SelfAttention.SCALE if scale is None else scale)
        if reverse:
            o = _unheads(_heads(o, inp["H"], 32).flip(1))
        return {"out": o}

    @staticmethod
    def bound(inp, ref):
        return {"out": (BF, _attn_bound(inp["q"], inp["k"], inp["v"], inp["H"], 32, SelfAttention.SCALE, True))}

    @staticmethod
    def misses(inp):
        return [("scale applied twice", SelfAttention.ref(inp, F64, scale=SelfAttention.SCALE ** 2)),
                ("heads reversed", SelfAttention.ref(inp, F64, reverse=True)), ("k and v swapped", SelfAttention.ref(inp, F64, swap=True))]


def small_attention_chunk(nkv, D):
    """keys per LDS chunk of small_attention_kernel<D> (attention.hip launch_small_attention: 64 KiB of fp32 K | V)"""
    return min(nkv, 64 * 1024 // (D * 8))


class SmallAttention:
    """few-key attention (small_attention_kernel<D>, D = 32 / 64, fp32 inside: b = 0 in _attn_bound), optional causal mask.  More than
    64 KiB / (8 D) keys (256 at D = 32, 128 at D = 64) pass through LDS in chunks, the running maximum / sum / output carried per query
    from one chunk to the next: the same key-ordered chain as one chunk, so the bound does not change.  Near misses: the scale applied
    twice; the diagonal masked (causal); the head order reversed; k and v swapped; and where more than one chunk runs: the keys beyond
    the first chunk dropped; the last chunk alone; the per-chunk softmaxes averaged (no rescale from chunk to chunk).
    fused (the CLIP towers' form): q, k, v are the column thirds of ONE [B, n, 3 H D] buffer, each read at the row pitch 3 H D; one more
    near miss there: the k and v slices exchanged -- which is "k and v swapped", kept under its own name for the fused layout."""
    name = "small_attention"
    exact = False

    @staticmethod
    def make(B, nq, nkv, H, D, causal=0, seed=91, fused=False):
        g = torch.Generator().manual_seed(seed)
        assert not fused or nq == nkv
        return {"q": bfr(torch.randn(B, nq, H * D, generator=g) * 1.5), "k": bfr(torch.randn(B, nkv, H * D, generator=g) * 1.5),
                "v": bfr(torch.randn(B, nkv, H * D, generator=g)), "H": H, "D": D, "causal": causal, "scale": D ** -0.5, "fused": fused}

    @staticmethod
    def ref(inp, dt, scale=None, swap=False, reverse=False, diag=False, keys=None, per_chunk=False):
        k, v = (inp["v"], inp["k"]) if swap else (inp["k"], inp["v"])
        H, D = inp["H"], inp["D"]
        s = _heads(inp["q"].to(dt), H, D) @ _heads(k.to(dt), H, D).transpose(-1, -2) * (inp["scale"] if scale is None else scale)
        if inp["causal"]:
            s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(0 if diag else 1), float("-inf"))
        if keys is not None:                                 # only the keys [lo, hi) are seen
            s = s.clone(); s[..., : keys[0]] = float("-inf"); s[..., keys[1]:] = float("-inf")
        vh = _heads(v.to(dt), H, D)
        if per_chunk:                                        # every chunk's own softmax, the chunks that hold a key averaged
            kc, nkv = small_attention_chunk(s.shape[-1], D), s.shape[-1]
            parts = [torch.nan_to_num(torch.softmax(s[..., j:j + kc], -1)) @ vh[..., j:j + kc, :] for j in range(0, nkv, kc)]
            seen = sum((torch.isfinite(s[..., j:j + kc]).any(-1, keepdim=True)).to(dt) for j in range(0, nkv, kc))
            o = _unheads(sum(parts) / seen.clamp(min=1))
        else:
            o = _unheads(torch.nan_to_num(torch.softmax(s, -1)) @ vh)
        if reverse:
            o = _unheads(_heads(o, H, D).flip(1))
        return {"out": o}

    @staticmethod
    def bound(inp, ref):
        return {"out": (BF, _attn_bound(inp["q"], inp["k"], inp["v"], inp["H"], inp["D"], inp["scale"], False, bool(inp["causal"])))}

    @staticmethod
    def misses(inp):
        m = [("scale applied twice", SmallAttention.ref(inp, F64, scale=inp["scale"] ** 2)), ("heads reversed", SmallAttention.ref(inp, F64, reverse=True)),
             ("k and v swapped", SmallAttention.ref(inp, F64, swap=True))]
        if inp["causal"]:
            m.append(("diagonal masked", SmallAttention.ref(inp, F64, diag=True)))
        if inp.get("fused"):
            m += [("k and v slices of the fused rows exchanged", SmallAttention.ref(inp, F64, swap=True)),
                  ("the q slice read where k belongs", {"out": _attn_masked(inp, inp["q"], inp["q"], inp["v"])})]
        nkv = inp["k"].shape[1]
        kc = small_attention_chunk(nkv, inp["D"])
        if nkv > kc:
            last = (nkv - 1) // kc * kc
            m += [("keys beyond the first chunk dropped", SmallAttention.ref(inp, F64, keys=(0, kc))),
                  ("the last chunk alone", SmallAttention.ref(inp, F64, keys=(last, nkv))),
                  ("per-chunk softmaxes averaged", SmallAttention.ref(inp, F64, per_chunk=True))]
        return m


def _attn_masked(inp, q, k, v):
    """SmallAttention.ref on other operands (the fused layout's column-offset near misses)"""
    return SmallAttention.ref(dict(inp, q=q, k=k, v=v), F64)["out"]


class XattnFused:
    """fused skinny cross-attention (xattn_fused_kernel / xattn_ln_fused_kernel): out = softmax over each head's group of k score columns
    of (x' G^T), times U^T, + bias + residual; x' = x, or bf16(LayerNorm(x; gamma, beta)) with the residual x itself (the LN form).
    Scores: a C-long chain e_S = (C + 4) u sum |x' G| (+ sum 2^-9 |x'| |G| + the LN error for the LN form); P rounded to bf16 for the
    second MFMA: e_P = P (2^-8 + 2^-22 (4 + |S|) + 2 max_group e_S + k u); a = e_P |U| + (ncols + 4) u (P |U| + |bias| + |res|), r = 2^-8.
    Near misses: one softmax over all columns instead of per head; the neighbouring head's probabilities; the residual dropped; the bias
    dropped; the last score column dropped; (LN form) the statistics of the next row."""
    name = "xattn_fused"
    exact = False

    @staticmethod
    def make(B, n, heads, k, bias=True, res=True, ln=False, seed=101):
        g = torch.Generator().manual_seed(seed)
        C, NP, ncols = heads * 32, 128, heads * k
        Gm = torch.zeros(B, NP, C); Um = torch.zeros(B, C, NP)
        Gm[:, :ncols] = torch.randn(B, ncols, C, generator=g) * (4.0 / C ** 0.5)
        Um[:, :, :ncols] = torch.randn(B, C, ncols, generator=g)
        inp = {"G": bfr(Gm), "U": bfr(Um), "ncols": ncols, "k": k, "heads": heads, "ln": ln,
               "bias": torch.randn(C, generator=g) if bias else None}
        if ln:
            inp["x"] = bfr(torch.randn(B, n, C, generator=g) * 1.7 + torch.randn(B, n, 1, generator=g) * 3)
            inp["gamma"], inp["beta"], inp["eps"] = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), 1e-5
        else:
            inp["x"] = bfr(torch.randn(B, n, C, generator=g))
            inp["res"] = bfr(torch.randn(B, n, C, generator=g)) if res else None
        return inp

    @staticmethod
    def xn(inp, dt, shift=False):
        x = inp["x"].to(dt)
        if not inp["ln"]:
            return x
        mean = x.mean(-1, keepdim=True); rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + inp["eps"])
        if shift:
            mean, rstd = mean.roll(-1, 1), rstd.roll(-1, 1)
        return (x - mean) * rstd * inp["gamma"].to(dt) + inp["beta"].to(dt)

    @staticmethod
    def probs(inp, dt, shift=False, one_group=False):
        nc, k = inp["ncols"], inp["k"]
        s = XattnFused.xn(inp, dt, shift) @ inp["G"][:, :nc].to(dt).transpose(1, 2)
        B, n, _ = s.shape
        if one_group:
            return torch.softmax(s, -1)
        return torch.softmax(s.reshape(B, n, nc // k, k), -1).reshape(B, n, nc)

    @staticmethod
    def ref(inp, dt, shift=False, one_group=False, roll_head=False, no_res=False, no_bias=False, drop_last=False):
        P = XattnFused.probs(inp, dt, shift, one_group)
        if roll_head:
            P = P.roll(inp["k"], -1)
        if drop_last:
            P = P.clone(); P[..., -1] = 0
        o = P @ inp["U"][:, :, : inp["ncols"]].to(dt).transpose(1, 2)
        if inp["bias"] is not None and not no_bias:
            o = o + inp["bias"].to(dt)
        if not no_res:
            if inp["ln"]:
                o = o + inp["x"].to(dt)
            elif inp["res"] is not None:
                o = o + inp["res"].to(dt)
        return {"out": o}

    @staticmethod
    def bound(inp, ref):
        nc, k, C = inp["ncols"], inp["k"], inp["x"].shape[2]
        G, Um = inp["G"][:, :nc].double(), inp["U"][:, :, :nc].double()
        xn = XattnFused.xn(inp, F64)
        e_S = (C + 4) * U * (xn.abs() @ G.abs().transpose(1, 2))
        if inp["ln"]:
            x = inp["x"].double()
            d = _cdiv(C, 64) + 14
            mean = x.mean(-1, keepdim=True); rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + inp["eps"])
            e_xn = 2.0 ** -9 * xn.abs() + inp["gamma"].double().abs() * U * (d * x.abs().mean(-1, keepdim=True) * rstd + (d + 8) * ((x - mean) * rstd).abs())
            e_S = e_S + e_xn @ G.abs().transpose(1, 2)
        S = xn @ G.transpose(1, 2)
        B, n, _ = S.shape
        P = XattnFused.probs(inp, F64)
        e_Sg = e_S.reshape(B, n, nc // k, k).amax(-1, keepdim=True).expand(B, n, nc // k, k).reshape(B, n, nc)
        e_P = P * (BF + 2.0 ** -22 * (4 + S.abs()) + 2 * e_Sg + k * U)
        tot = P @ Um.abs().transpose(1, 2)
        if inp["bias"] is not None:
            tot = tot + inp["bias"].double().abs()
        if inp["ln"]:
            tot = tot + inp["x"].double().abs()
        elif inp["res"] is not None:
            tot = tot + inp["res"].double().abs()
        return {"out": (BF, e_P @ Um.abs().transpose(1, 2) + (nc + 4) * U * tot)}

    @staticmethod
    def misses(inp):
        m = [("the neighbouring head's probabilities", XattnFused.ref(inp, F64, roll_head=True)), ("last score column dropped", XattnFused.ref(inp, F64, drop_last=True))]
        if inp["k"] > 1:
            m.append(("one softmax over all columns", XattnFused.ref(inp, F64, one_group=True)))
        if inp["ln"] or inp["res"] is not None:
            m.append(("residual dropped", XattnFused.ref(inp, F64, no_res=True)))
        if inp["bias"] is not None:
            m.append(("bias dropped", XattnFused.ref(inp, F64, no_bias=True)))
        if inp["ln"]:
            m.append(("LayerNorm statistics of the next row", XattnFused.ref(inp, F64, shift=True)))
        return m


# ============================================================================================================ head conv
class HeadConv:
    """GroupNorm(32) + SiLU (optional) + 3x3 conv to Cout <= 8 channels (rdm_op_head_conv: gn_stats + head_conv_kernel) -> fp32 NCHW.
    act = silu(GN(x)) with GroupNorm's error e_act (GroupNorm.bound on the stats path), then rounded to bf16 (2^-9 |act|); the fp32
    weights ride as bf16 hi + lo (2^-16 |w|), two product chains of 9 C.  r = 0, a = sum (e_act + 2^-9 |act|) |w| + 2^-16 sum |act w|
    + (18 C + 8) u (sum |act w| + |bias|).  Inputs: per-(sample, group) offsets.  Near misses: the taps flipped; the statistics of sample
    b + 1; SiLU dropped; the bias missing."""
    name = "head_conv"
    exact = False

    @staticmethod
    def make(B, H, W, C, Cout, norm=True, seed=111):
        g = torch.Generator().manual_seed(seed)
        x = _group_inputs(B, H * W, C, False, False, g, seed).reshape(B, H, W, C)
        x = bfr(x * 1.3 + torch.randn(B, 1, 1, C, generator=g))
        return {"x": x, "w": torch.randn(Cout, C, 3, 3, generator=g) / (3 * C ** 0.5), "bias": torch.randn(Cout, generator=g), "norm": norm,
                "gamma": 1 + 0.1 * torch.randn(C, generator=g), "beta": 0.1 * torch.randn(C, generator=g), "eps": 1e-5}

    @staticmethod
    def gn_inp(inp):
        B, H, W, C = inp["x"].shape
        return {"x": inp["x"].reshape(B, H * W, C), "gamma": inp["gamma"], "beta": inp["beta"], "eps": inp["eps"], "silu": 1}

    @staticmethod
    def act(inp, dt, shift=None, silu=1):
        if not inp["norm"]:
            return inp["x"].to(dt)
        gi = HeadConv.gn_inp(inp); gi["silu"] = silu
        return GroupNorm.ref(gi, dt, shift=shift)["out"].reshape(inp["x"].shape)

    @staticmethod
    def ref(inp, dt, act=None, flip=False, no_bias=False):
        a = HeadConv.act(inp, dt) if act is None else act
        w = inp["w"].to(dt).flip(2, 3) if flip else inp["w"].to(dt)
        return {"out": F.conv2d(a.permute(0, 3, 1, 2), w, None if no_bias else inp["bias"].to(dt), padding=1)}

    @staticmethod
    def bound(inp, ref):
        a = HeadConv.act(inp, F64)
        if inp["norm"]:
            gi = HeadConv.gn_inp(inp)
            e_act = GroupNorm.bound(gi, None)["out"][1].reshape(a.shape)
            e_act = e_act + 2.0 ** -9 * a.abs()
        else:
            e_act = torch.zeros_like(a)
        w = inp["w"].double().abs()
        cv = lambda t: F.conv2d(t.permute(0, 3, 1, 2), w, padding=1)
        Sa = cv(a.abs())
        C = a.shape[3]
        return {"out": (0.0, cv(e_act) + HILO * Sa + (18 * C + 8) * U * (Sa + inp["bias"].double().abs()[None, :, None, None]))}

    @staticmethod
    def misses(inp):
        m = [("taps flipped", HeadConv.ref(inp, F64, flip=True)), ("bias missing", HeadConv.ref(inp, F64, no_bias=True))]
        if inp["norm"]:
            m.append(("SiLU dropped", HeadConv.ref(inp, F64, act=HeadConv.act(inp, F64, silu=0))))
            if inp["x"].shape[0] > 1:
                m.append(("statistics of sample b + 1", HeadConv.ref(inp, F64, act=HeadConv.act(inp, F64, shift="sample"))))
        return m


# ============================================================================================================ stem conv / VALU head conv
def _conv_rowwrap(x, w):
    """3x3 conv of x [B, C, H, W] with the ROWS zero-padded but the columns taken at the flat index p + dx: at x = 0 / x = W - 1 the
    left / right tap is the last / first pixel of the neighbouring row (zero only in front of the first and behind the last padded row)"""
    B, C, H, W = x.shape
    flat = F.pad(F.pad(x, (0, 0, 1, 1)).reshape(B, C, (H + 2) * W), (1, 1))
    y = 0
    for t in range(9):
        start = (t // 3) * W + (t % 3)                       # (1 + dy) W + dx + 1
        y = y + torch.einsum("bcp,nc->bnp", flat[..., start:start + H * W], w[:, :, t // 3, t % 3])
    return y.reshape(B, -1, H, W)


def _conv_stacked(x, w):
    """the samples stacked vertically: each one's top / bottom pad row is its neighbour's edge row"""
    B, C, H, W = x.shape
    return F.conv2d(x.permute(1, 0, 2, 3).reshape(1, C, B * H, W), w, padding=1).reshape(-1, B, H, W).permute(1, 0, 2, 3)


class ConvIn:
    """The stem conv (rdm_op_conv_in: conv_in_kernel<OCT, CIN>, OCT = 4 when Cout % 32 == 0 else 0, CIN = 3 for Cin <= 3 else 4): 3x3,
    pad 1, x fp32 NCHW [B, Cin, H, W], w fp32 [Cout, Cin, 3, 3], bias fp32 -> bf16 NHWC.  A thread owns a pixel: its accumulator starts
    from the bias and takes one fp32 FMA per (channel, tap) -- a chain of 9 CIN = 9 Cin terms for Cin = 3 or 4 -- then one bf16 rounding:
    r = 2^-8, a = (9 Cin + 2) u S, S = sum |x| |w| + |b|.  Inputs: every channel plane carries its own offset.  Near misses: the taps
    flipped; the neighbouring sample's rows instead of the zero padding; row wrap (the flat-index neighbour p +- 1 at x = 0 / W - 1
    instead of zero); the channel planes rotated; the bias missing on the last 8 channels; the pixels behind the last whole 64 of a
    sample written as zero (a lane that leaves the pixel loop takes the staged stores of its wave with it)."""
    name = "conv_in"
    exact = False

    @staticmethod
    def make(B, Cin, H, W, Cout, seed=121):
        g = torch.Generator().manual_seed(seed)
        off = torch.tensor([1.5, -2.0, 0.7, 3.0])[:Cin]
        return {"x": torch.randn(B, Cin, H, W, generator=g) + off[None, :, None, None],
                "w": torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), "b": 0.5 * torch.randn(Cout, generator=g)}

    @staticmethod
    def ref(inp, dt, conv=None, x=None, w=None, bias_cut=False, tail_zero=False):
        x = (inp["x"] if x is None else x).to(dt)
        w = (inp["w"] if w is None else w).to(dt)
        b = inp["b"].to(dt).clone()
        if bias_cut:
            b[-8:] = 0
        y = (F.conv2d(x, w, padding=1) if conv is None else conv(x, w)) + b[None, :, None, None]
        y = y.permute(0, 2, 3, 1).contiguous()
        if tail_zero:
            B, H, W, N = y.shape
            y.view(B, H * W, N)[:, H * W // 64 * 64:] = 0
        return {"out": y}

    @staticmethod
    def bound(inp, ref):
        Cin = inp["x"].shape[1]
        S = F.conv2d(inp["x"].double().abs(), inp["w"].double().abs(), inp["b"].double().abs(), padding=1).permute(0, 2, 3, 1)
        return {"out": (BF, (9 * Cin + 2) * U * S)}

    @staticmethod
    def misses(inp):
        m = [("taps flipped", ConvIn.ref(inp, F64, w=inp["w"].flip(2, 3))), ("row wrap", ConvIn.ref(inp, F64, conv=_conv_rowwrap)),
             ("channel planes rotated", ConvIn.ref(inp, F64, x=inp["x"].roll(1, 1))),
             ("bias missing on the last 8 channels", ConvIn.ref(inp, F64, bias_cut=True)),
             ("pixels behind the last whole 64 written as zero", ConvIn.ref(inp, F64, tail_zero=True))]
        if inp["x"].shape[0] > 1:
            m.append(("neighbouring sample instead of zero padding", ConvIn.ref(inp, F64, conv=_conv_stacked)))
        return m


class ConvOut:
    """The VALU head conv (rdm_op_conv_out: conv_out_kernel, what Ops::head falls back to where W % 32 or an odd H rules out the fused
    head conv): 3x3, pad 1, x bf16 NHWC, w fp32 [Cout, Cin, 3, 3], bias fp32 -> fp32 NCHW.  Eight lanes share a pixel: a lane takes every
    eighth 16-byte piece of each tap's channel row, i.e. 9 Cin / 8 products summed in order in fp32, then three shuffle adds combine the
    eight lanes and the bias is added: r = 0, a = (9 Cin / 8 + 8) u S, S = sum |x| |w| + |b|.  Near misses: the taps flipped; the
    neighbouring sample's rows instead of the zero padding; row wrap; the bias missing; the output channels swapped; the last 64-channel
    slice dropped."""
    name = "conv_out"
    exact = False

    @staticmethod
    def make(B, H, W, Cin, Cout, seed=131):
        g = torch.Generator().manual_seed(seed)
        x = bfr(torch.randn(B, H, W, Cin, generator=g) + 0.5 * torch.randn(1, 1, 1, Cin, generator=g))
        return {"x": x, "w": torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5), "b": torch.randn(Cout, generator=g)}

    @staticmethod
    def ref(inp, dt, conv=None, w=None, no_bias=False, swap=False):
        x = inp["x"].to(dt).permute(0, 3, 1, 2)
        w = (inp["w"] if w is None else w).to(dt)
        y = F.conv2d(x, w, padding=1) if conv is None else conv(x, w)
        if not no_bias:
            y = y + inp["b"].to(dt)[None, :, None, None]
        return {"out": y.flip(1) if swap else y}

    @staticmethod
    def bound(inp, ref):
        Cin = inp["x"].shape[3]
        S = F.conv2d(inp["x"].double().abs().permute(0, 3, 1, 2), inp["w"].double().abs(), inp["b"].double().abs(), padding=1)
        return {"out": (0.0, (9 * Cin // 8 + 8) * U * S)}

    @staticmethod
    def misses(inp):
        w = inp["w"].clone(); w[:, -64:] = 0
        m = [("taps flipped", ConvOut.ref(inp, F64, w=inp["w"].flip(2, 3))), ("row wrap", ConvOut.ref(inp, F64, conv=_conv_rowwrap)),
             ("bias missing", ConvOut.ref(inp, F64, no_bias=True)), ("output channels swapped", ConvOut.ref(inp, F64, swap=True)),
             ("last 64-channel slice dropped", ConvOut.ref(inp, F64, w=w))]
        if inp["x"].shape[0] > 1:
            m.append(("neighbouring sample instead of zero padding", ConvOut.ref(inp, F64, conv=_conv_stacked)))
        return m


# ============================================================================================================ the parametrisations
# (case, shape kwargs, the launch path it reaches); the path strings come from the host-side launch rules above where they exist, so a
# test id names the kernel instantiation it exercises
_L, _LN, _CV, _GN, _LY, _SA, _SM, _XA, _HC = Linear, LinearLN, Conv3x3, GroupNorm, LayerNorm, SelfAttention, SmallAttention, XattnFused, HeadConv
_CI, _CO = ConvIn, ConvOut


def _lin(**kw):
    path = linear_path(kw["M"], kw["N"], kw["K"], kw.get("act", 0), kw.get("alpha", 1.0), kw.get("f32", False), kw.get("res", False),
                       kw.get("rows"), kw.get("mgemm", False))
    return (_L, kw, path + (": f32 residual in place" if kw.get("res_f32") else ""))


def _lnf(**kw):
    g = "GEGLU" if kw.get("act") == ACT_GEGLU else "plain"
    return (_LN, kw, f"lin4<{g}, WM{lin4_wm(kw['M'], kw['N'])}, LN>" + (": 2-slice K" if kw["K"] == 128 else ""))


def _conv(**kw):
    kind, S = conv_path(kw["B"], kw["H"], kw["W"], kw["C0"] + kw.get("C1", 0), kw["N"], kw.get("stride", 1), kw.get("ups", 0), kw.get("C1", 0) > 0,
                        kw.get("rowvec", False), kw.get("res", False))
    return (_CV, kw, kind + (f" + K-split {S} + splitk_finish" if S > 1 else "") + (": asym (Downsample)" if kw.get("asym") else ""))


def _gn(**kw):
    B, HW, C = kw["B"], kw["HW"], kw["C0"] + kw.get("C1", 0)
    plan = gn_onepass_plan(HW, C)
    path = f"gn_onepass<NV{plan[2]}, {plan[1]}>" if plan else "gn_stats + gn_apply"
    if plan is None:                                         # dispatch.hip gn_chunks: the pixel chunks of the statistics pass
        nchunk = min(32, max(1, HW // 64))
        if HW % nchunk:
            path += f": {nchunk} chunks of {_cdiv(HW, nchunk)} rows, the last one short"
    return (_GN, kw, path + (" (XCD block order)" if plan and B % 8 == 0 else ""))


def _cin(**kw):
    npix, grid = kw["H"] * kw["W"], min(_cdiv(kw["H"] * kw["W"], 512), _cdiv(2048, kw["B"]))      # misc.hip launch_conv_in
    path = f"conv_in_kernel<{4 if kw['Cout'] % 32 == 0 else 0}, {3 if kw['Cin'] <= 3 else 4}>: {npix} pixels"
    return (_CI, kw, path + (f", {grid} blocks x {_cdiv(npix, 512 * grid)} trips" if npix > 512 * grid else ""))


def _sm(**kw):
    kc = small_attention_chunk(kw["nkv"], kw["D"])
    path = f"small_attention_kernel<{kw['D']}>: " + ("causal, " if kw.get("causal") else "") + f"{_cdiv(kw['nkv'], kc)} key chunks"
    return (_SM, kw, path + (", fused q|k|v rows" if kw.get("fused") else ""))


def _ly(**kw):
    bf = not kw.get("f32", False) and kw["C"] % 8 == 0 and kw["C"] <= 1024
    if kw.get("out_f32"):
        assert kw.get("f32")
        return (_LY, kw, "layernorm_kernel<f32>: f32 out")
    return (_LY, kw, f"layernorm_bf16x8<{1 if kw['C'] <= 512 else 2}>" if bf else f"layernorm_kernel<{'f32' if kw.get('f32') else 'bf16'}>")


CASES = [
    # linear: igemm tiles, residual through the A stream, GEGLU tiles, fp32 out + alpha, SiLU / QuickGELU, row groups
    _lin(M=300, N=192, K=192),
    _lin(M=1000, N=128, K=128, res=True),
    _lin(M=8192, N=192, K=64, res=True),
    _lin(M=8192, N=256, K=128),
    _lin(M=65536, N=192, K=64, f32=True),
    _lin(M=65536, N=256, K=64, res=True),
    _lin(M=384, N=192, K=256, f32=True, alpha=0.125),
    _lin(M=384, N=192, K=256, act=ACT_SILU),
    _lin(M=384, N=192, K=256, act=ACT_QUICKGELU),
    _lin(M=200, N=1024, K=128, act=ACT_GEGLU),
    _lin(M=8192, N=1024, K=128, act=ACT_GEGLU),
    _lin(M=16384, N=2048, K=64, act=ACT_GEGLU),
    _lin(M=1000, N=192, K=128, rows=100),
    _lin(M=4096, N=384, K=384, rows=1000, res=True),
    # lin4: both wave arrangements, one / two tiles per block, a one-slice K, residual, no bias, GEGLU, two row groups
    _lin(M=49152, N=384, K=64),
    _lin(M=65536, N=384, K=128, res=True, bias=False),
    _lin(M=49152, N=192, K=128, res=True),
    _lin(M=32768, N=1536, K=128, act=ACT_GEGLU),
    _lin(M=49152, N=768, K=64, act=ACT_GEGLU),
    _lin(M=16384, N=576, K=64, act=ACT_GEGLU),
    _lin(M=65536, N=384, K=128, rows=32768, res=True),
    _lin(M=49152, N=576, K=64, rows=24576),
    # sgemm (M <= 128, K % 256 == 0): every epilogue, fp32 out
    _lin(M=3, N=256, K=256),
    _lin(M=33, N=512, K=256, f32=True),
    _lin(M=128, N=256, K=512, act=ACT_SILU),
    _lin(M=96, N=512, K=256, act=ACT_QUICKGELU, f32=True),
    _lin(M=64, N=1024, K=256, act=ACT_GEGLU),
    _lin(M=17, N=256, K=256, res=True, bias=False),
    # mgemm (RDM_MGEMM_ANY test hook, child process)
    _lin(M=1064, N=256, K=256, res=True, f32=True, mgemm=True),
    _lin(M=1000, N=192, K=512, act=ACT_SILU, mgemm=True),
    _lin(M=130, N=64, K=128, act=ACT_QUICKGELU, mgemm=True),
    # the CLIP towers' residual adds (rdm_op_linear_res_f32: fp32 residual, fp32 out, in place): the tiled kernel just above the 128-row
    # skinny rule with one ragged tile (2 x 77 rows), ragged past 256, 192- and 128-wide column tiles, several column tiles, c_proj's
    # reduction depth; and the fp32-out QuickGELU epilogue without a residual
    _lin(M=154, N=128, K=128, f32=True, res_f32=True),
    _lin(M=308, N=192, K=128, f32=True, res_f32=True),
    _lin(M=385, N=512, K=128, f32=True, res_f32=True),
    _lin(M=150, N=128, K=3072, f32=True, res_f32=True),
    _lin(M=231, N=512, K=128, act=ACT_QUICKGELU, f32=True),
    # LayerNorm folded into lin4
    _lnf(M=16384, N=1152, K=384, offset=True),
    _lnf(M=33024, N=192, K=192, bias=False, small_var=True),
    _lnf(M=8192, N=3072, K=384, act=ACT_GEGLU, offset=True),
    _lnf(M=8192, N=960, K=192, act=ACT_GEGLU),
    _lnf(M=4096, N=768, K=128, offset=True, bias=False),
    # conv3x3
    _conv(B=1, H=64, W=4, C0=128, N=128, res=True),
    _conv(B=2, H=64, W=4, C0=64, N=192, rowvec=True),
    _conv(B=1, H=64, W=4, C0=256, N=128, res=True),      # few tiles and four slices, but no halo4 geometry: no K-split may be chosen for it
    _conv(B=4, H=8, W=8, C0=128, N=192),
    _conv(B=4, H=8, W=8, C0=64, C1=64, N=128, rowvec=True, ld_pad=7, res=True),
    _conv(B=1, H=16, W=16, C0=128, N=192, rowvec=True, res=True),
    _conv(B=2, H=8, W=32, C0=64, N=128),
    _conv(B=1, H=4, W=64, C0=128, N=192, res=True),
    _conv(B=8, H=8, W=8, C0=256, N=192, rowvec=True),
    _conv(B=4, H=8, W=8, C0=192, C1=192, N=128, rowvec=True, res=True),
    _conv(B=2, H=16, W=16, C0=448, N=192),
    _conv(B=1, H=8, W=128, C0=64, N=128, rowvec=True),
    _conv(B=1, H=4, W=320, C0=64, N=128, res=True),
    _conv(B=1, H=2, W=64, C0=64, N=128, ups=1, rowvec=True),
    _conv(B=2, H=8, W=8, C0=128, N=192, ups=1),
    _conv(B=1, H=4, W=16, C0=64, N=72, ups=1),
    _conv(B=5, H=4, W=4, C0=64, N=128, res=True),
    _conv(B=3, H=4, W=4, C0=64, N=128, ups=1, res=True),
    _conv(B=2, H=16, W=16, C0=64, N=64, stride=2),
    # 192-wide strip tiles; odd widths, M a multiple of neither 256 nor 64, HW % 32 != 0 under a per-sample row, stride 2 on a non-square
    # input, the phase and dual-source upsample forms at odd widths (implicit GEMM)
    _conv(B=1, H=4, W=128, C0=64, N=192),
    _conv(B=2, H=8, W=192, C0=64, C1=64, N=192, rowvec=True, res=True),
    _conv(B=1, H=2, W=64, C0=64, N=192, ups=1, rowvec=True),
    _conv(B=2, H=5, W=7, C0=64, N=64),
    _conv(B=1, H=10, W=14, C0=64, C1=64, N=128, rowvec=True, ld_pad=5, res=True),
    _conv(B=3, H=6, W=10, C0=64, N=64, stride=2),
    _conv(B=2, H=5, W=7, C0=64, N=64, ups=1),
    _conv(B=1, H=5, W=7, C0=64, C1=64, N=72, ups=1),
    # the first-stage encoder's Downsample (rdm_op_conv3x3_down): a square and a non-square batch, ONE output pixel whose every border tap is
    # masked (2 x 2 input: the window's last row and column are all padding), and a 128-channel non-square input
    _conv(B=2, H=16, W=16, C0=64, N=64, stride=2, asym=1),
    _conv(B=3, H=6, W=10, C0=64, N=64, stride=2, asym=1),
    _conv(B=1, H=2, W=2, C0=64, N=128, stride=2, asym=1),
    _conv(B=1, H=10, W=14, C0=128, N=128, stride=2, asym=1),
    # stem conv, all four instantiations: one partial wave; direct stores, four input channels; a short second block; one pixel; a ragged
    # second grid-stride trip
    _cin(B=2, Cin=3, H=5, W=7, Cout=64),
    _cin(B=1, Cin=4, H=9, W=8, Cout=40),
    _cin(B=1, Cin=4, H=9, W=8, Cout=32),
    _cin(B=2, Cin=3, H=5, W=7, Cout=40),
    _cin(B=3, Cin=3, H=20, W=28, Cout=128),
    _cin(B=1, Cin=3, H=1, W=1, Cout=32),
    _cin(B=64, Cin=3, H=130, W=130, Cout=32),
    # GroupNorm
    _gn(B=8, HW=1024, C0=384, silu=1, offset=True),
    _gn(B=3, HW=1024, C0=384, silu=0, small_var=True),
    _gn(B=2, HW=1024, C0=576, C1=384, silu=1, offset=True),
    _gn(B=8, HW=256, C0=960, silu=1),
    _gn(B=8, HW=4, C0=64, silu=0),
    _gn(B=2, HW=816, C0=640, silu=1, offset=True),
    _gn(B=2, HW=4096, C0=64, silu=1, offset=True),
    _gn(B=2, HW=4096, C0=192, C1=192, silu=0, small_var=True),
    _gn(B=2, HW=1100, C0=64, silu=1, offset=True),
    _gn(B=2, HW=1100, C0=192, C1=192, silu=0, small_var=True),
    _gn(B=3, HW=35, C0=256, silu=1, offset=True),
    _gn(B=2, HW=50, C0=192, silu=0),
    _gn(B=2, HW=200, C0=128, C1=64, silu=1, offset=True),
    _gn(B=4, HW=2, C0=64, silu=0),
    # LayerNorm
    _ly(M=100, C=384, offset=True),
    _ly(M=77, C=512, f32=True, small_var=True),
    _ly(M=513, C=960, small_var=True),
    _ly(M=9, C=768, f32=True, offset=True),
    _ly(M=16384 + 13, C=384, offset=True),
    _ly(M=40, C=16),
    _ly(M=40, C=16, f32=True),
    _ly(M=50, C=1280, offset=True),
    # fp32 rows to fp32 rows (the image tower's ln_pre): the tiny tower's 5 rows of 128, one sample of ViT-B/32's 50 rows of 768
    _ly(M=5, C=128, f32=True, out_f32=True, offset=True),
    _ly(M=50, C=768, f32=True, out_f32=True, offset=True),
    _ly(M=50, C=768, f32=True, out_f32=True, small_var=True),
    # attention
    (_SA, dict(B=2, n=64, H=2, mode="vt"), "flash_d32_lds_kernel<false>"),
    (_SA, dict(B=1, n=256, H=3, mode="qkv"), "flash_d32_lds_kernel<true>"),
    (_SA, dict(B=2, n=96, H=2, mode="vt"), "flash_d32_kernel (n % 64 != 0)"),
    (_SA, dict(B=1, n=1024, H=2, mode="vt"), "flash_d32_lds_kernel<false>: n = 1024"),
    (_SA, dict(B=1, n=32, H=1, mode="vt"), "flash_d32_kernel: one 32-row tile"),
    (_SA, dict(B=2, n=160, H=2, mode="vt"), "flash_d32_kernel: n = 160"),
    (_SA, dict(B=1, n=800, H=1, mode="vt"), "flash_d32_kernel: n = 800"),
    (_SM, dict(B=2, nq=64, nkv=4, H=4, D=32), "small_attention_kernel<32>"),
    (_SM, dict(B=2, nq=77, nkv=77, H=2, D=64, causal=1), "small_attention_kernel<64>: causal"),
    (_SM, dict(B=2, nq=300, nkv=1, H=2, D=32), "small_attention_kernel<32>: one key"),
    (_SM, dict(B=1, nq=1024, nkv=16, H=6, D=32), "small_attention_kernel<32>: many queries, few keys"),
    _sm(B=2, nq=70, nkv=257, H=2, D=32),
    _sm(B=1, nq=600, nkv=600, H=1, D=32),
    _sm(B=2, nq=200, nkv=200, H=1, D=64, causal=1),
    # q, k, v as column slices of one [B, n, 3 H D] buffer (the CLIP towers): the text tower's 77 causal rows, the image tower's 50, and
    # the tiny image tower's 5 (fewer keys than a chunk holds, fewer queries than a wave)
    _sm(B=2, nq=77, nkv=77, H=2, D=64, causal=1, fused=True),
    _sm(B=3, nq=50, nkv=50, H=2, D=64, causal=0, fused=True),
    _sm(B=3, nq=5, nkv=5, H=2, D=64, causal=0, fused=True),
    (_XA, dict(B=2, n=64, heads=4, k=4), "xattn_fused_kernel: bias + residual"),
    (_XA, dict(B=2, n=32, heads=2, k=1, bias=False, res=False), "xattn_fused_kernel: no bias / residual"),
    (_XA, dict(B=8, n=64, heads=4, k=2), "xattn_fused_kernel: XCD block order"),
    (_XA, dict(B=2, n=96, heads=6, k=4, ln=True), "xattn_ln_fused_kernel"),
    # head conv
    (_HC, dict(B=2, H=32, W=64, C=192, Cout=3), "head_conv_kernel: GroupNorm + SiLU"),
    (_HC, dict(B=2, H=34, W=64, C=224, Cout=4), "head_conv_kernel: band split (H = 34)"),
    (_HC, dict(B=3, H=16, W=32, C=64, Cout=4, norm=False), "head_conv_kernel: no norm"),
    (_HC, dict(B=6, H=8, W=32, C=32, Cout=1), "head_conv_kernel: Cout = 1"),
    # the VALU head conv: odd sizes, a latent width of 28, one output channel
    (_CO, dict(B=2, H=5, W=7, Cin=64, Cout=3), "conv_out_kernel: 35 pixels"),
    (_CO, dict(B=1, H=20, W=28, Cin=128, Cout=4), "conv_out_kernel: 560 pixels, Cout = 4"),
    (_CO, dict(B=3, H=3, W=50, Cin=192, Cout=1), "conv_out_kernel: Cout = 1"),
]


def case_id(entry):
    case, kw, _ = entry
    return case.name + "-" + "-".join(f"{k}{v}" for k, v in kw.items())


def bf16_out(case, inp, key):
    """does the kernel write this output as bf16 (the stand-in rounds it the same way)"""
    if case is Linear:
        return not inp["f32"]
    if case is LayerNorm:
        return not inp.get("out_f32")
    return case not in (HeadConv, ConvOut)
