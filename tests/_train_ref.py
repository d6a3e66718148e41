"""Float64 restatements of the training-path primitives (csrc/backward.hip, misc.hip, the implicit-GEMM bmm), their per-element error
bounds and their near misses.  Shared by tests/test_gpu_training_ops.py (the HIP kernels) and tests/test_training_ops_cpu.py (an fp32
torch restatement standing in for the kernels).

Every op is a CASE: `make(**shape)` draws the inputs (CPU, fp32 tensors holding exact bf16 values where the kernel reads bf16),
`ref(inp, dt)` restates the op in dtype dt (float64: the reference; float32: the stand-in), `bound(inp, ref)` gives per output a
relative part r and an absolute part a, and `misses(inp)` lists near-miss references that encode a plausible bug.  An output passes
when |out - ref| <= r |ref| + a element by element; it must FAIL that test against every near miss (for some element).

Bound conventions (u = 2^-24):
  * r = 2^-8 for a bf16 output (one rounding), 0 for an fp32 output;
  * a = c u S, S the fp64 sum of the absolute values of the terms that formed the element, c the longest chain of dependent fp32
    roundings the launcher's geometry gives (restated below per op) or a stated multiple of the accumulation length;
  * __expf / rcp / the erf polynomial: a small relative term stated in the op's docstring.
No bound is scaled by a whole-tensor maximum."""
import math

import torch

U = 2.0 ** -24
BF = 2.0 ** -8
F64 = torch.float64


def bfr(t):
    return t.to(torch.bfloat16).to(torch.float32)


def rand(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return bfr(torch.randn(shape, generator=g) * scale + offset)


def row_offsets(rows, seed, lo=30.0, hi=100.0):
    """per-row (or per-group) offsets between lo and hi spreads, random signs: a statistic paired with the wrong row cannot pass"""
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(rows, generator=g)) * torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0)


def ratio(out, ref, bound):
    """max over elements of |out - ref| / bound (0 / 0 counts as 0, x / 0 as inf)"""
    d = (out.double() - ref.double()).abs()
    b = bound.double().expand_as(d)
    r = torch.where(d == 0, torch.zeros_like(d), d / b)
    return float(r.max()) if r.numel() else 0.0


def _cdiv(a, b):
    return -(-a // b)


# ============================================================================================================ elementwise / data movement
class Add:
    """out = a + b (bf16): one fp32 add, one bf16 rounding -> r = 2^-8, a = u (|a| + |b|).  Near miss: the last 8 elements unwritten."""
    name = "add"
    exact = False

    @staticmethod
    def make(n, seed=1):
        return {"a": rand((n,), seed), "b": rand((n,), seed + 1, 3.0)}

    @staticmethod
    def ref(inp, dt):
        return {"out": inp["a"].to(dt) + inp["b"].to(dt)}

    @staticmethod
    def bound(inp, ref):
        return {"out": (BF, U * (inp["a"].double().abs() + inp["b"].double().abs()))}

    @staticmethod
    def misses(inp):
        o = Add.ref(inp, F64)["out"].clone(); o[-8:] = 0
        return [("tail of 8 unwritten", {"out": o})]


def _silu_parts(v, dt):
    s = torch.sigmoid(v.to(dt))
    return v.to(dt), s


class Silu:
    """silu on an fp32 vector.  Forward (bf16 out): r = 2^-8 plus 2^-22 (1 + |v|) for __expf (argument rounding grows with |v|) and rcp.
    Gradient (fp32 out) dy s (1 + v (1 - s)), which cancels near v = -1.28: a = u (8 + 2|v|) |dy| s (1 + 2|v|), the absolute-value form
    of the product times the relative error of s.  Inputs stay within |v| <= 20 (beyond, exp(-v) overflows fp32 and s is 0 by
    construction).  Near misses: sigmoid instead of silu; sigmoid's own derivative s (1 - s); the v (1 - s) term dropped."""
    name = "silu"
    exact = False

    @staticmethod
    def make(n, grad, seed=2):
        v = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 4
        v[:4] = torch.tensor([-20.0, 20.0, -1.2785, 0.0])[: min(4, n)]
        v = v.clamp(-20, 20)
        inp = {"x": v, "grad": grad}
        if grad:
            inp["dy"] = torch.randn(n, generator=torch.Generator().manual_seed(seed + 1))
        return inp

    @staticmethod
    def ref(inp, dt, variant=None):
        v, s = _silu_parts(inp["x"], dt)
        if not inp["grad"]:
            return {"out": s if variant == "sigmoid" else v * s}
        dy = inp["dy"].to(dt)
        if variant == "sigmoid'":
            return {"out": dy * s * (1 - s)}
        if variant == "no v term":
            return {"out": dy * s}
        return {"out": dy * (s * (1 + v * (1 - s)))}

    @staticmethod
    def bound(inp, ref):
        v = inp["x"].double()
        if not inp["grad"]:
            return {"out": (BF + 2.0 ** -22 * (1 + v.abs()), torch.zeros(()))}
        s = torch.sigmoid(v)
        return {"out": (0.0, U * (8 + 2 * v.abs()) * inp["dy"].double().abs() * s * (1 + 2 * v.abs()))}

    @staticmethod
    def misses(inp):
        if not inp["grad"]:
            return [("sigmoid instead of silu", Silu.ref(inp, F64, "sigmoid"))]
        return [("sigmoid's derivative", Silu.ref(inp, F64, "sigmoid'")), ("v (1 - s) term dropped", Silu.ref(inp, F64, "no v term"))]


class Sumpool2:
    """2 x 2 sum pooling (bf16): three fp32 adds -> r = 2^-8, a = 3 u sum|x|.  Near misses: the mean instead of the sum; one tap dropped."""
    name = "sumpool2"
    exact = False

    @staticmethod
    def make(B, H, W, C, seed=3):
        return {"x": rand((B, 2 * H, 2 * W, C), seed)}

    @staticmethod
    def _pool(x):
        B, H2, W2, C = x.shape
        return x.reshape(B, H2 // 2, 2, W2 // 2, 2, C)

    @staticmethod
    def ref(inp, dt):
        return {"out": Sumpool2._pool(inp["x"].to(dt)).sum((2, 4))}

    @staticmethod
    def bound(inp, ref):
        return {"out": (BF, 3 * U * Sumpool2._pool(inp["x"].double().abs()).sum((2, 4)))}

    @staticmethod
    def misses(inp):
        p = Sumpool2._pool(inp["x"].double())
        return [("mean instead of sum", {"out": p.mean((2, 4))}), ("tap (1, 1) dropped", {"out": p.sum((2, 4)) - p[:, :, 1, :, 1]})]


class Transpose:
    """y = x^T (batched: per matrix), bitwise.  Near misses: the last output row left zero; the rows of each matrix reversed."""
    name = "transpose"
    exact = True

    @staticmethod
    def make(Z, rows, cols, seed=4):
        return {"x": rand((Z, rows, cols) if Z else (rows, cols), seed)}

    @staticmethod
    def ref(inp, dt):
        return {"out": inp["x"].transpose(-1, -2).to(dt)}

    @staticmethod
    def misses(inp):
        y = Transpose.ref(inp, F64)["out"]
        z = y.clone(); z[..., -1, :] = 0
        return [("last row unwritten", {"out": z}), ("rows reversed", {"out": y.flip(-2)})]


class Heads:
    """per-head split / merge (rdm_op_heads), bitwise, padding columns D..63 exactly zero.  Near misses: the head order reversed; each
    head one column short (column D - 1 not copied)."""
    name = "heads"
    exact = True

    @staticmethod
    def make(B, n, H, D, ldx, mode, seed=5):
        if mode == 2:
            x = rand((B * H, n, 64), seed)
            x[..., D:] = 7.0                                 # what mode 2 must ignore
            return {"x": x, "H": H, "D": D, "mode": 2}
        return {"x": rand((B, n, ldx), seed), "H": H, "D": D, "mode": mode}

    @staticmethod
    def ref(inp, dt, reverse=False, short=False):
        x, H, D, mode = inp["x"].to(dt), inp["H"], inp["D"], inp["mode"]
        if short:
            if mode == 2:
                x = x.clone(); x[..., D - 1] = 0
            else:
                x = x.clone(); x[..., [h * D + D - 1 for h in range(H)]] = 0
        if mode == 2:
            BH, n, _ = x.shape
            y = x[..., :D].reshape(BH // H, H, n, D)
            if reverse:
                y = y.flip(1)
            return {"out": y.permute(0, 2, 1, 3).reshape(BH // H, n, H * D)}
        B, n, _ = x.shape
        h = x[..., : H * D].reshape(B, n, H, D).permute(0, 2, 1, 3)
        if reverse:
            h = h.flip(1)
        out = torch.zeros(B, H, n, 64, dtype=dt)
        out[..., :D] = h
        out = out.reshape(B * H, n, 64)
        return {"out": out if mode == 0 else out.transpose(1, 2).contiguous()}

    @staticmethod
    def misses(inp):
        return [("head order reversed", Heads.ref(inp, F64, reverse=True)), ("one column short", Heads.ref(inp, F64, short=True))]


class Expand2:
    """2x expansion (rdm_op_expand2), bitwise: mode 0 zero insertion (zeros checked exactly), mode 1 nearest copy.  Near miss: the other
    mode."""
    name = "expand2"
    exact = True

    @staticmethod
    def make(B, H, W, C, mode, seed=6):
        return {"x": rand((B, H, W, C), seed), "mode": mode}

    @staticmethod
    def ref(inp, dt, mode=None):
        x = inp["x"].to(dt); mode = inp["mode"] if mode is None else mode
        B, H, W, C = x.shape
        if mode == 1:
            return {"out": x.repeat_interleave(2, 1).repeat_interleave(2, 2)}
        out = torch.zeros(B, 2 * H, 2 * W, C, dtype=dt)
        out[:, ::2, ::2] = x
        return {"out": out}

    @staticmethod
    def misses(inp):
        return [("the other mode", Expand2.ref(inp, F64, 1 - inp["mode"]))]


# ============================================================================================================ reductions
def colsum_depth(M, N):
    """longest chain of dependent fp32 adds in launch_colsum (one-stage: a row lane walks M / 4 rows, two tree levels; two-stage: a lane
    walks CS / RL rows of its chunk, RL lanes are added in sequence, the finish kernel walks nchunk / 16 partials, a 16-way tree)"""
    if N % 8 or M < 256:
        return _cdiv(M, 4) + 2
    nv = N // 8; colblocks = (nv + 31) // 32; VCB = _cdiv(nv, colblocks)
    CS = (M * colblocks + 1023) // 1024; CS = (CS + 7) & ~7; CS = min(max(CS, 64), 4096)
    RL = 256 // VCB
    return _cdiv(CS, RL) + RL + _cdiv(_cdiv(M, CS), 16) + 4


def colsum_chunk(M, N):
    if N % 8 or M < 256:
        return None
    nv = N // 8; colblocks = (nv + 31) // 32
    CS = (M * colblocks + 1023) // 1024; CS = (CS + 7) & ~7
    return min(max(CS, 64), 4096)


class Colsum:
    """column sums of a bf16 [M, N] matrix -> fp32: r = 0, a = (depth + 1) u sum|x| with depth = colsum_depth (the chain of dependent
    adds of the launch geometry, not M).  Inputs N(1, 1) (a bias gradient has a mean).  Near misses: the last row chunk dropped (one row
    on the one-stage path, the rows past the last full CS-row chunk on the two-stage path); the columns shifted by one."""
    name = "colsum"
    exact = False

    @staticmethod
    def make(M, N, seed=7):
        return {"x": rand((M, N), seed, offset=1.0)}

    @staticmethod
    def ref(inp, dt):
        return {"out": inp["x"].to(dt).sum(0)}

    @staticmethod
    def bound(inp, ref):
        M, N = inp["x"].shape
        return {"out": (0.0, (colsum_depth(M, N) + 1) * U * inp["x"].double().abs().sum(0))}

    @staticmethod
    def misses(inp):
        s = Colsum.ref(inp, F64)["out"]
        M, N = inp["x"].shape
        cs = colsum_chunk(M, N)
        tail = 1 if cs is None else (M % cs or cs)
        return [("last row chunk dropped", {"out": s - inp["x"][M - tail:].double().sum(0)}), ("columns shifted", {"out": s.roll(1)})]


def colsum_samples_depth(B, HW, N):
    if N % 8 or HW < 64:
        return _cdiv(HW, 4) + 2
    nchunk = max(1, min(1024 // B, HW // 64, 32)); CS = _cdiv(HW, nchunk)
    nv = N // 8; colblocks = (nv + 31) // 32; VCB = _cdiv(nv, colblocks)
    return _cdiv(CS, 256 // VCB) + 256 // VCB + nchunk


class ColsumSamples:
    """per-sample column sums bf16 [B, HW, N] -> bf16 [B, N]: r = 2^-8, a = (depth + 1) u sum|x| (depth: colsum_samples_depth).
    Near misses: the samples swapped; the last pixel dropped."""
    name = "colsum_samples"
    exact = False

    @staticmethod
    def make(B, HW, N, seed=8):
        return {"x": rand((B, HW, N), seed)}

    @staticmethod
    def ref(inp, dt):
        return {"out": inp["x"].to(dt).sum(1)}

    @staticmethod
    def bound(inp, ref):
        B, HW, N = inp["x"].shape
        return {"out": (BF, (colsum_samples_depth(B, HW, N) + 1) * U * inp["x"].double().abs().sum(1))}

    @staticmethod
    def misses(inp):
        s = ColsumSamples.ref(inp, F64)["out"]
        return [("samples swapped", {"out": s.roll(1, 0)}), ("last pixel dropped", {"out": s - inp["x"][:, -1].double()})]


class Bmm:
    """out[z] = alpha A[z] W[z]^T (MFMA, exact bf16 products, fp32 sums): r = 2^-8 (bf16 out) or 0, a = K u |alpha| sum_k |a_k w_k|.
    Near misses: alpha applied twice; the last 64-wide K chunk dropped."""
    name = "bmm"
    exact = False

    @staticmethod
    def make(Z, M, N, K, alpha, f32, seed=9):
        return {"a": rand((Z, M, K), seed), "w": rand((Z, N, K), seed + 1), "alpha": alpha, "f32": f32}

    @staticmethod
    def ref(inp, dt, alpha=None, kcut=None):
        a, w = inp["a"].to(dt), inp["w"].to(dt)
        if kcut:
            a, w = a[..., :kcut], w[..., :kcut]
        return {"out": (inp["alpha"] if alpha is None else alpha) * a @ w.transpose(1, 2)}

    @staticmethod
    def bound(inp, ref):
        K = inp["a"].shape[2]
        S = abs(inp["alpha"]) * inp["a"].double().abs() @ inp["w"].double().abs().transpose(1, 2)
        return {"out": (0.0 if inp["f32"] else BF, K * U * S)}

    @staticmethod
    def misses(inp):
        K = inp["a"].shape[2]
        return [("alpha applied twice", Bmm.ref(inp, F64, alpha=inp["alpha"] ** 2)), ("last K chunk dropped", Bmm.ref(inp, F64, kcut=K - 64))]


class Softmax:
    """row softmax fp32 -> bf16 over the first n_valid columns (0: all), padding exactly 0: r = 2^-8 + u (8 + 2 |s - max| + n_valid)
    (__expf's argument rounding grows with |s - max|, the row sum takes n_valid roundings).  Near misses: n_valid - 1 and n_valid + 1."""
    name = "softmax"
    exact = False

    @staticmethod
    def make(rows, n, n_valid, seed=10):
        g = torch.Generator().manual_seed(seed)
        return {"s": torch.randn(rows, n, generator=g) * 3, "n_valid": n_valid}

    @staticmethod
    def nv(inp):
        n = inp["s"].shape[1]; v = inp["n_valid"]
        return n if v == 0 else v

    @staticmethod
    def ref(inp, dt, nv=None):
        s = inp["s"].to(dt); nv = Softmax.nv(inp) if nv is None else nv
        out = torch.zeros_like(s)
        out[:, :nv] = torch.softmax(s[:, :nv], dim=1)
        return {"out": out}

    @staticmethod
    def bound(inp, ref):
        nv = Softmax.nv(inp)
        s = inp["s"].double()
        mx = s[:, :nv].max(1, keepdim=True).values
        return {"out": (BF + U * (8 + 2 * (s - mx).abs() + nv), torch.zeros(()))}

    @staticmethod
    def misses(inp):
        nv, n = Softmax.nv(inp), inp["s"].shape[1]
        out = []
        if nv > 1:
            out.append(("n_valid - 1", Softmax.ref(inp, F64, nv - 1)))
        if nv < n:
            out.append(("n_valid + 1", Softmax.ref(inp, F64, nv + 1)))
        return out


class SoftmaxBwd:
    """dS = P (dP - sum_j P_j dP_j), P bf16, dP fp32 -> bf16: r = 2^-8, a = u |P| (2 |dP| + 2 |sigma| + (n + 2) sum_j |P_j dP_j|)
    (the row sum is a chain of at most n adds).  Near misses: the row-sum term dropped; the sum missing the last 4 columns."""
    name = "softmax_bwd"
    exact = False

    @staticmethod
    def make(rows, n, seed=11):
        g = torch.Generator().manual_seed(seed)
        p = bfr(torch.softmax(torch.randn(rows, n, generator=g) * 2, 1))
        return {"p": p, "dp": torch.randn(rows, n, generator=g)}

    @staticmethod
    def ref(inp, dt, drop=0, nosum=False):
        p, dp = inp["p"].to(dt), inp["dp"].to(dt)
        n = p.shape[1]
        sig = (p[:, : n - drop] * dp[:, : n - drop]).sum(1, keepdim=True)
        return {"out": p * dp if nosum else p * (dp - sig)}

    @staticmethod
    def bound(inp, ref):
        p, dp = inp["p"].double(), inp["dp"].double()
        n = p.shape[1]
        sig = (p * dp).sum(1, keepdim=True)
        return {"out": (BF, U * p.abs() * (2 * dp.abs() + 2 * sig.abs() + (n + 2) * (p * dp).abs().sum(1, keepdim=True)))}

    @staticmethod
    def misses(inp):
        return [("row sum dropped", SoftmaxBwd.ref(inp, F64, nosum=True)), ("sum misses 4 columns", SoftmaxBwd.ref(inp, F64, drop=4))]


def _gelu(g, tanh=False):
    if tanh:
        return 0.5 * g * (1 + torch.tanh(math.sqrt(2 / math.pi) * (g + 0.044715 * g ** 3)))
    return 0.5 * g * (1 + torch.erf(g / math.sqrt(2)))


class Geglu:
    """GEGLU on pre = [x | gate] (bf16).  Forward h = x gelu(gate); backward dx = dh gelu(gate), dgate = dh x (Phi + gate phi).
    The kernel's erf is a polynomial (|err| <= 1.5e-7) around __expf: gelu carries an absolute error <= u |g| (8 + g^2) / 2, phi a
    relative u (4 + g^2 / 2).  Bounds: r = 2^-8, a = u |x| |g| (8 + g^2) / 2 + 2 u |out| (forward / dx); dgate adds
    u |dh x| (|g| phi (6 + g^2) + 4 (Phi + |g| phi)).  Near misses: tanh-approximated GELU; dgate without the g phi term."""
    name = "geglu"
    exact = False

    @staticmethod
    def make(M, F, bwd, seed=12):
        pre = rand((M, 2 * F), seed, 2.0)
        inp = {"pre": pre, "bwd": bwd}
        if bwd:
            inp["dh"] = rand((M, F), seed + 1)
        return inp

    @staticmethod
    def ref(inp, dt, tanh=False, no_gphi=False):
        pre = inp["pre"].to(dt); F = pre.shape[1] // 2
        a, g = pre[:, :F], pre[:, F:]
        if not inp["bwd"]:
            return {"out": a * _gelu(g, tanh)}
        dh = inp["dh"].to(dt)
        if tanh:
            gg = g.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                d = torch.autograd.grad(_gelu(gg, True).sum(), gg)[0]
            return {"out": torch.cat([dh * _gelu(g, True), dh * a * d], 1)}
        Phi = 0.5 * (1 + torch.erf(g / math.sqrt(2)))
        phi = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
        return {"out": torch.cat([dh * _gelu(g), dh * a * (Phi if no_gphi else Phi + g * phi)], 1)}

    @staticmethod
    def bound(inp, ref):
        pre = inp["pre"].double(); F = pre.shape[1] // 2
        a, g = pre[:, :F].abs(), pre[:, F:]
        ge = 0.5 * g.abs() * (8 + g * g)                     # gelu's absolute error / u
        out = ref["out"].double().abs()
        if not inp["bwd"]:
            return {"out": (BF, U * (a * ge + 2 * out))}
        dh = inp["dh"].double().abs()
        Phi = 0.5 * (1 + torch.erf(g / math.sqrt(2))); phi = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
        da = U * (dh * ge + 2 * out[:, :F])
        dg = U * (dh * a * (ge / g.abs().clamp_min(1e-30) * (g != 0) + g.abs() * phi * (6 + g * g) + 4 * (Phi + g.abs() * phi)) + 2 * out[:, F:])
        return {"out": (BF, torch.cat([da, dg], 1))}

    @staticmethod
    def misses(inp):
        m = [("tanh GELU", Geglu.ref(inp, F64, tanh=True))]
        if inp["bwd"]:
            m.append(("dgate without g phi", Geglu.ref(inp, F64, no_gphi=True)))
        return m


# ============================================================================================================ normalisation backward
class LayerNormBwd:
    """LayerNorm backward (rdm_op_layernorm_bwd[_add]): dx (bf16, + residual), dgamma, dbeta (fp32).  Statistics restated in fp64 from
    the same bf16 x, exact two-pass variance, as the forward applies them.

    Error model, d = ceil(C / 64) + 14 (the chain of a row sum: a lane's elements, then 6 shuffle levels): the mean is off by at most
    d u mean|x|, the rstd by (d + 8) u relative, so xh = (x - mean) rstd carries e_xh = u (d mean|x| rstd + (d + 8) |xh|) -- the first
    term is what a row with a large common offset costs an EXACT two-pass variance.  dx: r = 2^-8, a = rstd (e_s1 + |xh| e_s2 + |s2|
    e_xh + 3 u (|dxh| + |s1| + |xh s2|)) + (d + 8) u |dx| (+ 2^-8 |dx - res| for the generic kernels, which add the residual in a
    second rounding).  dgamma: a = sum_rows |dy| e_xh + c u sum |dy xh|, dbeta: a = c u sum |dy|, c the affine chain (rows_per_block / 4
    per wave, 2 tree levels, then the block partials: nb / 16 + 4 or nb).  Near misses: eps 1e-6 (rows of small variance), the residual
    dropped, the statistics of the next row."""
    name = "layernorm_bwd"
    exact = False

    @staticmethod
    def make(M, C, res=False, offset=False, small_var=False, seed=13):
        g = torch.Generator().manual_seed(seed)
        spread = 0.004 if small_var else 1.0
        off = row_offsets(M, seed + 1) * spread if offset else torch.full((M,), 0.3)
        x = bfr(torch.randn(M, C, generator=g) * spread * (0.5 + torch.rand(M, 1, generator=g)) + off[:, None])
        inp = {"x": x, "dy": bfr(torch.randn(M, C, generator=g)), "gamma": 1 + 0.1 * torch.randn(C, generator=g), "eps": 1e-5, "small_var": small_var}
        if res:
            inp["res"] = bfr(torch.randn(M, C, generator=g))
        return inp

    @staticmethod
    def stats(x, eps):
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        return mean, 1 / torch.sqrt(var + eps)

    @staticmethod
    def ref(inp, dt, eps=None, no_res=False, shift_stats=False):
        x, dy, gam = inp["x"].to(dt), inp["dy"].to(dt), inp["gamma"].to(dt)
        mean, rstd = LayerNormBwd.stats(x, inp["eps"] if eps is None else eps)
        if shift_stats:
            mean, rstd = mean.roll(-1, 0), rstd.roll(-1, 0)
        xh = (x - mean) * rstd
        dxh = dy * gam
        s1 = dxh.mean(1, keepdim=True); s2 = (dxh * xh).mean(1, keepdim=True)
        dx = rstd * (dxh - s1 - xh * s2)
        if "res" in inp and not no_res:
            dx = dx + inp["res"].to(dt)
        return {"dx": dx, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0)}

    @staticmethod
    def affine_chain(M, C):
        rpb = 64 if M >= 16384 else 16
        nb = _cdiv(M, rpb)
        vec = C % 8 == 0 and C <= 1024
        return rpb // 4 + 2 + (_cdiv(nb, 16) + 4 if vec else nb) + 1

    @staticmethod
    def bound(inp, ref):
        x, dy, gam = inp["x"].double(), inp["dy"].double(), inp["gamma"].double()
        M, C = x.shape
        d = _cdiv(C, 64) + 14
        mean, rstd = LayerNormBwd.stats(x, inp["eps"])
        xh = (x - mean) * rstd
        dxh = dy * gam
        s2 = (dxh * xh).mean(1, keepdim=True); s1 = dxh.mean(1, keepdim=True)
        e_xh = U * (d * x.abs().mean(1, keepdim=True) * rstd + (d + 8) * xh.abs())
        e_s1 = U * d * dxh.abs().mean(1, keepdim=True)
        e_s2 = U * d * (dxh * xh).abs().mean(1, keepdim=True) + (dxh.abs() * e_xh).mean(1, keepdim=True)
        g = rstd * (dxh - s1 - xh * s2)
        a_dx = rstd * (e_s1 + xh.abs() * e_s2 + s2.abs() * e_xh + 3 * U * (dxh.abs() + s1.abs() + (xh * s2).abs())) + (d + 8) * U * g.abs()
        if "res" in inp and not (C % 8 == 0 and C <= 1024):
            a_dx = a_dx + BF * g.abs()
        c = LayerNormBwd.affine_chain(M, C)
        return {"dx": (BF, a_dx), "dgamma": (0.0, (dy.abs() * e_xh).sum(0) + c * U * (dy * xh).abs().sum(0)),
                "dbeta": (0.0, c * U * dy.abs().sum(0))}

    @staticmethod
    def misses(inp):
        m = [("statistics of the next row", LayerNormBwd.ref(inp, F64, shift_stats=True))]
        if inp["small_var"]:                                 # eps only matters against a variance of its own order
            m.append(("eps 1e-6", LayerNormBwd.ref(inp, F64, eps=1e-6)))
        if "res" in inp:
            m.append(("residual dropped", LayerNormBwd.ref(inp, F64, no_res=True)))
        return m


class GroupNormBwd:
    """GroupNorm(32) (+SiLU) backward (rdm_op_groupnorm_bwd_add): dx (bf16, + residual), dgamma, dbeta (fp32).

    Error model: xh carries e_xh = u (c_s mean|x| rstd + 2 (|x| + |mean|) rstd + k |xh|).  Vectorised path (C <= 2048): the forward's
    statistics kernel sums x and x^2 in fp32 per pixel chunk (a chain of c_s = rows_per_chunk / R + R + cg + 2 roundings), finished in
    double, so the variance is off by c_s u mean(x^2) and k = 4 + c_s mean(x^2) / (2 var).  Generic path: two fp32 passes over the
    group, c_s = n / 256 + 8 and k = c_s + 8.  With
    SiLU dz = dy silu'(z) carries e_dz = u |dy| (8 + 2|z|)(1 + |z|) + |dy| |gamma| e_xh / 2 (|silu''| <= 1/2).  The group sums S1, S2
    are chains of at most c = HW + cg + 320 roundings (a thread's pixels, the R row lanes, the chunks, the channels of a group).
    dx: r = 2^-8, a = rstd (e_S1 + |xh| e_S2 + |S2/n| e_xh + |gamma| e_dz + 4 u (|dxh| + |S1/n| + |xh S2/n|)) (+ 2^-8 |dx - res| when
    the generic kernels add the residual in a second rounding).  dgamma: a = sum (|dz| e_xh + |xh| e_dz) + c' u sum |dz xh|; dbeta:
    a = sum e_dz + c' u sum |dz|, c' = HW + B + 320.  Near misses: eps 1e-6 (groups of small variance), SiLU flipped, the residual
    dropped, the statistics of the next group."""
    name = "groupnorm_bwd"
    exact = False

    @staticmethod
    def make(B, HW, C, silu, res=False, offset=False, small_var=False, seed=14):
        g = torch.Generator().manual_seed(seed)
        spread = 0.004 if small_var else 1.0
        off = (row_offsets(B * 32, seed + 1) * spread if offset else torch.full((B * 32,), 0.3)).reshape(B, 1, 32, 1)
        x = torch.randn(B, HW, 32, C // 32, generator=g) * spread * (0.5 + torch.rand(B, 1, 32, 1, generator=g)) + off
        inp = {"x": bfr(x.reshape(B, HW, C)), "dy": bfr(torch.randn(B, HW, C, generator=g)), "gamma": 1 + 0.1 * torch.randn(C, generator=g),
               "beta": 0.1 * torch.randn(C, generator=g), "eps": 1e-5, "silu": silu, "small_var": small_var}
        if res:
            inp["res"] = bfr(torch.randn(B, HW, C, generator=g))
        return inp

    @staticmethod
    def _parts(inp, dt, eps=None, silu=None, shift_stats=False):
        x, dy = inp["x"].to(dt), inp["dy"].to(dt)
        B, HW, C = x.shape
        xg = x.reshape(B, HW, 32, C // 32)
        mean = xg.mean((1, 3), keepdim=True)
        rstd = 1 / torch.sqrt(((xg - mean) ** 2).mean((1, 3), keepdim=True) + (inp["eps"] if eps is None else eps))
        if shift_stats:
            mean, rstd = mean.roll(1, 2), rstd.roll(1, 2)
        xh = ((xg - mean) * rstd).reshape(B, HW, C)
        gam, bet = inp["gamma"].to(dt), inp["beta"].to(dt)
        z = xh * gam + bet
        s = torch.sigmoid(z)
        sg = s * (1 + z * (1 - s))
        dz = dy * sg if (inp["silu"] if silu is None else silu) else dy
        return x, dy, xh, z, dz, gam, rstd

    @staticmethod
    def ref(inp, dt, eps=None, silu=None, no_res=False, shift_stats=False):
        x, dy, xh, z, dz, gam, rstd = GroupNormBwd._parts(inp, dt, eps, silu, shift_stats)
        B, HW, C = x.shape
        dxh = (dz * gam).reshape(B, HW, 32, C // 32); xhg = xh.reshape(B, HW, 32, C // 32)
        m1 = dxh.mean((1, 3), keepdim=True); m2 = (dxh * xhg).mean((1, 3), keepdim=True)
        dx = (rstd * (dxh - m1 - xhg * m2)).reshape(B, HW, C)
        if "res" in inp and not no_res:
            dx = dx + inp["res"].to(dt)
        return {"dx": dx, "dgamma": (dz * xh).sum((0, 1)), "dbeta": dz.sum((0, 1))}

    @staticmethod
    def bound(inp, ref):
        x, dy, xh, z, dz, gam, rstd = GroupNormBwd._parts(inp, F64)
        B, HW, C = x.shape
        cg = C // 32
        xg = x.reshape(B, HW, 32, cg); mean = xg.mean((1, 3), keepdim=True)
        if C % 8 == 0 and C <= 2048:
            nchunk = max(1, min(64, 2048 // B, HW // 32)); R = max(1, 256 // (C // 8))
            c_s = _cdiv(_cdiv(HW, nchunk), R) + R + cg + 2
            var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
            k = 4 + c_s * (xg * xg).mean((1, 3), keepdim=True) / (2 * var)
        else:
            c_s = _cdiv(HW * cg, 256) + 8
            k = c_s + 8
        e_xh = (U * (c_s * xg.abs().mean((1, 3), keepdim=True) * rstd + 2 * (xg.abs() + mean.abs()) * rstd
                     + k * xh.reshape(B, HW, 32, cg).abs())).reshape(B, HW, C)
        if inp["silu"]:
            e_dz = U * dy.abs() * (8 + 2 * z.abs()) * (1 + z.abs()) + 0.5 * dy.abs() * gam.abs() * e_xh
        else:
            e_dz = torch.zeros_like(dz)
        c = HW + cg + 320
        G = lambda t: t.reshape(B, HW, 32, cg)
        dxh = dz * gam
        m1 = G(dxh).mean((1, 3), keepdim=True); m2 = G(dxh * xh).mean((1, 3), keepdim=True)
        e_m1 = U * c * G(dxh.abs()).mean((1, 3), keepdim=True) + G(gam.abs() * e_dz).mean((1, 3), keepdim=True)
        e_m2 = U * c * G((dxh * xh).abs()).mean((1, 3), keepdim=True) + G(dxh.abs() * e_xh + xh.abs() * gam.abs() * e_dz).mean((1, 3), keepdim=True)
        a_dx = rstd * (e_m1 + G(xh).abs() * e_m2 + m2.abs() * G(e_xh) + G(gam.abs() * e_dz)
                       + 4 * U * (G(dxh).abs() + m1.abs() + (G(xh) * m2).abs()))
        a_dx = a_dx.reshape(B, HW, C)
        if "res" in inp and not (C % 8 == 0 and C <= 2048):
            a_dx = a_dx + BF * (rstd * (G(dxh) - m1 - G(xh) * m2)).reshape(B, HW, C).abs()
        c2 = HW + B + 320
        return {"dx": (BF, a_dx), "dgamma": (0.0, (dz.abs() * e_xh + xh.abs() * e_dz).sum((0, 1)) + c2 * U * (dz * xh).abs().sum((0, 1))),
                "dbeta": (0.0, e_dz.sum((0, 1)) + c2 * U * dz.abs().sum((0, 1)))}

    @staticmethod
    def misses(inp):
        m = [("SiLU flipped", GroupNormBwd.ref(inp, F64, silu=1 - inp["silu"])), ("statistics of the next group", GroupNormBwd.ref(inp, F64, shift_stats=True))]
        if inp["small_var"]:
            m.append(("eps 1e-6", GroupNormBwd.ref(inp, F64, eps=1e-6)))
        if "res" in inp:
            m.append(("residual dropped", GroupNormBwd.ref(inp, F64, no_res=True)))
        return m


class ConvDgrad:
    """3x3 conv (stride 1, pad 1) input gradient: dx = conv(dy, flipped transposed W) through the forward kernels (bf16 out): r = 2^-8,
    a = 9 N u sum |dy w| (K = 9 N products, exact in fp32).  Near misses: the taps not flipped; the last 64 output-gradient channels
    dropped (a K tail)."""
    name = "conv3x3_dgrad"
    exact = False

    @staticmethod
    def make(B, H, W, C, N, seed=15):
        return {"dy": rand((B, H, W, N), seed), "w": rand((N, 3, 3, C), seed + 1, (9 * C) ** -0.5)}

    @staticmethod
    def ref(inp, dt, noflip=False, ncut=None, absval=False):
        dy, w = inp["dy"].to(dt), inp["w"].to(dt)
        if absval:
            dy, w = dy.abs(), w.abs()
        if ncut:
            dy, w = dy[..., :ncut], w[:ncut]
        if noflip:
            w = w.flip(1, 2)
        B, H, W, N = dy.shape
        wt = w.permute(0, 3, 1, 2)                                         # [N, C, 3, 3]
        dx = torch.nn.grad.conv2d_input((B, wt.shape[1], H, W), wt, dy.permute(0, 3, 1, 2), padding=1)
        return {"out": dx.permute(0, 2, 3, 1)}

    @staticmethod
    def bound(inp, ref):
        N = inp["dy"].shape[3]
        return {"out": (BF, 9 * N * U * ConvDgrad.ref(inp, F64, absval=True)["out"])}

    @staticmethod
    def misses(inp):
        N = inp["dy"].shape[3]
        return [("taps not flipped", ConvDgrad.ref(inp, F64, noflip=True)), ("last 64 channels dropped", ConvDgrad.ref(inp, F64, ncut=N - 64))]


# ============================================================================================================ attention backward
def _split(t, H, ld=None):
    B, n, _ = t.shape
    return t[..., : H * 32].reshape(B, n, H, 32).permute(0, 2, 1, 3)


def _merge(t):
    B, H, n, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, H * 32)


class _AttnBase:
    """shared restatement: S = q k^T, P = softmax(scale S), dP = dO v^T, dS = P (dP - D), dq = scale dS k, dk = scale dS^T q, dv = P^T dO.
    Bounds (u = 2^-24, r = 2^-8 on every bf16 output): e_P = P (b + 2^-22 (4 + scale |S|) + 64 u scale sum|q k| + m u), b = 2^-8 when the
    kernel rounds P / dS to bf16 for its MFMAs (fused kernel) else 0; e_dP = 32 u sum|dO v|; e_D = 32 u sum|dO o| (fused) or
    sum (e_P |dP| + P e_dP) + m u sum |P dP| (small); e_dS = e_P |dP - D| + P (e_dP + e_D) + (b + 2 u) |dS|.
    dv: a = sum_q e_P |dO| + n u sum_q |P dO|; dk: a = scale (sum_q e_dS |q| + n u sum_q |dS q|); dq: a = scale (sum_k e_dS |k| + m u
    sum_k |dS k|).  Near misses: the scale applied twice to dq / dk; the head order reversed."""
    exact = False

    @staticmethod
    def core(q, k, v, do, o, H, scale, dt, scale2=1.0):
        qh, kh, vh, doh = _split(q.to(dt), H), _split(k.to(dt), H), _split(v.to(dt), H), _split(do.to(dt), H)
        S = qh @ kh.transpose(-1, -2)
        P = torch.softmax(S * scale, -1)
        dP = doh @ vh.transpose(-1, -2)
        D = (doh * _split(o.to(dt), H)).sum(-1, keepdim=True) if o is not None else (P * dP).sum(-1, keepdim=True)
        dS = P * (dP - D)
        sc = scale * scale2
        return {"dq": _merge(sc * dS @ kh), "dk": _merge(sc * dS.transpose(-1, -2) @ qh), "dv": _merge(P.transpose(-1, -2) @ doh)}

    @staticmethod
    def bounds(q, k, v, do, o, H, scale, pb):
        F = F64
        qh, kh, vh, doh = (_split(t.to(F), H) for t in (q, k, v, do))
        n, m = qh.shape[2], kh.shape[2]
        S = qh @ kh.transpose(-1, -2); P = torch.softmax(S * scale, -1)
        dP = doh @ vh.transpose(-1, -2)
        if o is not None:
            oh = _split(o.to(F), H)
            D = (doh * oh).sum(-1, keepdim=True); e_D = 32 * U * (doh * oh).abs().sum(-1, keepdim=True)
        else:
            D = (P * dP).sum(-1, keepdim=True)
        dS = P * (dP - D)
        b = BF if pb else 0.0
        e_P = P * (b + 2.0 ** -22 * (4 + scale * S.abs()) + 64 * U * scale * (qh.abs() @ kh.abs().transpose(-1, -2)) + m * U)
        e_dP = 32 * U * (doh.abs() @ vh.abs().transpose(-1, -2))
        if o is None:
            e_D = (e_P * dP.abs() + P * e_dP).sum(-1, keepdim=True) + m * U * (P * dP).abs().sum(-1, keepdim=True)
        e_dS = e_P * (dP - D).abs() + P * (e_dP + e_D) + (b + 2 * U) * dS.abs()
        a_dv = e_P.transpose(-1, -2) @ doh.abs() + n * U * (P.transpose(-1, -2) @ doh.abs())
        a_dk = scale * (e_dS.transpose(-1, -2) @ qh.abs() + n * U * (dS.abs().transpose(-1, -2) @ qh.abs()))
        a_dq = scale * (e_dS @ kh.abs() + m * U * (dS.abs() @ kh.abs()))
        return {"dq": (BF, _merge(a_dq)), "dk": (BF, _merge(a_dk)), "dv": (BF, _merge(a_dv))}

    @staticmethod
    def reverse_heads(out, H):
        return {k: _merge(_split(v, H).flip(1)) for k, v in out.items()}


class AttentionBwd(_AttnBase):
    __doc__ = "fused attention backward, d_head 32, scale 32^-0.5, o = the bf16 forward output.\n" + _AttnBase.__doc__
    name = "attention_bwd"
    SCALE = 32 ** -0.5

    @staticmethod
    def make(B, n, m, H, seed=16):
        g = torch.Generator().manual_seed(seed)
        q, k, v = (bfr(torch.randn(B, l, H * 32, generator=g) * s) for l, s in ((n, 1.5), (m, 1.5), (m, 1.0)))
        o = bfr(_merge(torch.softmax(_split(q.double(), H) @ _split(k.double(), H).transpose(-1, -2) * AttentionBwd.SCALE, -1) @ _split(v.double(), H)))
        return {"q": q, "k": k, "v": v, "o": o, "do": bfr(torch.randn(B, n, H * 32, generator=g)), "H": H}

    @staticmethod
    def ref(inp, dt, scale2=1.0):
        return _AttnBase.core(inp["q"], inp["k"], inp["v"], inp["do"], inp["o"], inp["H"], AttentionBwd.SCALE, dt, scale2)

    @staticmethod
    def bound(inp, ref):
        return _AttnBase.bounds(inp["q"], inp["k"], inp["v"], inp["do"], inp["o"], inp["H"], AttentionBwd.SCALE, True)

    @staticmethod
    def misses(inp):
        r = AttentionBwd.ref(inp, F64)
        return [("scale applied twice", AttentionBwd.ref(inp, F64, AttentionBwd.SCALE)), ("head order reversed", _AttnBase.reverse_heads(r, inp["H"]))]


class SmallAttentionBwd(_AttnBase):
    __doc__ = ("few-key attention backward (1..32 keys), fp32 inside, row pitches ldq / ldkv / ldo >= 32 H (k and v share a pitch: "
               "slices of one [B, m, ldkv] tensor pair).\n" + _AttnBase.__doc__)
    name = "small_attention_bwd"

    @staticmethod
    def make(B, nq, nkv, H, pad_q=0, pad_kv=0, pad_o=0, scale=0.2, seed=17):
        g = torch.Generator().manual_seed(seed)
        C = H * 32
        return {"q": bfr(torch.randn(B, nq, C + pad_q, generator=g) * 1.5), "kv": bfr(torch.randn(B, nkv, 2 * (C + pad_kv), generator=g)),
                "do": bfr(torch.randn(B, nq, C + pad_o, generator=g)), "H": H, "scale": scale, "pad_kv": pad_kv}

    @staticmethod
    def kv(inp):
        C = inp["H"] * 32 + inp["pad_kv"]
        return inp["kv"][..., :C], inp["kv"][..., C:]

    @staticmethod
    def ref(inp, dt, scale2=1.0):
        k, v = SmallAttentionBwd.kv(inp)
        return _AttnBase.core(inp["q"], k, v, inp["do"], None, inp["H"], inp["scale"], dt, scale2)

    @staticmethod
    def bound(inp, ref):
        k, v = SmallAttentionBwd.kv(inp)
        return _AttnBase.bounds(inp["q"], k, v, inp["do"], None, inp["H"], inp["scale"], False)

    @staticmethod
    def misses(inp):
        r = SmallAttentionBwd.ref(inp, F64)
        return [("scale applied twice", SmallAttentionBwd.ref(inp, F64, inp["scale"])), ("head order reversed", _AttnBase.reverse_heads(r, inp["H"]))]


# ============================================================================================================ optimizer, EMA, loss-side glue
def bc_rel_error(beta, step, fp32):
    """relative error of the bias correction 1 - beta^step as the kernel receives it.  Taken in double on the host and rounded once to
    fp32: u.  Taken in fp32 from an fp32 beta (1.f - powf(b, step)): beta itself is off by up to 2^-25 (half an ulp below 1), which
    beta^step carries as step beta^(step-1) 2^-25; powf adds 2 ulp of beta^step, the subtraction one rounding -- all divided by the small
    difference 1 - beta^step (the cancellation: 2^-25 / 1e-3 = 3e-5 at beta 0.999, step 1)."""
    bc = 1.0 - beta ** step
    if not fp32:
        return U
    return (step * beta ** (step - 1) * 2.0 ** -25 + 4 * U * beta ** step) / bc + U


class AdamW:
    """One AdamW step (rdm_op_adamw, rdm_op_adamw_multi): torch.optim.AdamW's update written out in fp64 with the betas, lr, eps and weight
    decay as the Python doubles the caller wrote:
        p1 = p (1 - lr wd);  m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g^2;  p' = p1 - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),
    bc_i = 1 - b_i^step.  Outputs p, m, v (fp32) and the bf16 copy pb.  Bounds (u = 2^-24, tiny = 2^-126 for a flushed subnormal):
      m: a_m = u (|m'| + |b1 m| + 2 |(1 - b1) g|) + tiny: the fma's rounding, b1 and 1 - b1 as fp32 numbers, the product (1 - b1) g;
      v: a_v = u (|v'| + |b2 v| + 3 |(1 - b2) g^2|) + tiny (two products);
      p: R = sqrt(v') / sqrt(bc2), D = R + eps, T = (lr / bc1) m' / D:
         e_D = R (a_v / v' + 3 u + e_bc2 / 2) + u eps + u D      (|sqrt(1 + d) - 1| <= |d|; sqrtf, sqrtf, the division; eps as fp32; the add)
         e_T = |T| (5 u + e_bc1 + e_D / (D - e_D)) + (lr / bc1) a_m / (D - e_D)    (lr, bc1, lr / bc1, the product, the division)
         a_p = u (2 |p1| + 3 lr wd |p|) + e_T + u |p'|
         with e_bc1, e_bc2 = bc_rel_error: THE EXPLICIT TERM of the bias corrections (u when they are taken in double on the host);
      pb: r = 2^-8, a = a_p.
    Elements 0..3 have g = 0 and v = 0 (the denominator is eps), 4..7 also carry a moment m != 0 (steps > 1), 8..11 a tiny v = 1e-30 with
    g = 1e-14 and p = 0 (so are all elements of a tensor shorter than 12).  Near misses: eps inside the square root; no bias correction (steps <= 2); the decay added to the gradient
    (Adam with L2, not AdamW; wd > 0)."""
    name = "adamw"
    exact = False
    BC_FP32 = False                                       # the library takes both corrections in double on the host
    LR, EPS = 1e-3, 1e-8

    @staticmethod
    def _one(n, step, seed):
        g_ = torch.Generator().manual_seed(seed)
        p = torch.randn(n, generator=g_); g = torch.randn(n, generator=g_) * 0.3
        if step == 1:
            m, v = torch.zeros(n), torch.zeros(n)
        else:
            m = torch.randn(n, generator=g_) * 0.1; v = (torch.randn(n, generator=g_) * 0.3) ** 2
        if n >= 12:
            g[:8] = 0; v[:8] = 0; m[:4] = 0
            g[8:12] = 1e-14; p[8:12] = 0
            if step > 1:
                v[8:12] = 1e-30; m[8:12] = 1e-15
        else:                                                # a tensor of a few elements: all of the tiny kind
            g[:] = 1e-14; p[:] = 0
            if step > 1:
                v[:] = 1e-30; m[:] = 1e-15
        return p, g, m, v

    @staticmethod
    def make(sizes, step, betas, wd, seed=18):
        parts = [AdamW._one(n, step, seed + 7 * i) for i, n in enumerate(sizes)]
        p, g, m, v = (torch.cat([q[j] for q in parts]) for j in range(4))
        return {"p": p, "g": g, "m": m, "v": v, "sizes": list(sizes), "step": step, "betas": betas, "wd": wd, "lr": AdamW.LR, "eps": AdamW.EPS}

    @staticmethod
    def ref(inp, dt, eps_inside=False, no_bc=False, l2=False):
        p, g, m, v = (inp[k].to(dt) for k in "pgmv")
        (b1, b2), t, lr, eps, wd = inp["betas"], inp["step"], inp["lr"], inp["eps"], inp["wd"]
        bc1, bc2 = (1.0, 1.0) if no_bc else (1 - b1 ** t, 1 - b2 ** t)
        if l2:
            g = g + wd * p; p1 = p
        else:
            p1 = p * (1 - lr * wd)
        if dt == torch.float32:                            # the stand-in: the kernel's fused multiply-add (one rounding), betas as fp32 numbers
            fma = lambda b, x, y: (float(torch.tensor(b, dtype=dt)) * x.double() + y.double()).to(dt)
            m1 = fma(b1, m, (1 - b1) * g)
            v1 = fma(b2, v, (1 - b2) * g * g)
        else:
            m1 = b1 * m + (1 - b1) * g
            v1 = b2 * v + (1 - b2) * g * g
        den = torch.sqrt(v1 / bc2 + eps) if eps_inside else torch.sqrt(v1) / math.sqrt(bc2) + eps
        p2 = p1 - (lr / bc1) * m1 / den
        return {"p": p2, "m": m1, "v": v1, "pb": p2}

    @staticmethod
    def bound_terms(inp, fp32_bc):
        """-> (a_m, a_v, a_p, the part of a_p that is the bc2 term)"""
        p, g, m, v = (inp[k].double() for k in "pgmv")
        (b1, b2), t, lr, eps, wd = inp["betas"], inp["step"], inp["lr"], inp["eps"], inp["wd"]
        r = AdamW.ref(inp, F64)
        tiny = 2.0 ** -126
        a_m = U * (r["m"].abs() + (b1 * m).abs() + 2 * ((1 - b1) * g).abs()) + tiny
        a_v = U * (r["v"].abs() + (b2 * v).abs() + 3 * ((1 - b2) * g * g).abs()) + tiny
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        e1, e2 = bc_rel_error(b1, t, fp32_bc), bc_rel_error(b2, t, fp32_bc)
        R = torch.sqrt(r["v"]) / math.sqrt(bc2); D = R + eps
        dv = torch.where(r["v"] > 0, a_v / r["v"].clamp_min(1e-300), torch.zeros_like(R)).clamp(max=1.0)
        e_D0 = R * (dv + 3 * U) + U * eps + U * D
        e_D = e_D0 + R * e2 / 2
        T = (lr / bc1) * r["m"] / D
        e_T = T.abs() * (5 * U + e1 + e_D / (D - e_D)) + (lr / bc1) * a_m / (D - e_D)
        p1 = p * (1 - lr * wd)
        a_p = U * (2 * p1.abs() + 3 * lr * wd * p.abs()) + e_T + U * r["p"].abs()
        return a_m, a_v, a_p, T.abs() * (R * e2 / 2) / (D - e_D)

    @staticmethod
    def bound(inp, ref):
        a_m, a_v, a_p, _ = AdamW.bound_terms(inp, AdamW.BC_FP32)
        return {"m": (0.0, a_m), "v": (0.0, a_v), "p": (0.0, a_p), "pb": (BF, a_p)}

    @staticmethod
    def misses(inp):
        out = [("eps inside the square root", AdamW.ref(inp, F64, eps_inside=True))]
        if inp["step"] <= 2:
            out.append(("no bias correction", AdamW.ref(inp, F64, no_bc=True)))
        if inp["wd"] > 0:
            out.append(("decay added to the gradient", AdamW.ref(inp, F64, l2=True)))
        return out


class Ema:
    """LitEma update s' = s - omd (s - p) on fp32 (rdm_op_ema, rdm_op_ema_multi): the difference, omd as an fp32 number, the product, the
    final subtraction: a = u (|s'| + 3 |omd (s - p)|).  Near misses: the sign of the step flipped; decay and 1 - decay swapped."""
    name = "ema"
    exact = False

    @staticmethod
    def make(sizes, omd, seed=19):
        g = torch.Generator().manual_seed(seed)
        n = sum(sizes)
        s = torch.randn(n, generator=g)
        return {"s": s, "p": s + 0.05 * torch.randn(n, generator=g), "sizes": list(sizes), "omd": omd}

    @staticmethod
    def ref(inp, dt, omd=None, sign=1.0):
        s, p = inp["s"].to(dt), inp["p"].to(dt)
        return {"out": s - sign * (inp["omd"] if omd is None else omd) * (s - p)}

    @staticmethod
    def bound(inp, ref):
        s, p = inp["s"].double(), inp["p"].double()
        return {"out": (0.0, U * (ref["out"].abs() + 3 * (inp["omd"] * (s - p)).abs()))}

    @staticmethod
    def misses(inp):
        return [("sign flipped", Ema.ref(inp, F64, sign=-1.0)), ("decay and 1 - decay swapped", Ema.ref(inp, F64, omd=1 - inp["omd"]))]


class QSample:
    """x_t = a[b] x0 + b[b] noise (rdm_op_q_sample), fp32 NCHW in; out fp32 NCHW and / or nhwc bf16 [B, H, W, cpad] whose channels >= C
    are exactly zero.  Two products and an add: a = 2 u (|a x0| + |b noise|) (r = 2^-8 for nhwc; the zero padding has bound 0).  Near
    misses: the coefficients of the next sample; the two coefficients swapped."""
    name = "q_sample"
    exact = False

    @staticmethod
    def make(B, C, H, W, cpad, nchw, seed=20):
        g = torch.Generator().manual_seed(seed)
        abar = 0.02 + 0.96 * torch.rand(B, generator=g)
        return {"x0": torch.randn(B, C, H, W, generator=g), "noise": torch.randn(B, C, H, W, generator=g), "a": abar.sqrt(), "b": (1 - abar).sqrt(),
                "cpad": cpad, "nchw": nchw}

    @staticmethod
    def _pack(inp, v):
        out = {}
        if inp["nchw"]:
            out["out"] = v
        if inp["cpad"]:
            B, C, H, W = v.shape
            z = torch.zeros(B, H, W, inp["cpad"], dtype=v.dtype)
            z[..., :C] = v.permute(0, 2, 3, 1)
            out["nhwc"] = z
        return out

    @staticmethod
    def ref(inp, dt, roll=0, swap=False):
        a, b = inp["a"].to(dt).roll(roll)[:, None, None, None], inp["b"].to(dt).roll(roll)[:, None, None, None]
        if swap:
            a, b = b, a
        return QSample._pack(inp, a * inp["x0"].to(dt) + b * inp["noise"].to(dt))

    @staticmethod
    def bound(inp, ref):
        a, b = inp["a"].double()[:, None, None, None], inp["b"].double()[:, None, None, None]
        t = QSample._pack(inp, 2 * U * ((a * inp["x0"].double()).abs() + (b * inp["noise"].double()).abs()))
        return {k: (BF if k == "nhwc" else 0.0, v) for k, v in t.items()}

    @staticmethod
    def misses(inp):
        return [("coefficients of the next sample", QSample.ref(inp, F64, roll=-1)), ("coefficients swapped", QSample.ref(inp, F64, swap=True))]


class MseLoss:
    """se[b] = mean_{c, h, w} (eps - target)^2 and deps = coef[b] (eps - target) (rdm_op_mse_loss): eps / deps bf16 NHWC with row pitch
    ldc >= C (the padding channels of eps hold garbage and are ignored, those of deps are exactly zero), target fp32 NCHW.  One block per
    sample: a lane walks ceil(HW / 256) pixels x C channels, then the 256-lane tree (8 levels), then the division: se: a = (ceil(HW / 256)
    C + 8 + 4) u se (all terms positive; + 4: the difference twice, the square, the division).  deps: r = 2^-8, a = 2 u |coef d|.
    Near misses: the mean taken over ldc channels (ldc > C); the last pixel missing from se; the coefficient of the next sample."""
    name = "mse_loss"
    exact = False

    @staticmethod
    def make(B, C, H, W, ldc, deps, seed=21):
        g = torch.Generator().manual_seed(seed)
        return {"eps": bfr(torch.randn(B, H, W, ldc, generator=g)), "target": torch.randn(B, C, H, W, generator=g),
                "coef": (0.5 + torch.rand(B, generator=g)) * 1e-2 if deps else None}

    @staticmethod
    def ref(inp, dt, div_ldc=False, drop_last=False, roll=0):
        B, C, H, W = inp["target"].shape
        ldc = inp["eps"].shape[3]
        d = inp["eps"].to(dt)[..., :C] - inp["target"].to(dt).permute(0, 2, 3, 1)
        sq = d * d
        if drop_last:
            sq = sq.clone(); sq[:, -1, -1] = 0
        out = {"se": sq.sum((1, 2, 3)) / ((ldc if div_ldc else C) * H * W)}
        if inp["coef"] is not None:
            z = torch.zeros(B, H, W, ldc, dtype=dt)
            z[..., :C] = inp["coef"].to(dt).roll(roll)[:, None, None, None] * d
            out["deps"] = z
        return out

    @staticmethod
    def bound(inp, ref):
        B, C, H, W = inp["target"].shape
        out = {"se": (0.0, (_cdiv(H * W, 256) * C + 12) * U * ref["se"].abs())}
        if "deps" in ref:
            out["deps"] = (BF, 2 * U * ref["deps"].abs())
        return out

    @staticmethod
    def misses(inp):
        m = [("last pixel missing from se", MseLoss.ref(inp, F64, drop_last=True))]
        if inp["eps"].shape[3] > inp["target"].shape[1]:
            m.append(("mean over ldc channels", MseLoss.ref(inp, F64, div_ldc=True)))
        if inp["coef"] is not None:
            m.append(("coefficient of the next sample", MseLoss.ref(inp, F64, roll=-1)))
        return m


class WhereRows:
    """out[b, :] = mask[b] ? a[b, :] : x[b, :] (rdm_op_where_rows), bitwise.  Near misses: the mask inverted; the mask of the next row."""
    name = "where_rows"
    exact = True

    @staticmethod
    def make(rows, n, seed=22):
        g = torch.Generator().manual_seed(seed)
        mask = torch.rand(rows, generator=g) < 0.5
        mask[0] = True
        if rows > 1:
            mask[1] = False
        return {"mask": mask, "a": torch.randn(rows, n, generator=g), "x": torch.randn(rows, n, generator=g)}

    @staticmethod
    def ref(inp, dt, mask=None):
        mk = inp["mask"] if mask is None else mask
        return {"out": torch.where(mk[:, None], inp["a"].to(dt), inp["x"].to(dt))}

    @staticmethod
    def misses(inp):
        return [("mask inverted", WhereRows.ref(inp, F64, ~inp["mask"])), ("mask of the next row", WhereRows.ref(inp, F64, inp["mask"].roll(-1)))]


class TimestepEmbedding:
    """ldm timestep_embedding (rdm_op_timestep_embedding): out bf16 [B, ld] = [cos(t f_j) | sin(t f_j) | zero tail], f_j = exp(-ln(1e4) j /
    half), against fp64 cos | sin.  The columns dim .. ld - 1 are the documented zero tail (bound 0: exactly zero); `guard` is the row after
    the last one, which the kernel must leave untouched (the test fills it with 7 beforehand).
    Device error: the exponent -9.2103 j / half is two fp32 operations on an fp32 constant (3 u of up to 9.21), expf adds 2 ulp: f_j is off
    by e_f = (3 x 9.21 + 4) u relative; the product t f_j one more u; cosf / sinf take that argument error (t f_j up to 999) at slope <= 1
    and add 2 ulp of a value <= 1: a = (e_f + u) t f_j + 4 u, r = 2^-8.  Near misses: sin | cos; the exponent over half - 1; t + 1."""
    name = "timestep_embedding"
    exact = False

    @staticmethod
    def make(B, dim, ld, seed=23):
        t = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(seed))
        t[0] = 0
        t[-1] = 999
        return {"t": t, "dim": dim, "ld": ld}

    @staticmethod
    def arg(inp, dt=F64, den=None, dt_=0):
        half = inp["dim"] // 2
        f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dt) / (half if den is None else den))
        return (inp["t"] + dt_).to(dt)[:, None] * f

    @staticmethod
    def ref(inp, dt, swap=False, den=None, dt_=0):
        a = TimestepEmbedding.arg(inp, dt, den, dt_)
        B, half = a.shape
        out = torch.zeros(B, inp["ld"], dtype=dt)
        out[:, :half], out[:, half:2 * half] = (torch.sin(a), torch.cos(a)) if swap else (torch.cos(a), torch.sin(a))
        return {"out": out, "guard": torch.full((inp["ld"],), 7.0, dtype=dt)}

    @staticmethod
    def bound(inp, ref):
        a = TimestepEmbedding.arg(inp)
        e = ((3 * 9.2104 + 4) * U + U) * a + 4 * U
        full = torch.zeros_like(ref["out"])
        full[:, :a.shape[1]] = e; full[:, a.shape[1]:2 * a.shape[1]] = e
        return {"out": (BF, full), "guard": (0.0, torch.zeros(()))}

    @staticmethod
    def misses(inp):
        half = inp["dim"] // 2
        m = [("sin | cos", TimestepEmbedding.ref(inp, F64, swap=True)), ("t + 1", TimestepEmbedding.ref(inp, F64, dt_=1))]
        if half > 1:
            m.append(("exponent over half - 1", TimestepEmbedding.ref(inp, F64, den=half - 1)))
        return m



# ============================================================================================================ the check itself
BF16_OUT = {"add", "sumpool2", "colsum_samples", "softmax", "softmax_bwd", "geglu", "conv3x3_dgrad", "attention_bwd", "small_attention_bwd",
            "transpose", "heads", "expand2"}


def _bf16_out(case, inp, k):
    return (case.name in BF16_OUT) or k in ("dx", "pb", "nhwc", "deps") or (case.name == "timestep_embedding" and k == "out") or (case.name == "silu" and not inp["grad"]) or (case.name == "bmm" and not inp["f32"])


def standin(case, inp, bf16_out=_bf16_out):
    """the fp32 torch restatement standing in for the kernel (CPU test): fp32 arithmetic, outputs rounded like the kernel's
    (bf16_out(case, inp, key): which outputs the kernel writes as bf16 -- the forward ops pass their own rule)"""
    out = case.ref(inp, torch.float32)
    res = {}
    for k, v in out.items():
        bf_out = bf16_out(case, inp, k)
        res[k] = bfr(v) if bf_out else v
    return res


def check(case, inp, out):
    """assert the outputs are within bound of the fp64 reference and outside it against every near miss; -> (worst ratio, smallest
    near-miss ratio) for the report"""
    ref = case.ref(inp, F64)
    assert set(out) == set(ref), (set(out), set(ref))
    # a near miss that coincides with the reference at this shape (rows reversed on one row) cannot be told apart by anything: skipped
    misses = [(l, m) for l, m in case.misses(inp) if any(not torch.equal(m[k].double(), ref[k].double()) for k in m)]
    assert misses, "every case has a near miss"
    if case.exact:
        for k in ref:
            assert out[k].shape == ref[k].shape, (k, out[k].shape, ref[k].shape)
            bad = (out[k].double() != ref[k]).sum().item()
            assert bad == 0, f"{case.name}.{k}: {bad} elements differ (bitwise equality expected)"
        margins = []
        for label, mref in misses:
            ndiff = sum(int((out[k].double() != mref[k]).sum()) for k in mref)
            assert ndiff > 0, f"{case.name}: near miss '{label}' is not told apart"
            margins.append(ndiff)
        return 0.0, min(margins)
    bnd = case.bound(inp, ref)
    worst = 0.0
    for k in ref:
        r, a = bnd[k]
        assert out[k].shape == ref[k].shape, (k, out[k].shape, ref[k].shape)
        assert torch.isfinite(out[k]).all(), f"{case.name}.{k}: non-finite output"
        q = ratio(out[k], ref[k], r * ref[k].abs() + a)
        assert q <= 1.0, f"{case.name}.{k}: worst error / bound = {q:.3g}"
        worst = max(worst, q)
    margin = math.inf
    for label, mref in misses:
        q = max(ratio(out[k], mref[k], bnd[k][0] * mref[k].abs() + bnd[k][1]) for k in mref)
        assert q > 1.0, f"{case.name}: near miss '{label}' is within bound (ratio {q:.3g})"
        margin = min(margin, q)
    return worst, margin


# ============================================================================================================ the parametrisations
# (case, shape kwargs, the launch path it reaches) -- shared by the GPU test and the CPU test; ids map every path to a test
CASES = [
    (Add, dict(n=13), "add: 8-wide vectors + a 5-element tail"),
    (Add, dict(n=4099), "add: tail of 3"),
    (Add, dict(n=8 * 300001), "add: no tail, many blocks"),
    (Silu, dict(n=1001, grad=False), "silu: bf16 forward"),
    (Silu, dict(n=1001, grad=True), "silu: fp32 gradient"),
    (Silu, dict(n=2_500_000, grad=True), "silu: grid-stride loop"),
    (Sumpool2, dict(B=2, H=4, W=4, C=8), "sumpool2: one vector per pixel"),
    (Sumpool2, dict(B=3, H=16, W=8, C=200), "sumpool2: 25 vectors"),
    (Colsum, dict(M=100, N=64), "colsum: one-stage (M < 256)"),
    (Colsum, dict(M=1000, N=36), "colsum: one-stage (N % 8 != 0)"),
    (Colsum, dict(M=1000, N=64), "colsum: two-stage, chunk clamped at 64"),
    (Colsum, dict(M=300_000, N=320), "colsum: two-stage, mid chunk"),
    (Colsum, dict(M=4_300_000, N=8), "colsum: two-stage, chunk clamped at 4096"),
    (ColsumSamples, dict(B=3, HW=48, N=64), "colsum_samples: HW < 64 path"),
    (ColsumSamples, dict(B=2, HW=60, N=20), "colsum_samples: N % 8 != 0 path"),
    (ColsumSamples, dict(B=4, HW=1024, N=320), "colsum_samples: two-stage"),
    (Transpose, dict(Z=0, rows=1, cols=1), "transpose: 1 x 1"),
    (Transpose, dict(Z=0, rows=33, cols=65), "transpose: partial tiles"),
    (Transpose, dict(Z=0, rows=70_000, cols=3), "transpose: > 65535 rows"),
    (Transpose, dict(Z=3, rows=33, cols=65), "transpose_batched: partial tiles"),
    (Transpose, dict(Z=2, rows=1, cols=100), "transpose_batched: one row"),
    (Heads, dict(B=2, n=5, H=3, D=32, ldx=96, mode=0), "heads mode 0"),
    (Heads, dict(B=2, n=7, H=2, D=40, ldx=96, mode=0), "heads mode 0: D = 40, ldx > H D"),
    (Heads, dict(B=1, n=9, H=1, D=64, ldx=64, mode=0), "heads mode 0: D = 64"),
    (Heads, dict(B=2, n=5, H=3, D=32, ldx=104, mode=1), "heads mode 1: ldx > H D"),
    (Heads, dict(B=1, n=70, H=2, D=1, ldx=2, mode=1), "heads mode 1: D = 1"),
    (Heads, dict(B=2, n=5, H=3, D=32, ldx=96, mode=2), "heads mode 2"),
    (Heads, dict(B=1, n=6, H=2, D=40, ldx=80, mode=2), "heads mode 2: D = 40"),
    (Expand2, dict(B=2, H=3, W=5, C=8, mode=0), "expand2 mode 0"),
    (Expand2, dict(B=1, H=16, W=16, C=64, mode=1), "expand2 mode 1"),
    (Bmm, dict(Z=3, M=100, N=70, K=128, alpha=1.0, f32=False), "bmm: bf16 out, ragged M / N"),
    (Bmm, dict(Z=2, M=257, N=130, K=192, alpha=0.5, f32=True), "bmm: fp32 out, alpha"),
    (Bmm, dict(Z=8, M=64, N=1024, K=128, alpha=0.25, f32=False), "bmm: wide N"),
    (Softmax, dict(rows=7, n=12, n_valid=5), "softmax: boundary inside a float4"),
    (Softmax, dict(rows=5, n=64, n_valid=0), "softmax: n_valid = 0 (all)"),
    (Softmax, dict(rows=3, n=64, n_valid=64), "softmax: n_valid = n"),
    (Softmax, dict(rows=6, n=64, n_valid=1), "softmax: n_valid = 1"),
    (Softmax, dict(rows=9, n=1000, n_valid=997), "softmax: n > 256 (a lane walks the row 4 times)"),
    (Softmax, dict(rows=40_000, n=8, n_valid=7), "softmax: rows > 32768 (grid-stride)"),
    (SoftmaxBwd, dict(rows=5, n=12), "softmax_bwd: short rows"),
    (SoftmaxBwd, dict(rows=9, n=1000), "softmax_bwd: n > 256"),
    (SoftmaxBwd, dict(rows=40_000, n=8), "softmax_bwd: grid-stride"),
    (Geglu, dict(M=1, F=8, bwd=False), "geglu forward: one vector"),
    (Geglu, dict(M=37, F=320, bwd=False), "geglu forward"),
    (Geglu, dict(M=37, F=320, bwd=True), "geglu backward"),
    (Geglu, dict(M=3, F=8, bwd=True), "geglu backward: one vector per row"),
    (LayerNormBwd, dict(M=64, C=100, res=True, offset=True), "layernorm_bwd: generic (C % 8 != 0), residual, offset rows"),
    (LayerNormBwd, dict(M=33, C=1280), "layernorm_bwd: generic (C > 1024)"),
    (LayerNormBwd, dict(M=16400, C=64, res=True), "layernorm_bwd: rows_per_block 64 (M >= 16384)"),
    (LayerNormBwd, dict(M=8, C=320, offset=True), "layernorm_bwd: vec NV=1, offset rows"),
    (LayerNormBwd, dict(M=40, C=512, res=True, offset=True, small_var=True), "layernorm_bwd: small variance (eps), offset rows"),
    (LayerNormBwd, dict(M=70, C=768, res=True, offset=True), "layernorm_bwd: vec NV=2, residual, offset rows"),
    (LayerNormBwd, dict(M=20, C=1280, offset=True, small_var=True), "layernorm_bwd: generic, small variance, offset rows"),
    (GroupNormBwd, dict(B=2, HW=64, C=2560, silu=1, res=True), "groupnorm_bwd: generic (C > 2048), SiLU, residual"),
    (GroupNormBwd, dict(B=2, HW=64, C=2560, silu=0, offset=True, small_var=True), "groupnorm_bwd: generic, small variance, offset groups"),
    (GroupNormBwd, dict(B=3, HW=16, C=320, silu=1), "groupnorm_bwd: vec, nchunk 1 (HW < 64)"),
    (GroupNormBwd, dict(B=1040, HW=4, C=64, silu=0, res=True), "groupnorm_bwd: vec, nchunk 1 (B > 1024)"),
    (GroupNormBwd, dict(B=2, HW=256, C=256, silu=1, res=True, offset=True, small_var=True), "groupnorm_bwd: vec, SiLU, small variance, offset groups"),
    (GroupNormBwd, dict(B=2, HW=1024, C=640, silu=0, offset=True), "groupnorm_bwd: vec, several chunks, offset groups"),
    (ConvDgrad, dict(B=4, H=8, W=8, C=256, N=512), "conv3x3_dgrad: 8x8 with K-split"),
    (ConvDgrad, dict(B=2, H=16, W=16, C=128, N=128), "conv3x3_dgrad: 16x16"),
    (ConvDgrad, dict(B=1, H=32, W=32, C=192, N=64), "conv3x3_dgrad: 32 wide"),
    (ConvDgrad, dict(B=1, H=8, W=64, C=128, N=128), "conv3x3_dgrad: 64 wide"),
    (ConvDgrad, dict(B=1, H=4, W=128, C=128, N=64), "conv3x3_dgrad: 128 wide (strips)"),
    (AttentionBwd, dict(B=2, n=96, m=64, H=3), "attention_bwd: n = 96 (partly idle 4-wave blocks)"),
    (AttentionBwd, dict(B=2, n=64, m=160, H=3), "attention_bwd: m = 160"),
    (AttentionBwd, dict(B=1, n=1024, m=32, H=2), "attention_bwd: n = 1024, m = 32"),
    (AttentionBwd, dict(B=1, n=32, m=1024, H=2), "attention_bwd: n = 32, m = 1024"),
    (SmallAttentionBwd, dict(B=2, nq=300, nkv=1, H=2), "small_attention_bwd: one key, two query blocks"),
    (SmallAttentionBwd, dict(B=1, nq=77, nkv=3, H=3), "small_attention_bwd: 3 keys"),
    (SmallAttentionBwd, dict(B=2, nq=64, nkv=5, H=2, pad_q=16, pad_kv=32, pad_o=8), "small_attention_bwd: 5 keys, row pitches > C"),
    (SmallAttentionBwd, dict(B=1, nq=260, nkv=32, H=1, pad_q=8, pad_kv=8, pad_o=24), "small_attention_bwd: 32 keys, pitches > C"),
    (AdamW, dict(sizes=(2049,), step=1, betas=(0.9, 0.999), wd=1e-2), "adamw: step 1, beta2 0.999 (the bc2 cancellation), 2049 elements"),
    (AdamW, dict(sizes=(2047,), step=2, betas=(0.9, 0.999), wd=0.0), "adamw: step 2, no decay, 2047 elements"),
    (AdamW, dict(sizes=(2048,), step=10000, betas=(0.9, 0.999), wd=1e-2), "adamw: step 10000, 2048 elements"),
    (AdamW, dict(sizes=(1,), step=1, betas=(0.9, 0.95), wd=1e-2), "adamw: one element, beta2 0.95"),
    (AdamW, dict(sizes=(2049,), step=2, betas=(0.9, 0.95), wd=0.0), "adamw: step 2, beta2 0.95, no decay"),
    (AdamW, dict(sizes=(5000,), step=10000, betas=(0.9, 0.95), wd=1e-2), "adamw: step 10000, beta2 0.95"),
    (AdamW, dict(sizes=(1, 2047, 2048, 2049) * 13, step=1, betas=(0.9, 0.999), wd=1e-2), "adamw_multi: 52 tensors (two launches), step 1"),
    (AdamW, dict(sizes=(2049, 1, 2048, 2047) * 13, step=2, betas=(0.9, 0.95), wd=0.0), "adamw_multi: 52 tensors, step 2, no decay"),
    (AdamW, dict(sizes=(1, 2047, 2048, 2049) * 13, step=10000, betas=(0.9, 0.999), wd=1e-2), "adamw_multi: 52 tensors, step 10000"),
    (Ema, dict(sizes=(1,), omd=1e-4), "ema: one element"),
    (Ema, dict(sizes=(2047,), omd=1e-4), "ema: 2047 elements"),
    (Ema, dict(sizes=(2048,), omd=0.1), "ema: 2048 elements"),
    (Ema, dict(sizes=(2049,), omd=1e-4), "ema: 2049 elements"),
    (Ema, dict(sizes=(1, 2047, 2048, 2049) * 13, omd=1e-4), "ema_multi: 52 tensors (two launches)"),
    (QSample, dict(B=3, C=3, H=15, W=17, cpad=8, nchw=True), "q_sample: both outputs, HW = 255, cpad 8 > C"),
    (QSample, dict(B=2, C=4, H=25, W=44, cpad=0, nchw=True), "q_sample: NCHW only, HW = 1100"),
    (QSample, dict(B=5, C=3, H=1, W=1, cpad=64, nchw=False), "q_sample: NHWC only, HW = 1, cpad 64"),
    (MseLoss, dict(B=3, C=3, H=1, W=1, ldc=8, deps=True), "mse_loss: HW = 1, ldc > C"),
    (MseLoss, dict(B=2, C=3, H=15, W=17, ldc=64, deps=True), "mse_loss: HW = 255, ldc 64"),
    (MseLoss, dict(B=3, C=4, H=25, W=44, ldc=4, deps=True), "mse_loss: HW = 1100, ldc = C"),
    (MseLoss, dict(B=2, C=3, H=25, W=44, ldc=8, deps=False), "mse_loss: without deps"),
    (WhereRows, dict(rows=1, n=1), "where_rows: one element"),
    (WhereRows, dict(rows=7, n=2049), "where_rows: 7 rows of 2049"),
    (WhereRows, dict(rows=300, n=77), "where_rows: 300 rows"),
    (TimestepEmbedding, dict(B=4, dim=192, ld=192), "timestep_embedding: ld = dim, t = 0 and 999"),
    (TimestepEmbedding, dict(B=5, dim=64, ld=72), "timestep_embedding: ld > dim (zero tail, guard row)"),
    (TimestepEmbedding, dict(B=2, dim=2, ld=8), "timestep_embedding: dim 2"),
]


def case_id(entry):
    case, kw, _ = entry
    def short(v):
        if isinstance(v, tuple) and len(v) > 4:
            return f"{len(v)}x{max(v)}"
        return "_".join(str(x) for x in v) if isinstance(v, tuple) else v
    return case.name + "-" + "-".join(f"{k}{short(v)}" for k, v in kw.items())
