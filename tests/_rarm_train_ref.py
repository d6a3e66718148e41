"""Float64 restatements, per-element bounds and near misses of the three kernels of the RARM training step -- the backward of the causal
d_head-64 attention (csrc/backward.hip: causal_bwd_*_kernel), the gradient of the mean token NLL (csrc/rarm.hip: rarm_nll_bwd_kernel) and
the gradient of the token embedding (embedding_grad_kernel) -- and TorchOps, a CPU stand-in for the `Context` methods that
rdm_amd.training_rarm calls.  Shared by tests/test_gpu_rarm_train.py (the HIP kernels through the C ABI) and tests/test_rarm_train_cpu.py
(fp32 torch restatements standing in for them).  Same CASE contract as tests/_train_ref.py: `make / ref / bound / misses / standin`, held
together by _train_ref.check()."""
import math

import torch

import _fwd_ref as R
import _rarm_seq_ref as S
from _train_ref import BF, F64, U, bfr

D64 = 64


# ============================================================================================================ causal attention backward
class CausalAttentionBwd:
    """causal_bwd_{prep,dkv,dq}_kernel.  Operands as CausalAttention.make plus dO and o = the forward output rounded to bf16.
    S = q k^T, P = softmax(scale S under the causal mask), dP = dO v^T, D = dO . o, dS = P (dP - D), dq = scale dS k, dk = scale dS^T q,
    dv = P^T dO.  Bounds: the formulas of _train_ref._AttnBase.bounds (fused kernel: P and dS rounded to bf16, b = 2^-8) with the
    contraction-length constants doubled for d = 64 -- e_P = P (b + 2^-22 (4 + scale |S|) + 128 u scale sum|q k| + n u),
    e_dP = 64 u sum|dO v|, e_D = 64 u sum|dO o|, e_dS = e_P |dP - D| + P (e_dP + e_D) + (b + 2 u) |dS|; dv: a = sum_q e_P |dO| + n u sum_q
    P |dO|, dk: a = scale (sum_q e_dS |q| + n u sum_q |dS q|), dq: a = scale (sum_k e_dS |k| + n u sum_k |dS k|), r = 2^-8.  Every term
    carries a factor P, which is EXACTLY zero on a masked entry: the mask admits no error.
    Near misses: the diagonal masked, one key ahead visible, no mask, the scale applied twice to dq / dk, the head order reversed, dk and
    dv swapped.  (At n = 1 the second and third coincide with the reference, and dq = dk = 0 makes the scale miss coincide too; check()
    drops those.)"""
    name = "causal_attention_d64_bwd"
    exact = False
    SCALE = S.CausalAttention.SCALE

    @staticmethod
    def make(B, n, H, seed=93):
        inp = dict(S.CausalAttention.make(B, n, H, seed=seed))
        g = torch.Generator().manual_seed(seed + 1000)
        inp["do"] = bfr(torch.randn(B, n, H * D64, generator=g))
        inp["o"] = bfr(S.CausalAttention.ref(inp, F64)["out"].float())
        return inp

    @staticmethod
    def _parts(inp, dt, diagonal=1):
        H = inp["H"]
        qh, kh, vh, doh, oh = (R._heads(inp[k].to(dt), H, D64) for k in ("q", "k", "v", "do", "o"))
        Sx = qh @ kh.transpose(-1, -2)
        s = Sx * CausalAttentionBwd.SCALE
        if diagonal is not None:
            s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(diagonal), float("-inf"))
        P = torch.nan_to_num(torch.softmax(s, -1))
        dP = doh @ vh.transpose(-1, -2)
        Dd = (doh * oh).sum(-1, keepdim=True)
        return qh, kh, vh, doh, oh, Sx, P, dP, Dd

    @staticmethod
    def ref(inp, dt, diagonal=1, scale2=1.0, reverse=False, swap=False, pb=False):
        """pb: P and dS rounded to bf16 before the products that consume them (the kernel's MFMA operands)"""
        qh, kh, vh, doh, oh, Sx, P, dP, Dd = CausalAttentionBwd._parts(inp, dt, diagonal)
        dS = P * (dP - Dd)
        if pb:
            P, dS = bfr(P.float()).to(dt), bfr(dS.float()).to(dt)
        sc = CausalAttentionBwd.SCALE * scale2
        out = {"dq": R._unheads(sc * (dS @ kh)), "dk": R._unheads(sc * (dS.transpose(-1, -2) @ qh)), "dv": R._unheads(P.transpose(-1, -2) @ doh)}
        if reverse:
            out = {k: R._unheads(R._heads(v, inp["H"], D64).flip(1)) for k, v in out.items()}
        if swap:
            out["dk"], out["dv"] = out["dv"], out["dk"]
        return out

    @staticmethod
    def bound(inp, ref):
        qh, kh, vh, doh, oh, Sx, P, dP, Dd = CausalAttentionBwd._parts(inp, F64)
        n, scale, b = qh.shape[2], CausalAttentionBwd.SCALE, BF
        dS = P * (dP - Dd)
        e_P = P * (b + 2.0 ** -22 * (4 + scale * Sx.abs()) + 2 * D64 * U * scale * (qh.abs() @ kh.abs().transpose(-1, -2)) + n * U)
        e_dP = D64 * U * (doh.abs() @ vh.abs().transpose(-1, -2))
        e_D = D64 * U * (doh * oh).abs().sum(-1, keepdim=True)
        e_dS = e_P * (dP - Dd).abs() + P * (e_dP + e_D) + (b + 2 * U) * dS.abs()
        a_dv = e_P.transpose(-1, -2) @ doh.abs() + n * U * (P.transpose(-1, -2) @ doh.abs())
        a_dk = scale * (e_dS.transpose(-1, -2) @ qh.abs() + n * U * (dS.abs().transpose(-1, -2) @ qh.abs()))
        a_dq = scale * (e_dS @ kh.abs() + n * U * (dS.abs() @ kh.abs()))
        return {"dq": (BF, R._unheads(a_dq)), "dk": (BF, R._unheads(a_dk)), "dv": (BF, R._unheads(a_dv))}

    @staticmethod
    def misses(inp):
        f = CausalAttentionBwd.ref
        return [("diagonal masked", f(inp, F64, diagonal=0)), ("one key ahead visible", f(inp, F64, diagonal=2)), ("no mask", f(inp, F64, diagonal=None)),
                ("scale applied twice to dq / dk", f(inp, F64, scale2=CausalAttentionBwd.SCALE)), ("heads reversed", f(inp, F64, reverse=True)),
                ("dk and dv swapped", f(inp, F64, swap=True))]

    @staticmethod
    def standin(inp):
        """fp32 arithmetic, P and dS rounded to bf16, the outputs rounded to bf16"""
        return {k: bfr(v) for k, v in CausalAttentionBwd.ref(inp, torch.float32, pb=True).items()}


# ============================================================================================================ gradient of the mean NLL
class NllBwd:
    """rarm_nll_bwd_kernel: dlogits = gscale (softmax(row) - onehot(target)), fp32 arithmetic, one rounding to bf16 (r = 2^-8); rows as
    Nll.make (N(0, s) for s in {1, 3, 12}, the dominated row 3, the constant row 4), gscale = 1 / rows.
    Absolute part, from the error of an fp32 softmax p^ = fl(exp(fl(x - m))) fl(1 / s^), u = 2^-24:
      * the exponent x - m is rounded once: a relative error |x - m| u of the exponential; expf itself is good to 2 ulp = 4 u;
      * s^ sums terms that each carry that error, E = sum_j p_j (|x_j - m| + 4) u relative to s, and adds c = V / 1024 + 12 roundings in its
        longest chain (a thread's float4 partial sums, their pairwise adds, the 6-step butterfly, the two adds of the wave sums);
      * the reciprocal, the product, the subtraction of the one-hot and the product with gscale: 4 roundings of values no larger than
        p + onehot.
    a = |gscale| u (p (|x - m| + 4 + E / u + c) + 4 (p + onehot)) + 2^-125: the last term is fp32's smallest normal number, twice (a
    product that leaves the normal range may be flushed to zero).
    Near misses: the one-hot at target + 1; gscale applied twice; the one-hot left out."""
    name = "rarm_nll_bwd"
    exact = False

    @staticmethod
    def make(rows, V, seed=97):
        inp = dict(S.Nll.make(rows, V, seed=seed))
        inp["gscale"] = 1.0 / rows
        return inp

    @staticmethod
    def ref(inp, dt, shift=0, gscale2=1.0, onehot=True):
        lg = inp["logits"].to(dt)
        p = torch.softmax(lg, -1)
        if onehot:
            tg = (inp["targets"] + shift) % lg.shape[1]
            p = p - torch.nn.functional.one_hot(tg, lg.shape[1]).to(dt)
        return {"dlogits": p * (inp["gscale"] * gscale2)}

    @staticmethod
    def bound(inp, ref):
        lg = inp["logits"].double()
        V = lg.shape[1]
        xm = (lg - lg.max(-1, keepdim=True).values).abs()
        p = torch.softmax(lg, -1)
        oh = torch.nn.functional.one_hot(inp["targets"], V).double()
        E = (p * (xm + 4)).sum(-1, keepdim=True)
        c = V / 1024 + 12
        return {"dlogits": (BF, abs(inp["gscale"]) * U * (p * (xm + 4 + E + c) + 4 * (p + oh)) + 2.0 ** -125)}

    @staticmethod
    def misses(inp):
        return [("one-hot at target + 1", NllBwd.ref(inp, F64, shift=1)), ("gscale applied twice", NllBwd.ref(inp, F64, gscale2=inp["gscale"])),
                ("one-hot left out", NllBwd.ref(inp, F64, onehot=False))]

    @staticmethod
    def standin(inp):
        return {"dlogits": bfr(NllBwd.ref(inp, torch.float32)["dlogits"])}


NLL_BWD_SHAPES = S.NLL_SHAPES + [(64, 1002)]       # V = 1002: odd rows start 8 bytes off a 16-byte boundary


# ============================================================================================================ gradient of the embedding
class EmbeddingGrad:
    """embedding_grad_kernel: dw[v] = sum of dy[m] over tokens[m] == v, fp32, rows of unused ids zero.  Tokens: random ids, `dup` copies of
    the last id (V - 1: the sos id of the model) spread over the sequence.  Bound per element (fp32 output, r = 0): count(v) u sum |dy| over
    the rows of v -- count - 1 dependent fp32 additions; an unused row admits nothing but zero.  Near misses: the ids shifted by one;
    duplicates counted once (the first occurrence only)."""
    name = "embedding_grad"
    exact = False

    @staticmethod
    def make(M, V, C, dup, seed=99):
        g = torch.Generator().manual_seed(seed)
        tok = torch.randint(0, V - 1, (M,), generator=g)
        tok[torch.randperm(M, generator=g)[:dup]] = V - 1
        return {"tokens": tok, "dy": bfr(torch.randn(M, C, generator=g)), "V": V}

    @staticmethod
    def ref(inp, dt, shift=0, once=False):
        tok, dy = (inp["tokens"] + shift) % inp["V"], inp["dy"].to(dt)
        if once:
            first = torch.zeros(inp["V"], dtype=torch.bool)
            keep = torch.zeros(tok.shape[0], dtype=torch.bool)
            for m, t in enumerate(tok.tolist()):
                keep[m] = not first[t]
                first[t] = True
            tok, dy = tok[keep], dy[keep]
        return {"dw": torch.zeros((inp["V"], dy.shape[1]), dtype=dt).index_add_(0, tok, dy)}

    @staticmethod
    def bound(inp, ref):
        V = inp["V"]
        cnt = torch.zeros(V, dtype=F64).index_add_(0, inp["tokens"], torch.ones(inp["tokens"].shape[0], dtype=F64))
        sa = torch.zeros((V, inp["dy"].shape[1]), dtype=F64).index_add_(0, inp["tokens"], inp["dy"].double().abs())
        return {"dw": (0.0, cnt[:, None] * U * sa)}

    @staticmethod
    def misses(inp):
        return [("ids shifted by one", EmbeddingGrad.ref(inp, F64, shift=1)), ("duplicates counted once", EmbeddingGrad.ref(inp, F64, once=True))]

    @staticmethod
    def standin(inp):
        return EmbeddingGrad.ref(inp, torch.float32)


# (M, V, C, dup): the tiny model's b t with the sos id three times, most rows unused | the shipped table and width, one id 64 times
EMBED_SHAPES = [(36, 1002, 128, 3), (512, 16386, 768, 64)]


# ============================================================================================================ the Context stand-in
def _b(t):
    return t.to(torch.bfloat16)


class TorchOps:
    """CPU stand-in for the `_lib.Context` methods rdm_amd.training / training_rarm call on the RARM path: fp32 torch arithmetic on the same
    operands, every output the kernels write as bf16 rounded to bf16."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def _check_ids(self, what, ids, n, name):
        assert int(ids.min()) >= 0 and int(ids.max()) < n, (what, name)

    def op_layernorm(self, x, gamma, beta, eps=1e-5):
        return _b(torch.nn.functional.layer_norm(x.float(), x.shape[-1:], gamma, beta, eps))

    def op_layernorm_bwd(self, x, dy, gamma, eps=1e-5, residual=None):
        xf, d = x.float(), dy.float()
        mu = xf.mean(-1, keepdim=True); rstd = (xf.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
        xh = (xf - mu) * rstd
        dxh = d * gamma
        dx = rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))
        if residual is not None:
            dx = dx + residual.float().reshape(dx.shape)
        return _b(dx), (d * xh).sum(0), d.sum(0)

    def op_linear(self, a, w, bias=None, residual=None, act=0, alpha=1.0, out_f32=False):
        assert act == 0 and a.shape[1] % 64 == 0, "the GEMM's contraction length is a multiple of 64"
        y = alpha * (a.float() @ w.float().t())
        if bias is not None:
            y = y + bias
        if residual is not None:
            y = y + residual.float().reshape(y.shape)
        return y if out_f32 else _b(y)

    def op_transpose(self, x):
        return x.t().contiguous()

    def op_transpose_batched(self, x):
        return x.transpose(1, 2).contiguous()

    def op_linear_wgrad(self, dy, a):
        return dy.float().t() @ a.float()

    def op_colsum(self, x):
        return x.float().sum(0)

    def op_geglu(self, pre, dh=None):
        F = pre.shape[1] // 2
        a, g = pre[:, :F].float(), pre[:, F:].float()
        phi = 0.5 * (1 + torch.erf(g / math.sqrt(2.0)))
        if dh is None:
            return _b(a * g * phi)
        d = dh.float()
        return _b(torch.cat([d * g * phi, d * a * (phi + g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi))], 1))

    def op_heads(self, x, H, D, mode, n=None):
        assert D == 64
        if mode == 2:
            return R._unheads(x.reshape(-1, H, x.shape[1], 64)).contiguous()
        h = R._heads(x, H, D).reshape(-1, x.shape[1], D)
        return h.contiguous() if mode == 0 else h.transpose(1, 2).contiguous()

    def op_bmm(self, a, w, alpha=1.0, out_f32=False):
        assert a.shape[2] % 64 == 0, "the GEMM's contraction length is a multiple of 64"
        y = alpha * (a.float() @ w.float().transpose(1, 2))
        return y if out_f32 else _b(y)

    def op_softmax(self, s, n_valid=0):
        nv = n_valid or s.shape[-1]
        p = torch.zeros_like(s)
        p[..., :nv] = torch.softmax(s[..., :nv], -1)
        return _b(p)

    def op_softmax_bwd(self, p, dp):
        pf = p.float()
        return _b(pf * (dp - (pf * dp).sum(-1, keepdim=True)))

    def op_causal_attention_d64(self, qkv, heads, scale, kcache=None, vcache=None):
        self.calls.append("op_causal_attention_d64")
        C = heads * 64
        inp = {"q": qkv[..., :C].float(), "k": qkv[..., C:2 * C].float(), "v": qkv[..., 2 * C:].float(), "H": heads}
        return _b(S.CausalAttention.ref(inp, torch.float32, scale=scale, pb=True)["out"])

    def op_causal_attention_d64_bwd(self, qkv, out, dout, heads, scale):
        self.calls.append("op_causal_attention_d64_bwd")
        assert abs(scale - CausalAttentionBwd.SCALE) < 1e-9
        C = heads * 64
        inp = {"q": qkv[..., :C].float(), "k": qkv[..., C:2 * C].float(), "v": qkv[..., 2 * C:].float(), "H": heads, "do": dout.float(), "o": out.float()}
        g = CausalAttentionBwd.ref(inp, torch.float32, pb=True)
        return _b(torch.cat([g["dq"], g["dk"], g["dv"]], -1))

    def op_rarm_nll_bwd(self, logits, targets, gscale, want_nll=False, out=None, nll_out=None):
        self.calls.append("op_rarm_nll_bwd")
        assert logits.dtype == torch.float32 and logits.shape[0] <= 2048
        dl = _b(NllBwd.ref({"logits": logits, "targets": targets, "gscale": gscale}, torch.float32)["dlogits"])
        nll = S.Nll.ref({"logits": logits, "targets": targets}, torch.float32)["nll"]
        if out is not None:
            out.copy_(dl); dl = out
        if nll_out is not None:
            nll_out.copy_(nll); nll = nll_out
        return (dl, nll) if (want_nll or nll_out is not None) else dl

    def op_embedding_grad(self, tokens, dy, V, out=None):
        self.calls.append("op_embedding_grad")
        return EmbeddingGrad.ref({"tokens": tokens.reshape(-1), "dy": dy.float(), "V": V}, torch.float32)["dw"]

    def op_adamw_multi(self, ps, gs, ms, vs, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, p_bf16s=None):
        """torch.optim.AdamW's update (decoupled decay, bias correction), in place"""
        b1, b2 = betas
        for i, (p, g, m, v) in enumerate(zip(ps, gs, ms, vs)):
            p.mul_(1 - lr * weight_decay)
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            p.addcdiv_(m / (1 - b1 ** step), (v / (1 - b2 ** step)).sqrt() + eps, value=-lr)
            if p_bf16s is not None and p_bf16s[i] is not None:
                p_bf16s[i].copy_(p)


# ============================================================================================================ whole-model references
def tiny_problem(b=3, t=12, k=4, seed=7, round_weights=True):
    """the tiny RARM spec with synthetic weights, tokens (sos first), targets and bf16-rounded neighbours.
    round_weights=True (the gradient comparisons): the weights hold exact bf16 values, so the kernels and the fp64 reference read the same
    numbers.  round_weights=False (the optimisation curves): fp32 weights, as the masters of a training run are.  From bf16-EXACT masters
    the first AdamW steps of size lr = 1e-4 are below half a bf16 ulp of every weight above 2^-5, and round-to-nearest hands the kernels
    the unchanged start value until the master has drifted far enough; that stalls the curve for a step (measured with fp32 torch autograd
    reading bf16-rounded weights: 7.710, 7.473, 6.915 against 7.710, 7.174, 6.654 unrounded) and is a property of such a start point, not
    of the step under test."""
    from oracle import rarm as orarm
    from oracle import unet as ounet
    spec = orarm.tiny_rarm_spec()
    rw = bfr if round_weights else (lambda v: v)
    sd = {k_: rw(torch.as_tensor(v).float()) for k_, v in ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=4321).items()}
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, spec.vocab_out, (b, t), generator=g)
    tokens = torch.cat([torch.full((b, 1), spec.vocab_in - 1), codes[:, :-1]], 1)
    context = bfr(torch.randn(b, k, spec.context_dim, generator=g) * 0.45)
    return spec, sd, tokens, codes, context


def autograd_loss_and_grads(sd, spec, tokens, targets, context, dt):
    """oracle.rarm.rarm_forward under torch autograd in dtype dt -> (loss, {name: gradient in the state dict's layout})"""
    from oracle import rarm as orarm
    with torch.enable_grad():
        p = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in sd.items()}
        logits = orarm.rarm_forward(p, spec, tokens, context.to(dt))
        loss = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), targets.reshape(-1))
        loss.backward()
    return float(loss.detach()), {k: v.grad.detach() for k, v in p.items()}


def torch_adamw_losses(sd, spec, tokens, targets, context, steps, lr):
    """the reference optimisation: fp32 autograd through oracle.rarm.rarm_forward + torch.optim.AdamW(betas=(0.9, 0.95)) over all
    parameters -> ([loss before each step], loss after the last step)"""
    from oracle import rarm as orarm
    with torch.enable_grad():
        p = {k: v.detach().float().clone().requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.AdamW(list(p.values()), lr=lr, betas=(0.9, 0.95))
        f = lambda: torch.nn.functional.cross_entropy(orarm.rarm_forward(p, spec, tokens, context.float()).reshape(-1, spec.vocab_out), targets.reshape(-1))
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            loss = f()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        with torch.no_grad():
            final = float(f())
    return losses, final, {k: v.detach() for k, v in p.items()}
