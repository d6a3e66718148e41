"""The RARM transformer stage by stage, TEACHER-FORCED, in both passes: every tensor rdm_debug_tap shows of csrc/rarm_exec.hip (blocks
4000 rarm_prepare, 4100 the decode step rarm_step, 4200 the whole-sequence pass rarm_seq_body: include/rdm_hip.h) is compared with a
float64 restatement of ITS stage on the tapped tensors in front of it, element by element, under the bound the project already states for
the kernel that runs the stage -- no tolerance of its own:
  skinny / mid-size GEMMs of the decode step      _decode_ref.LinearRows, in the form rdm_linear_rows_select reports for the shape
  K/V-cache and neighbour attention of the step    _decode_ref.DecodeAttention (the cache REBUILT from the tapped q|k|v of the earlier
                                                   positions of the same layer -- of either pass)
  the one-launch cross-attention and its norm3     _decode_ref.XattnDecode, on the G / UT that rarm_prepare built
  token + positional embedding                     _decode_ref.Embed (bitwise)
  GEMMs of the whole-sequence pass, ctxkv, G, UT   _fwd_ref.Linear;   LayerNorm passes   _fwd_ref.LayerNorm
  neighbour attention of the whole-sequence pass   _fwd_ref.SmallAttention;   causal attention   _rarm_seq_ref.CausalAttention
  casts, expand_heads (its 1 / 8 is exact), the transpose, the zero rows of ctxkv: bitwise (folded into the operands where untapped).
On top of each class's own near misses every stage carries WIRING near misses -- the same stage restated on the operands a wiring error
would hand it (the neighbouring layer's weights, the bias left off, the residual of the block's input, layer l +- 1's slice of ctxkv / G /
UT, the conditional half's neighbours under the unconditional half) -- and the tapped tensor must fall OUTSIDE the bound against each.

One walk per executor (`walk_prepare`, `walk_step`, `walk_seq`) states the wiring once; a visitor decides what a stage does with it:
`Checker` compares the library's taps (tests/test_gpu_rarm_stages.py), `Standin` computes the stage in fp32 with bf16 storage and so
produces a tap dictionary without a GPU -- optionally with ONE wiring error planted (tests/test_rarm_stages_cpu.py).
A tap dictionary is {(block, sub): tensor}: block 4100 [steps, rows, width], the others [rows, width] ([B, 128, C] for G / UT)."""
import math

import torch

import _decode_ref as DR
import _fwd_ref as R
from _rarm_seq_ref import CausalAttention
from _train_ref import F64, bfr, check, ratio, row_offsets
from oracle import rarm as orarm, unet as ounet

PREPARE, STEP, SEQ = 4000, 4100, 4200
BF16, F32 = torch.bfloat16, torch.float32
NP = 128
XGEMM_FROM = 384                       # sequences from which the decode step's cross-attention runs as GEMMs (outside deterministic mode)
_STAGES = {1: "norm1", 2: "q|k|v", 3: "self-attention heads", 4: "x + attn1.to_out", 5: "norm2", 6: "attn2.to_q", 7: "cross-attention heads",
           8: "x + attn2", 9: "norm3", 10: "GEGLU hidden", 11: "x + ff.net.2"}
_OWN = {PREPARE: {1: "context cast", 2: "ctxkv"}, STEP: {1: "embedding", 2: "final x cast", 3: "logits"}, SEQ: {1: "embedding", 2: "final x cast", 3: "logits"}}


def stage_name(key):
    block, sub = key
    who = {PREPARE: "prepare", STEP: "step", SEQ: "seq"}[block]
    layer, stage = divmod(sub, 16)
    if layer == 0:
        return f"{who} {_OWN[block][stage]}"
    return f"{who} block {layer - 1} " + ({1: "G", 2: "UT"}[stage] if block == PREPARE else _STAGES[stage])


def one_launch(spec, k, B2, det):
    """does the decode step take the one-launch cross-attention (rarm_prepare's rule)"""
    C = spec.inner_dim
    return spec.n_heads * k <= NP and C <= 1024 and C % 64 == 0 and (det or B2 < XGEMM_FROM)


def select(M, N, K, act=R.ACT_NONE, ln=False, det=False):
    """the launch form of a one-row-per-sequence projection, as the library's own dispatch reports it (host only)"""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    return _lib.linear_rows_select(M, N, K, act, ln, det)


def step_stages(spec, B2, k, det):
    """the block stages a decode step of B2 rows holds in memory: {stage: (width, dtype)}"""
    C = spec.inner_dim
    fused = one_launch(spec, k, B2, det)
    st = {2: (3 * C, BF16), 3: (C, BF16), 4: (C, F32), 8: (C, F32), 10: (4 * C, BF16), 11: (C, F32)}
    if select(B2, 3 * C, C, ln=True, det=det)[0] == "refused":
        st[1] = (C, BF16)
    if fused:
        st[9] = (C, BF16)
    else:
        st.update({6: (C, BF16), 7: (C, BF16)})
        if select(B2, C, C, ln=True, det=det)[0] == "refused":
            st[5] = (C, BF16)
        if select(B2, 8 * C, C, act=R.ACT_GEGLU, ln=True, det=det)[0] == "refused":
            st[9] = (C, BF16)
    return dict(sorted(st.items()))


def tap_shapes(spec, block, B, B2, k, steps=None, t=None, det=False, head=True, decode=True):
    """{(block, sub): (shape, dtype)} of every stage an executor shows, in execution order (decode: the entry runs decode steps, so
    rarm_prepare builds G / UT where they take the one-launch form; head: the call computes logits)"""
    C, V, depth = spec.inner_dim, spec.vocab_out, spec.depth
    out = {}
    if block == PREPARE:
        out[(PREPARE, 1)] = ((B * k, spec.context_dim), BF16)
        out[(PREPARE, 2)] = ((B2 * k, depth * 2 * C), BF16)
        if decode and one_launch(spec, k, B2, det):
            for l in range(depth):
                out[(PREPARE, 16 * (l + 1) + 1)] = ((B, NP, C), BF16)
                out[(PREPARE, 16 * (l + 1) + 2)] = ((B, NP, C), BF16)
        return out
    lead = (steps, B2) if block == STEP else (B2 * t,)
    blockst = step_stages(spec, B2, k, det) if block == STEP else {s: (C * {2: 3, 10: 4}.get(s, 1), F32 if s in (4, 8, 11) else BF16) for s in range(1, 12)}
    out[(block, 1)] = (lead + (C,), F32)
    for l in range(depth):
        for s, (w, dt) in blockst.items():
            out[(block, 16 * (l + 1) + s)] = (lead + (w,), dt)
    if head:
        out[(block, 2)] = (lead + (C,), BF16)
        out[(block, 3)] = (lead + (V,), F32)
    return out


# ============================================================================================================ weights
def synth_weights(spec, seed):
    """The seeded ounet.synth_state_dict of the spec, with two tensors re-spread so that every near miss of the stage classes can be told
    apart on the model's OWN activations, as the classes' make() arrange for their random operands:
      * the token embedding's rows get a spread and a mean each: even ids 0.5 x [0.75, 1.25) around +[0.5, 1.5], odd ids 1.5 x [0.75, 1.25)
        around -[0.5, 1.5] -- _decode_ref.XattnDecode.make's rows -- and `tokens()` alternates the parity from one sequence to the next
        (as drawn, every row has mean 0 and the same spread to 2.5 %: LayerNorm statistics of the neighbouring row would pass every bound);
      * the gate half of ff.net.0.proj is three times as large (gates of a few units: erf and tanh GELU differ by more than the hidden
        tensor's bf16 rounding only there)."""
    sd = ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=seed)
    C = spec.inner_dim
    g = torch.Generator().manual_seed(seed + 1)
    odd = (torch.arange(spec.vocab_in) % 2).float()[:, None]
    spread = (0.5 + odd) * (0.75 + 0.5 * torch.rand(spec.vocab_in, 1, generator=g))
    sd["proj_in.weight"] = sd["proj_in.weight"] * math.sqrt(C) * spread + row_offsets(spec.vocab_in, seed + 2, 0.5, 1.5).abs()[:, None] * (1 - 2 * odd)
    for i in range(spec.depth):
        sd[f"transformer_blocks.{i}.ff.net.0.proj.weight"][4 * C:] *= 3.0
    return sd


class Net:
    """the state dict as the executor holds it: matrices rounded to bf16, vectors and the two embedding tables fp32"""

    def __init__(self, sd, spec):
        self.spec = spec
        self.C, self.H, self.depth, self.L, self.V = spec.inner_dim, spec.n_heads, spec.depth, spec.sequence_length, spec.vocab_out
        self.emb = sd["proj_in.weight"].float()
        self.pos = sd["positional_encoding"].float().t().contiguous()
        self.wpo, self.bpo = bfr(sd["proj_out.weight"][:, :, 0].float()), sd["proj_out.bias"].float()
        self.layers = []
        for i in range(spec.depth):
            p = f"transformer_blocks.{i}."
            w, v = (lambda n: bfr(sd[p + n].float())), (lambda n: sd[p + n].float())
            self.layers.append({
                "ln1": (v("norm1.weight"), v("norm1.bias")), "ln2": (v("norm2.weight"), v("norm2.bias")), "ln3": (v("norm3.weight"), v("norm3.bias")),
                "wqkv": torch.cat([w("attn1.to_q.weight"), w("attn1.to_k.weight"), w("attn1.to_v.weight")]),
                "wo1": w("attn1.to_out.0.weight"), "bo1": v("attn1.to_out.0.bias"), "wq2": w("attn2.to_q.weight"),
                "wkv2": torch.cat([w("attn2.to_k.weight"), w("attn2.to_v.weight")]), "wo2": w("attn2.to_out.0.weight"), "bo2": v("attn2.to_out.0.bias"),
                "wff1": w("ff.net.0.proj.weight"), "bff1": v("ff.net.0.proj.bias"), "wff2": w("ff.net.2.weight"), "bff2": v("ff.net.2.bias")})
        assert spec.depth >= 2, "layers must differ: the wiring near misses read the neighbouring layer"

    def near(self, l):
        """the neighbouring layer a wiring error would read"""
        return l + 1 if l + 1 < self.depth else l - 1

    def kvw(self, shift=0):
        """rows of the all-layer neighbour projection; shift: every layer's slice holding the weights of layer l + shift"""
        return torch.cat([self.layers[(l + shift) % self.depth]["wkv2"] for l in range(self.depth)])


def tokens(spec, b, t, g):
    """[b, t] token ids: sequence s holds ids of the parity of s (synth_weights: neighbouring sequences differ in spread and mean)"""
    return 2 * torch.randint(0, spec.vocab_out // 2, (b, t), generator=g) + (torch.arange(b) % 2)[:, None]


class _GegluLinear(R.Linear):
    """_fwd_ref.Linear for the whole-sequence pass's GEGLU projection.  Its near miss "tanh GELU" differs from the erf form by at most
    4.7e-4 |value|, while the class's bound carries 1.13 (K + 8) u S |value| for the gate's accumulation error, S the gate's sum of
    absolute products: at K = 768 on a LayerNorm output that term alone is 8e-4 |value| and more, so the bound admits the near miss
    itself as a correct answer and no output can be told from it.  The near miss is kept wherever the bound does tell it from the fp64
    reference (the tiny spec, K = 128: margin 5) and dropped where it lies within the bound of the reference at every element."""

    @staticmethod
    def misses(inp):
        ref = R.Linear.ref(inp, F64)
        r, a = R.Linear.bound(inp, ref)["out"]
        told = lambda m: ratio(m["out"], ref["out"], r * ref["out"].abs() + a) > 1.0
        return [(l, m) for l, m in R.Linear.misses(inp) if l != "tanh GELU" or told(m)]


# ============================================================================================================ stage operands
def _lin(a, w, b=None, act=R.ACT_NONE, f32=False, res=None):
    return {"a": a.float(), "w": w, "b": b, "act": act, "f32": f32, "alpha": 1.0, "rows": None, "mgemm": False, "res": res, "res_f32": res is not None}


def _ln(x, gb):
    return {"x": x.float(), "f32": True, "gamma": gb[0], "beta": gb[1], "eps": 1e-5, "small_var": False, "out_f32": False}


def _rows(form, w, b=None, a=None, x=None, gb=None, act=R.ACT_NONE, res=None, f32=False, det=False):
    """a _decode_ref.LinearRows case on given operands: a (bf16 rows) or LayerNorm(x; gb) formed in the kernel; res: the fp32 residual
    stream the output is added to in place.  The rows of the output buffers beyond M hold a fill the kernel must leave."""
    M = (a if a is not None else x).shape[0]
    No = w.shape[0] // 2 if act == R.ACT_GEGLU else w.shape[0]
    inp = {"M": M, "form": tuple(form), "act": act, "ln": x is not None, "det": det, "outs": "f32" if f32 else "bf16", "eps": 1e-5, "w": w, "b": b,
           "res": res is not None, "buf16": torch.full((M + DR.PAD, No), 5.5)}
    if x is not None:
        inp["x"], inp["gamma"], inp["beta"] = x.float(), gb[0], gb[1]
    else:
        inp["a"] = a.float()
    inp["buf32"] = torch.full((M + DR.PAD, No), -7.25)
    if res is not None:
        inp["buf32"][:M] = res.float()
    return inp


def _self_attn(qkv, K, V, pos):
    return DR.DecodeAttention.from_state(qkv.float(), K, V, pos)


def _cross_attn(q, kv, C, H, l, other, batch=None):
    """the decode step's neighbour attention as _decode_ref.DecodeAttention reads it: a [B, k + 1, 4 C] buffer whose column blocks 2, 3
    are this layer's K | V and 0, 1 another layer's; row k of a sequence is what follows its rows in memory: the next sequence's first"""
    B, k = kv.shape[:2]
    blk = lambda j: kv[:, :, 2 * j * C:2 * (j + 1) * C]
    buf = torch.cat([blk(other), blk(l)], 2).float()
    buf = torch.cat([buf, buf[:, :1].roll(-1, 0)], 1)
    return {"mode": "cross", "B": B, "H": H, "scale": DR.D ** -0.5, "fewkey": (batch or B) >= 128 and k <= 8, "q": q.float(), "n": k, "cap": k + 1, "ld": 4 * C,
            "ordinary": [buf], "caches": [buf]}


def _attn(q, k, v, H, causal):
    return {"q": q.float(), "k": k.float(), "v": v.float(), "H": H, "D": 64, "causal": causal, "scale": 64 ** -0.5, "fused": False}


def expand_heads(kv, H, scale):
    """misc.hip expand_heads_kernel: [B, k, C] -> [B, 128, C], row h k + j = neighbour j's columns of head h (times scale), zero elsewhere"""
    B, k, C = kv.shape
    d = C // H
    out = torch.zeros(B, NP, C)
    for h in range(H):
        out[:, h * k:(h + 1) * k, h * d:(h + 1) * d] = kv[:, :, h * d:(h + 1) * d].float() * scale
    return bfr(out)


# ============================================================================================================ visitors
class Key:
    """where a stage's tensor sits in the tap dictionary: (block, sub), the decode step it belongs to, the rows of the tap it covers"""

    def __init__(self, block, sub, step=None, rows=None, shape=None):
        self.tap, self.step, self.rows, self.shape = (block, sub), step, rows, shape      # shape: of the tap, where it is not [rows, width]

    @property
    def name(self):
        return stage_name(self.tap) + (f" (step {self.step})" if self.step is not None else "")


def _miss_ratio(case, inp, got, mref, bnd):
    if case.exact:
        return float(sum(int((got[k].double() != mref[k].double()).sum()) for k in mref))
    return max(ratio(got[k], mref[k], bnd[k][0] * mref[k].double().abs() + bnd[k][1]) for k in mref)


class Checker:
    """holds the taps it is given to every stage's bound and near misses; report: {(block, sub): (worst error / bound, closest near miss)}"""

    def __init__(self, taps):
        self.taps, self.report = taps, {}

    def get(self, key):
        t = self.taps[key.tap]
        t = t[key.step] if key.step is not None else t
        return t[key.rows] if key.rows is not None else t

    def _note(self, key, worst, margin):
        w0, m0 = self.report.get(key.tap, (0.0, math.inf))
        self.report[key.tap] = (max(w0, worst), min(m0, margin))

    def exact(self, key, want, wiring=()):
        got = self.get(key)
        assert tuple(got.shape) == tuple(want.shape), f"{key.name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
        bad = int((got.float() != want.float()).sum())
        assert bad == 0, f"{key.name}: {bad} of {got.numel()} elements differ (bitwise equality expected)"
        margin = math.inf
        for label, other in wiring:
            n = int((got.float() != other.float()).sum())
            assert n > 0, f"{key.name}: wiring near miss '{label}' is not told apart"
            margin = min(margin, n)
        self._note(key, 0.0, margin)
        return got

    def stage(self, outs, case, inp, wiring=()):
        """outs: {the case's output name: (Key, dtype)}"""
        first = next(iter(outs.values()))[0]
        got, full = {o: self.get(k) for o, (k, _) in outs.items()}, {}
        for o, t in got.items():
            t = t.float().reshape(-1, t.shape[-1])
            if case is DR.LinearRows:                        # the rows of the buffer beyond M: untouched
                t = torch.cat([t, inp["buf16" if o == "out" else "buf32"][inp["M"]:]])
            full[o] = t
        ref = case.ref(inp, F64)
        full = {o: t.reshape(ref[o].shape) for o, t in full.items()}
        try:
            worst, margin = check(case, inp, full)
            bnd = None if case.exact else case.bound(inp, ref)
            for label, alt in wiring:
                q = _miss_ratio(case, inp, full, case.ref(alt, F64), bnd)
                assert q > (0 if case.exact else 1.0), f"wiring near miss '{label}' is within bound (ratio {q:.3g})"
                margin = min(margin, q)
        except AssertionError as e:
            raise AssertionError(f"{first.name}: {e}") from None
        for k, _ in outs.values():
            self._note(k, worst, margin)
        return got if len(got) > 1 else next(iter(got.values()))


class Standin:
    """computes every stage in fp32 with the library's storage types from the walk's own operands: a tap dictionary without a GPU.
    plant = (stage name as stage_name() gives it, without the step; near-miss label): that stage is computed on the near miss's operands
    (a wiring near miss of the walk, or one of the case's own near misses) wherever it occurs."""

    def __init__(self, plant=None):
        self.plant, self.parts, self.planted = plant, {}, 0

    def _hit(self, key, label):
        return self.plant is not None and self.plant == (stage_name(key.tap), label)

    def _put(self, key, t):
        self.parts.setdefault(key.tap, {}).setdefault(key.step, []).append(t if key.shape is None else t.reshape(key.shape))

    def exact(self, key, want, wiring=()):
        for label, other in wiring:
            if self._hit(key, label):
                want, self.planted = other, self.planted + 1
        self._put(key, want)
        return want

    def stage(self, outs, case, inp, wiring=()):
        first = next(iter(outs.values()))[0]
        out = None
        for label, alt in wiring:
            if self._hit(first, label):
                out, self.planted = case.ref(alt, F32), self.planted + 1
        if out is None and self.plant is not None and self.plant[0] == stage_name(first.tap):
            own = dict(case.misses(inp))
            if self.plant[1] in own:
                out, self.planted = {o: t.float() for o, t in own[self.plant[1]].items()}, self.planted + 1
        if out is None:
            out = case.ref(inp, F32)
        res = {}
        for o, (k, dt) in outs.items():
            t = out[o].float()
            if case is DR.LinearRows:
                t = t[:inp["M"]]
            t = t.reshape(-1, t.shape[-1]).to(dt)
            self._put(k, t)
            res[o] = t
        return res if len(res) > 1 else next(iter(res.values()))

    @property
    def taps(self):
        out = {}
        for tap, steps in self.parts.items():
            per = [torch.cat(v) for _, v in sorted(steps.items(), key=lambda kv: -1 if kv[0] is None else kv[0])]
            out[tap] = per[0] if None in steps else torch.stack(per)
        return out


# ============================================================================================================ the three walks
def walk_prepare(v, net, context, B2, k, fused):
    """rarm_prepare on context [B, k, context_dim]; -> {"ctxkv": [B2, k, kv_total], "G": [...], "UT": [...] per layer (fused)}"""
    B, C, H, depth = context.shape[0], net.C, net.H, net.depth
    cb = v.exact(Key(PREPARE, 1), bfr(context.float()).reshape(B * k, -1).to(BF16))
    kv = v.stage({"out": (Key(PREPARE, 2, rows=slice(0, B * k)), BF16)}, R.Linear, _lin(cb, net.kvw()),
                 [("the neighbouring layer's weights", _lin(cb, net.kvw(1)))])
    if B2 > B:
        zero = v.exact(Key(PREPARE, 2, rows=slice(B * k, B2 * k)), torch.zeros((B2 - B) * k, depth * 2 * C, dtype=BF16),
                       [("the unconditional half given the conditional half's neighbours", kv)])
        kv_all = torch.cat([kv, zero])
    else:
        kv_all = kv
    prep = {"ctxkv": kv_all.reshape(B2, k, depth * 2 * C), "G": [], "UT": []}
    if fused:
        kvb = kv.reshape(B, k, depth * 2 * C)
        for l in range(depth):
            lw, o = net.layers[l], net.near(l)
            ke = lambda j: expand_heads(kvb[..., 2 * j * C:2 * j * C + C], H, 1.0 / math.sqrt(C // H)).reshape(B * NP, C)
            ve = lambda j: expand_heads(kvb[..., 2 * j * C + C:2 * (j + 1) * C], H, 1.0).reshape(B * NP, C)
            G = v.stage({"out": (Key(PREPARE, 16 * (l + 1) + 1, shape=(B, NP, C)), BF16)}, R.Linear, _lin(ke(l), lw["wq2"].t().contiguous()),
                        [(f"layer {o}'s offset in ctxkv", _lin(ke(o), lw["wq2"].t().contiguous())),
                         ("the neighbouring layer's weights", _lin(ke(l), net.layers[o]["wq2"].t().contiguous())),
                         ("W_q not transposed", _lin(ke(l), lw["wq2"]))])
            UT = v.stage({"out": (Key(PREPARE, 16 * (l + 1) + 2, shape=(B, NP, C)), BF16)}, R.Linear, _lin(ve(l), lw["wo2"]),
                         [(f"layer {o}'s offset in ctxkv", _lin(ve(o), lw["wo2"])), ("the neighbouring layer's weights", _lin(ve(l), net.layers[o]["wo2"])),
                          ("the keys where the values belong", _lin(expand_heads(kvb[..., 2 * l * C:2 * l * C + C], H, 1.0).reshape(B * NP, C), lw["wo2"]))])
            prep["G"].append(G.reshape(B, NP, C))
            prep["UT"].append(UT.reshape(B, NP, C))
    return prep


def new_cache(net, B2):
    """the decode step's K / V cache as the reference keeps it: per layer [K, V], each [B2, H, L, 64] fp32, zero where nothing is written"""
    return [[torch.zeros(B2, net.H, net.L, 64), torch.zeros(B2, net.H, net.L, 64)] for _ in range(net.depth)]


def cache_put(cache, l, qkv, pos, C):
    """rows `pos` (an int, or [t] positions with qkv [B2, t, 3 C]) of layer l's cache from a q|k|v tensor"""
    B2, H = cache[l][0].shape[:2]
    q = qkv.float()
    if q.ndim == 2:
        cache[l][0][:, :, pos] = q[:, C:2 * C].reshape(B2, H, 64)
        cache[l][1][:, :, pos] = q[:, 2 * C:].reshape(B2, H, 64)
    else:
        t = q.shape[1]
        cache[l][0][:, :, pos] = q[..., C:2 * C].reshape(B2, t, H, 64).transpose(1, 2)
        cache[l][1][:, :, pos] = q[..., 2 * C:].reshape(B2, t, H, 64).transpose(1, 2)


def walk_step(v, net, s, pos, tokens, cache, prep, B, k, det=False, form_rows=None, head=True):
    """decode step number s of an entry: tokens [B2] at position pos.  cache: new_cache() holding the positions < pos (updated in place);
    prep: walk_prepare's result; B: the sequences that have neighbours (B2 = 2 B in a guided call); form_rows: the rows of the batch the
    kernels were chosen for, where the walk sees only some of its sequences."""
    B2, C, H, V = tokens.shape[0], net.C, net.H, net.V
    fr = form_rows or B2
    fused = one_launch(net.spec, k, fr, det)
    sel = lambda N, K, act=R.ACT_NONE, ln=False: select(fr, N, K, act, ln, det)
    key = lambda layer, stage: Key(STEP, 16 * layer + stage, step=s)
    x = v.stage({"x": (key(0, 1), F32)}, DR.Embed, {"emb": net.emb, "pos_t": net.pos, "pos": pos, "t": None, "seq0": 0, "n_seq": None, "tokens": tokens})

    def ln_rows(layer, ln_stage, stage, xin, gb, w, b=None, act=R.ACT_NONE, gb_near=None, w_near=None, b_near=None):
        """a projection of LayerNorm(xin): inside the skinny GEMM where the selector takes the shape, else a LayerNorm pass and a GEMM"""
        mk = lambda **kw: _rows(kw.pop("form"), det=det, act=act, **kw)
        if sel(w.shape[0], C, act, True)[0] == "refused":
            n = v.stage({"out": (key(layer, ln_stage), BF16)}, R.LayerNorm, _ln(xin, gb))
            f = sel(w.shape[0], C, act)
            wiring = [("the neighbouring layer's weights", mk(form=f, w=w_near, b=b_near, a=n))]
            if b is not None:
                wiring.append(("the bias left off", mk(form=f, w=w, a=n)))
            return v.stage({"out": (key(layer, stage), BF16)}, DR.LinearRows, mk(form=f, w=w, b=b, a=n), wiring)
        f = sel(w.shape[0], C, act, True)
        wiring = [("the neighbouring layer's weights", mk(form=f, w=w_near, b=b_near, x=xin, gb=gb_near))]
        if b is not None:
            wiring.append(("the bias left off", mk(form=f, w=w, x=xin, gb=gb)))
        return v.stage({"out": (key(layer, stage), BF16)}, DR.LinearRows, mk(form=f, w=w, b=b, x=xin, gb=gb), wiring)

    def res_rows(layer, stage, a, w, b, res, w_near, b_near, res_block=None):
        """x + a w^T + b into the fp32 residual stream"""
        f = sel(w.shape[0], w.shape[1])
        mk = lambda **kw: _rows(f, f32=True, det=det, **kw)
        wiring = [("the neighbouring layer's weights", mk(w=w_near, b=b_near, a=a, res=res)), ("the bias left off", mk(w=w, a=a, res=res))]
        if res_block is not None:
            wiring.append(("the residual taken from the block's input", mk(w=w, b=b, a=a, res=res_block)))
        return v.stage({"out32": (key(layer, stage), F32)}, DR.LinearRows, mk(w=w, b=b, a=a, res=res), wiring)

    for l in range(net.depth):
        lw, nw, o, L1 = net.layers[l], net.layers[net.near(l)], net.near(l), l + 1
        x_in = x
        qkv = ln_rows(L1, 1, 2, x_in, lw["ln1"], lw["wqkv"], gb_near=nw["ln1"], w_near=nw["wqkv"])
        ao = v.stage({"out": (key(L1, 3), BF16)}, DR.DecodeAttention, _self_attn(qkv, cache[l][0], cache[l][1], pos))
        cache_put(cache, l, qkv, pos, C)
        x4 = res_rows(L1, 4, ao, lw["wo1"], lw["bo1"], x_in, nw["wo1"], nw["bo1"])
        if fused:
            xa = lambda xx, w, G, UT, bias=True: {"x": xx.float(), "gamma": w["ln2"][0], "beta": w["ln2"][1], "eps": 1e-5, "heads": H, "k": k, "Bc": B, "NP": NP,
                                                  "bias": w["bo2"] if bias else torch.zeros(C), "G": G.float(), "UT": UT.float(), "ln3": True,
                                                  "gamma3": w["ln3"][0], "beta3": w["ln3"][1]}
            G, UT = prep["G"], prep["UT"]
            got = v.stage({"x": (key(L1, 8), F32), "ln3": (key(L1, 9), BF16)}, DR.XattnDecode, xa(x4, lw, G[l], UT[l]),
                          [(f"layer {o}'s G and UT", xa(x4, lw, G[o], UT[o])), ("the neighbouring layer's weights", xa(x4, nw, G[l], UT[l])),
                           ("the bias left off", xa(x4, lw, G[l], UT[l], bias=False)), ("the residual taken from the block's input", xa(x_in, lw, G[l], UT[l]))])
            x8, n3 = got["x"], got["ln3"]
            ff = v.stage({"out": (key(L1, 10), BF16)}, DR.LinearRows,
                         _rows(sel(8 * C, C, R.ACT_GEGLU), lw["wff1"], lw["bff1"], a=n3, act=R.ACT_GEGLU, det=det),
                         [("the neighbouring layer's weights", _rows(sel(8 * C, C, R.ACT_GEGLU), nw["wff1"], nw["bff1"], a=n3, act=R.ACT_GEGLU, det=det)),
                          ("the bias left off", _rows(sel(8 * C, C, R.ACT_GEGLU), lw["wff1"], a=n3, act=R.ACT_GEGLU, det=det))])
        else:
            q2 = ln_rows(L1, 5, 6, x4, lw["ln2"], lw["wq2"], gb_near=nw["ln2"], w_near=nw["wq2"])
            kv = prep["ctxkv"]
            wiring = [(f"layer {o}'s offset in ctxkv", _cross_attn(q2, kv, C, H, o, l, fr))]
            if B2 > B:
                wiring.append(("the unconditional half given the conditional half's neighbours", _cross_attn(q2, torch.cat([kv[:B], kv[:B2 - B]]), C, H, l, o, fr)))
            ao2 = v.stage({"out": (key(L1, 7), BF16)}, DR.DecodeAttention, _cross_attn(q2, kv, C, H, l, o, fr), wiring)
            x8 = res_rows(L1, 8, ao2, lw["wo2"], lw["bo2"], x4, nw["wo2"], nw["bo2"], res_block=x_in)
            ff = ln_rows(L1, 9, 10, x8, lw["ln3"], lw["wff1"], lw["bff1"], R.ACT_GEGLU, gb_near=nw["ln3"], w_near=nw["wff1"], b_near=nw["bff1"])
        x = res_rows(L1, 11, ff, lw["wff2"], lw["bff2"], x8, nw["wff2"], nw["bff2"], res_block=x_in)
    if not head:
        return None
    xb = v.exact(key(0, 2), bfr(x.float()).to(BF16))
    f = sel(V, C)
    return v.stage({"out32": (key(0, 3), F32)}, DR.LinearRows, _rows(f, net.wpo, net.bpo, a=xb, f32=True, det=det),
                   [("the bias left off", _rows(f, net.wpo, a=xb, f32=True, det=det))])


def walk_seq(v, net, tokens, B2, t, prep, B, k, cache=None, head=True, cache_pos=None):
    """the whole-sequence pass over positions 0 .. t-1 of B2 sequences; tokens [tok_rows, >= t], sequence s reads row s % tok_rows.
    cache: new_cache() to receive the K / V rows of every layer (rdm_rarm_sample_prefill's hand-over), at the rows cache_pos (the
    positions themselves; a stand-in with a planted error passes others)."""
    C, H, V = net.C, net.H, net.V
    key = lambda layer, stage: Key(SEQ, 16 * layer + stage)
    x = v.stage({"x": (key(0, 1), F32)}, DR.Embed, {"emb": net.emb, "pos_t": net.pos, "pos": None, "t": t, "seq0": 0, "n_seq": B2, "tokens": tokens})
    kv = prep["ctxkv"]
    for l in range(net.depth):
        lw, nw, o, L1 = net.layers[l], net.layers[net.near(l)], net.near(l), l + 1
        near = ("the neighbouring layer's weights",)
        x_in = x
        n1 = v.stage({"out": (key(L1, 1), BF16)}, R.LayerNorm, _ln(x_in, lw["ln1"]), [near + (_ln(x_in, nw["ln1"]),)])
        qkv = v.stage({"out": (key(L1, 2), BF16)}, R.Linear, _lin(n1, lw["wqkv"]), [near + (_lin(n1, nw["wqkv"]),)])
        q3 = qkv.float().reshape(B2, t, 3 * C)
        if cache is not None:
            cache_put(cache, l, q3, torch.arange(t) if cache_pos is None else cache_pos, C)
        ao = v.stage({"out": (key(L1, 3), BF16)}, CausalAttention, _attn(q3[..., :C], q3[..., C:2 * C], q3[..., 2 * C:], H, 1))
        x4 = v.stage({"out": (key(L1, 4), F32)}, R.Linear, _lin(ao, lw["wo1"], lw["bo1"], f32=True, res=x_in.float()),
                     [near + (_lin(ao, nw["wo1"], nw["bo1"], f32=True, res=x_in.float()),)])
        n2 = v.stage({"out": (key(L1, 5), BF16)}, R.LayerNorm, _ln(x4, lw["ln2"]), [near + (_ln(x4, nw["ln2"]),)])
        q2 = v.stage({"out": (key(L1, 6), BF16)}, R.Linear, _lin(n2, lw["wq2"]), [near + (_lin(n2, nw["wq2"]),)])
        sm = lambda kv_, j: _attn(q2.reshape(B2, t, C), kv_[..., 2 * j * C:2 * j * C + C], kv_[..., 2 * j * C + C:2 * (j + 1) * C], H, 0)
        wiring = [(f"layer {o}'s offset in ctxkv", sm(kv, o))]
        if B2 > B:
            wiring.append(("the unconditional half given the conditional half's neighbours", sm(torch.cat([kv[:B], kv[:B2 - B]]), l)))
        ao2 = v.stage({"out": (key(L1, 7), BF16)}, R.SmallAttention, sm(kv, l), wiring)
        x8 = v.stage({"out": (key(L1, 8), F32)}, R.Linear, _lin(ao2, lw["wo2"], lw["bo2"], f32=True, res=x4.float()),
                     [near + (_lin(ao2, nw["wo2"], nw["bo2"], f32=True, res=x4.float()),),
                      ("the residual taken from the block's input", _lin(ao2, lw["wo2"], lw["bo2"], f32=True, res=x_in.float()))])
        n3 = v.stage({"out": (key(L1, 9), BF16)}, R.LayerNorm, _ln(x8, lw["ln3"]), [near + (_ln(x8, nw["ln3"]),)])
        ff = v.stage({"out": (key(L1, 10), BF16)}, _GegluLinear, _lin(n3, lw["wff1"], lw["bff1"], act=R.ACT_GEGLU),
                     [near + (_lin(n3, nw["wff1"], nw["bff1"], act=R.ACT_GEGLU),), ("the bias left off", _lin(n3, lw["wff1"], act=R.ACT_GEGLU))])
        x = v.stage({"out": (key(L1, 11), F32)}, R.Linear, _lin(ff, lw["wff2"], lw["bff2"], f32=True, res=x8.float()),
                    [near + (_lin(ff, nw["wff2"], nw["bff2"], f32=True, res=x8.float()),),
                     ("the residual taken from the block's input", _lin(ff, lw["wff2"], lw["bff2"], f32=True, res=x_in.float()))])
    if not head:
        return None
    xb = v.exact(key(0, 2), bfr(x.float()).to(BF16))
    return v.stage({"out": (key(0, 3), F32)}, R.Linear, _lin(xb, net.wpo, net.bpo, f32=True))


# ============================================================================================================ whole entries
def decode_positions(cond_len, steps, prefill=False):
    """the positions of the decode steps of one sampling call, in order (rarm_sample_run)"""
    first = cond_len - 1 if prefill and cond_len > 1 else 0
    return list(range(first, cond_len - 1 + steps))


def sample_tokens(cond, sampled, pos, guided):
    """the token column a sampling call feeds at position pos: cond [B, cond_len], sampled [B, steps] (what the call returned)"""
    col = cond[:, pos] if pos < cond.shape[1] else sampled[:, pos - cond.shape[1]]
    return torch.cat([col, col]) if guided else col


def run_forward(v, net, tokens, context, det=False, form_rows=None):
    """rdm_rarm_forward over tokens [b, t]"""
    b, t = tokens.shape
    k = context.shape[1]
    prep = walk_prepare(v, net, context, b, k, one_launch(net.spec, k, form_rows or b, det))
    cache = new_cache(net, b)
    for i in range(t):
        walk_step(v, net, i, i, tokens[:, i], cache, prep, b, k, det, form_rows)
    return v


def run_forward_seq(v, net, tokens, context):
    """rdm_rarm_forward_seq over tokens [b, t]"""
    b, t = tokens.shape
    k = context.shape[1]
    prep = walk_prepare(v, net, context, b, k, False)
    walk_seq(v, net, tokens, b, t, prep, b, k)
    return v


def run_sample(v, net, cond, sampled, context, guided, prefill=False, cache_pos=None):
    """rdm_rarm_sample / rdm_rarm_sample_prefill with the tokens it drew given (teacher-forced): cond [B, cond_len], sampled [B, steps]"""
    B, k = context.shape[:2]
    B2 = 2 * B if guided else B
    prep = walk_prepare(v, net, context, B2, k, one_launch(net.spec, k, B2, False))
    cache = new_cache(net, B2)
    pos = decode_positions(cond.shape[1], sampled.shape[1], prefill)
    if pos[0] > 0:
        walk_seq(v, net, cond, B2, pos[0], prep, B, k, cache=cache, head=False, cache_pos=cache_pos)
    for s, p in enumerate(pos):
        walk_step(v, net, s, p, sample_tokens(cond, sampled, p, guided), cache, prep, B, k)
    return v


def summary(rep):
    return "\n".join(f"  {stage_name(key)}: worst error / bound {w:.3g}, closest near miss {m:.3g}" for key, (w, m) in rep.items())
