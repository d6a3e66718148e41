"""GPU suite of the RARM sampler's nucleus (top-p) filter, through the C ABI (rdm_op_rarm_sampler_top_p, rdm_rarm_sample_top_p),
against the float64 restatement of its definition in tests/_nucleus_ref.py.  Everything is deterministic given the caller's
uniforms, so kept counts and tokens are compared for EQUALITY; the only rows left out are those the kernel's fp32 sums cannot decide.

The band eps (u = 2^-24), from the kernel's own summation order (csrc/rarm.hip, the nucleus instantiation of rarm_sample_kernel):
  * a term is e^_i = v_exp_f32(fl(fl(g_i - max) * log2e)): the subtraction, the product and the fp32 constant each move the exponent
    by at most u |x_i| (x_i = g_i - max, in natural units), the instruction is good to 1 ulp = 2 u:  |e^_i - e_i| <= (3 |x_i| + 2) u e_i;
  * a mass M^(theta) adds the terms at or above theta in a fixed tree: four chains of 16 per thread, (a0 + a1) + (a2 + a3), six butterfly
    levels in the wave, (w0 + w1) + (w2 + w3): no term passes through more than 16 + 2 + 6 + 2 = 26 additions of non-negative numbers:
        |M^ - M| <= u [ (26 + 2) M + 3 sum_{set} |x_i| e_i ]
    and the same for the total T^ (the mass of all top-k survivors), which is added in the same tree;
  * the kernel asks M^(theta) >= fl(top_p * T^).  It can answer differently from M(theta) / T >= top_p only if
        |M(theta) / T - top_p| <= u (28 + 3 X) (1 + top_p) + u top_p =: eps,      X = sum_K p_i |x_i|
    (M / T <= 1, the set's share of X is at most X).  r|ref| + c u S form: r = 0 (fp32), S = the mass, c = 28 + 3 X.  eps is evaluated PER
    ROW in float64 (`nr.mass_band`); on these inputs it is 3e-6 to 5e-6, below the 1e-5 the row counts of the case tables were taken at.
  * a row is DECIDED when both M(theta*) - top_p and top_p - M(next larger present value) exceed eps: then the kernel's search must stop
    at theta* exactly, whatever its rounding.
  * the draw (unchanged code) adds 64-term chunks and then 256 partials serially (depth 320) and compares with fl(u * total):
        eps_draw = u (2 (322 + 3 X_n) + 1),  X_n over the nucleus;  a token is compared where |u - every CDF edge| > eps_draw."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import rarm as orarm
from oracle import unet as ounet
from oracle import vqdecoder as ovq

import _nucleus_ref as nr
from _util import golden

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

V = 16384
TOP_PS = (0.5, 0.9, 0.95)


def _cfg(spec):
    from rdm_amd import _lib
    return _lib.make_rarm_cfg(in_channels=spec.vocab_in, out_channels=spec.vocab_out, n_heads=spec.n_heads, d_head=spec.d_head,
                              depth=spec.depth, context_dim=spec.context_dim, sequence_length=spec.sequence_length)


def _load(ctx, spec, seed):
    from rdm_amd import packing
    sd = ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=seed)
    cfg = _cfg(spec)
    ctx.load_rarm(cfg, packing.pack("rarm", cfg, sd))
    return sd


def _golden_rows():
    """The four guided rows of rarm_shipped_deep.npz (2 stored steps x 2 sequences): conditional, unconditional, scale, T, top-k."""
    g = golden("rarm_shipped_deep.npz")
    raw = torch.from_numpy(g["raw_logits"])                       # [2 steps][cond rows 0,1 then uncond rows 0,1][vocab]
    lc = torch.cat([raw[0, :2], raw[1, :2]]); lu = torch.cat([raw[0, 2:], raw[1, 2:]])
    return g, lc, lu, float(g["guidance_scale"]), float(g["temperature"]), int(g["top_k"])


def _op(ctx, lc, lu, u, scale, T, top_k, top_p):
    logits = lc if lu is None else torch.cat([lc, lu])
    tok, kept = ctx.op_rarm_sampler(logits, u, guidance_scale=scale if lu is not None else 1.0, temperature=T, top_k=top_k, top_p=top_p,
                                    return_kept=True)
    return tok.cpu(), kept.cpu().long()


def _random_case(sigma, seed=123, rows=256):
    rng = np.random.default_rng(seed)
    g = torch.from_numpy((rng.standard_normal((rows, V)) * sigma).astype(np.float32))
    u = torch.from_numpy(rng.random(rows).astype(np.float32))
    return g, u


def _decided_tokens(g, keep, u):
    want, edge, xn = nr.draw(g, keep, u)
    return want, edge > nr.draw_band(xn)


# ------------------------------------------------------------------------------------------------------------ 1. identity
def test_top_p_one_is_the_old_entry_bit_for_bit(ctx):
    """The new entries with top_p = 1 against the old ones: the op at vocabulary 16 384 on the golden's stored logits (the kept count is
    then the top-k survivors'), rdm_rarm_sample_top_p on the tiny model with the golden's uniforms."""
    from rdm_amd import _lib
    g, lc, lu, scale, T, K = _golden_rows()
    rng = np.random.default_rng(3)
    lc64, lu64 = lc.repeat_interleave(64, 0), lu.repeat_interleave(64, 0)
    u = torch.from_numpy(rng.random(256).astype(np.float32))
    old = ctx.op_rarm_sampler(torch.cat([lc64, lu64]), u, guidance_scale=scale, temperature=T, top_k=K).cpu()
    new, kept = _op(ctx, lc64, lu64, u, scale, T, K, 1.0)
    assert torch.equal(new, old)
    gl = nr.guided_logits(lc64, lu64, scale, T)
    assert torch.equal(kept, (orarm.top_k_logits(gl, K) > -float("inf")).sum(-1))
    gt = golden("rarm_tiny.npz")
    spec = orarm.tiny_rarm_spec()
    _load(ctx, spec, int(gt["seed"]))
    steps, B = gt["uniforms"].shape
    cond = torch.full((B, 1), spec.vocab_in - 1, dtype=torch.long)
    ut = torch.from_numpy(gt["uniforms"]); cx = torch.from_numpy(gt["ctx"])
    kw = dict(temperature=float(gt["temperature"]), top_k=int(gt["top_k"]), guidance_scale=float(gt["guidance_scale"]))
    old = ctx.rarm_sample(cond, cx, steps, ut, **kw).cpu()
    d = ctx.device
    a = _lib.RarmSampleArgs(batch=B, k=cx.shape[1], cond_len=1, steps=steps, temperature=kw["temperature"], top_k=kw["top_k"],
                            guidance_scale=kw["guidance_scale"])
    cond_d, cx_d, ut_d = cond.to(d), cx.to(d).contiguous(), ut.to(d).contiguous()
    out = torch.empty((B, steps), device=d, dtype=torch.int64)
    rc = _lib.lib.rdm_rarm_sample_top_p(ctx._h, C.byref(a), 1.0, _lib._ptr(cond_d), _lib._ptr(cx_d), _lib._ptr(ut_d), _lib._ptr(out))
    assert rc == 0, _lib.lib.rdm_last_error(ctx._h)
    assert torch.equal(out.cpu(), old)
    assert torch.equal(ctx.rarm_sample(cond, cx, steps, ut, top_p=1.0, **kw).cpu(), old)


# ------------------------------------------------------------------------------------------------------------ 2. real logits
@pytest.mark.parametrize("top_p", TOP_PS)
def test_nucleus_exact_on_stored_reference_logits(ctx, top_p):
    """The four guided rows of the golden (raw_logits, top-k 256, the file's scale and temperature), 64 uniforms per row: the kept count
    equals the restatement's and EVERY token equals its draw (the rows' smallest mass margin is 1e-4, far outside the band)."""
    g, lc, lu, scale, T, K = _golden_rows()
    gl = nr.guided_logits(lc, lu, scale, T)
    r = nr.nucleus(gl, K, top_p)
    print(f"top_p {top_p}: kept {r['count'].tolist()}, mass margins {[f'{m:.2e}' for m in r['margin'].tolist()]}, "
          f"band {[f'{e:.1e}' for e in nr.mass_band(r['xk'], top_p).tolist()]}")
    u = torch.from_numpy(np.random.default_rng(11).random(256).astype(np.float32))
    tok, kept = _op(ctx, lc.repeat_interleave(64, 0), lu.repeat_interleave(64, 0), u, scale, T, K, top_p)
    assert torch.equal(kept, r["count"].repeat_interleave(64))
    want, _, _ = nr.draw(gl.repeat_interleave(64, 0), r["keep"].repeat_interleave(64, 0), u)
    print(f"  token mismatches {int((tok != want).sum())} of 256; distinct tokens drawn {len(set(tok.tolist()))}")
    assert torch.equal(tok, want)


# ------------------------------------------------------------------------------------------------------------ 3. random logits
RANDOM_CASES = [(3.0, 256, TOP_PS), (6.0, 256, TOP_PS), (6.0, None, TOP_PS), (3.0, None, (0.5,))]


@pytest.mark.parametrize("sigma,top_k,top_ps", RANDOM_CASES, ids=lambda v: str(v))
def test_nucleus_on_random_logits(ctx, sigma, top_k, top_ps):
    """256 rows of N(0, sigma^2) at vocabulary 16 384, unguided, temperature 1 (the kernel's logits are the inputs bit for bit).  On
    every decided row (module docstring) the kept count is equal; tokens are equal wherever u is outside the draw's band of every CDF
    edge.  At most 5 % of a case's rows may be undecided.  (sigma 3 without top-k only at top_p 0.5: above it the nucleus holds hundreds
    to thousands of tokens of probability around 1e-5, and a sixth or more of the rows sit inside any fp32 band.)"""
    g, u = _random_case(sigma)
    for top_p in top_ps:
        r = nr.nucleus(g, top_k, top_p)
        eps = nr.mass_band(r["xk"], top_p)
        decided = r["margin"] > eps
        tok, kept = _op(ctx, g, None, u, 1.0, 1.0, top_k, top_p)
        want, tok_ok = _decided_tokens(g, r["keep"], u)
        und = int((~decided).sum())
        print(f"sigma {sigma} top_k {top_k} top_p {top_p}: band {float(eps.min()):.2e}..{float(eps.max()):.2e}, undecided rows {und} of {len(u)}, "
              f"kept {int(r['count'].min())}..{int(r['count'].max())}, count mismatches on decided {int((kept != r['count'])[decided].sum())}, "
              f"on undecided {int((kept != r['count'])[~decided].sum())}, tokens compared {int((decided & tok_ok).sum())}, "
              f"token mismatches {int((tok != want)[decided & tok_ok].sum())}")
        assert und <= 0.05 * len(u)
        assert torch.equal(kept[decided], r["count"][decided])
        assert torch.equal(tok[decided & tok_ok], want[decided & tok_ok])


def test_nucleus_above_the_register_resident_vocabulary(ctx):
    """Vocabularies above 16 384 take the kernel's loop from LDS: 20 000 entries, sigma 6, top-k 256 and none.  Its per-thread chains are
    ceil(V / 1024) = 20 long: depth 20 + 2 + 6 + 2 = 30 in the band."""
    rng = np.random.default_rng(31)
    g = torch.from_numpy((rng.standard_normal((32, 20000)) * 6.0).astype(np.float32))
    u = torch.from_numpy(rng.random(32).astype(np.float32))
    for top_k in (256, None):
        for top_p in (0.5, 0.9):
            r = nr.nucleus(g, top_k, top_p)
            decided = r["margin"] > nr.mass_band(r["xk"], top_p, depth=30)
            tok, kept = _op(ctx, g, None, u, 1.0, 1.0, top_k, top_p)
            want, tok_ok = _decided_tokens(g, r["keep"], u)
            print(f"vocab 20000 top_k {top_k} top_p {top_p}: undecided {int((~decided).sum())} of 32")
            assert int((~decided).sum()) <= 0.05 * 32
            assert torch.equal(kept[decided], r["count"][decided])
            assert torch.equal(tok[decided & tok_ok], want[decided & tok_ok])
            old = ctx.op_rarm_sampler(g, u, top_k=top_k).cpu()
            new, _ = _op(ctx, g, None, u, 1.0, 1.0, top_k, 1.0)
            assert torch.equal(new, old)


# ------------------------------------------------------------------------------------------------------------ 4. near misses
def test_nucleus_is_none_of_the_near_misses(ctx):
    """The kernel's kept counts match the right restatement on all decided rows of the random case (sigma 3, top-k 256) and differ, on at
    least one decided row, from each wrong one: mass relative to the whole vocabulary, the crossing token dropped, top-p before top-k;
    on the golden's guided rows, from the nucleus of the unguided (conditional) logits; on a planted tie, from the cut tie group."""
    g, u = _random_case(3.0)
    for top_p in (0.9, 0.95):
        r = nr.nucleus(g, 256, top_p)
        decided = r["margin"] > nr.mass_band(r["xk"], top_p)
        _, kept = _op(ctx, g, None, u, 1.0, 1.0, 256, top_p)
        assert torch.equal(kept[decided], r["count"][decided])
        for variant in ("whole_vocab", "strict", "p_before_k"):
            wrong = nr.nucleus(g, 256, top_p, variant=variant)["count"]
            n = int((kept != wrong)[decided].sum())
            print(f"top_p {top_p} near miss {variant}: differs on {n} of {int(decided.sum())} decided rows")
            assert n >= 1
    _, lc, lu, scale, T, K = _golden_rows()
    gl = nr.guided_logits(lc, lu, scale, T)
    u4 = torch.full((4,), 0.5)
    for top_p in TOP_PS:
        _, kept = _op(ctx, lc, lu, u4, scale, T, K, top_p)
        right = nr.nucleus(gl, K, top_p)["count"]
        unguided = nr.nucleus(nr.guided_logits(lc, None, 1.0, T), K, top_p)["count"]
        print(f"top_p {top_p}: guided nucleus {right.tolist()}, nucleus of the unguided logits {unguided.tolist()}, kernel {kept.tolist()}")
        assert torch.equal(kept, right) and not torch.equal(kept, unguided)
    g1, i_a, i_b, top_p = _planted_tie()
    _, kept = _op(ctx, g1, None, torch.full((1,), 0.5), 1.0, 1.0, 256, top_p)
    right, cut = nr.nucleus(g1, 256, top_p), nr.nucleus(g1, 256, top_p, variant="cut_tie")
    assert int(cut["count"]) == int(right["count"]) - 1
    assert int(kept) == int(right["count"]) and int(kept) != int(cut["count"])


# ------------------------------------------------------------------------------------------------------------ 5. planted tie
def _planted_tie():
    """A row of the random case whose nucleus edge is moved onto a tie: the first token BELOW the nucleus of top_p = 0.9 is given the
    value of the last one inside, and top_p is put in the middle of the (now doubled) step, so that the pair straddles the edge with a
    mass margin of half that token's probability (> 1e-3)."""
    g, _ = _random_case(6.0)
    for row in range(g.shape[0]):
        r = nr.nucleus(g[row:row + 1], 256, 0.9)
        n = int(r["count"])
        if n < 2:
            continue
        order = torch.argsort(g[row], descending=True)
        i_a, i_b = int(order[n - 1]), int(order[n])
        g1 = g[row:row + 1].clone()
        g1[0, i_b] = g1[0, i_a]
        p = nr.probs_of(g1, orarm.top_k_logits(g1.double(), 256) > -float("inf"))[0]
        above = float(p[order[:n - 1]].sum())
        top_p = above + float(p[i_a]) * 0.5                    # reached by the first of the pair only: the second is the tie
        r1 = nr.nucleus(g1, 256, top_p)
        if float(p[i_a]) > 4e-3 and float(r1["margin"]) > 1e-3 and top_p < 0.999:
            assert int(r1["count"]) == n + 1 and bool(r1["keep"][0, i_a]) and bool(r1["keep"][0, i_b])
            return g1, i_a, i_b, top_p
    raise AssertionError("no row with a heavy enough boundary token")


def test_planted_boundary_tie_is_kept_whole(ctx):
    g1, i_a, i_b, top_p = _planted_tie()
    r = nr.nucleus(g1, 256, top_p)
    u = torch.from_numpy(np.random.default_rng(77).random(64).astype(np.float32))
    c = nr.probs_of(g1, r["keep"])[0].cumsum(0)
    for j, i in enumerate((i_a, i_b)):                          # two of the 64 uniforms aim at the middle of the pair's own CDF intervals
        u[j] = float((c[i - 1] if i > 0 else 0.0) + c[i]) / 2
    tok, kept = _op(ctx, g1.repeat(64, 1), None, u, 1.0, 1.0, 256, top_p)
    want, _, _ = nr.draw(g1.repeat(64, 1), r["keep"].repeat(64, 1), u)
    print(f"planted boundary tie at top_p {top_p:.6f}: margin {float(r['margin']):.2e}, kept {int(kept[0])} (restatement {int(r['count'])}), "
          f"draws of the tied pair: {int((tok == i_a).sum())} + {int((tok == i_b).sum())}, mismatches {int((tok != want).sum())} of 64")
    assert torch.equal(kept, r["count"].repeat(64))
    assert torch.equal(tok, want)
    assert int((want == i_a).sum()) >= 1 and int((want == i_b).sum()) >= 1       # both members are drawn: neither was cut


# ------------------------------------------------------------------------------------------------------------ 6. batch independence
def test_nucleus_does_not_depend_on_the_batch(ctx):
    """A row's token and kept count are the same bits alone (b = 1) and as row 37 of 64, guided and not, and two calls give equal bits."""
    g, u = _random_case(3.0, rows=64)
    _, lc, lu, scale, T, K = _golden_rows()
    for top_p in (0.5, 0.95):
        tok, kept = _op(ctx, g, None, u, 1.0, 1.0, 256, top_p)
        tok2, kept2 = _op(ctx, g, None, u, 1.0, 1.0, 256, top_p)
        assert torch.equal(tok, tok2) and torch.equal(kept, kept2)
        t1, k1 = _op(ctx, g[37:38], None, u[37:38], 1.0, 1.0, 256, top_p)
        assert int(t1) == int(tok[37]) and int(k1) == int(kept[37])
        lcb, lub = lc[torch.arange(64) % 4], lu[torch.arange(64) % 4]
        tok, kept = _op(ctx, lcb, lub, u, scale, T, K, top_p)
        t1, k1 = _op(ctx, lcb[37:38], lub[37:38], u[37:38], scale, T, K, top_p)
        assert int(t1) == int(tok[37]) and int(k1) == int(kept[37])


# ------------------------------------------------------------------------------------------------------------ 7. the loop
def test_nucleus_sampling_loop_matches_restated_loop(ctx):
    """rdm_rarm_sample_top_p on the one-layer, bias-dominated model of test_rarm_sampler_kernel_matches_oracle: 32 steps, top-k 256,
    top_p 0.9, guided and unguided, against the restated loop over oracle.rarm.rarm_forward.  Agreement >= 0.98, that test's bound for
    the same fp32-against-bf16 logit noise."""
    from rdm_amd import packing
    spec = orarm.RarmSpec(vocab_in=4098, vocab_out=4096, n_heads=1, d_head=64, depth=1, context_dim=64, sequence_length=40)
    sd = ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=5)
    sd["proj_out.weight"] = sd["proj_out.weight"] * 1e-3
    sd["proj_out.bias"] = torch.from_numpy(np.random.default_rng(6).standard_normal(4096).astype(np.float32) * 3.0)
    cfg = _cfg(spec)
    ctx.load_rarm(cfg, packing.pack("rarm", cfg, sd))
    B, steps = 7, 32
    rng = np.random.default_rng(9)
    u = torch.from_numpy(rng.random((steps, B)).astype(np.float32))
    cctx = torch.from_numpy((rng.standard_normal((B, 2, 64)) * 0.45).astype(np.float32))
    cond = torch.full((B, 1), 4097, dtype=torch.long)
    for scale in (1.0, 3.0):
        got = ctx.rarm_sample(cond, cctx, steps, u, temperature=1.3, top_k=256, guidance_scale=scale, top_p=0.9).cpu()
        plain = ctx.rarm_sample(cond, cctx, steps, u, temperature=1.3, top_k=256, guidance_scale=scale).cpu()
        x = cond.clone()
        r = torch.cat((cctx, torch.zeros_like(cctx))) if scale > 1.0 else cctx
        for s in range(steps):
            lg = orarm.rarm_forward(sd, spec, torch.cat((x, x)) if scale > 1.0 else x, r)[:, -1]
            gl = nr.guided_logits(lg[:B], lg[B:], scale, 1.3) if scale > 1.0 else nr.guided_logits(lg, None, 1.0, 1.3)
            tok, _, _ = nr.draw(gl, nr.nucleus(gl, 256, 0.9)["keep"], u[s])
            x = torch.cat((x, tok[:, None]), dim=1)
        want = x[:, 1:]
        agree = (got == want).float().mean().item()
        print(f"nucleus loop scale {scale}: token agreement {agree:.4f}; tokens that differ from the top_p = 1 run {int((got != plain).sum())} of {got.numel()}")
        assert agree >= 0.98
        assert not torch.equal(got, plain)


# ------------------------------------------------------------------------------------------------------------ 8. surface, script
def test_latent_image_retro_sampling_util_top_p(ctx):
    """LatentImageRETRO.sampling_util(top_p=0.9) (the call the reference asserts away, transformer.py:279-280) returns images of the right
    shape, and its tokens differ from the top_p = 1 run with the same uniforms."""
    from rdm_amd.models.autoregression.transformer import LatentImageRETRO
    spec = orarm.RarmSpec(vocab_in=514, vocab_out=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64)
    vspec = ovq.tiny_vqgan_spec()
    tcfg = {"params": dict(in_channels=spec.vocab_in, out_channels=spec.vocab_out, n_heads=spec.n_heads, d_head=64, depth=spec.depth,
                           context_dim=512, sequence_length=spec.sequence_length, continuous=False, causal=True)}
    fcfg = {"params": {"embed_dim": 64, "n_embed": 512, "ddconfig": {"z_channels": 64, "ch": 64, "ch_mult": vspec.ch_mult, "num_res_blocks": 1,
                                                                   "resolution": 32, "attn_resolutions": vspec.attn_resolutions}}}
    m = LatentImageRETRO(tcfg, fcfg, mask_token=512, sos_token=513, nn_memory=np.arange(500), k_nn=4, ctx=ctx)
    m.load_transformer_state_dict(ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=777))
    m.load_first_stage_state_dict(ounet.synth_state_dict(ovq.vq_param_shapes(vspec), seed=888))
    rng = np.random.default_rng(21)
    r = torch.from_numpy((rng.standard_normal((3, 4, 512)) * 0.45).astype(np.float32))
    u = torch.from_numpy(rng.random((64, 3)).astype(np.float32))
    _, c = m.encode_to_c(torch.zeros((3, 0)))
    z0 = torch.zeros((3, 0), dtype=torch.long)
    img = m.sampling_util(64, z0, r, c, 1.0, 50, (3, 64, 8, 8), top_p=0.9, uniforms=u, guidance_scale=2.0)
    assert img.shape == (3, 3, 32, 32) and bool(torch.isfinite(img).all())
    t9 = m.sample(z0, r, c, 64, sample=True, top_k=50, top_p=0.9, uniforms=u, guidance_scale=2.0).cpu()
    t1 = m.sample(z0, r, c, 64, sample=True, top_k=50, top_p=1.0, uniforms=u, guidance_scale=2.0).cpu()
    assert t9.shape == t1.shape == (3, 64) and not torch.equal(t9, t1)
    assert torch.equal(m.decode_to_img(t9, None).cpu(), img.cpu())
    amax = m.sample(z0, r, c, 64, sample=False, top_p=0.3, uniforms=u, guidance_scale=2.0).cpu()       # arg-max: top_p has no effect
    assert torch.equal(amax, m.sample(z0, r, c, 64, sample=False, uniforms=u, guidance_scale=2.0).cpu())
    out = m.sample_from_rdata(2, nn_embeddings=torch.zeros(2, 1, 512), code_side_len=8, z_dimensionality=64, top_k=10, top_p=0.9)
    assert out["samples_with_sampled_nns"].shape == (2, 3, 32, 32)


def test_rarm_sample_script_top_p(tmp_path):
    """`scripts/rarm_sample.py --synthetic --top_p 0.9` end to end on the shipped architecture."""
    from PIL import Image
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "rarm_sample.py")
    sp = importlib.util.spec_from_file_location("rarm_sample_native_top_p", path)
    mod = importlib.util.module_from_spec(sp); sp.loader.exec_module(mod)
    opt = mod.parse_args(["--synthetic", "--synthetic_db_rows", "20000", "--gpu", "0", "-bs", "2", "-n", "1", "--seed", "7", "--k_nn", "8",
                          "--top_p", "0.9", "-s", str(tmp_path)])
    assert opt.top_p == 0.9
    model = mod.load_model(opt)
    mod.sample(model, opt)
    files = sorted(tmp_path.iterdir())
    assert len(files) == 2
    px = [np.asarray(Image.open(f)) for f in files]
    assert all(v.shape == (256, 256, 3) and v.dtype == np.uint8 for v in px) and len(np.unique(px[0])) > 16
    model.ctx.close()


# ------------------------------------------------------------------------------------------------------------ 9. errors
@pytest.mark.parametrize("bad", [0.0, -0.1, 1.5, float("nan")])
def test_bad_top_p_is_an_argument_error_on_both_entries(ctx, bad):
    """Refused on the host, before any launch: return code -1 and a message naming top_p; the context works afterwards."""
    from rdm_amd import _lib
    d = ctx.device
    g, u = _random_case(3.0, rows=4)
    gd, ud = g.to(d), u.to(d)
    out = torch.full((4,), -7, device=d, dtype=torch.int64)
    kept = torch.full((4,), -7, device=d, dtype=torch.int32)
    rc = _lib.lib.rdm_op_rarm_sampler_top_p(ctx._h, _lib._ptr(gd), 4, V, 0, 1.0, 1.0, 256, bad, _lib._ptr(ud), _lib._ptr(out), _lib._ptr(kept))
    msg = _lib.lib.rdm_last_error(ctx._h).decode()
    assert rc == -1 and "top_p" in msg and "rdm_op_rarm_sampler_top_p" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((kept == -7).all())
    spec = orarm.tiny_rarm_spec()
    gt = golden("rarm_tiny.npz")
    _load(ctx, spec, int(gt["seed"]))
    steps, B = gt["uniforms"].shape
    cond = torch.full((B, 1), spec.vocab_in - 1, dtype=torch.long, device=d)
    cx = torch.from_numpy(gt["ctx"]).to(d).contiguous(); ut = torch.from_numpy(gt["uniforms"]).to(d).contiguous()
    a = _lib.RarmSampleArgs(batch=B, k=cx.shape[1], cond_len=1, steps=steps, temperature=1.0, top_k=50, guidance_scale=1.0)
    toks = torch.full((B, steps), -7, device=d, dtype=torch.int64)
    rc = _lib.lib.rdm_rarm_sample_top_p(ctx._h, C.byref(a), bad, _lib._ptr(cond), _lib._ptr(cx), _lib._ptr(ut), _lib._ptr(toks))
    msg = _lib.lib.rdm_last_error(ctx._h).decode()
    assert rc == -1 and "top_p" in msg and "rdm_rarm_sample_top_p" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((toks == -7).all())
    with pytest.raises(_lib.RdmError, match="top_p"):
        ctx.op_rarm_sampler(g, u, top_k=256, top_p=bad)
    with pytest.raises(_lib.RdmError, match="top_p"):
        ctx.rarm_sample(cond, cx, steps, ut, top_k=50, top_p=bad)
    tok, k = _op(ctx, g, None, u, 1.0, 1.0, 256, 0.9)          # the context is usable afterwards
    assert int(tok.min()) >= 0 and int(tok.max()) < V and int(k.min()) >= 1
    assert ctx.rarm_sample(cond, cx, steps, ut, top_k=50, top_p=0.9).shape == (B, steps)
