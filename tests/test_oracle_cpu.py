"""CPU suite: the oracle against the golden vectors generated from the reference's in-tree classes
(tools/gen_golden.py) and against the known-answer schedule constants of SURVEY.md appendix C."""
import numpy as np
import pytest
import torch

from oracle import clip as oclip
from oracle import diffusion as odiff
from oracle import retrieval as oret
from oracle import unet as ounet
from oracle import vqdecoder as ovq

from _util import golden

torch.set_grad_enabled(False)


def test_unet_tiny_matches_reference_golden():
    g = golden("unet_tiny.npz")
    spec = ounet.tiny_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=int(g["seed"]))
    y = ounet.unet_forward(sd, spec, torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g["ctx"]))
    assert np.abs(y.numpy() - g["eps"]).max() <= 5e-5


def test_unet_shipped_param_count_and_blocks():
    spec = ounet.shipped_spec()
    shapes = ounet.param_shapes(spec)
    assert sum(int(np.prod(s)) for s in shapes.values()) == 400_920_579
    assert len(shapes) == 688
    n_res = sum(1 for _, ls in spec.blocks for l in ls if l[0] == "res")
    n_st = sum(1 for _, ls in spec.blocks for l in ls if l[0] == "st")
    assert (n_res, n_st) == (22, 16)
    heads = [l[2] for _, ls in spec.blocks for l in ls if l[0] == "st"]
    assert heads == [12, 12, 18, 18, 30, 30, 30, 30, 30, 30, 18, 18, 18, 12, 12, 12]   # demo_rdm.ipynb:112-127


def test_attention_golden():
    g = golden("attention.npz")
    C, heads = 128, 4
    shapes_st = {"st.norm.weight": (C,), "st.norm.bias": (C,)}
    # rebuild the exact shapes dict the generator used (names from the reference module)
    tb = "transformer_blocks.0"
    names = {f"norm.weight": (C,), "norm.bias": (C,), "proj_in.weight": (C, C, 1, 1), "proj_in.bias": (C,),
             f"{tb}.attn1.to_q.weight": (C, C), f"{tb}.attn1.to_k.weight": (C, C), f"{tb}.attn1.to_v.weight": (C, C),
             f"{tb}.attn1.to_out.0.weight": (C, C), f"{tb}.attn1.to_out.0.bias": (C,),
             f"{tb}.ff.net.0.proj.weight": (8 * C, C), f"{tb}.ff.net.0.proj.bias": (8 * C,),
             f"{tb}.ff.net.2.weight": (C, 4 * C), f"{tb}.ff.net.2.bias": (C,),
             f"{tb}.attn2.to_q.weight": (C, C), f"{tb}.attn2.to_k.weight": (C, 512), f"{tb}.attn2.to_v.weight": (C, 512),
             f"{tb}.attn2.to_out.0.weight": (C, C), f"{tb}.attn2.to_out.0.bias": (C,),
             f"{tb}.norm1.weight": (C,), f"{tb}.norm1.bias": (C,), f"{tb}.norm2.weight": (C,), f"{tb}.norm2.bias": (C,),
             f"{tb}.norm3.weight": (C,), f"{tb}.norm3.bias": (C,), "proj_out.weight": (C, C, 1, 1), "proj_out.bias": (C,)}
    sd = ounet.synth_state_dict(names, seed=int(g["seed"]))
    y = ounet.spatial_transformer({"st." + k: v for k, v in sd.items()}, "st", torch.from_numpy(g["st_x"]),
                                  torch.from_numpy(g["st_ctx"]), heads)
    assert np.abs(y.numpy() - g["st_y"]).max() <= 2e-5 * max(1.0, np.abs(g["st_y"]).max())


def test_clip_tiny_golden():
    g = golden("clip_tiny.npz")
    spec = oclip.tiny_clip_spec()
    sd = ounet.synth_state_dict(oclip.clip_param_shapes(spec), seed=int(g["seed"]))
    sd["positional_embedding"] = sd["positional_embedding"] * 0.1
    t = oclip.encode_text(sd, spec, torch.from_numpy(g["tokens"]))
    i = oclip.encode_image(sd, spec, torch.from_numpy(g["image"]))
    assert np.abs(t.numpy() - g["text_out"]).max() <= 5e-5
    assert np.abs(i.numpy() - g["image_out"]).max() <= 5e-5


def test_schedule_known_answers():
    """SURVEY.md appendix C."""
    s = odiff.Schedule()
    ac = s.alphas_cumprod.double().numpy()
    for idx, val in ((0, 0.9985), (1, 0.996994427069975), (21, 0.9657320290842367), (500, 0.11492200085532281),
                     (981, 2.0195601706088703e-4), (999, 1.4230397519201791e-4)):
        assert abs(ac[idx] - val) <= 2e-7 * max(val, 1e-3)
    ts, a_t, a_prev, sigma, s1m = odiff.ddim_schedule(s, 50, 0.0)
    assert ts[0] == 1 and ts[-1] == 981 and len(ts) == 50 and ts[1] == 21
    assert odiff.make_ddim_timesteps(100)[-1] == 991 and odiff.make_ddim_timesteps(250)[-1] == 997
    assert abs(float(a_prev[0]) - 0.9985) < 1e-6 and abs(float(a_prev[49]) - 2.9478561805828586e-4) < 1e-9
    assert float(sigma.abs().max()) == 0.0
    _, _, _, sig1, _ = odiff.ddim_schedule(s, 50, 1.0)
    assert abs(float(sig1[0]) - 0.02743208756763818) < 1e-6 and abs(float(sig1[49]) - 0.5611383276027714) < 1e-5
    assert abs(float(s.posterior_variance[1]) - 7.525194283185552e-4) < 1e-9
    assert abs(float(s.posterior_log_variance_clipped[0]) + 46.051701859880914) < 1e-4
    # one DDIM step, index 49, eta 0, x = 1, eps = 0.5
    x = torch.ones(1, 1, 1, 1)
    xp, x0 = odiff.p_sample_ddim(lambda x_, t_, c_: torch.full_like(x_, 0.5), x, None, torch.tensor([981]), 49,
                                 odiff.ddim_schedule(s, 50, 0.0))
    assert abs(float(x0) - 35.18726080835689) < 2e-3 and abs(float(xp) - 1.1040677094017173) < 1e-5


def test_exact_topk_ties_and_order():
    rng = np.random.default_rng(0)
    db = (rng.standard_normal((1000, 64)) * 0.45).astype(np.float16)
    db[500] = db[10]; db[700] = db[10]          # duplicates -> index tie-break
    dbn = oret.normalize_db(db)
    q = db[10:11].astype(np.float32)
    idx, sc = oret.exact_topk(dbn, oret.normalize_queries(q), 4, chunk=300)
    assert idx[0, :3].tolist() == [10, 500, 700]
    assert np.all(np.diff(sc[0]) <= 0)


def test_retro_cond_and_uint8():
    q = np.arange(8, dtype=np.float32).reshape(2, 4)
    r = np.arange(2 * 3 * 4, dtype=np.float16).reshape(2, 3, 4)
    rc = oret.assemble_retro_cond(q, r, 3)
    assert rc.shape == (2, 3, 4) and np.array_equal(rc[:, 0], q) and np.array_equal(rc[:, 1:], r[:, :2].astype(np.float32))
    assert np.array_equal(oret.assemble_retro_cond(q, r, 3, omit_query=True), r.astype(np.float32))
    uc = oret.unconditional_conditioning(np.ones(4, np.float32), (2, 3, 4), 0.0, 3)
    assert uc.shape == (2, 3, 4) and not uc.any()
    img = np.array([[[[-2.0, -1.0], [0.0, 0.999]]]], dtype=np.float32)
    assert oret.custom_to_np_uint8(img).reshape(-1).tolist() == [0, 0, 127, 254]


def test_tokenizer_known_answer_fixture():
    g = golden("tokenizer.npz")
    assert g["tokens"][0, :13].tolist() == [49406, 320, 900, 4298, 2337, 320, 8786, 267, 2870, 525, 7483, 49407, 0]


def test_vq_oracle_shapes_and_quantise():
    spec = ovq.tiny_vq_spec()
    sd = ounet.synth_state_dict(ovq.vq_param_shapes(spec), seed=5)
    z = torch.from_numpy(np.random.default_rng(1).standard_normal((1, 3, 16, 16)).astype(np.float32))
    img, idx = ovq.vq_decode(sd, spec, z, return_indices=True)
    assert img.shape == (1, 3, 64, 64) and idx.shape == (256,)
    e = sd["quantize.embedding.weight"]
    zf = z.permute(0, 2, 3, 1).reshape(-1, 3)
    d = ((zf[:, None] - e[None]) ** 2).sum(-1)
    assert (d.argmin(1) == idx).float().mean() > 0.99


# ---- full-size fixtures (tools/gen_golden_full.py): the oracle reproduces the stored reference values at the shipped size
def test_streaming_topk_equals_exact_topk():
    rng = np.random.default_rng(0)
    db = (rng.standard_normal((5000, 64)) * 0.45).astype(np.float16); db[4000] = db[3]; db[4999] = db[3]
    q = (rng.standard_normal((7, 64)) * 0.45).astype(np.float32); q[0] = db[3].astype(np.float32)
    dbn, qn = oret.normalize_db(db), oret.normalize_queries(q)
    want = oret.exact_topk(dbn, qn, 5)
    st = oret.StreamingTopK(qn, 5)
    for r0 in range(0, 5000, 1300):
        n = oret.StreamingTopK.normalize_chunk(torch.from_numpy(db[r0:r0 + 1300]))
        assert np.array_equal(n.numpy(), dbn[r0:r0 + 1300])
        st.push(n, r0)
    got = st.result()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_full_vq_golden_reproduces():
    g = golden("full_vq.npz")
    vs = ovq.shipped_vq_spec()
    sd = ounet.synth_state_dict(ovq.vq_param_shapes(vs), seed=int(g["seed"]))
    img, idx = ovq.vq_decode(sd, vs, torch.from_numpy(g["z"]), return_indices=True)
    assert np.array_equal(idx.numpy().astype(np.int32), g["indices"])
    assert np.abs(img.numpy() - g["image"].astype(np.float32)).max() <= 4e-3          # stored as fp16


def test_full_ddim_golden_first_step_reproduces():
    """One CFG step of the 50-step trajectory at the shipped size (the stored values come from the reference UNetModel class)."""
    g = golden("full_ddim_k4.npz")
    spec = ounet.shipped_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=1234)
    sched = odiff.Schedule()
    sch = odiff.ddim_schedule(sched, 50, 0.0)
    x_T, cond = torch.from_numpy(g["x_T"]), torch.from_numpy(g["cond"])
    assert np.array_equal(g["xin_0"], g["x_T"])
    t = torch.full((1,), int(sch[0][-1]), dtype=torch.long)
    x, px0 = odiff.p_sample_ddim(lambda x, t, c: ounet.unet_forward(sd, spec, x, t, c), x_T, cond, t, 49, sch, scale=2.0, uc=torch.zeros_like(cond))
    assert np.abs(x.numpy() - g["x_0"]).max() <= 1e-4 * np.abs(g["x_0"]).max()
    assert np.abs(px0.numpy() - g["px0_0"]).max() <= 1e-4 * np.abs(g["px0_0"]).max()


def test_rarm_oracle_matches_reference_golden():
    from oracle import rarm as orarm
    g = golden("rarm_tiny.npz")
    spec = orarm.tiny_rarm_spec()
    sd = ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=int(g["seed"]))
    y = orarm.rarm_forward(sd, spec, torch.from_numpy(g["tokens"]), torch.from_numpy(g["ctx"]))
    assert np.abs(y.numpy() - g["logits"]).max() <= 5e-5 * np.abs(g["logits"]).max() + 5e-5
    cond = torch.full((3, 1), spec.vocab_in - 1, dtype=torch.long)
    out, lg = orarm.rarm_sample(sd, spec, cond, torch.from_numpy(g["ctx"]), g["uniforms"].shape[0], torch.from_numpy(g["uniforms"]),
                                temperature=float(g["temperature"]), top_k=int(g["top_k"]), guidance_scale=float(g["guidance_scale"]))
    assert np.array_equal(out.numpy(), g["sampled"])


def test_vqgan_oracle_shapes():
    spec = ovq.vqgan_f16_spec()
    shapes = ovq.vq_param_shapes(spec)
    assert "decoder.up.4.attn.2.q.weight" in shapes and "decoder.up.3.attn.0.q.weight" not in shapes
    assert shapes["decoder.conv_in.weight"] == (512, 256, 3, 3) and shapes["quantize.embedding.weight"] == (16384, 256)


def test_bulk_topk_oracle_equals_exact_topk():
    rng = np.random.default_rng(1)
    db = (rng.standard_normal((6000, 64)) * 0.45).astype(np.float16); db[5000] = db[7]; db[5999] = db[7]
    q = (rng.standard_normal((300, 64)) * 0.45).astype(np.float32); q[3] = db[7].astype(np.float32)
    dbn, qn = oret.normalize_db(db), oret.normalize_queries(q)
    a = oret.exact_topk(dbn, qn, 20)
    b = oret.exact_topk_bulk(dbn, qn, 20, qblock=128, chunk=2048)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_emulated_unet_is_exact_algebra_without_rounding():
    """oracle/unet_emul.py restates the LIBRARY's arithmetic (bf16 storage points + its algebraic re-associations: per-sample G / U
    cross-attention, ff.net.2 x proj_out as one map, Upsample by output phase, SiLU folded into the time-embedding MLP, attn2's bias in
    attn1.to_out's start values for zero-neighbour rows).  With the rounding switched off those re-associations must reproduce the fp32
    oracle -- itself pinned bit for bit to the reference's classes -- to fp32 round-off: the emulator's algebra is verified without a GPU."""
    from oracle import unet as ounet
    from oracle.unet_emul import unet_forward_emulated
    spec = ounet.tiny_spec()
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=11)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 3, 16, 16, generator=g)
    t = torch.tensor([981, 981, 501, 21])
    ctx = torch.randn(4, 4, 512, generator=g) * 0.45
    ctx[2:] = 0                                                     # the unconditional half of a guided batch
    ref = ounet.unet_forward(sd, spec, x, t, ctx)
    for rows in (None, 2):                                          # generic path for every row / the zero-neighbour shortcut for rows 2, 3
        got = unet_forward_emulated(sd, spec, x, t, ctx, ctx_rows=rows, rounding=False)
        e = float((got - ref).norm() / ref.norm())
        assert e <= 2e-5, (rows, e)
    # and with the rounding on it sits where the library sits: a bf16 distance away, not further
    got = unet_forward_emulated(sd, spec, x, t, ctx, ctx_rows=2)
    e = float((got - ref).norm() / ref.norm())
    assert 1e-4 < e <= 2.5e-2, e


def test_emulated_unet_is_exact_algebra_at_a_non_square_size():
    """The same pin at latent 12 x 20 with self-attention at every level (240 / 60 / 15 tokens): 240 and 60 are no multiples of 32, where
    the restatement follows small_attention_kernel (fp32 probabilities), and every level is non-square with an odd width at the bottom --
    what tests/test_gpu_emul.py trusts the emulator for at sizes other than the training size."""
    from dataclasses import replace
    from oracle import unet as ounet
    from oracle.unet_emul import unet_forward_emulated
    spec = replace(ounet.tiny_spec(), attention_resolutions=(1, 2, 4))
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=12)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 12, 20, generator=g)
    t = torch.tensor([700, 33])
    ctx = torch.randn(2, 4, 512, generator=g) * 0.45
    ctx[1] = 0
    ref = ounet.unet_forward(sd, spec, x, t, ctx)
    taps = {}
    got = unet_forward_emulated(sd, spec, x, t, ctx, rounding=False, taps=taps)
    e = float((got - ref).norm() / ref.norm())
    assert e <= 2e-5, e
    assert {v.shape[1] for v in taps.values()} == {240, 60, 15}
    e = float((unet_forward_emulated(sd, spec, x, t, ctx) - ref).norm() / ref.norm())
    assert 1e-4 < e <= 2.5e-2, e


def test_emulated_vq_decoder_is_exact_algebra_at_a_non_square_size():
    """The decoder restatement at a 5 x 7 latent (35 tokens in the mid AttnBlock, odd widths 7 / 14 / 28), rounding off, against the fp32 oracle."""
    from oracle import unet as ounet, vqdecoder as ovq
    from oracle.vq_emul import vq_decode_emulated
    spec = ovq.tiny_vq_spec()
    sd = ounet.synth_state_dict(ovq.vq_param_shapes(spec), seed=5)
    z = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(6))
    ref = ovq.vq_decode(sd, spec, z, force_not_quantize=True)
    assert tuple(ref.shape) == (2, 3, 20, 28)
    got = vq_decode_emulated(sd, spec, z, force_not_quantize=True, rounding=False)
    e = float((got - ref).norm() / ref.norm())
    assert e <= 2e-5, e


def test_emulated_vq_decoder_is_exact_algebra_without_rounding():
    from oracle import unet as ounet, vqdecoder as ovq
    from oracle.vq_emul import vq_decode_emulated
    spec = ovq.tiny_vq_spec()
    sd = ounet.synth_state_dict(ovq.vq_param_shapes(spec), seed=5)
    z = torch.randn(2, 3, spec.z_res, spec.z_res, generator=torch.Generator().manual_seed(2))
    for fnq in (True, False):
        ref = ovq.vq_decode(sd, spec, z, force_not_quantize=fnq)
        got = vq_decode_emulated(sd, spec, z, force_not_quantize=fnq, rounding=False)
        e = float((got - ref).norm() / ref.norm())
        assert e <= 2e-5, (fnq, e)
    e = float((vq_decode_emulated(sd, spec, z, force_not_quantize=True) - ovq.vq_decode(sd, spec, z, force_not_quantize=True)).norm() / ref.norm())
    assert 1e-4 < e <= 2.5e-2, e


def test_winograd_restatement_is_exact_algebra_and_its_bf16_error_is_the_measured_one():
    """Round 6 (verdict item 1a): oracle/unet_emul.py's Winograd F(2x2, 3x3) conv -- the accuracy half of the Winograd decision, run on the CPU by
    tools/wino_accuracy.py -- equals F.conv2d with the rounding switched off, and with a fused bf16-MFMA kernel's roundings (bf16 U and V, fp32 sums and
    output transform) sits at ~4e-3 per conv on unit-scale data (the direct conv's single output rounding: 1.7e-3): profiles/r06_wino_accuracy.log."""
    import torch.nn.functional as F
    from oracle.unet_emul import wino_conv3x3, _R
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 64, 16, 16, generator=g); w = torch.randn(32, 64, 3, 3, generator=g) * (9 * 64) ** -0.5
    ref = F.conv2d(x, w, padding=1)
    assert float((wino_conv3x3(x, w, _R(False)) - ref).norm() / ref.norm()) <= 2e-6
    bf = lambda t: t.to(torch.bfloat16).float()
    xb, wb = bf(x), bf(w)
    refb = F.conv2d(xb, wb, padding=1)
    e1 = float((wino_conv3x3(xb, wb, _R(True)) - refb).norm() / refb.norm())
    e2 = float((wino_conv3x3(xb, wb, _R(True), two_stage=True) - refb).norm() / refb.norm())
    assert 2e-3 <= e1 <= 6e-3 and e1 <= e2 <= 7e-3

