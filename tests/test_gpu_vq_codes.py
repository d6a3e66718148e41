"""GPU suite of the VQGAN-f16 encode path through the C ABI: the nearest-code kernel (rdm_op_vq_nearest_code) against fp64 distances,
the wide-latent encoder (rdm_vq_encode) against the oracle, rdm_vq_encode_indices teacher-forced on the library's own latent, and
the LatentImageRETRO mirror's encode_to_z / log_images / image completion plus scripts/rarm_sample.py --complete_from.

Acceptance rule of an index (per row): idx == argmin of the fp64 distances, or
    d64[idx] - min d64 <= gamma [(|z| + |e_idx|)^2 + (|z| + |e_best|)^2],   gamma = (E + 3) 2^-24,
the worst-case fp32 evaluation error of the two distances for any summation order; at most 1 % of the rows may pass through the
tolerance clause.  Sequences are compared teacher-forced (one flipped index changes everything a sampler draws after it)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import rarm as orarm
from oracle import unet as ounet
from oracle import vqdecoder as ovq

from _util import rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ the kernel alone
def _codebook(N, E):
    return ounet.synth_state_dict({"quantize.embedding.weight": (N, E)}, seed=888)["quantize.embedding.weight"]


def _rows(e, M):
    """First half: codebook rows + 0.5 / sqrt(E) noise; second half: randn / sqrt(E)."""
    N, E = e.shape
    g = torch.Generator().manual_seed(5)
    h = M // 2
    pick = torch.randint(0, N, (h,), generator=g)
    near = e[pick] + 0.5 / np.sqrt(E) * torch.randn((h, E), generator=g)
    far = torch.randn((M - h, E), generator=g) / np.sqrt(E)
    return torch.cat([near, far]).contiguous()


def _judge(idx, z, e, what):
    """-> number of rows accepted through the tolerance clause; asserts the rule and the 1 % cap."""
    idx = idx.cpu().long()
    N, E = e.shape
    assert idx.shape == (z.shape[0],) and int(idx.min()) >= 0 and int(idx.max()) < N
    z64, e64 = z.double(), e.double()
    d = (z64 ** 2).sum(1, keepdim=True) + (e64 ** 2).sum(1) - 2 * z64 @ e64.t()
    best = d.argmin(1)
    exact = idx == best
    rows = torch.arange(z.shape[0])
    gap = d[rows, idx] - d[rows, best]
    zn, en_i, en_b = z64.norm(dim=1), e64[idx].norm(dim=1), e64[best].norm(dim=1)
    gamma = (E + 3) * 2.0 ** -24
    tol = gamma * ((zn + en_i) ** 2 + (zn + en_b) ** 2)
    ok = exact | (gap <= tol)
    n_tol = int((~exact).sum())
    print(f"{what}: {z.shape[0]} rows, {n_tol} not the fp64 arg-min (largest gap / tolerance {float((gap / tol).max()):.3g}), {int((~ok).sum())} outside the rule")
    assert bool(ok.all())
    assert n_tol <= 0.01 * z.shape[0]
    return n_tol


@pytest.fixture(scope="module")
def shipped_codebook():
    return _codebook(16384, 256)


def test_nearest_code_small(ctx):
    """(a) M = 192, N = 512, E = 64: two row tiles, four code tiles."""
    e = _codebook(512, 64); z = _rows(e, 192)
    idx = ctx.vq_nearest_code(z, e)
    assert idx.dtype == torch.int32
    _judge(idx, z, e, "nearest code 192 x 512 x 64")
    zq, ref = ovq.vq_quantize({"quantize.embedding.weight": e}, z.t().reshape(1, 64, 192, 1))
    print("  agreement with the fp32 oracle:", float((idx.cpu().long() == ref).float().mean()))


def test_nearest_code_shipped_codebook_with_code_split(ctx, shipped_codebook):
    """(b) M = 512, N = 16384, E = 256: the shipped codebook; four row tiles, so the 128 code tiles are split over the grid."""
    e = shipped_codebook; z = _rows(e, 512)
    idx = ctx.vq_nearest_code(z, e)
    _judge(idx, z, e, "nearest code 512 x 16384 x 256")
    zq, ref = ovq.vq_quantize({"quantize.embedding.weight": e}, z.t().reshape(1, 256, 512, 1))
    print("  agreement with the fp32 oracle:", float((idx.cpu().long() == ref).float().mean()))


def test_nearest_code_ragged_and_zero_rows(ctx):
    """(c) M = 70, N = 1000, E = 128: neither a multiple of the tile; two all-zero rows, which a zero-padded code (score 0) would win."""
    e = _codebook(1000, 128); z = _rows(e, 70)
    z[11] = 0; z[69] = 0
    idx = ctx.vq_nearest_code(z, e)
    _judge(idx, z, e, "nearest code 70 x 1000 x 128")
    want = int((e.double() ** 2).sum(1).argmin())
    assert int(idx[11]) == want and int(idx[69]) == want             # z = 0: the shortest code (its fp32 norm is unique here)
    # N = 1, M = 1
    assert ctx.vq_nearest_code(z[:1], e[:1]).tolist() == [0]


def test_nearest_code_non_finite_rows_stay_in_range(ctx):
    e = _codebook(1000, 128); z = _rows(e, 70)
    z[3, 5] = float("nan"); z[4, 0] = float("inf"); z[5] = float("-inf"); z[6] = 3e38
    idx = ctx.vq_nearest_code(z, e).cpu().long()
    assert int(idx.min()) >= 0 and int(idx.max()) < 1000
    keep = torch.ones(70, dtype=torch.bool); keep[3:7] = False
    clean = ctx.vq_nearest_code(z[keep], e).cpu().long()
    assert torch.equal(idx[keep], clean)                               # finite rows are not disturbed by their neighbours


@pytest.mark.parametrize("N,E", [(1024, 64), (16384, 256)])
def test_nearest_code_exact_ties_go_to_the_lowest_index(ctx, N, E, shipped_codebook):
    """(d) duplicated codebook rows straddling registers, lane halves, waves, code tiles and code splits; z = those rows: the LOWER index,
    at a row count where every code tile is its own split and at one where a block walks the whole codebook."""
    e = (shipped_codebook if N == 16384 else _codebook(N, E)).clone()
    pairs = [(3, N // 2 + 37), (N // 4 - 1, N - 1), (5, 70), (9, 13), (130, 131), (200, 200 + 128), (N // 2 - 1, N // 2)]
    for lo, hi in pairs:
        e[hi] = e[lo]
    lows = torch.tensor([p[0] for p in pairs])
    z = torch.cat([e[lows], e[torch.tensor([p[1] for p in pairs])]])
    want = torch.cat([lows, lows]).int()
    got = ctx.vq_nearest_code(z, e).cpu()
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    reps = 66000 // z.shape[0] + 1                                       # > 512 row tiles: one split
    big = ctx.vq_nearest_code(z.repeat(reps, 1), e).cpu()
    assert torch.equal(big, want.repeat(reps))


def test_nearest_code_is_bitwise_independent_of_the_batch(ctx, shipped_codebook):
    """(e) 256 rows alone (2 row tiles, every code tile its own split) and inside M = 4096 (32 row tiles, 16 splits): equal indices,
    no tolerance; two calls repeat."""
    e = shipped_codebook
    z = _rows(e, 4096)
    sel = slice(1000, 1256)                                              # straddles the near / far halves' row tiles unevenly
    whole = ctx.vq_nearest_code(z, e).cpu()
    alone = ctx.vq_nearest_code(z[sel].contiguous(), e).cpu()
    assert torch.equal(alone, whole[sel])
    assert torch.equal(whole, ctx.vq_nearest_code(z, e).cpu())
    odd = ctx.vq_nearest_code(z[7:200].contiguous(), e).cpu()            # a ragged count at another tile offset
    assert torch.equal(odd, whole[7:200])


def test_nearest_code_rejects_what_it_cannot_run(ctx):
    """(f) E = 96 and null pointers: an argument error, nothing launched (the output keeps its fill)."""
    from rdm_amd import _lib
    out = torch.full((8,), -7, dtype=torch.int32, device=ctx.device)
    z = torch.zeros(8, 96, device=ctx.device); e = torch.zeros(16, 96, device=ctx.device)
    rc = _lib.lib.rdm_op_vq_nearest_code(ctx._h, _lib._ptr(z), _lib._ptr(e), 8, 16, 96, _lib._ptr(out))
    assert rc != 0 and "96" in _lib.lib.rdm_last_error(ctx._h).decode()
    z = torch.zeros(8, 64, device=ctx.device); e = torch.zeros(16, 64, device=ctx.device)
    for args in ((None, _lib._ptr(e), 8, 16, 64, _lib._ptr(out)), (_lib._ptr(z), None, 8, 16, 64, _lib._ptr(out)), (_lib._ptr(z), _lib._ptr(e), 8, 16, 64, None),
                 (_lib._ptr(z), _lib._ptr(e), 0, 16, 64, _lib._ptr(out)), (_lib._ptr(z), _lib._ptr(e), 8, 16, 576, _lib._ptr(out))):
        assert _lib.lib.rdm_op_vq_nearest_code(ctx._h, *args) != 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    with pytest.raises(_lib.RdmError):
        ctx.vq_nearest_code(torch.zeros(8, 96), torch.zeros(16, 96))
    with pytest.raises(_lib.RdmError):
        ctx.vq_nearest_code(torch.zeros(8, 64), torch.zeros(16, 128))


# ------------------------------------------------------------------------------------------------ encoder and rdm_vq_encode_indices
def _vq_cfg(spec):
    from rdm_amd import _lib
    return _lib.make_vq_cfg(embed_dim=spec.embed_dim, n_embed=spec.n_embed, z_channels=spec.z_channels, ch=spec.ch, ch_mult=spec.ch_mult,
                            num_res_blocks=spec.num_res_blocks, resolution=spec.resolution, attn_resolutions=spec.attn_resolutions)


def _first_stage_sd(spec):
    shapes = dict(ovq.vq_param_shapes(spec)); shapes.update(ovq.vq_encoder_param_shapes(spec))
    return ounet.synth_state_dict(shapes, seed=888)


def _images(n, spec):
    return torch.from_numpy(np.random.default_rng(6).uniform(-1.0, 1.0, (n, 3, spec.resolution, spec.resolution)).astype(np.float32))


def _load_first_stage(ctx, spec, sd):
    from rdm_amd import packing
    cfg = _vq_cfg(spec)
    ctx.load_vq(cfg, packing.pack("vq", cfg, sd))
    ctx.load_vq_encoder(cfg, packing.pack("vqenc", cfg, sd))
    return cfg


@pytest.fixture(scope="module")
def tiny_stage():
    spec = ovq.tiny_vqgan_spec()
    return spec, _first_stage_sd(spec)


@pytest.mark.parametrize("which", ["tiny", "f16"])
def test_vq_encode_and_encode_indices(ctx, which, tiny_stage):
    """Bounds: the project's for the VQ-f4 encoder (2.5e-2) and for the deeper f16 decoder (3.5e-2).  Measured on an MI355X: vq_encode rel L2
    against the fp32 oracle 1.00e-2 (tiny, B = 3) and 1.13e-2 (f16, B = 1); every index the fp64 arg-min of the native latent; agreement
    with the all-oracle indices (fp32 encoder -> quantise) 0.995 (tiny, 192 tokens) and 0.973 (f16, 256 tokens) -- reported, not asserted:
    the latent's bf16-path error moves near-tied tokens to a neighbouring code."""
    if which == "tiny":
        spec, sd = tiny_stage
        B, bound = 3, 2.5e-2
    else:
        spec = ovq.vqgan_f16_spec(); sd = _first_stage_sd(spec)
        B, bound = 1, 3.5e-2
    _load_first_stage(ctx, spec, sd)
    x = _images(B, spec)
    z = ctx.vq_encode(x).cpu()
    ref = ovq.vq_encode(sd, spec, x)
    e = rel_l2(z, ref)
    print(f"vqgan {which} vq_encode rel L2:", e)
    assert z.shape == ref.shape == (B, spec.embed_dim, spec.z_res, spec.z_res)
    assert e <= bound
    quant, idx = ctx.vq_encode_indices(x, return_quant=True)
    quant, idx = quant.cpu(), idx.cpu()
    assert idx.dtype == torch.int64 and idx.shape == (B, spec.z_res ** 2)
    assert torch.equal(idx, ctx.vq_encode_indices(x).cpu())
    cb = sd["quantize.embedding.weight"]
    flat = z.permute(0, 2, 3, 1).reshape(-1, spec.embed_dim)
    _judge(idx.reshape(-1), flat, cb, f"vqgan {which} encode_indices, teacher-forced on the native latent")
    _, forced = ovq.vq_quantize(sd, z)
    print("  agreement with the fp32 oracle quantiser on the native latent:", float((idx.reshape(-1) == forced).float().mean()))
    assert torch.equal(quant, cb[idx.reshape(-1)].reshape(B, spec.z_res, spec.z_res, spec.embed_dim).permute(0, 3, 1, 2))
    _, all_oracle = ovq.vq_quantize(sd, ref)
    print("  agreement with the all-oracle indices (fp32 encoder -> quantise):", float((idx.reshape(-1) == all_oracle).float().mean()))
    img = ctx.vq_decode_indices(idx).cpu()
    assert img.shape == x.shape and bool(torch.isfinite(img).all())


def test_encode_indices_needs_encoder_and_decoder_of_one_wide_cfg(tiny_stage):
    from rdm_amd import _lib, packing
    spec, sd = tiny_stage
    cfg = _vq_cfg(spec)
    c = _lib.Context(0)
    try:
        x = _images(1, spec)
        with pytest.raises(_lib.RdmError):
            c.vq_encode_indices(x)
        c.load_vq_encoder(cfg, packing.pack("vqenc", cfg, sd))
        with pytest.raises(_lib.RdmError, match="load_vq"):
            c.vq_encode_indices(x)
        other = _lib.make_vq_cfg(embed_dim=128, n_embed=64, z_channels=64, ch=spec.ch, ch_mult=spec.ch_mult, num_res_blocks=spec.num_res_blocks,
                                 resolution=spec.resolution, attn_resolutions=spec.attn_resolutions)
        from rdm_amd import synthetic
        c.load_vq(other, packing.pack("vq", other, synthetic.vq_state_dict(other, 1)))
        with pytest.raises(_lib.RdmError, match="different cfgs"):
            c.vq_encode_indices(x)
        c.load_vq(cfg, packing.pack("vq", cfg, sd))
        assert c.vq_encode_indices(x).shape == (1, spec.z_res ** 2)
        with pytest.raises(_lib.RdmError):
            c.vq_encode_indices(torch.zeros(1, 3, 16, 16))
    finally:
        c.close()


def test_encode_indices_rows_are_independent_of_the_batch(ctx, tiny_stage):
    spec, sd = tiny_stage
    _load_first_stage(ctx, spec, sd)
    x = _images(5, spec)
    five = ctx.vq_encode_indices(x).cpu()
    three = ctx.vq_encode_indices(x[:3]).cpu()
    print("tiny encode_indices, 3 images alone vs inside 5: differing indices", int((five[:3] != three).sum()))
    assert torch.equal(five[:3], three)


def test_encode_walked_in_sample_ranges(ctx, tiny_stage, tmp_path):
    """A child process with RDM_VQ_RANGE=2 encodes 5 tiny images in ranges of 2, 2, 1: the indices and the latent of the one-range call."""
    spec, sd = tiny_stage
    _load_first_stage(ctx, spec, sd)
    x = _images(5, spec)
    whole = ctx.vq_encode_indices(x).cpu()
    whole_z = ctx.vq_encode(x).cpu()
    out = tmp_path / "ranges.npz"
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, numpy as np, torch\n"
        f"sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})\n"
        "import rdm_amd\nfrom rdm_amd import _lib, packing\nfrom oracle import vqdecoder as ovq, unet as ounet\n"
        "torch.set_grad_enabled(False)\nctx = _lib.Context(0)\nspec = ovq.tiny_vqgan_spec()\n"
        "shapes = dict(ovq.vq_param_shapes(spec)); shapes.update(ovq.vq_encoder_param_shapes(spec))\n"
        "sd = ounet.synth_state_dict(shapes, seed=888)\n"
        "cfg = _lib.make_vq_cfg(embed_dim=spec.embed_dim, n_embed=spec.n_embed, z_channels=spec.z_channels, ch=spec.ch, ch_mult=spec.ch_mult,\n"
        "                       num_res_blocks=spec.num_res_blocks, resolution=spec.resolution, attn_resolutions=spec.attn_resolutions)\n"
        "ctx.load_vq(cfg, packing.pack('vq', cfg, sd)); ctx.load_vq_encoder(cfg, packing.pack('vqenc', cfg, sd))\n"
        "x = torch.from_numpy(np.random.default_rng(6).uniform(-1.0, 1.0, (5, 3, spec.resolution, spec.resolution)).astype(np.float32))\n"
        "quant, idx = ctx.vq_encode_indices(x, return_quant=True)\n"
        f"np.savez({str(out)!r}, idx=idx.cpu().numpy(), quant=quant.cpu().numpy(), z=ctx.vq_encode(x).cpu().numpy())\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RDM_VQ_RANGE="2"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    print("encode in ranges of 2 vs one range of 5: differing indices", int((torch.from_numpy(got["idx"]) != whole).sum()),
          "latent rel L2", rel_l2(torch.from_numpy(got["z"]), whole_z))
    assert torch.equal(torch.from_numpy(got["idx"]), whole)
    cb = sd["quantize.embedding.weight"]
    assert torch.equal(torch.from_numpy(got["quant"]), cb[whole.reshape(-1)].reshape(5, spec.z_res, spec.z_res, spec.embed_dim).permute(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------ mirror and script
def _mirror(ctx, tiny_stage):
    from rdm_amd.models.autoregression.transformer import LatentImageRETRO
    vspec, fsd = tiny_stage
    spec = orarm.RarmSpec(vocab_in=514, vocab_out=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64)
    tcfg = {"params": dict(in_channels=spec.vocab_in, out_channels=spec.vocab_out, n_heads=spec.n_heads, d_head=64, depth=spec.depth,
                           context_dim=512, sequence_length=spec.sequence_length, continuous=False, causal=True)}
    fcfg = {"params": {"embed_dim": 64, "n_embed": 512, "ddconfig": {"z_channels": 64, "ch": 64, "ch_mult": vspec.ch_mult, "num_res_blocks": 1,
                                                                   "resolution": 32, "attn_resolutions": vspec.attn_resolutions}}}
    m = LatentImageRETRO(tcfg, fcfg, mask_token=512, sos_token=513, k_nn=4, ctx=ctx)
    m.load_transformer_state_dict(ounet.synth_state_dict(orarm.rarm_param_shapes(spec), seed=777))
    m.load_first_stage_state_dict(fsd)                                  # carries encoder.* keys: the encoder is loaded too
    rng = np.random.default_rng(21)
    batch = {"image": _images(4, vspec).permute(0, 2, 3, 1).contiguous(), "nn_embeddings": torch.from_numpy((rng.standard_normal((4, 4, 512)) * 0.45).astype(np.float32))}
    return m, batch


def test_log_images_surface_and_seeded_repeat(ctx, tiny_stage):
    m, batch = _mirror(ctx, tiny_stage)
    assert ctx.vqenc_cfg is not None
    quant_z, idx = m.encode_to_z(batch["image"].permute(0, 3, 1, 2))
    assert quant_z.shape == (4, 64, 8, 8) and idx.shape == (4, 64)
    rec = m.decode_to_img(idx, quant_z.shape)
    assert rec.shape == (4, 3, 32, 32) and bool(torch.isfinite(rec).all())
    logs = []
    for _ in range(2):
        torch.manual_seed(4); torch.cuda.manual_seed_all(4); np.random.seed(4)
        logs.append({k: v.cpu() for k, v in m.log_images(batch, N=3, top_k=50).items()})
    assert sorted(logs[0]) == ["inputs", "reconstructions", "samples_full", "samples_full_p_0.50", "samples_full_p_1.00", "samples_half"]
    for k, v in logs[0].items():
        assert v.shape == (3, 3, 32, 32) and bool(torch.isfinite(v).all()), k
        assert torch.equal(v, logs[1][k]), k
    assert torch.equal(logs[0]["inputs"], batch["image"][:3].permute(0, 3, 1, 2))
    three = m.decode_to_img(m.encode_to_z(batch["image"][:3].permute(0, 3, 1, 2))[1]).cpu()      # the same calls at the same batch
    assert torch.equal(logs[0]["reconstructions"], three)
    assert not torch.equal(logs[0]["samples_full"], logs[0]["samples_full_p_1.00"])      # other neighbours (all mask token), other draws


def test_completion_is_greedy_decoding_behind_the_given_prefix(ctx, tiny_stage):
    """Arg-max completion of the last 32 of 64 codes: teacher-fed with [sos | z[:, :32] | out[:-1]], the transformer's arg-max at every
    completed position is the token the sampling loop emitted.  Where it is not, the two logits must be a near-tie: within 4e-2 of the
    row's logit RMS (twice the project's 2e-2 logits bound for the bf16 decode path, one for each of the two tokens)."""
    m, batch = _mirror(ctx, tiny_stage)
    x = batch["image"].permute(0, 3, 1, 2)
    r = batch["nn_embeddings"].to(ctx.device)
    _, z = m.encode_to_z(x)
    _, c = m.encode_to_c(torch.zeros((4, 0)))
    out = m.sample(z[:, :32], r, c, steps=32)
    assert out.shape == (4, 64) and torch.equal(out[:, :32], z[:, :32])
    assert int(out.min()) >= 0 and int(out.max()) < 512
    seq = torch.cat([c.to(ctx.device), out[:, :-1]], dim=1)
    lg = ctx.rarm_forward(seq, r)[:, 32:]                                # logits that predict positions 32 .. 63
    greedy = lg.argmax(-1)
    differ = greedy != out[:, 32:]
    print("completion: positions whose teacher-forced arg-max is another token:", int(differ.sum()), "of", differ.numel())
    if bool(differ.any()):
        top = lg.max(-1).values; mine = lg.gather(-1, out[:, 32:, None])[..., 0]; rms = lg.pow(2).mean(-1).sqrt()
        assert bool(((top - mine)[differ] <= 4e-2 * rms[differ]).all())
    again = m.sample(z[:, :32], r, c, steps=32)
    assert torch.equal(again, out)


def _rarm_script():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "rarm_sample.py")
    spec = importlib.util.spec_from_file_location("rarm_sample_native_complete", path)
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_rarm_sample_script_complete_from(tmp_path):
    """scripts/rarm_sample.py --synthetic --complete_from on the shipped architecture: two images -> CLIP image embedding -> retrieval ->
    VQGAN-f16 encode -> the first 8 code rows kept, 128 tokens sampled -> decode; the four PNGs at 256 x 256."""
    from PIL import Image
    src = tmp_path / "src"; src.mkdir()
    rng = np.random.default_rng(12)
    for i, (h, w) in enumerate(((300, 400), (256, 256))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / f"im{i}.png")
    dst = tmp_path / "out"; dst.mkdir()
    mod = _rarm_script()
    opt = mod.parse_args(["--synthetic", "--synthetic_db_rows", "20000", "--gpu", "0", "-bs", "2", "-n", "1", "--seed", "7", "--complete_from", str(src),
                          "-s", str(dst)])
    model = mod.load_model(opt)
    stamp = mod.sample(model, opt)
    files = sorted(p.name for p in dst.iterdir())
    assert files == sorted(f"{stamp}-{key}-run0-sample{i}.png" for key in ("samples_half", "reconstructions") for i in range(2))
    px = {f: np.asarray(Image.open(dst / f)) for f in files}
    assert all(v.shape == (256, 256, 3) and v.dtype == np.uint8 for v in px.values())
    assert len(np.unique(px[files[0]])) > 16
    model.ctx.close()
