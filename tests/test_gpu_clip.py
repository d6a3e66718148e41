"""The CLIP towers (rdm_clip_encode_text / rdm_clip_encode_image: the query of every retrieval) held to per-stage, per-element references.

  * TEACHER-FORCED, stage by stage: one forward per rdm_debug_tap key (blocks 2000 / 3000, include/rdm_hip.h); every GEMM, LayerNorm and
    attention output is compared with the float64 restatement of its op ON THE LIBRARY'S OWN tapped inputs under the per-element bound of
    tests/_fwd_ref.py, near misses included (tests/_clip_ref.py; pinned without a GPU by tests/test_clip_emul_cpu.py);
  * the glue kernels (token + positional embedding, EOT gather, patch matrix, cls | patches + positional, cls gather) BITWISE -- an fp32
    add and a copy have one correct answer -- at B = 3 and at the smallest batch that sends each kernel's grid-stride loop on a second trip;
  * rdm_set_deterministic's promise on the towers: a sample's embedding bitwise independent of the batch it is computed in;
  * the argument checks in front of the embedding kernel, which indexes its table by the token id as given.
The whole-tower fp32 goldens (tests/test_gpu_models.py, test_gpu_full.py: 2e-2) stay as they are."""
import ctypes

import pytest
import torch

import _clip_ref as CR
from oracle import clip as oclip, unet as ounet
from oracle.clip_emul import IMAGE, TEXT, clip_image_emulated, clip_text_emulated, eot_columns, patchify

from _util import rel_l2, spec_to_clip_cfg

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
torch.set_num_threads(min(16, torch.get_num_threads()))
B = 3


@pytest.fixture(scope="module")
def tiny(ctx):
    from rdm_amd import packing
    spec = oclip.tiny_clip_spec()
    sd = ounet.synth_state_dict(oclip.clip_param_shapes(spec), seed=11)
    cfg = spec_to_clip_cfg(spec)
    ctx.load_clip(cfg, packing.pack("clip", cfg, sd))
    yield ctx, spec, sd
    ctx.debug_tap(None, -1)


def _tap(ctx, run, key, shape, dtype):
    """one forward with the tap on `key` -> the stage on the CPU, in the type the library stores it in"""
    buf = torch.full(shape, float("nan"), device=ctx.device, dtype=dtype)      # (a tap that never fires leaves NaN, not a stale stage)
    ctx.debug_tap(buf, key[0], key[1])
    try:
        run()
        torch.cuda.synchronize()
    finally:
        ctx.debug_tap(None, -1)
    out = buf.cpu()
    assert not torch.isnan(out).any(), f"tap {key}: not (wholly) written"
    return out


def _library_stages(ctx, spec, tower, run, nb):
    return {key: _tap(ctx, run, key, (rows, width), dt) for key, (rows, width, dt) in CR.tap_shapes(spec, tower, nb).items()}


def _image(spec, nb, seed=6, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(nb, 3, spec.image_resolution, spec.image_resolution, generator=g, device=device)


# ---------------------------------------------------------------------------------------------------- stage by stage
def test_text_tower_stage_by_stage(tiny):
    ctx, spec, sd = tiny
    tokens = CR.text_tokens(spec, B)
    dev_tokens = tokens.to(ctx.device)
    out = ctx.clip_encode_text(dev_tokens)
    lib = _library_stages(ctx, spec, TEXT, lambda: ctx.clip_encode_text(dev_tokens), B)
    rep = CR.check_text_stages(sd, spec, tokens, lib)
    print("[clip] text tower, teacher-forced on the library's own taps:\n" + CR.summary(rep))
    assert torch.equal(lib[(TEXT, 4)], out.cpu()), "the last tap is the embedding the call returns"
    e = rel_l2(out, clip_text_emulated(sd, spec, tokens))
    print(f"[clip] text embedding, library vs its free-running restatement: {e:.3e}")
    assert e <= 2e-2


def test_image_tower_stage_by_stage(tiny):
    ctx, spec, sd = tiny
    image = _image(spec, B)
    dev_image = image.to(ctx.device)
    out = ctx.clip_encode_image(dev_image)
    lib = _library_stages(ctx, spec, IMAGE, lambda: ctx.clip_encode_image(dev_image), B)
    rep = CR.check_image_stages(sd, spec, image, lib)
    print("[clip] image tower, teacher-forced on the library's own taps:\n" + CR.summary(rep))
    assert torch.equal(lib[(IMAGE, 7)], out.cpu()), "the last tap is the embedding the call returns"
    e = rel_l2(out, clip_image_emulated(sd, spec, image))
    print(f"[clip] image embedding, library vs its free-running restatement: {e:.3e}")
    assert e <= 2e-2


def test_tap_is_clipped_to_its_buffer_and_off_means_off(tiny):
    ctx, spec, sd = tiny
    tokens = CR.text_tokens(spec, B).to(ctx.device)
    plain = ctx.clip_encode_text(tokens)
    key, rows, Wd = (TEXT, 16 + 4), B * spec.context_length, spec.transformer_width
    whole = _tap(ctx, lambda: ctx.clip_encode_text(tokens), key, (rows, Wd), torch.float32)
    # a buffer of 10 rows inside a larger tensor: the rows behind it keep their sentinel
    big = torch.full((rows, Wd), -7.0, device=ctx.device)
    ctx.debug_tap(big[:10], key[0], key[1])
    try:
        tapped = ctx.clip_encode_text(tokens)
        torch.cuda.synchronize()
    finally:
        ctx.debug_tap(None, -1)
    assert torch.equal(big[:10].cpu(), whole[:10]) and bool((big[10:] == -7.0).all())
    assert torch.equal(tapped, plain), "a tap changes no result"
    # off: the next forward writes nothing
    big.fill_(-7.0)
    again = ctx.clip_encode_text(tokens)
    torch.cuda.synchronize()
    assert bool((big == -7.0).all()) and torch.equal(again, plain)
    # a key of the other tower never fires
    ctx.debug_tap(big, IMAGE, 16 + 4)
    try:
        ctx.clip_encode_text(tokens)
        torch.cuda.synchronize()
    finally:
        ctx.debug_tap(None, -1)
    assert bool((big == -7.0).all())


# ---------------------------------------------------------------------------------------------------- glue kernels at a second trip
def test_text_glue_kernels_bitwise_on_a_second_grid_stride_trip(tiny):
    """B = 107: 107 * 77 * 128 elements > 4096 blocks * 256 threads, the embedding kernel's cap; one block per sequence in the EOT gather"""
    ctx, spec, sd = tiny
    nb, L, Wd = 107, spec.context_length, spec.transformer_width
    assert nb * L * Wd > 4096 * 256 >= (nb - 1) * L * Wd
    tokens = CR.text_tokens(spec, nb, seed=9)
    assert len(set(eot_columns(tokens).tolist())) > 50
    dev = tokens.to(ctx.device)
    run = lambda: ctx.clip_encode_text(dev)
    emb = _tap(ctx, run, (TEXT, 1), (nb * L, Wd), torch.float32)
    want = (sd["token_embedding.weight"][tokens] + sd["positional_embedding"]).reshape(nb * L, Wd)
    assert torch.equal(emb, want), f"{int((emb != want).sum())} elements of the embedding differ"
    last = _tap(ctx, run, (TEXT, 16 * spec.transformer_layers + 7), (nb * L, Wd), torch.float32)
    eot = _tap(ctx, run, (TEXT, 2), (nb, Wd), torch.float32)
    assert torch.equal(eot, last.reshape(nb, L, Wd)[torch.arange(nb), tokens.argmax(dim=-1)])


def test_patch_matrix_bitwise_on_a_second_grid_stride_trip(tiny):
    """B = 171: 171 * 4 * 3072 elements > 8192 blocks * 256 threads"""
    ctx, spec, sd = tiny
    nb, P = 171, spec.vision_patch_size
    GG, K = (spec.image_resolution // P) ** 2, 3 * P * P
    assert nb * GG * K > 8192 * 256 >= (nb - 1) * GG * K
    image = _image(spec, nb, seed=10, device=ctx.device)
    got = _tap(ctx, lambda: ctx.clip_encode_image(image), (IMAGE, 1), (nb * GG, K), torch.bfloat16)
    want = patchify(image.cpu(), P).to(torch.bfloat16)
    assert torch.equal(got, want), f"{int((got != want).sum())} elements of the patch matrix differ"


def test_assemble_and_cls_gather_bitwise_on_a_second_grid_stride_trip(tiny):
    """assemble: B = 1639 (1639 * 5 * 128 elements > 4096 * 256); cls gather: B = 2049 (2049 * 128 > 1024 * 256)"""
    ctx, spec, sd = tiny
    Wd = spec.vision_width
    GG = (spec.image_resolution // spec.vision_patch_size) ** 2
    nb = 1639
    assert nb * (GG + 1) * Wd > 4096 * 256 >= (nb - 1) * (GG + 1) * Wd
    image = _image(spec, nb, seed=11, device=ctx.device)
    run = lambda: ctx.clip_encode_image(image)
    pe = _tap(ctx, run, (IMAGE, 2), (nb * GG, Wd), torch.float32)
    x0 = _tap(ctx, run, (IMAGE, 3), (nb * (GG + 1), Wd), torch.float32)
    want = torch.cat([sd["visual.class_embedding"].expand(nb, 1, Wd), pe.reshape(nb, GG, Wd)], 1) + sd["visual.positional_embedding"]
    assert torch.equal(x0, want.reshape(-1, Wd)), f"{int((x0 != want.reshape(-1, Wd)).sum())} elements of cls | patches + positional differ"
    nb = 2049
    assert nb * Wd > 1024 * 256 >= (nb - 1) * Wd
    image = _image(spec, nb, seed=12, device=ctx.device)
    last = _tap(ctx, run, (IMAGE, 16 * spec.vision_layers + 7), (nb * (GG + 1), Wd), torch.float32)
    cls = _tap(ctx, run, (IMAGE, 5), (nb, Wd), torch.float32)
    assert torch.equal(cls, last.reshape(nb, GG + 1, Wd)[:, 0])


# ---------------------------------------------------------------------------------------------------- deterministic mode
def test_deterministic_mode_makes_an_embedding_independent_of_its_batch(tiny):
    """include/rdm_hip.h rdm_set_deterministic: 'a sample's result is bitwise independent of the batch it is computed in'.  Text: 77, 154,
    308 rows; image: 5, 150, 300 rows -- across the 128-row skinny rule and the 128 / 256-row tiles of the towers' linears."""
    ctx, spec, sd = tiny
    was = ctx.deterministic
    ctx.set_deterministic(True)
    try:
        tokens = CR.text_tokens(spec, 4, seed=21).to(ctx.device)
        rows = {nb: ctx.clip_encode_text(tokens[:nb].contiguous())[0].cpu() for nb in (1, 2, 4)}
        for nb in (2, 4):
            assert torch.equal(rows[1], rows[nb]), f"text: sample 0 at batch {nb} differs from batch 1 in {int((rows[1] != rows[nb]).sum())} elements"
        image = _image(spec, 60, seed=22, device=ctx.device)
        rows = {nb: ctx.clip_encode_image(image[:nb].contiguous())[0].cpu() for nb in (1, 30, 60)}
        for nb in (30, 60):
            assert torch.equal(rows[1], rows[nb]), f"image: sample 0 at batch {nb} differs from batch 1 in {int((rows[1] != rows[nb]).sum())} elements"
    finally:
        ctx.set_deterministic(was)
    assert ctx.deterministic == was


def test_deterministic_mode_across_the_tall_tile_rule(tiny):
    """The tiled GEMM goes from 128- to 256-row tiles once 256-row tiles fill the chip (igemm.hip launch_igemm: ceil(M / 256) column-tile
    rows x column tiles >= 256): at the tiny text width from 16129 rows on for c_fc (four 128-wide column tiles) and 32513 for q|k|v (two
    192-wide), i.e. between 200 and 423 sequences.  A row's sums must not notice."""
    ctx, spec, sd = tiny
    nb = 423
    assert nb * spec.context_length > 32513
    was = ctx.deterministic
    ctx.set_deterministic(True)
    try:
        tokens = CR.text_tokens(spec, nb, seed=23).to(ctx.device)
        one = ctx.clip_encode_text(tokens[:1].contiguous())[0].cpu()
        many = ctx.clip_encode_text(tokens)[0].cpu()
    finally:
        ctx.set_deterministic(was)
    assert torch.equal(one, many), f"sample 0 at batch {nb} differs from batch 1 in {int((one != many).sum())} elements"


# ---------------------------------------------------------------------------------------------------- refusals
def test_token_ids_outside_the_vocabulary_and_empty_batches_are_refused(tiny):
    from rdm_amd import _lib
    ctx, spec, sd = tiny
    V, L = spec.vocab_size, spec.context_length
    good = CR.text_tokens(spec, B)
    before = ctx.clip_encode_text(good.to(ctx.device)).cpu()
    for bad in (V, -1):
        t = good.clone(); t[1, 5] = bad
        with pytest.raises(_lib.RdmError, match=rf"tokens must lie in \[0, {V}\)"):
            ctx.clip_encode_text(t.to(ctx.device))
    # b = 0: refused by the C entries themselves (the binding has nothing to check on an empty batch)
    out = torch.empty((1, spec.embed_dim), device=ctx.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    dev_good = good.to(ctx.device)
    assert _lib.lib.rdm_clip_encode_text(ctx._h, ptr(dev_good), 0, ptr(out)) != 0
    assert "at least one" in _lib.lib.rdm_last_error(ctx._h).decode()
    image = _image(spec, 1, device=ctx.device)
    assert _lib.lib.rdm_clip_encode_image(ctx._h, ptr(image), 0, ptr(out)) != 0
    assert "at least one" in _lib.lib.rdm_last_error(ctx._h).decode()
    with pytest.raises(_lib.RdmError, match="at least one"):
        ctx.clip_encode_text(torch.zeros((0, L), dtype=torch.long, device=ctx.device))
    # the last valid id passes, and the context works afterwards
    t = good.clone(); t[1, 5] = V - 1
    assert torch.isfinite(ctx.clip_encode_text(t.to(ctx.device))).all()
    assert torch.equal(ctx.clip_encode_text(dev_good).cpu(), before)
