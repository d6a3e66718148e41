"""Error behaviour of the C ABI (include/rdm_hip.h: every entry returns 0 or a negative code and leaves a message in rdm_last_error)
and of the ctypes binding's argument checks: calls before weights / database are loaded, wrong shapes, out-of-range k / S / positions,
blobs that do not match the manifest -- and the context stays usable after every one of them."""
import numpy as np
import pytest
import torch

from oracle import rarm as orarm
from oracle import unet as ounet
from oracle import vqdecoder as ovq

from _util import spec_to_unet_cfg, spec_to_vq_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture()
def fresh():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _err(fn):
    from rdm_amd._lib import RdmError
    with pytest.raises(RdmError) as e:
        fn()
    msg = str(e.value)
    assert len(msg) > 20, msg                   # code + a real message, not an empty string
    return msg


def test_calls_before_load_fail_with_a_message(fresh):
    d = fresh.device
    x = torch.zeros(1, 3, 16, 16, device=d); t = torch.zeros(1, dtype=torch.long, device=d); c = torch.zeros(1, 4, 512, device=d)
    assert "not loaded" in _err(lambda: fresh.unet_forward(x, t, c))
    assert "not loaded" in _err(lambda: fresh.vq_decode(x))
    assert "no database" in _err(lambda: fresh.knn(torch.zeros(2, 512, device=d), 4))
    assert "no database" in _err(lambda: fresh.db_gather(torch.zeros(2, 4, dtype=torch.int32, device=d), 512))
    _err(lambda: fresh.clip_encode_text(torch.zeros(1, 77, dtype=torch.long, device=d)))
    _err(lambda: fresh.rarm_forward(torch.zeros(1, 4, dtype=torch.long, device=d), torch.zeros(1, 2, 512, device=d)))


def test_knn_argument_checks(fresh):
    d = fresh.device
    g = torch.Generator(device=d).manual_seed(1)
    db = torch.randn(1000, 512, device=d, generator=g).half()
    fresh.db_load(db)
    q = torch.randn(3, 512, device=d, generator=g)
    assert "k > 28" in _err(lambda: fresh.knn(q, 29))
    small = torch.randn(5, 512, device=d, generator=g).half()
    fresh.db_load(small)
    assert "exceeds" in _err(lambda: fresh.knn(q, 6))
    # still usable, and exact
    idx, sc = fresh.knn(q, 5)
    ref = (torch.nn.functional.normalize(q.double(), dim=1) @ torch.nn.functional.normalize(small.double(), dim=1).T).argsort(dim=1, descending=True)
    assert torch.equal(idx.cpu().long() & 0xffffffff, ref.cpu())


def test_blob_and_shape_mismatches(fresh):
    from rdm_amd import _lib, packing
    spec = ounet.tiny_spec()
    cfg = spec_to_unet_cfg(spec)
    sd = ounet.synth_state_dict(ounet.param_shapes(spec), seed=3)
    blob = packing.pack("unet", cfg, sd)
    assert "manifest" in _err(lambda: fresh.load_unet(cfg, blob[:-256]))
    fresh.load_unet(cfg, blob)
    d = fresh.device
    B, k = 2, 4
    x = torch.zeros(B, spec.in_channels, 16, 16, device=d); t = torch.zeros(B, dtype=torch.long, device=d)
    c = torch.zeros(B, k, spec.context_dim, device=d)
    fresh.unet_forward(x, t, c)                                            # fine
    _err(lambda: fresh.unet_forward(x, t, c[:, 0]))                        # [B, 512] instead of [B, k, 512]
    _err(lambda: fresh.unet_forward(x, t[:1], c))                          # timestep vector of the wrong length
    _err(lambda: fresh.unet_forward(x, t, c[:1]))                          # conditioning for a different batch
    ac = torch.linspace(0.999, 0.005, 1000)
    _err(lambda: fresh.ddim_sample(4, x, c, c[:, :2], ac, scale=2.0))      # unconditional conditioning with another k
    _err(lambda: fresh.ddim_sample(4, x, c, None, ac, eta=1.0, noise=torch.zeros(3, B, 3, 16, 16, device=d)))   # noise stack shorter than the loop
    assert "bad schedule" in _err(lambda: fresh.ddim_sample(0, x, c, None, ac, want_intermediates=True))   # S = 0 reaches the library
    z, _, _ = fresh.ddim_sample(4, x, c, None, ac)                         # and the context is still alive
    assert torch.isfinite(z).all()


def test_refused_load_leaves_the_loaded_model_usable(fresh):
    """A load that is refused -- here for its blob size -- changes nothing: the model loaded before gives the same bits afterwards.
    The refused cfg is the loaded one with one res block fewer per level, so a library that mixed the new layer graph with the old
    blob would still read inside the blob and write the same output sizes: it shows as unequal outputs."""
    from dataclasses import replace
    from rdm_amd import packing
    d = fresh.device
    g = torch.Generator().manual_seed(11)
    small = replace(ovq.tiny_vq_spec(), resolution=32); big = replace(small, num_res_blocks=small.num_res_blocks + 1)
    blob = packing.pack("vq", spec_to_vq_cfg(big), ounet.synth_state_dict(ovq.vq_param_shapes(big), seed=5))
    fresh.load_vq(spec_to_vq_cfg(big), blob)
    z = (torch.randn(2, 3, big.z_res, big.z_res, generator=g) * 0.6).to(d)
    img1 = fresh.vq_decode(z)
    assert "manifest" in _err(lambda: fresh.load_vq(spec_to_vq_cfg(small), blob))
    img2 = fresh.vq_decode(z)
    assert img1.shape == (2, 3, 32, 32) and torch.isfinite(img1).all() and float(img1.abs().max()) > 0
    assert torch.equal(img1, img2)

    small = ounet.tiny_spec(); big = replace(small, num_res_blocks=small.num_res_blocks + 1)
    blob = packing.pack("unet", spec_to_unet_cfg(big), ounet.synth_state_dict(ounet.param_shapes(big), seed=3))
    fresh.load_unet(spec_to_unet_cfg(big), blob)
    x = torch.randn(2, big.in_channels, 16, 16, generator=g).to(d); t = torch.tensor([10, 500], device=d)
    c = (torch.randn(2, 4, big.context_dim, generator=g) * 0.45).to(d)
    eps1 = fresh.unet_forward(x, t, c)
    assert "manifest" in _err(lambda: fresh.load_unet(spec_to_unet_cfg(small), blob))
    eps2 = fresh.unet_forward(x, t, c)
    assert torch.isfinite(eps1).all() and float(eps1.abs().max()) > 0
    assert torch.equal(eps1, eps2)


def test_cfgs_the_builders_cannot_walk_are_refused_by_the_load_entries(fresh):
    """Level counts outside the cfg's arrays and a zero head count are refused on the host with a message (no kernel runs): the
    builders would index past ch_mult / divide by zero."""
    from oracle import clip as oclip
    from rdm_amd import _lib
    from _util import spec_to_clip_cfg
    blob = np.zeros(256, np.uint8)
    for n in (0, _lib.RDM_MAX_LEVELS + 1):
        for load in (fresh.load_vq, fresh.load_vq_encoder):
            cfg = spec_to_vq_cfg(ovq.tiny_vq_spec()); cfg.n_ch_mult = n
            assert "unsupported" in _err(lambda: load(cfg, blob))
    cfg = spec_to_clip_cfg(oclip.tiny_clip_spec()); cfg.transformer_heads = 0
    assert "unsupported clip cfg" in _err(lambda: fresh.load_clip(cfg, blob))
    assert fresh.vq_cfg is None and fresh.vqenc_cfg is None and fresh.clip_cfg is None
    assert "not loaded" in _err(lambda: fresh.vq_decode(torch.zeros(1, 3, 16, 16, device=fresh.device)))


def test_no_device_memory_growth_across_calls_and_contexts():
    """hipMemGetInfo at the same point of three context lifetimes and over twelve rounds of every sampling entry (DDIM, VQ decode, online
    and bulk kNN, RARM sampling): the library's scratch is sized once and reused, and rdm_ctx_destroy gives everything back."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, packing

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    levels = []
    for rep in range(3):
        ctx = _lib.Context(0); d = ctx.device
        spec = ounet.tiny_spec(); cfg = spec_to_unet_cfg(spec)
        ctx.load_unet(cfg, packing.pack("unet", cfg, ounet.synth_state_dict(ounet.param_shapes(spec), seed=1)))
        vspec = ovq.tiny_vq_spec(); vcfg = spec_to_vq_cfg(vspec)
        ctx.load_vq(vcfg, packing.pack("vq", vcfg, ounet.synth_state_dict(ovq.vq_param_shapes(vspec), seed=5)))
        rs = orarm.RarmSpec(vocab_in=514, vocab_out=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64)
        rcfg = _lib.make_rarm_cfg(in_channels=514, out_channels=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64)
        ctx.load_rarm(rcfg, packing.pack("rarm", rcfg, ounet.synth_state_dict(orarm.rarm_param_shapes(rs), seed=7)))
        g = torch.Generator(device=d).manual_seed(0)
        db = torch.randn(50000, 512, device=d, generator=g).half(); ctx.db_load(db); del db
        x = torch.randn(4, 3, 16, 16, device=d, generator=g); c = torch.randn(4, 4, 512, device=d, generator=g); uc = torch.zeros_like(c)
        ac = torch.linspace(0.9999, 0.005, 1000)
        marks = []
        for it in range(12):
            z = ctx.ddim_sample(4, x, c, uc, ac, scale=2.0)[0]
            img = ctx.vq_decode(z)
            idx, sc = ctx.knn(torch.randn(200 if it % 2 else 7, 512, device=d, generator=g), 20 if it % 2 else 4)
            toks = ctx.rarm_sample(torch.full((3, 1), 513, device=d, dtype=torch.long), c[:3], 16, torch.rand(16, 3, device=d, generator=g),
                                   top_k=50, guidance_scale=2.0)
            del z, img, idx, sc, toks
            torch.cuda.empty_cache()
            marks.append(free())
        assert marks[1] - marks[-1] < (4 << 20), f"device memory grows across calls: {marks}"      # after the second round nothing is allocated
        levels.append(marks[-1])
        ctx.close(); del ctx, x, c, uc
        torch.cuda.empty_cache()
    assert abs(levels[0] - levels[2]) < (4 << 20), f"a closed context leaves device memory behind: {levels}"


def test_token_and_code_ids_out_of_range_are_refused(fresh):
    """nn.Embedding (RetrievalPatchTransformer.proj_in) and taming's get_codebook_entry raise on an id outside the table; the
    kernels would read row 0 instead: the binding checks the range (advisor finding, round 2)."""
    from rdm_amd import _lib, packing
    d = fresh.device
    rs = orarm.RarmSpec(vocab_in=514, vocab_out=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64)
    rcfg = _lib.make_rarm_cfg(in_channels=514, out_channels=512, n_heads=2, d_head=64, depth=2, context_dim=512, sequence_length=64)
    fresh.load_rarm(rcfg, packing.pack("rarm", rcfg, ounet.synth_state_dict(orarm.rarm_param_shapes(rs), seed=7)))
    ctx2 = torch.zeros(2, 2, 512, device=d)
    assert "[0, 514)" in _err(lambda: fresh.rarm_forward(torch.full((2, 3), 514, dtype=torch.long, device=d), ctx2))
    assert "[0, 514)" in _err(lambda: fresh.rarm_sample(torch.full((2, 1), -1, dtype=torch.long, device=d), ctx2, 4, torch.rand(4, 2, device=d), top_k=8))
    fresh.rarm_forward(torch.full((2, 3), 513, dtype=torch.long, device=d), ctx2)          # the last valid id passes


def test_single_op_entry_points_reject_unsupported_shapes(fresh):
    """The single-kernel ops added in round 3 state their shape contract instead of running something else."""
    d = fresh.device
    bf = lambda *s: torch.zeros(*s, device=d, dtype=torch.bfloat16)
    # token-major-V flash attention: n must be a multiple of 64
    assert "multiple of 64" in _err(lambda: fresh.op_self_attention_qkv(bf(1, 32, 3 * 64), 2))
    # fused cross-attention: C % 64, softmax group in {1, 2, 4}, LayerNorm form takes no separate residual
    G, U = bf(1, 128, 96), bf(1, 96, 128)
    assert "unsupported shape" in _err(lambda: fresh.op_xattn_fused(bf(1, 32, 96), G, U, None, None, 12, 4))
    G, U = bf(1, 128, 64), bf(1, 64, 128)
    assert "unsupported shape" in _err(lambda: fresh.op_xattn_fused(bf(1, 32, 64), G, U, None, None, 6, 3))
    g = torch.ones(64, device=d)
    assert "res must be null" in _err(lambda: fresh.op_xattn_fused(bf(1, 32, 64), G, U, None, bf(1, 32, 64), 8, 4, ln=(g, g, 1e-5)))
    # fused head: W % 32, C <= 240
    w = torch.zeros(3, 64, 3, 3, device=d)
    assert "unsupported shape" in _err(lambda: fresh.op_head_conv(bf(1, 8, 24, 64), w, None))
    w = torch.zeros(3, 256, 3, 3, device=d)
    assert "unsupported shape" in _err(lambda: fresh.op_head_conv(bf(1, 8, 32, 256), w, None))
    # and the context still works
    out = fresh.op_head_conv(bf(1, 8, 32, 64), torch.zeros(3, 64, 3, 3, device=d), None)
    assert out.shape == (1, 3, 8, 32) and float(out.abs().max()) == 0.0


def test_stem_and_valu_head_conv_entries_state_their_shape_contract(fresh):
    """rdm_op_conv_in / rdm_op_conv_out answer what their launchers would refuse with a message, not a bare HIP error code, and the context
    keeps working after each refusal."""
    d = fresh.device
    f32 = lambda *s: torch.zeros(*s, device=d)
    bf = lambda *s: torch.zeros(*s, device=d, dtype=torch.bfloat16)
    ok_in = lambda: fresh.op_conv_in(f32(1, 3, 4, 5) + 1, f32(8, 3, 3, 3), f32(8) + 2)
    ok_out = lambda: fresh.op_conv_out(bf(1, 4, 5, 64), f32(2, 64, 3, 3), f32(2) + 3)
    msg = _err(lambda: fresh.op_conv_in(f32(1, 5, 4, 4), f32(8, 5, 3, 3), f32(8)))                   # Cin = 5
    assert "rdm_op_conv_in" in msg and "unsupported shape" in msg and "Cin 5" in msg
    assert tuple(ok_in().shape) == (1, 4, 5, 8) and float((ok_in().float() - 2).abs().max()) == 0.0
    msg = _err(lambda: fresh.op_conv_in(f32(1, 3, 4, 4), f32(12, 3, 3, 3), f32(12)))                 # Cout % 8
    assert "rdm_op_conv_in" in msg and "unsupported shape" in msg and "Cout 12" in msg
    assert float((ok_in().float() - 2).abs().max()) == 0.0
    msg = _err(lambda: fresh.op_conv_out(bf(1, 4, 4, 96), f32(3, 96, 3, 3), f32(3)))                 # Cin % 64
    assert "rdm_op_conv_out" in msg and "unsupported shape" in msg and "Cin 96" in msg
    assert tuple(ok_out().shape) == (1, 2, 4, 5) and float((ok_out() - 3).abs().max()) == 0.0
    msg = _err(lambda: fresh.op_conv_out(bf(1, 4, 4, 64), f32(5, 64, 3, 3), f32(5)))                 # Cout = 5
    assert "rdm_op_conv_out" in msg and "unsupported shape" in msg and "Cout 5" in msg
    assert float((ok_out() - 3).abs().max()) == 0.0


def test_training_primitives_refuse_bad_sizes(fresh):
    """The backward primitives check their sizes at the C ABI instead of launching a zero-size grid or returning a bare HIP error: each
    refusal names the op, and the context keeps working afterwards."""
    from rdm_amd import _lib
    d = fresh.device
    L = _lib.lib
    bf = torch.zeros(4096, device=d, dtype=torch.bfloat16); f = torch.zeros(4096, device=d)
    x, y, o = bf.data_ptr(), torch.zeros_like(bf).data_ptr(), torch.zeros_like(bf).data_ptr()
    g, g2, g3 = f.data_ptr(), torch.zeros_like(f).data_ptr(), torch.zeros_like(f).data_ptr()
    call = lambda rc: fresh._check(rc)
    assert "rdm_op_layernorm_bwd" in _err(lambda: call(L.rdm_op_layernorm_bwd(fresh._h, x, y, g, 0, 64, 1e-5, o, g2, g3)))      # M = 0
    assert "rdm_op_layernorm_bwd" in _err(lambda: call(L.rdm_op_layernorm_bwd(fresh._h, x, y, g, 4, 0, 1e-5, o, g2, g3)))      # C = 0
    assert "rdm_op_transpose" in _err(lambda: call(L.rdm_op_transpose(fresh._h, x, y, 0, 8)))                                   # rows = 0
    assert "rdm_op_transpose" in _err(lambda: call(L.rdm_op_transpose(fresh._h, x, y, 8, -1)))                                  # cols < 0
    assert "rdm_op_transpose_batched" in _err(lambda: call(L.rdm_op_transpose_batched(fresh._h, x, y, 2, 0, 8)))                # rows = 0
    assert "rdm_op_transpose_batched" in _err(lambda: call(L.rdm_op_transpose_batched(fresh._h, x, y, 2, 8, 0)))                # cols = 0
    assert "rdm_op_softmax" in _err(lambda: call(L.rdm_op_softmax(fresh._h, g, x, 0, 8, 0)))                                    # rows = 0
    assert "n_valid" in _err(lambda: call(L.rdm_op_softmax(fresh._h, g, x, 4, 8, -1)))                                          # n_valid < 0
    assert "n_valid" in _err(lambda: call(L.rdm_op_softmax(fresh._h, g, x, 4, 8, 9)))                                           # n_valid > n
    assert "rdm_op_heads" in _err(lambda: call(L.rdm_op_heads(fresh._h, x, y, 1, 4, 2, 0, 64, 0)))                              # D = 0
    assert "rdm_op_heads" in _err(lambda: call(L.rdm_op_heads(fresh._h, x, y, 1, 4, 2, 65, 130, 0)))                            # D > 64
    assert "rdm_op_heads" in _err(lambda: call(L.rdm_op_heads(fresh._h, x, y, 1, 4, 2, 32, 63, 1)))                             # ldx < H D
    assert "rdm_op_heads" in _err(lambda: call(L.rdm_op_heads(fresh._h, x, y, 1, 4, 2, 32, 64, 3)))                             # mode 3
    assert "rdm_op_colsum" in _err(lambda: call(L.rdm_op_colsum(fresh._h, x, g, 0, 8)))                                         # M = 0
    assert "rdm_op_colsum" in _err(lambda: call(L.rdm_op_colsum(fresh._h, x, g, 8, 0)))                                         # N = 0
    assert "rdm_op_add" in _err(lambda: call(L.rdm_op_add(fresh._h, x, y, o, 0)))                                               # n = 0
    # the context still works, and each of these ops still runs at a valid size
    a = torch.arange(24, device=d, dtype=torch.float32).reshape(3, 8).to(torch.bfloat16)
    assert torch.equal(fresh.op_transpose(a), a.t())
    assert torch.equal(fresh.op_add(a, a), (a.float() * 2).to(torch.bfloat16))
    assert torch.equal(fresh.op_colsum(a), a.float().sum(0))
    assert torch.equal(fresh.op_softmax(torch.zeros(2, 8, device=d), n_valid=8), torch.full((2, 8), 0.125, device=d, dtype=torch.bfloat16))
