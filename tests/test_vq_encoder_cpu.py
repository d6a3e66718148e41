"""CPU pins of the first-stage encoder's restatement (oracle/vq_emul.py::vq_encode_emulated) and of the layer-by-layer comparison
tests/test_gpu_vq_encoder.py holds the library to (tests/_vqenc_ref.py):
  * rounding off, the restatement is exact algebra: it equals the fp32 oracle (oracle/vqdecoder.py::vq_encode) to 2e-5 (measured 9e-7 .. 1.3e-6);
  * its layer taps are the layers vq_encoder_param_shapes implies, in number and shape;
  * the comparison, fed the taps of a restatement that is wrong in ONE place where the GPU test feeds it the library's, fails at that place:
    a Downsample padded (1, 0, 1, 0) at exactly the Downsample layers (about 1.3), a dropped nin_shortcut bias at exactly its block
    (8e-2 .. 1e-1), GroupNorm eps 1e-5 in at least one layer (1.4e-3 .. 1.7e-3 against a block's 1e-3); the unaltered one errs by exactly 0."""
import pytest
import torch

from oracle import vq_emul
from oracle import vqdecoder as ovq

import _vqenc_ref as V
from _util import rel_l2

torch.set_grad_enabled(False)
NAMES = list(V.MODELS)


@pytest.mark.parametrize("name", NAMES)
def test_emulated_encoder_is_exact_algebra_without_rounding(name):
    spec, sd, x, _, z_emu, ref = V.model(name)
    got = vq_emul.vq_encode_emulated(sd, spec, x, rounding=False)
    e = rel_l2(got, ref)
    print(f"[vqenc] {name}: restatement without rounding vs fp32 oracle {e:.3e}; with rounding {rel_l2(z_emu, ref):.3e}")
    assert got.shape == ref.shape and e <= 2e-5, e
    assert 1e-4 < rel_l2(z_emu, ref) <= 2.5e-2          # rounding on: the bf16 storage distance, not zero


@pytest.mark.parametrize("name", NAMES)
def test_tap_count_and_shapes_follow_the_parameter_table(name):
    spec, sd, x, taps = V.model(name)[:4]
    table = V.layers(spec, tuple(x.shape))
    assert len(taps) == len(table) == V.N_LAYERS[name]
    for tp, (nm, kind, shp) in zip(taps, table):
        assert tuple(tp.shape) == shp, (nm, tuple(tp.shape), shp)
    f = 2 ** (len(spec.ch_mult) - 1)
    assert tuple(V.model(name)[4].shape) == (x.shape[0], spec.embed_dim, x.shape[2] // f, x.shape[3] // f)


@pytest.mark.parametrize("name", NAMES)
def test_unaltered_taps_compare_at_exactly_zero(name):
    lib, z = V.altered_taps(name, "none")
    rows, e_z = V.teacher_forced(name, lib, z)
    assert all(e == 0.0 for _, _, e in rows) and e_z == 0.0, rows


@pytest.mark.parametrize("name", NAMES)
def test_wrong_side_downsample_padding_fails_at_exactly_the_downsample_layers(name):
    lib, z = V.altered_taps(name, "pad")
    rows, _ = V.teacher_forced(name, lib, z)
    V.report(f"{name}, Downsample padded (1, 0, 1, 0)", rows)
    down = [nm for nm, _, _ in rows if nm.endswith("downsample")]
    assert len(down) == len(V.model(name)[0].ch_mult) - 1
    assert V.exceeding(rows) == down
    assert all(e > 0.5 for nm, _, e in rows if nm in down)
    assert all(e == 0.0 for nm, _, e in rows if nm not in down)


@pytest.mark.parametrize("name", NAMES)
def test_dropped_nin_shortcut_bias_fails_at_its_block(name):
    lib, z = V.altered_taps(name, "nin_bias")
    rows, _ = V.teacher_forced(name, lib, z)
    V.report(f"{name}, a nin_shortcut bias dropped", rows)
    block = V.first_nin_shortcut(name)[1]
    assert V.exceeding(rows) == [block]
    assert all(e == 0.0 for nm, _, e in rows if nm != block)


@pytest.mark.parametrize("name", NAMES)
def test_groupnorm_eps_1e5_fails_in_some_layer(name):
    lib, z = V.altered_taps(name, "eps")
    rows, _ = V.teacher_forced(name, lib, z)
    V.report(f"{name}, GroupNorm eps 1e-5", rows)
    assert V.exceeding(rows), "eps 1e-5 instead of 1e-6 passes every layer bound"
    # what the whole-latent assertion alone sees of it: nothing -- the altered restatement sits inside 2.5e-2 of the fp32 oracle
    assert rel_l2(z, V.model(name)[5]) <= 2.5e-2


def test_quantiser_bound_holds_for_an_fp32_evaluation_of_the_kernels_formula():
    """The per-pixel bound tests/test_gpu_vq_encoder.py holds vq_quantize_kernel to past its grid cap, checked here first: an fp32 numpy
    evaluation of the kernel's formula on the same 1 x 3 x 520 x 512 input passes it at every pixel, and a quantiser that skips the
    pixels behind the 262 144th (the grid-stride loop's second trip left out: index 0, z passed through) does not."""
    spec, sd, z = V.quantizer_case()
    e = sd["quantize.embedding.weight"]
    assert z.shape[2] * z.shape[3] > 1024 * 256 and tuple(e.shape) == (512, 3)
    zq, idx = V.quantize_fp32_formula(z, e)
    worst = V.check_quantized(z, e, zq, idx)
    print(f"[vqenc] quantiser, fp32 formula on the CPU: worst (d[idx] - min d) / bound {worst:.3g}")
    assert float((idx.long() == ovq.vq_quantize(sd, z)[1]).float().mean()) > 0.999          # the oracle's own argmin: near-ties only
    idx2 = idx.clone(); idx2[1024 * 256:] = 0
    with pytest.raises(AssertionError, match="further than the bound"):
        V.check_quantized(z, e, zq, idx2)
    zq2 = zq.clone(); zq2.view(-1)[-1] += 1e-6
    with pytest.raises(AssertionError, match="zq differs"):
        V.check_quantized(z, e, zq2, idx)


def test_forcing_does_not_write_to_the_shared_reference():
    spec, sd, x, taps, z_emu, _ = V.model("tiny")
    before = [t.clone() for t in taps]
    V.teacher_forced("tiny", V.altered_taps("tiny", "pad")[0])
    assert all(torch.equal(a, b) for a, b in zip(before, V.model("tiny")[3]))
    assert vq_emul.DOWN_PAD == (0, 1, 0, 1) and vq_emul.GN_EPS == 1e-6
    assert torch.equal(vq_emul.vq_encode_emulated(sd, spec, x), z_emu)
