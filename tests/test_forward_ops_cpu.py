"""CPU check of the forward-op references (tests/_fwd_ref.py) that tests/test_gpu_forward_ops.py holds the HIP kernels to: an fp32 torch
restatement of each op stands in for the kernel.  It must pass every per-element bound and fall outside the bound against every near
miss -- so the bounds are wide enough for honest fp32 arithmetic and narrow enough to catch the bugs the near misses encode."""
import pytest
import torch

import _fwd_ref as R
from _train_ref import check, standin

torch.set_num_threads(min(16, torch.get_num_threads()))

# the largest shapes exist for the GPU launch geometry (lin4 tile counts, M > 16384 rows); on the CPU their smaller siblings carry the
# same checks
_CPU_CASES = [e for e in R.CASES if not (e[0] in (R.Linear, R.LinearLN) and e[1]["M"] * e[1]["N"] > 20_000_000)]


@pytest.mark.parametrize("entry", _CPU_CASES, ids=[R.case_id(e) for e in _CPU_CASES])
def test_fp32_restatement_within_bound_and_near_misses_outside(entry):
    case, kw, path = entry
    inp = case.make(**kw)
    worst, margin = check(case, inp, standin(case, inp, R.bf16_out))
    print(f"{path}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def test_every_forward_op_is_parametrised():
    names = {e[0].name for e in R.CASES}
    assert names == {"linear", "linear_ln", "conv3x3", "groupnorm", "layernorm", "self_attention", "small_attention", "xattn_fused", "head_conv",
                     "conv_in", "conv_out"}


def test_case_ids_name_every_launch_path():
    paths = " | ".join(e[2] for e in R.CASES)
    for kernel in ("halo4<2>", "halo4<3>", "halo4<2, STRIP>", "halo4<3, STRIP>", "conv_in_kernel<4, 3>", "conv_in_kernel<4, 4>", "conv_in_kernel<0, 3>", "conv_in_kernel<0, 4>",
                   "conv_out_kernel", "small_attention_kernel<32>: 2 key chunks", "small_attention_kernel<32>: 3 key chunks",
                   "small_attention_kernel<64>: causal, 2 key chunks", "gn_stats + gn_apply: 17 chunks of 65 rows, the last one short",
                   "blocks x 2 trips", "K-split 2", "K-split 3", "igemm phase2", "igemm conv", "igemm conv: asym (Downsample)",
                   "igemm ups", "igemm<128, 128", "igemm<256, 192", "igemm<128, 192", "igemm<256, 128", "res_k", "igemm<256, 256, GEGLU>",
                   "igemm<128, 128, GEGLU>", "igemm<256, 128, GEGLU>", "lin4<plain, WM1>", "lin4<plain, WM2>", "lin4<GEGLU, WM1>",
                   "lin4<GEGLU, WM2>", "rowvec", "sgemm", "mgemm", "LN>", "gn_onepass<NV", ", 512>", ", 1024>", "gn_stats + gn_apply",
                   "XCD block order", "layernorm_bf16x8<1>", "layernorm_bf16x8<2>", "layernorm_kernel<f32>", "layernorm_kernel<bf16>",
                   "flash_d32_lds_kernel<false>", "flash_d32_lds_kernel<true>", "flash_d32_kernel", "small_attention_kernel<32>",
                   "small_attention_kernel<64>", "xattn_fused_kernel", "xattn_ln_fused_kernel", "head_conv_kernel",
                   # the forms only the CLIP towers run
                   "igemm<128, 128>: f32 residual in place", "igemm<128, 192>: f32 residual in place", "layernorm_kernel<f32>: f32 out",
                   "small_attention_kernel<64>: causal, 1 key chunks, fused q|k|v rows", "small_attention_kernel<64>: 1 key chunks, fused q|k|v rows"):
        assert kernel in paths, kernel


def test_downsample_cases_are_the_encoders_and_each_has_its_three_misses():
    """The asym (Downsample) form of the conv3x3 case: the four shapes rdm_op_conv3x3_down is run at, the fp64 reference is
    conv2d(pad(x, (0, 1, 0, 1)), w, stride 2) + bias, each shape carries the symmetric-padding, wrong-side-padding and dropped-bias near
    misses (check() above has shown the fp32 stand-in outside the bound against each), and odd sizes are not a case."""
    import torch.nn.functional as F
    down = [e[1] for e in R.CASES if e[0] is R.Conv3x3 and e[1].get("asym")]
    assert [(k["B"], k["H"], k["W"], k["C0"], k["N"]) for k in down] == [(2, 16, 16, 64, 64), (3, 6, 10, 64, 64), (1, 2, 2, 64, 128), (1, 10, 14, 128, 128)]
    for kw in down:
        inp = R.Conv3x3.make(**kw)
        x, w = inp["x"].double().permute(0, 3, 1, 2), inp["w"].double()
        want = (F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2) + inp["b"].double()[None, :, None, None]).permute(0, 2, 3, 1)
        ref = R.Conv3x3.ref(inp, torch.float64)["out"]
        assert ref.shape == (kw["B"], kw["H"] // 2, kw["W"] // 2, kw["N"]) and torch.equal(ref, want)
        labels = [m[0] for m in R.Conv3x3.misses(inp)]
        assert sum(("symmetric padding" in s) + ("wrong side" in s) + (s == "bias dropped") for s in labels) == 3, labels
    with pytest.raises(AssertionError):
        R.Conv3x3.make(B=1, H=5, W=6, C0=64, N=64, stride=2, asym=1)


def test_bf16_ksplit_planes_fall_outside_the_bound():
    """A plausible precision regression of the K-split: the fp32 partial planes rounded to bf16 before the finisher adds them.  An
    fp32 emulation of it must fail the conv bound on a K-split case (the planes cancel, so each is large while the sum is small)."""
    entry = next(e for e in R.CASES if e[0] is R.Conv3x3 and "K-split 2" in e[2])
    inp = R.Conv3x3.make(**entry[1])
    S, C = inp["S"], inp["x"].shape[3]
    ns = C // 64
    y = 0
    for s in range(S):
        lo, hi = s * ns // S * 64, (s + 1) * ns // S * 64
        y = y + R.bfr(R.Conv3x3.conv(inp, torch.float32, x=inp["x"][..., lo:hi], w=inp["w"][:, lo:hi]))
    out = {"out": R.bfr(R.Conv3x3.epilogue(inp, torch.float32, y))}
    with pytest.raises(AssertionError, match="worst error / bound"):
        check(R.Conv3x3, inp, out)

