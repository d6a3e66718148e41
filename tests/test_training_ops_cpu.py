"""CPU check of the training-op references (tests/_train_ref.py) that tests/test_gpu_training_ops.py holds the HIP kernels to: an fp32
torch restatement of each op stands in for the kernel.  It must pass every per-element bound and fall outside the bound against every
near miss -- so the bounds are wide enough for honest fp32 arithmetic and narrow enough to catch the bugs the near misses encode."""
import pytest
import torch

import _train_ref as R

# the largest shapes exist for the GPU launch geometry; on the CPU their smaller siblings carry the same checks
_CPU_CASES = [e for e in R.CASES if not (e[0] is R.Colsum and e[1]["M"] > 1_000_000)]


@pytest.mark.parametrize("entry", _CPU_CASES, ids=[R.case_id(e) for e in _CPU_CASES])
def test_fp32_restatement_within_bound_and_near_misses_outside(entry):
    case, kw, path = entry
    inp = case.make(**kw)
    worst, margin = R.check(case, inp, R.standin(case, inp))
    print(f"{path}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def test_every_primitive_is_parametrised():
    names = {e[0].name for e in R.CASES}
    assert names == {"add", "silu", "sumpool2", "colsum", "colsum_samples", "transpose", "heads", "expand2", "bmm", "softmax", "softmax_bwd",
                     "geglu", "layernorm_bwd", "groupnorm_bwd", "conv3x3_dgrad", "attention_bwd", "small_attention_bwd"}


def test_colsum_geometry_reaches_both_chunk_clamps():
    assert R.colsum_chunk(1000, 64) == 64 and R.colsum_chunk(4_300_000, 8) == 4096
    assert R.colsum_chunk(100, 64) is None and R.colsum_chunk(1000, 36) is None
    assert 64 < R.colsum_chunk(300_000, 320) < 4096


def test_one_pass_layernorm_statistics_fall_outside_the_bound():
    """The defect the LayerNorm backward had: E[x^2] - mean^2 in fp32 on rows whose mean is 60-100x their spread.  An fp32 emulation of
    it (the kernel's lane-strided partial sums) must fail the dgamma bound on the offset-row case."""
    inp = R.LayerNormBwd.make(M=8, C=320, offset=True)
    x = inp["x"]
    M, C = x.shape
    lanes = x.reshape(M, C // 64, 64)                    # element c goes to lane c % 64
    s = lanes.sum(1).sum(1, keepdim=True); ss = (lanes * lanes).sum(1).sum(1, keepdim=True)
    mean = s / C
    rstd = torch.rsqrt(torch.clamp(ss / C - mean * mean, min=0) + inp["eps"])
    xh = (x - mean) * rstd
    out = R.standin(R.LayerNormBwd, inp)
    out["dgamma"] = (inp["dy"] * xh).sum(0)
    with pytest.raises(AssertionError, match="dgamma"):
        R.check(R.LayerNormBwd, inp, out)
