"""CPU check of the reference that tests/test_gpu_vq_attn.py holds rdm_op_vq_attention to (tests/_vq_attn_ref.py): an fp32 torch restatement
of the kernel's arithmetic -- the normalised probability rounded to bf16 -- must stay inside the derived per-element bound at every case
the GPU test runs, and every near miss must fall outside it.  This pins the inputs: the GPU test cannot pass vacuously."""
import pytest
import torch

import _vq_attn_ref as R
from _train_ref import check

torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_kernel_arithmetic_within_bound_and_near_misses_outside(case):
    inp = R.make_case(case)
    worst, margin = check(R.VqAttention, inp, R.kernel_arithmetic(inp))
    print(f"{R.case_id(case)}: worst error / bound {worst:.3g}, closest near miss {margin:.3g}")


def test_every_near_miss_is_exercised_somewhere():
    """each of the five near misses differs from the reference (and so is checked) in at least one case"""
    seen = set()
    for case in R.CASES:
        inp = R.make_case(case)
        ref = R.VqAttention.ref(inp, R.F64)["out"]
        seen |= {label for label, m in R.VqAttention.misses(inp) if not torch.equal(m["out"], ref)}
    assert seen == {"scale C^-1", "k and v swapped", "padding keys leak probability", "last key tile out of the normaliser", "bias_v omitted"}


def test_online_softmax_form_is_a_different_rounding():
    """Why the kernel sweeps the keys twice: the usual online-softmax form rounds the UNNORMALISED probability to bf16 and divides the
    accumulator at the end.  It is inside the same bound (it is no bug) but not the library's arithmetic: it differs from the restatement
    of oracle/vq_emul.py's order on a fair share of the elements."""
    inp = R.make_case(R.CASES[2])
    q, k, v = inp["q"], inp["k"], inp["v"]
    s = q @ k.transpose(1, 2) * torch.tensor(R.VqAttention.scale(inp), dtype=torch.float32)
    e = torch.exp(s - s.max(2, keepdim=True).values)
    online = R.bfr((R.bfr(e) @ v) / e.sum(2, keepdim=True) + inp["bias"])
    ours = R.kernel_arithmetic(inp)["out"]
    frac = float((online != ours).float().mean())
    print(f"online-softmax rounding differs on {frac:.3f} of the elements")
    assert frac > 0.01
