"""CPU pins of what tests/test_gpu_rarm_stages.py trusts: the stage-by-stage comparison of tests/_rarm_stage_ref.py.
  * an fp32 torch stand-in with the library's storage types (bf16 activations, fp32 residual stream) runs both executors -- the decode
    step in its one-launch and its GEMM form, guided and not, the whole-sequence pass, and the hand-over between them -- and produces
    the tap dictionary the library shows: every stage passes its per-element bound and lies outside it against every near miss, the
    wiring near misses included, so the bounds admit honest arithmetic and the near misses are told apart on this model's own tensors;
  * each wiring error, planted in the stand-in ONE at a time, is reported, and reported AT the stage it breaks."""
import re

import pytest
import torch

import _rarm_stage_ref as S
from oracle import rarm as orarm

torch.set_grad_enabled(False)
torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.fixture(scope="module")
def tiny():
    spec = orarm.tiny_rarm_spec()
    return spec, S.Net(S.synth_weights(spec, 77), spec)


def _inputs(spec, b, k, t, seed=3):
    g = torch.Generator().manual_seed(seed)
    return S.tokens(spec, b, t, g), torch.randn(b, k, spec.context_dim, generator=g) * 0.45


@pytest.fixture(scope="module")
def wide():
    """the shipped width (12 heads x 64, vocab 16386 / 16384, L = 256) with only the depth cut to 2"""
    spec = orarm.RarmSpec(depth=2)
    return spec, S.Net(S.synth_weights(spec, 78), spec)


WIDE = {"one-launch": (S.run_forward, (2, 8, 3)), "GEMM form": (S.run_forward, (2, 16, 2)), "whole sequence across a 32-row tile": (S.run_forward_seq, (2, 8, 33))}


@pytest.mark.parametrize("case", list(WIDE))
def test_standin_passes_every_stage_at_the_shipped_width(wide, case):
    """the GPU suite's shipped-width cases: the near misses are told apart on this model's activations too"""
    spec, net = wide
    run, shape = WIDE[case]
    taps = run(S.Standin(), net, *_inputs(spec, *shape)).taps
    rep = run(S.Checker(taps), net, *_inputs(spec, *shape)).report
    print(f"[rarm stages] shipped width, {case}, the stand-in in the library's place:\n" + S.summary(rep))
    assert set(rep) == set(taps) and all(w <= 1.0 and m > 0 for w, m in rep.values())


def _run(net, case, v):
    spec = net.spec
    if case == "decode one-launch":                  # b = 3, k = 4, t = 6
        return S.run_forward(v, net, *_inputs(spec, 3, 4, 6))
    if case == "decode GEMM form":                   # 2 heads * 65 neighbours > 128
        return S.run_forward(v, net, *_inputs(spec, 3, 65, 3))
    if case == "whole sequence":
        return S.run_forward_seq(v, net, *_inputs(spec, 3, 4, 7))
    tok, ctx = _inputs(spec, 3, 65 if "GEMM" in case else 4, 8)
    if case == "guided one-launch":                  # cond_len 2, 3 steps, B2 = 6
        return S.run_sample(v, net, tok[:, :2], tok[:, 2:5], ctx, guided=True)
    if case == "guided GEMM form":
        return S.run_sample(v, net, tok[:, :1], tok[:, 1:3], ctx, guided=True)
    if case == "guided hand-over":                   # cond_len 5, 2 steps: positions 0 .. 3 in the whole-sequence pass
        return S.run_sample(v, net, tok[:, :5], tok[:, 5:7], ctx, guided=True, prefill=True)
    raise KeyError(case)


CASES = ["decode one-launch", "decode GEMM form", "whole sequence", "guided one-launch", "guided GEMM form", "guided hand-over"]


@pytest.fixture(scope="module")
def standins(tiny):
    """the unplanted stand-in's taps of every case, computed once"""
    _, net = tiny
    return {case: _run(net, case, S.Standin()).taps for case in CASES}


@pytest.mark.parametrize("case", CASES)
def test_standin_passes_every_stage(tiny, standins, case):
    spec, net = tiny
    taps = standins[case]
    rep = _run(net, case, S.Checker(taps)).report
    print(f"[rarm stages] {case}, the stand-in in the library's place:\n" + S.summary(rep))
    assert set(rep) == set(taps), "every tapped stage is checked"
    assert all(w <= 1.0 and m > 0 for w, m in rep.values())


def test_taps_are_keyed_and_shaped_as_the_library_shows_them(tiny, standins):
    spec, _ = tiny
    want = {**S.tap_shapes(spec, S.PREPARE, 3, 3, 4), **S.tap_shapes(spec, S.STEP, 3, 3, 4, steps=6)}
    got = standins["decode one-launch"]
    assert list(got) == list(want), "execution order"
    for key, (shape, dt) in want.items():
        assert tuple(got[key].shape) == shape and got[key].dtype == dt, (S.stage_name(key), tuple(got[key].shape), got[key].dtype)
    # the one-launch form holds neither norm2, to_q nor the attention heads in memory; the GEMM form holds all three behind the LayerNorm passes it needs
    assert not {5, 6, 7} & set(S.step_stages(spec, 3, 4, False)) and {6, 7} <= set(S.step_stages(spec, 3, 65, False))
    assert set(S.step_stages(spec, 384, 4, False)) == set(range(1, 12)) and 6 not in S.step_stages(spec, 384, 4, True)
    want = {**S.tap_shapes(spec, S.PREPARE, 3, 6, 4), **S.tap_shapes(spec, S.SEQ, 3, 6, 4, t=4, head=False), **S.tap_shapes(spec, S.STEP, 3, 6, 4, steps=2)}
    got = standins["guided hand-over"]
    assert set(got) == set(want)
    for key, (shape, dt) in want.items():
        assert tuple(got[key].shape) == shape and got[key].dtype == dt, (S.stage_name(key), tuple(got[key].shape), got[key].dtype)


# (case, the stage the error is planted in -- and must be reported at --, the near miss planted)
_W, _B, _R = "the neighbouring layer's weights", "the bias left off", "the residual taken from the block's input"
_U = "the unconditional half given the conditional half's neighbours"
PLANTS = [
    ("decode one-launch", "prepare ctxkv", _W), ("decode one-launch", "prepare block 0 G", "layer 1's offset in ctxkv"),
    ("decode one-launch", "prepare block 1 UT", "layer 0's offset in ctxkv"), ("decode one-launch", "prepare block 1 G", _W),
    ("decode one-launch", "step embedding", "position one further on"), ("decode one-launch", "step block 0 q|k|v", _W),
    ("decode one-launch", "step block 1 self-attention heads", "row t not attended"),
    ("decode one-launch", "step block 1 self-attention heads", "one row past the range attended"),
    ("decode one-launch", "step block 0 x + attn1.to_out", _B), ("decode one-launch", "step block 1 x + attn1.to_out", _W),
    ("decode one-launch", "step block 0 x + attn2", "layer 1's G and UT"), ("decode one-launch", "step block 1 x + attn2", _R),
    ("decode one-launch", "step block 1 x + attn2", _B), ("decode one-launch", "step block 0 GEGLU hidden", _B),
    ("decode one-launch", "step block 1 x + ff.net.2", _R), ("decode one-launch", "step block 0 x + ff.net.2", _W),
    ("decode one-launch", "step logits", _B),
    ("decode GEMM form", "step block 0 attn2.to_q", _W), ("decode GEMM form", "step block 0 cross-attention heads", "layer 1's offset in ctxkv"),
    ("decode GEMM form", "step block 1 x + attn2", _R), ("decode GEMM form", "step block 1 x + attn2", _B),
    ("guided one-launch", "prepare ctxkv", _U), ("guided one-launch", "step block 0 x + attn2", "a b >= Bc row given row b - Bc's attention"),
    ("guided one-launch", "step block 1 x + attn2", "bias left off the zero-neighbour rows"),
    ("guided GEMM form", "step block 1 cross-attention heads", _U),
    ("whole sequence", "seq embedding", "position one further on"), ("whole sequence", "seq block 0 q|k|v", _W),
    ("whole sequence", "seq block 1 x + attn1.to_out", "bias dropped"), ("whole sequence", "seq block 0 cross-attention heads", "layer 1's offset in ctxkv"),
    ("whole sequence", "seq block 1 x + attn2", _R), ("whole sequence", "seq block 1 x + ff.net.2", _R), ("whole sequence", "seq block 0 norm3", _W),
    ("guided hand-over", "seq block 0 cross-attention heads", _U), ("guided hand-over", "step block 1 self-attention heads", "row t not attended"),
]


@pytest.mark.parametrize("case,stage,label", PLANTS, ids=[f"{c}-{s}-{l}".replace(" ", "_") for c, s, l in PLANTS])
def test_planted_wiring_error_fails_at_the_stage_it_breaks(tiny, case, stage, label):
    _, net = tiny
    bad = _run(net, case, S.Standin(plant=(stage, label)))
    assert bad.planted > 0, "the plant names a stage and a near miss of this case"
    with pytest.raises(AssertionError, match="^" + re.escape(stage)) as err:
        _run(net, case, S.Checker(bad.taps))
    print(f"[rarm stages] {case}, {stage} with '{label}': {err.value}")


def test_hand_over_cache_one_row_off_fails_at_the_first_decode_attention(tiny):
    """the decode steps behind a prefix are referenced from the whole-sequence pass's q|k|v: a stand-in whose whole-sequence pass writes
    its K / V rows one cache row further on passes every stage of that pass and fails at the first cache attention that reads them"""
    spec, net = tiny
    tok, ctx = _inputs(spec, 3, 4, 8)
    bad = S.run_sample(S.Standin(), net, tok[:, :5], tok[:, 5:7], ctx, guided=True, prefill=True, cache_pos=torch.arange(4) + 1)
    with pytest.raises(AssertionError, match="^" + re.escape("step block 0 self-attention heads (step 0)")) as err:
        _run(net, "guided hand-over", S.Checker(bad.taps))
    print(f"[rarm stages] hand-over cache one row off: {err.value}")
