"""CPU pins of what tests/test_gpu_clip.py trusts: oracle/clip_emul.py (the library's CLIP arithmetic restated) and the stage-by-stage
comparison of tests/_clip_ref.py.
  * rounding off, the restatement is exact algebra: it equals oracle/clip.py -- itself pinned to the reference's classes by golden
    vectors -- to fp32 round-off (2e-5, the figure the other emulators are pinned at in tests/test_oracle_cpu.py);
  * rounding on, its taps stand in for the library's in the GPU suite's comparison: every stage passes its per-element bound, so the bounds
    admit honest fp32 arithmetic with bf16 storage where the library has it;
  * seven near-miss towers -- each one plausible defect -- fail, and fail AT the stage they break."""
import re

import pytest
import torch

import _clip_ref as CR
from oracle import clip as oclip, unet as ounet
from oracle.clip_emul import IMAGE, TEXT, clip_image_emulated, clip_text_emulated, eot_columns, stage_name

torch.set_grad_enabled(False)
torch.set_num_threads(min(16, torch.get_num_threads()))
B = 3


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def tiny():
    spec = oclip.tiny_clip_spec()
    sd = ounet.synth_state_dict(oclip.clip_param_shapes(spec), seed=11)
    tokens = CR.text_tokens(spec, B)
    image = torch.randn(B, 3, spec.image_resolution, spec.image_resolution, generator=torch.Generator().manual_seed(6))
    return spec, sd, tokens, image


def test_argmax_returns_the_first_maximum():
    """what `tokens.argmax` means in the reference (model.py:318), the oracle and the EOT check: the FIRST of equal maxima"""
    t = torch.tensor([[5, 9, 1, 9, 9], [7, 7, 7, 7, 7], [0, 1, 2, 3, 3]])
    assert t.argmax(dim=-1).tolist() == [1, 0, 3]
    assert eot_columns(t).tolist() == [1, 0, 3] and eot_columns(t, last=True).tolist() == [4, 4, 4]


def test_token_rows_cover_the_eot_edges(tiny):
    spec, _, tokens, _ = tiny
    L = spec.context_length
    col = eot_columns(tokens)
    assert col[0] == 0 and col[1] == L - 1 and col[2] == 7 and len(set(col.tolist())) == B
    assert int((tokens[2] == tokens[2].max()).sum()) == 2 and eot_columns(tokens, last=True)[2] == 40
    assert int(tokens.min()) >= 0 and int(tokens.max()) == spec.vocab_size - 1


def test_emulated_towers_are_exact_algebra_without_rounding(tiny):
    spec, sd, tokens, image = tiny
    e_t = _rel(clip_text_emulated(sd, spec, tokens, rounding=False), oclip.encode_text(sd, spec, tokens))
    e_i = _rel(clip_image_emulated(sd, spec, image, rounding=False), oclip.encode_image(sd, spec, image))
    print(f"[clip emul] rounding off vs oracle/clip.py: text {e_t:.3e}, image {e_i:.3e}")
    assert e_t <= 2e-5 and e_i <= 2e-5
    # rounding on: at the bf16 storage distance, where the library's whole-tower checks sit (tests/test_gpu_models.py: 2e-2)
    r_t = _rel(clip_text_emulated(sd, spec, tokens), oclip.encode_text(sd, spec, tokens))
    r_i = _rel(clip_image_emulated(sd, spec, image), oclip.encode_image(sd, spec, image))
    print(f"[clip emul] rounding on vs oracle/clip.py: text {r_t:.3e}, image {r_i:.3e}")
    assert e_t < r_t <= 2e-2 and e_i < r_i <= 2e-2


def test_emulated_vitb32_block_is_exact_algebra_without_rounding():
    """one ViT-B/32-shaped resblock per tower (width 768 / 12 heads over 50 tokens; width 512 / 8 heads over 77)"""
    spec = oclip.ClipSpec(vision_layers=1, transformer_layers=1, vocab_size=512)
    sd = ounet.synth_state_dict(oclip.clip_param_shapes(spec), seed=12)
    g = torch.Generator().manual_seed(13)
    tokens = CR.text_tokens(spec, 3)
    image = torch.randn(2, 3, 224, 224, generator=g)
    e_t = _rel(clip_text_emulated(sd, spec, tokens, rounding=False), oclip.encode_text(sd, spec, tokens))
    e_i = _rel(clip_image_emulated(sd, spec, image, rounding=False), oclip.encode_image(sd, spec, image))
    print(f"[clip emul] ViT-B/32-shaped block, rounding off: text {e_t:.3e}, image {e_i:.3e}")
    assert e_t <= 2e-5 and e_i <= 2e-5


def test_taps_are_keyed_and_shaped_as_the_library_shows_them(tiny):
    spec, sd, tokens, image = tiny
    for tower, run, x in ((TEXT, clip_text_emulated, tokens), (IMAGE, clip_image_emulated, image)):
        taps = {}
        out = run(sd, spec, x, taps=taps)
        shapes = CR.tap_shapes(spec, tower, B)
        assert list(taps) == list(shapes), "execution order"
        for key, (rows, width, _) in shapes.items():
            assert tuple(taps[key].shape) == (rows, width), (stage_name(key), tuple(taps[key].shape))
        assert torch.equal(out, taps[(tower, 4 if tower == TEXT else 7)])


def test_forced_stage_replaces_what_follows(tiny):
    spec, sd, tokens, _ = tiny
    free = {}
    clip_text_emulated(sd, spec, tokens, taps=free)
    key = (TEXT, 16 + 4)
    own = {}
    out = clip_text_emulated(sd, spec, tokens, taps=own, forced={key: torch.zeros_like(free[key])})
    assert torch.equal(own[key], free[key]) and not torch.equal(own[(TEXT, 16 + 5)], free[(TEXT, 16 + 5)])
    assert not torch.equal(out, free[(TEXT, 4)])


def test_every_stage_of_the_restatement_passes_its_bound(tiny):
    spec, sd, tokens, image = tiny
    taps = {}
    clip_text_emulated(sd, spec, tokens, taps=taps)
    rep = CR.check_text_stages(sd, spec, tokens, taps)
    print("[clip emul] text tower, the restatement standing in for the library:\n" + CR.summary(rep))
    assert list(rep) and set(rep) == set(CR.tap_shapes(spec, TEXT, B))
    taps = {}
    clip_image_emulated(sd, spec, image, taps=taps)
    rep = CR.check_image_stages(sd, spec, image, taps)
    print("[clip emul] image tower, the restatement standing in for the library:\n" + CR.summary(rep))
    assert set(rep) == set(CR.tap_shapes(spec, IMAGE, B))


# (variant, tower, the stage it must fail at)
_NEAR_MISS_TOWERS = [
    ("pos_shift", TEXT, (TEXT, 1)), ("pos_shift", IMAGE, (IMAGE, 3)), ("cls_last", IMAGE, (IMAGE, 3)), ("no_causal", TEXT, (TEXT, 16 + 3)),
    ("erf_gelu", TEXT, (TEXT, 16 + 6)), ("erf_gelu", IMAGE, (IMAGE, 16 + 6)), ("heads_d_major", TEXT, (TEXT, 16 + 3)),
    ("heads_d_major", IMAGE, (IMAGE, 16 + 3)), ("patch_yxc", IMAGE, (IMAGE, 1)), ("eot_last", TEXT, (TEXT, 2)),
]


@pytest.mark.parametrize("variant,tower,key", _NEAR_MISS_TOWERS, ids=[f"{v}-{'text' if t == TEXT else 'image'}" for v, t, _ in _NEAR_MISS_TOWERS])
def test_near_miss_tower_fails_at_the_stage_it_breaks(tiny, variant, tower, key):
    spec, sd, tokens, image = tiny
    taps = {}
    if tower == TEXT:
        clip_text_emulated(sd, spec, tokens, taps=taps, variant=variant)
        run = lambda: CR.check_text_stages(sd, spec, tokens, taps)
    else:
        clip_image_emulated(sd, spec, image, taps=taps, variant=variant)
        run = lambda: CR.check_image_stages(sd, spec, image, taps)
    with pytest.raises(AssertionError, match="^" + re.escape(stage_name(key) + ":")) as err:
        run()
    print(f"[clip emul] {variant}: {err.value}")
