"""CPU side of the device noise: the numpy restatement (tests/_rng_ref.py) and the library's host function reproduce the Random123 known
answers of Philox4x32-10 and agree on random counters; the reference normals have the moments of N(0, 1) and uncorrelated rows and steps;
MinimalRETRODiffusion hands device_noise through as (noise_seed, noise_row0) without drawing anything; a seed together with a noise stack
is refused; scripts/rdm_sample.py has --eta and --device_noise."""
import os

import numpy as np
import pytest
import torch

import _rng_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, words)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def _lib_words(counter, key):
    """The library's host function on a raw (counter, key): counter = (block, step, row, stream), key = (seed lo, seed hi)."""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    block, step, row, stream = counter
    return _lib.rng_words(key[0] | (key[1] << 32), row, step, stream, block)


def test_known_answers_reference_and_library():
    for counter, key, want in KNOWN_ANSWERS:
        got = [int(v) for v in ref.philox4x32_10(counter, key)]
        assert got == list(want), f"reference: {[hex(v) for v in got]}"
        got = [int(v) for v in _lib_words(counter, key)]
        assert got == list(want), f"rdm_rng_words: {[hex(v) for v in got]}"


def test_library_words_equal_the_reference_on_random_counters():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    rng = np.random.default_rng(2024)
    cases = [(int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)),
              int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))) for _ in range(300)]
    cases += [(2 ** 63, 0, 0, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 7, 1, 2 ** 32 - 1), (2 ** 63 + 12345, 2 ** 32 - 1, 0, 0, 3), (1, 2 ** 32 - 1, 249, 1, 0)]
    assert any(s >= 2 ** 63 for s, *_ in cases[:300])
    for seed, row, step, stream, block in cases:
        want = ref.block_words(seed, row, step, stream, block)
        got = _lib.rng_words(seed, row, step, stream, block)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (seed, row, step, stream, block)
    # the layout: element e of a row is word e & 3 of block e >> 2
    w = ref.words(5, 3, 2, 11, 4, 1)
    for b in range(2):
        for e in range(11):
            assert w[b, e] == _lib.rng_words(5, 3 + b, 4, 1, e >> 2)[e & 3]


def test_reference_normals_have_normal_moments_and_independent_rows_and_steps():
    """Seed 0, stream 1, rows 0-7, steps 1-8, 768 elements each (n = 49152): the standardised deviations of the mean, the variance and the
    fourth moment from 0, 1 and 3 stay below 4 (standard errors 1 / sqrt n, sqrt(2 / n), sqrt(96 / n)), as do the correlations between two
    rows and between two steps over the 768 elements.  Fixed inputs: nothing can flake."""
    z = np.stack([ref.normals(0, 0, 8, 768, step, 1)[0] for step in range(1, 9)])          # [step, row, element]
    n = z.size
    assert n == 49152 and np.isfinite(z).all() and np.abs(z).max() <= 5.78
    mean, var, m4 = z.mean(), z.var(), (z ** 4).mean()
    figures = (abs(mean) * np.sqrt(n), abs(var - 1) * np.sqrt(n / 2), abs(m4 - 3) * np.sqrt(n / 96))
    corr_rows = np.corrcoef(z[0, 0], z[0, 1])[0, 1]
    corr_steps = np.corrcoef(z[0, 0], z[1, 0])[0, 1]
    print(f"[device noise] moments: mean {figures[0]:.2f}, var {figures[1]:.2f}, m4 {figures[2]:.2f} sigma; "
          f"corr rows {abs(corr_rows) * np.sqrt(768):.2f}, steps {abs(corr_steps) * np.sqrt(768):.2f} sigma")
    assert all(f < 4 for f in figures), figures
    assert abs(corr_rows) * np.sqrt(768) < 4 and abs(corr_steps) * np.sqrt(768) < 4
    # the uniforms are strictly inside (0, 1) at both ends of the word range
    assert 0 < ref.uniforms(0) < ref.uniforms(0xFFFFFFFF) < 1


class StubCtx:
    """Stands in for the library context: records what reaches it, returns tensors of the shapes the library would."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def vq_decode(self, z, force_not_quantize=False, return_indices=False):
        return z.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)

    def op_randn(self, seed, B, per_row, row0=0, step=0, stream=0):
        self.calls.append(("op_randn", dict(seed=seed, B=B, per_row=per_row, row0=row0, step=step, stream=stream)))
        return torch.zeros(B, per_row)

    def ddim_sample(self, S, x_T, cond, uncond, alphas_cumprod, eta=0.0, scale=1.0, noise=None, log_every_t=100, temperature=1.0,
                    want_intermediates=False, seed=None, row0=0, shape=None):
        self.calls.append(("ddim_sample", dict(x_T=x_T, noise=noise, seed=seed, row0=row0, eta=eta)))
        z = torch.zeros((cond.shape[0],) + tuple(shape)) if x_T is None else x_T * 0.5
        return z, z[None], z[None]

    def ddpm_sample(self, timesteps, x_T, cond, noise=None, sched=None, clip_denoised=True, temperature=1.0, seed=None, row0=0, shape=None):
        self.calls.append(("ddpm_sample", dict(x_T=x_T, noise=noise, seed=seed, row0=row0, shape=shape)))
        return torch.zeros((cond.shape[0],) + tuple(shape)) if x_T is None else x_T * 0.25


def _model(ctx, image_size=8):
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    return MinimalRETRODiffusion(unet_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, ctx=ctx, image_size=image_size)


def _last(ctx, name):
    return [kw for n, kw in ctx.calls if n == name][-1]


def test_sample_shard_device_noise_passes_seed_and_row0_and_draws_nothing(monkeypatch):
    """Rows [1, 3) of a batch of 3 with device_noise: sample_log gets noise_seed = the call's shared seed and noise_row0 = 1, no x_T and no
    noise stack, and parallel.per_sample_noise is never called; the library context then sees seed / row0 and no stack (DDIM eta = 1) and
    no x_T either (DDPM)."""
    from rdm_amd import parallel
    ctx = StubCtx()
    m = _model(ctx)
    m.set_distributed(True)
    n = 3
    c = torch.zeros(n, 4, 512)

    def refuse(*a, **k):
        raise AssertionError("per_sample_noise was called under device_noise")
    monkeypatch.setattr(parallel, "per_sample_noise", refuse)
    seen = []
    inner = m.sample_log
    monkeypatch.setattr(m, "sample_log", lambda **kw: (seen.append(kw), inner(**kw))[1])

    torch.manual_seed(21)
    img = m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, n, 2.0, dict(ddim=True, ddim_steps=5, eta=1.0), device_noise=True)
    torch.manual_seed(21)
    base = parallel.shared_seed("cpu")
    kw = seen[-1]
    assert kw["noise_seed"] == base and kw["noise_row0"] == 1 and kw.get("x_T") is None and kw.get("noise") is None
    call = _last(ctx, "ddim_sample")
    assert call["seed"] == base and call["row0"] == 1 and call["noise"] is None and call["eta"] == 1.0
    start = _last(ctx, "op_randn")                                    # the logged starting latent: stream 0 of the same rows
    assert start == dict(seed=base, B=2, per_row=3 * 8 * 8, row0=1, step=0, stream=0)
    assert tuple(img.shape) == (2, 3, 32, 32)
    # the DDPM loop: no x_T reaches the library at all
    ctx.calls.clear()
    torch.manual_seed(22)
    m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, n, 1.0, dict(ddim=False, ddim_steps=None, timesteps=4, custom_shape=(3, 16, 24)),
                    device_noise=True)
    torch.manual_seed(22)
    base = parallel.shared_seed("cpu")
    assert [name for name, _ in ctx.calls] == ["ddpm_sample"]
    call = _last(ctx, "ddpm_sample")
    assert call == dict(x_T=None, noise=None, seed=base, row0=1, shape=(3, 16, 24))
    # PLMS draws no per-step noise: the seed gives the starting latent only
    ctx.plms_sample = lambda S, x_T, *a, **k: (x_T * 0.5, x_T[None], x_T[None])
    ctx.calls.clear()
    m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, n, 2.0, dict(ddim=True, ddim_steps=5, plms=True), device_noise=True)
    assert [name for name, _ in ctx.calls] == ["op_randn"] and _last(ctx, "op_randn")["row0"] == 1 and _last(ctx, "op_randn")["stream"] == 0
    # an explicit stack together with the flag is refused
    with pytest.raises(ValueError, match="noise"):
        m._sample_shard(c, torch.zeros_like(c), 0, n, n, 2.0, dict(ddim=True, ddim_steps=5, eta=1.0, noise=torch.zeros(5, 3, 3, 8, 8)), device_noise=True)


def test_sample_shard_without_the_flag_calls_what_it_called_before():
    """No device_noise: x_T and the stack are drawn row by row with parallel.per_sample_noise and the library sees no seed."""
    from rdm_amd import parallel
    ctx = StubCtx()
    m = _model(ctx)
    m.set_distributed(True)
    n, S = 3, 5
    c = torch.zeros(n, 4, 512)
    torch.manual_seed(31)
    m._sample_shard(c[1:], torch.zeros_like(c[1:]), 1, 3, n, 2.0, dict(ddim=True, ddim_steps=S, eta=1.0))
    torch.manual_seed(31)
    base = parallel.shared_seed("cpu")
    assert [name for name, _ in ctx.calls] == ["ddim_sample"]
    call = _last(ctx, "ddim_sample")
    steps = len(range(0, m.num_timesteps, m.num_timesteps // S))
    assert call["seed"] is None and call["row0"] == 0
    assert torch.equal(call["x_T"], parallel.per_sample_noise(base, [1, 2], (3, 8, 8)))
    assert torch.equal(call["noise"], parallel.per_sample_noise(base + 1, [1, 2], (steps, 3, 8, 8)).transpose(0, 1).contiguous())
    ctx.calls.clear()
    torch.manual_seed(32)
    m._sample_shard(c, torch.zeros_like(c), 0, n, n, 1.0, dict(ddim=False, ddim_steps=None, timesteps=4))
    torch.manual_seed(32)
    base = parallel.shared_seed("cpu")
    call = _last(ctx, "ddpm_sample")
    assert call["seed"] is None and call["shape"] is None and tuple(call["noise"].shape) == (4, n, 3, 8, 8)
    assert torch.equal(call["x_T"], parallel.per_sample_noise(base, range(n), (3, 8, 8)))


def test_a_seed_together_with_a_noise_stack_is_refused():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    from rdm_amd.models.diffusion.ddim import DDIMSampler
    cond = torch.zeros(2, 4, 512)
    stack = torch.zeros(4, 2, 3, 8, 8)
    # the binding refuses before it touches the context (none exists on this machine)
    with pytest.raises(_lib.RdmError, match="not both"):
        _lib.Context.ddim_sample(None, 4, None, cond, None, np.linspace(0.99, 0.01, 1000), eta=1.0, noise=stack, seed=3)
    with pytest.raises(_lib.RdmError, match="not both"):
        _lib.Context.ddpm_sample(None, 4, None, cond, stack, {}, seed=3)
    for bad in (dict(row0=-1), dict(row0=2 ** 32 - 2)):
        with pytest.raises(_lib.RdmError, match="32 bits"):
            _lib._noise_seed("ddim_sample", 3, bad["row0"], 2)
    assert _lib._noise_seed("ddim_sample", -1, 2 ** 32 - 3, 2) == (2 ** 64 - 1, 2 ** 32 - 3)
    # and so do the samplers
    ctx = StubCtx()
    m = _model(ctx)
    with pytest.raises(ValueError, match="noise"):
        DDIMSampler(m).sample(4, 2, (3, 8, 8), conditioning=cond, eta=1.0, verbose=False, noise=stack, noise_seed=3)
    with pytest.raises(ValueError, match="noise"):
        m.sample(cond=cond, batch_size=2, timesteps=4, noise=stack, noise_seed=3)
    assert not ctx.calls


def test_rdm_sample_eta_and_device_noise_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("rdm_sample_device_noise_cpu", os.path.join(ROOT, "scripts", "rdm_sample.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    opt = mod.parse_args([])
    assert opt.eta == 0.0 and opt.device_noise is False
    assert mod._sampler_kwargs(opt, None) == {}                      # default: the calls are the reference's
    opt = mod.parse_args(["--eta", "0.5", "--device_noise"])
    assert opt.eta == 0.5 and opt.device_noise is True
    assert mod._sampler_kwargs(opt, None) == {"eta": 0.5, "device_noise": True}
    assert mod._sampler_kwargs(mod.parse_args(["--device_noise", "--plms"]), None) == {"plms": True, "device_noise": True}
    acts = {a.option_strings[0]: a for a in mod.build_parser()._actions}
    assert "[native]" in acts["--eta"].help and "[native]" in acts["--device_noise"].help and acts["--eta"].type is float
    assert "--eta" in mod.__doc__ and "--device_noise" in mod.__doc__
