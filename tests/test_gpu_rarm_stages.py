"""The RARM transformer's executors (csrc/rarm_exec.hip: rarm_prepare, the decode step rarm_step, the whole-sequence pass rarm_seq_body)
held stage by stage, per element, TEACHER-FORCED: one call per rdm_debug_tap key (blocks 4000 / 4100 / 4200, include/rdm_hip.h) into a
NaN-prefilled buffer, every tapped tensor compared with the float64 restatement of ITS stage on the library's own tapped inputs under the
bound the project already states for the kernel that runs it, class and wiring near misses included (tests/_rarm_stage_ref.py, pinned
without a GPU by tests/test_rarm_stages_cpu.py).  Shapes: the smallest that reach each form --
  * the decode step's one-launch cross-attention (heads * k <= 128) and its GEMM form by neighbour count and by batch (384 rows; the
    same call in deterministic mode takes the one-launch form), at the tiny spec and at the shipped width with the depth cut to 2;
  * guided sampling: the zeroed unconditional half of ctxkv, the unconditional rows' cross-attention = x + bias;
  * the whole-sequence pass at t = 7, t = L = 24, across a 32-row tile (t = 33 at the shipped width), and over two ranges of its
    RARM_SEQ_ROWS walk (1366 sequences of 24 positions: the second range holds one sequence);
  * the hand-over: the decode steps behind rdm_rarm_sample_prefill's whole-sequence prefix read the cache that pass filled;
  * the tap's own discipline.
The whole-model goldens (tests/test_gpu_rarm.py, test_gpu_rarm_seq.py) stay as they are."""
import pytest
import torch

import _rarm_stage_ref as S
from _train_ref import U
from oracle import rarm as orarm

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
torch.set_num_threads(min(16, torch.get_num_threads()))

_MODELS = {}


def _model(ctx, name):
    """load the tiny spec, or the shipped width (12 heads x 64, context 512, vocab 16386 / 16384, L = 256) with only the depth cut to 2"""
    from rdm_amd import _lib, packing
    if name not in _MODELS:
        spec = orarm.tiny_rarm_spec() if name == "tiny" else orarm.RarmSpec(depth=2)
        sd = S.synth_weights(spec, 77 if name == "tiny" else 78)
        cfg = _lib.make_rarm_cfg(in_channels=spec.vocab_in, out_channels=spec.vocab_out, n_heads=spec.n_heads, d_head=spec.d_head,
                                 depth=spec.depth, context_dim=spec.context_dim, sequence_length=spec.sequence_length)
        _MODELS[name] = (spec, S.Net(sd, spec), cfg, packing.pack("rarm", cfg, sd))
    spec, net, cfg, blob = _MODELS[name]
    ctx.load_rarm(cfg, blob)
    return spec, net


@pytest.fixture(autouse=True)
def _tap_off(ctx):
    yield
    ctx.debug_tap(None, -1)


def _inputs(spec, b, k, t, seed=3):
    g = torch.Generator().manual_seed(seed)
    return S.tokens(spec, b, t, g), torch.randn(b, k, spec.context_dim, generator=g) * 0.45


def _tap(ctx, run, key, shape, dtype, pick=None):
    """one call with the tap on `key` -> (the stage on the CPU in the type the library stores it in -- pick: of it, what the test reads --,
    what the call returned)"""
    buf = torch.full(shape, float("nan"), device=ctx.device, dtype=dtype)      # (a tap that never fires leaves NaN, not a stale stage)
    ctx.debug_tap(buf, key[0], key[1])
    try:
        res = run()
        torch.cuda.synchronize()
    finally:
        ctx.debug_tap(None, -1)
    assert not bool(torch.isnan(buf).any()), f"tap {S.stage_name(key)}: not (wholly) written"
    return (buf if pick is None else pick(key, buf)).cpu(), res


def _taps(ctx, run, shapes, pick=None, same=None):
    """{key: tensor} over `shapes`; same: what every call must return (a tap changes no result)"""
    out = {}
    for key, (shape, dt) in shapes.items():
        out[key], res = _tap(ctx, run, key, shape, dt, pick)
        if same is not None:
            assert torch.equal(res, same), f"the call with tap {S.stage_name(key)} returned another result"
    return out


def _report(what, rep, shapes):
    assert set(rep) == set(shapes), "every tapped stage is checked"
    print(f"[rarm stages] {what}, teacher-forced on the library's own taps:\n" + S.summary(rep))


def _seq_pick(seqs, B, B2, k, t=None):
    """the rows of the sequences `seqs` of a tap of a B2-row call (on the device, before the copy)"""
    idx = torch.as_tensor(seqs)

    def pick(key, buf):
        i = idx.to(buf.device)
        if key[0] == S.PREPARE:
            if key[1] > 16:
                return buf[i]
            return buf.reshape(B if key[1] == 1 else B2, k, -1)[i].reshape(len(seqs) * k, -1)
        if key[0] == S.STEP:
            return buf[:, i]
        return buf.reshape(B2, t, -1)[i].reshape(len(seqs) * t, -1)
    return pick


# ---------------------------------------------------------------------------------------------------- the decode step
@pytest.mark.parametrize("model,b,k,t,form", [("tiny", 3, 4, 6, "one-launch"), ("shipped width", 2, 8, 3, "one-launch"),
                                              ("tiny", 3, 65, 3, "GEMM"), ("shipped width", 2, 16, 2, "GEMM")],
                         ids=["tiny-one_launch", "shipped_width-one_launch", "tiny-gemm_by_k", "shipped_width-gemm_by_k"])
def test_decode_step_stage_by_stage(ctx, model, b, k, t, form):
    spec, net = _model(ctx, model)
    assert S.one_launch(spec, k, b, False) == (form == "one-launch")
    tokens, context = _inputs(spec, b, k, t)
    dt, dc = tokens.to(ctx.device), context.to(ctx.device)
    plain = ctx.rarm_forward(dt, dc)
    shapes = {**S.tap_shapes(spec, S.PREPARE, b, b, k), **S.tap_shapes(spec, S.STEP, b, b, k, steps=t)}
    taps = _taps(ctx, lambda: ctx.rarm_forward(dt, dc), shapes, same=plain)
    rep = S.run_forward(S.Checker(taps), net, tokens, context).report
    _report(f"{model} decode step, {form} cross-attention, b = {b}, k = {k}, t = {t}", rep, shapes)
    assert torch.equal(taps[(S.STEP, 3)].transpose(0, 1), plain.cpu()), "the logits tap of every step is what the call returns"


@pytest.mark.parametrize("det", [False, True], ids=["fast-gemm_by_batch", "deterministic-one_launch"])
def test_decode_step_at_384_rows(ctx, det):
    """384 sequences: the GEMM form by batch, every LayerNorm a pass of its own (all eleven stages); in deterministic mode the same call
    keeps the one-launch form.  Sequences are independent: the stages of sequences 0, 1, 191 and 383 are referenced."""
    spec, net = _model(ctx, "tiny")
    b, k, t, seqs = 384, 4, 2, [0, 1, 191, 383]
    assert S.one_launch(spec, k, b, det) == det and (det or set(S.step_stages(spec, b, k, det)) == set(range(1, 12)))
    tokens, context = _inputs(spec, b, k, t, seed=4)
    dt, dc = tokens.to(ctx.device), context.to(ctx.device)
    was = ctx.deterministic
    ctx.set_deterministic(det)
    try:
        plain = ctx.rarm_forward(dt, dc)
        shapes = {**S.tap_shapes(spec, S.PREPARE, b, b, k, det=det), **S.tap_shapes(spec, S.STEP, b, b, k, steps=t, det=det)}
        taps = _taps(ctx, lambda: ctx.rarm_forward(dt, dc), shapes, pick=_seq_pick(seqs, b, b, k), same=plain)
    finally:
        ctx.set_deterministic(was)
    rep = S.run_forward(S.Checker(taps), net, tokens[seqs], context[seqs], det=det, form_rows=b).report
    _report(f"tiny decode step, 384 sequences, {'deterministic' if det else 'fast'} mode", rep, shapes)


# ---------------------------------------------------------------------------------------------------- sampling
def _sample(ctx, spec, net, B, k, cond_len, steps, guided, prefill):
    tok, context = _inputs(spec, B, k, cond_len, seed=5)
    uniforms = torch.rand(steps, B, generator=torch.Generator().manual_seed(6))
    run = lambda: ctx.rarm_sample(tok, context, steps, uniforms, guidance_scale=2.0 if guided else 1.0, prefill=prefill)
    sampled = run()
    B2 = 2 * B if guided else B
    pos = S.decode_positions(cond_len, steps, prefill)
    shapes = {**S.tap_shapes(spec, S.PREPARE, B, B2, k), **S.tap_shapes(spec, S.STEP, B, B2, k, steps=len(pos))}
    if pos[0] > 0:
        shapes.update(S.tap_shapes(spec, S.SEQ, B, B2, k, t=pos[0], head=False))
    taps = _taps(ctx, run, shapes, same=sampled)
    rep = S.run_sample(S.Checker(taps), net, tok, sampled.cpu(), context, guided, prefill).report
    return taps, rep, shapes


def test_guided_sampling_stage_by_stage(ctx):
    """rdm_rarm_sample, guidance 2.0, B = 3 (six rows), cond_len 2, 3 steps -> decode steps at positions 0 .. 3"""
    spec, net = _model(ctx, "tiny")
    B, k, C = 3, 4, spec.inner_dim
    taps, rep, shapes = _sample(ctx, spec, net, B, k, 2, 3, guided=True, prefill=False)
    _report("tiny guided sampling, B = 3, cond_len 2, 3 steps", rep, shapes)
    assert taps[(S.STEP, 1)].shape[0] == 4
    assert not bool(taps[(S.PREPARE, 2)][B * k:].float().abs().max() > 0), "the unconditional rows of ctxkv are bitwise zero"
    for l in range(spec.depth):                      # the unconditional rows' cross-attention: x + bias, to the rounding of one fp32 add (XattnDecode's bound there)
        x4, x8 = taps[(S.STEP, 16 * (l + 1) + 4)][:, B:].double(), taps[(S.STEP, 16 * (l + 1) + 8)][:, B:].double()
        bias = net.layers[l]["bo2"].double()
        q = float(((x8 - (x4 + bias)).abs() / (3 * U * (x4.abs() + bias.abs()))).max())
        print(f"[rarm stages] block {l}: unconditional rows' x + attn2 against x + bias, worst error / bound {q:.3g}")
        assert q <= 1.0


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_hand_over_from_the_whole_sequence_pass_to_the_decode_steps(ctx, guided):
    """rdm_rarm_sample_prefill, cond_len 5, 2 steps: positions 0 .. 3 in one whole-sequence pass that fills the K / V cache, the decode
    steps at positions 4 and 5 -- their cache attention referenced from the pass's tapped q|k|v plus the decode taps after them"""
    spec, net = _model(ctx, "tiny")
    taps, rep, shapes = _sample(ctx, spec, net, 3, 4, 5, 2, guided=guided, prefill=True)
    _report(f"tiny hand-over, {'guided, ' if guided else ''}cond_len 5, 2 steps", rep, shapes)
    assert taps[(S.SEQ, 1)].shape[0] == (6 if guided else 3) * 4 and taps[(S.STEP, 1)].shape[0] == 2


# ---------------------------------------------------------------------------------------------------- the whole-sequence pass
@pytest.mark.parametrize("model,b,k,t", [("tiny", 3, 4, 7), ("tiny", 3, 4, 24), ("shipped width", 2, 8, 33)], ids=["tiny-t7", "tiny-t24", "shipped_width-t33"])
def test_whole_sequence_pass_stage_by_stage(ctx, model, b, k, t):
    spec, net = _model(ctx, model)
    tokens, context = _inputs(spec, b, k, t)
    dt, dc = tokens.to(ctx.device), context.to(ctx.device)
    plain = ctx.rarm_forward_seq(dt, dc)
    shapes = {**S.tap_shapes(spec, S.PREPARE, b, b, k, decode=False), **S.tap_shapes(spec, S.SEQ, b, b, k, t=t)}
    taps = _taps(ctx, lambda: ctx.rarm_forward_seq(dt, dc), shapes, same=plain)
    rep = S.run_forward_seq(S.Checker(taps), net, tokens, context).report
    _report(f"{model} whole-sequence pass, b = {b}, k = {k}, t = {t}", rep, shapes)
    assert torch.equal(taps[(S.SEQ, 3)].reshape(b, t, -1), plain.cpu()), "the logits tap is what the call returns"


def test_whole_sequence_pass_over_two_ranges(ctx):
    """1366 sequences of 24 positions: 32784 rows > the 32768 of one range, so the second range holds ONE sequence (1365), written at
    its own row offset of the tap and read at its own offset of ctxkv; sequences 0, 1364 (the first range's last) and 1365 are referenced"""
    spec, net = _model(ctx, "tiny")
    b, k, t, seqs = 1366, 4, 24, [0, 1364, 1365]
    assert (b - 1) * t == 32760 <= 32768 < b * t
    tokens, context = _inputs(spec, b, k, t, seed=7)
    dt, dc = tokens.to(ctx.device), context.to(ctx.device)
    shapes = {**S.tap_shapes(spec, S.PREPARE, b, b, k, decode=False), **S.tap_shapes(spec, S.SEQ, b, b, k, t=t)}
    taps = _taps(ctx, lambda: ctx.rarm_forward_seq(dt, dc)[seqs], shapes, pick=_seq_pick(seqs, b, b, k, t))
    rep = S.run_forward_seq(S.Checker(taps), net, tokens[seqs], context[seqs]).report
    _report("tiny whole-sequence pass, 1366 sequences x 24 positions in two ranges (sequences 0, 1364, 1365)", rep, shapes)


# ---------------------------------------------------------------------------------------------------- the tap itself
def test_tap_is_clipped_to_its_buffer_and_off_means_off(ctx):
    spec, net = _model(ctx, "tiny")
    b, k, t, C = 3, 4, 6, spec.inner_dim
    tokens, context = _inputs(spec, b, k, t)
    dt, dc = tokens.to(ctx.device), context.to(ctx.device)
    step, seq = lambda: ctx.rarm_forward(dt, dc), lambda: ctx.rarm_forward_seq(dt, dc)
    plain, plain_seq = step(), seq()
    key = (S.STEP, 16 + 4)
    whole, _ = _tap(ctx, step, key, (t, b, C), torch.float32)
    # a buffer of four and a half steps inside a larger tensor: the steps behind it keep their sentinel, the half step is clipped
    big = torch.full((t * b, C), -7.0, device=ctx.device)
    n = 4 * b + 1
    ctx.debug_tap(big[:n], *key)
    tapped = step()
    torch.cuda.synchronize()
    ctx.debug_tap(None, -1)
    assert torch.equal(big[:n].cpu(), whole.reshape(t * b, C)[:n]) and bool((big[n:] == -7.0).all())
    assert torch.equal(tapped, plain), "a tap changes no result"
    # off: the next call writes nothing
    big.fill_(-7.0)
    again = step()
    torch.cuda.synchronize()
    assert bool((big == -7.0).all()) and torch.equal(again, plain)
    # a decode-step key is silent in the whole-sequence pass, a whole-sequence key in the decode steps; a prepare key fires in both
    for block, run, want in ((S.STEP, seq, plain_seq), (S.SEQ, step, plain)):
        ctx.debug_tap(big, block, 16 + 4)
        res = run()
        torch.cuda.synchronize()
        ctx.debug_tap(None, -1)
        assert bool((big == -7.0).all()) and torch.equal(res, want)
    # the whole-sequence pass clips too
    whole_seq, _ = _tap(ctx, seq, (S.SEQ, 16 + 4), (b * t, C), torch.float32)
    ctx.debug_tap(big[:10], S.SEQ, 16 + 4)
    res = seq()
    torch.cuda.synchronize()
    ctx.debug_tap(None, -1)
    assert torch.equal(big[:10].cpu(), whole_seq[:10]) and bool((big[10:] == -7.0).all()) and torch.equal(res, plain_seq)
