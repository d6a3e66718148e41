"""The DDIM, PLMS and DDPM step kernels (csrc/sampler_steps.hip) alone, through rdm_op_ddim_step / rdm_op_plms_step / rdm_op_ddpm_step, stack
and seeded: every element of every output against the float64 restatements of tests/_step_ref.py within the bounds derived there
(scalar tail, float4 path, a misaligned operand, the second trip of each kernel's stride loop, aliased outputs, every optional output),
into sentinel-guarded buffers; the seeded forms bit for bit against the unseeded ones fed rdm_op_randn's output; every refusal; the
device expf behind DDPM's sd; and the host wiring of the three loops: each logged step of the DDIM and PLMS loops, and a DDPM chain,
rebuilt with the op entries from scalars the test computes itself, bit for bit in deterministic mode."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _step_ref as R
from _util import rel_l2
from test_gpu_plms import tiny  # noqa: F401  (fixture: the tiny UNet on the session context)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENTINEL = 0x7FC5A5A5        # a quiet NaN with a payload no kernel produces: an element left unwritten stays NaN, a guard keeps these bits
FRONT, BACK = 4, 4           # guard elements around every buffer; FRONT keeps an offset-0 operand 16-byte aligned
SEED = 0x5EED0123456789AB


class Bufs:
    """Device buffers with guard elements on both sides.  put(): an input, whose host array is kept so that it can be shown unchanged
    (no second device copy); out(): an output full of the sentinel.  off: floats past a 16-byte aligned address."""

    def __init__(self, ctx):
        self.d, self.items = ctx.device, []

    def _new(self, n, off, what, host=None):
        buf = torch.full((FRONT + off + n + BACK,), SENTINEL, dtype=torch.int32, device=self.d).view(torch.float32)
        t = buf[FRONT + off:FRONT + off + n]
        assert t.data_ptr() % 16 == 4 * (off % 4) and t.is_contiguous()
        self.items.append([buf, FRONT + off, n, host, what])
        return t

    def put(self, a, off=0, what="input"):
        if a is None:
            return None
        t = self._new(a.size, off, what, a)
        t.copy_(torch.from_numpy(a))
        return t

    def out(self, n, off=0, what="output"):
        return self._new(n, off, what)

    def check(self, written=()):
        """guards intact everywhere; every input that is not in `written` (aliased with an output) unchanged"""
        torch.cuda.synchronize()
        skip = {t.data_ptr() for t in written if t is not None}
        for buf, lo, n, host, what in self.items:
            bits = buf.view(torch.int32)
            assert bool((bits[:lo] == SENTINEL).all()) and bool((bits[lo + n:] == SENTINEL).all()), f"{what}: written outside its {n} elements"
            if host is not None and buf[lo:lo + n].data_ptr() not in skip:
                assert np.array_equal(_np(buf[lo:lo + n]).view(np.uint32), host.view(np.uint32)), f"{what}: an input changed"

    def drop(self, *tensors):
        """forget checked buffers, so that their memory is free once the caller's own references are gone"""
        gone = {t.data_ptr() for t in tensors if t is not None}
        self.items = [it for it in self.items if it[0][it[1]:it[1] + it[2]].data_ptr() not in gone]


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(kind, case_id, lines, margin):
    print(f"[step ops] {kind} {case_id}: " + "; ".join(lines) + f"; closest near miss {margin:.3g}")


# ---- the unseeded kernels, element by element
@pytest.mark.parametrize("config", list(R.DDIM_CONFIGS))
@pytest.mark.parametrize("n,off,point", R.GRID, ids=R.GRID_IDS)
def test_ddim_step_per_element_against_fp64(ctx, n, off, point, config):
    """ddim_step_kernel is scalar only: n = 2048 * 256 + 1 puts one element on the stride loop's second trip.  x and every output start
    `off` floats past an aligned address."""
    cfg, _, _, _, dup, pred, in_place = R.DDIM_CONFIGS[config]
    arr, sc = R.ddim_case(n, point, config)
    b = Bufs(ctx)
    x, eps, noise = b.put(arr["x"], off, "x"), b.put(arr["eps"], 0, "eps"), b.put(arr["noise"], 0, "noise")
    x_prev = x if in_place else b.out(n, off, "x_prev")
    x_dup = b.out(n, off, "x_dup") if dup else None
    pred_x0 = b.out(n, off, "pred_x0") if pred else None
    ctx.op_ddim_step(x, eps, noise, sc["cfg"], sc["scale"], sc["a_t"], sc["a_prev"], sc["sigma_t"], sc["s1m"], sc["temperature"], x_prev,
                     x_dup=x_dup, pred_x0=pred_x0)
    b.check(written=[x_prev])
    got = {"x_prev": _np(x_prev)}
    if pred:
        got["pred_x0"] = _np(pred_x0)
    lines, _, margin = R.check("ddim", arr, sc, got, R.ddim_misses(sc["cfg"], arr["noise"], sc["sigma_t"], sc["temperature"]))
    _report("ddim", f"{config} n={n} offset={off} index={R.DDIM_POINTS[point]}", lines, margin)
    if dup:
        assert _same_bits(x_dup, x_prev)


@pytest.mark.parametrize("config", list(R.PLMS_CONFIGS))
@pytest.mark.parametrize("n,off,point", R.GRID, ids=R.GRID_IDS)
def test_plms_step_per_element_against_fp64(ctx, n, off, point, config):
    """plms_step_kernel<4> at offset 0 and n % 4 == 0 (second trip: n / 4 > 2048 * 256), else <1> (second trip: n > 2048 * 256; offset 1
    puts an n % 4 == 0 call there).  Every configuration runs unaliased with x_dup and pred_x0; order 3 runs again as the loop's full ring
    does -- e_store = h3, x_out = x -- and must return the same bits."""
    cfg, mode, order = R.PLMS_CONFIGS[config]
    arr, sc = R.plms_case(n, point, config)
    args = (sc["cfg"], sc["scale"], sc["a_t"], sc["a_prev"], sc["s1m"], mode, order)
    b = Bufs(ctx)
    x, eps = b.put(arr["x"], off, "x"), b.put(arr["eps"], 0, "eps")
    e_prev, h1, h2, h3 = (b.put(arr[k], 0, k) for k in ("e_prev", "h1", "h2", "h3"))
    x_out, x_dup, pred_x0 = b.out(n, off, "x_out"), b.out(n, off, "x_dup"), b.out(n, off, "pred_x0")
    e_store = b.out(n, off, "e_store") if mode != R.PLMS_EULER_B else None
    ctx.op_plms_step(x, eps, *args, x_out, e_prev=e_prev, h1=h1, h2=h2, h3=h3, e_store=e_store, x_dup=x_dup, pred_x0=pred_x0)
    b.check()
    got = {"x_out": _np(x_out), "pred_x0": _np(pred_x0)}
    if e_store is not None:
        got["e_store"] = _np(e_store)
    lines, _, margin = R.check("plms", arr, sc, got, R.plms_misses(sc["cfg"], mode, order))
    _report("plms", f"{config} n={n} offset={off} index={R.DDIM_POINTS[point]}", lines, margin)
    assert _same_bits(x_dup, x_out)
    if e_store is not None and not cfg:
        assert _same_bits(e_store, eps), "the unguided e_t is eps itself"
    if order == 3:
        # the first run's outputs are on the host by now (got): its buffers go before the aliased run's are made, so that the largest
        # case holds ten buffers of n elements at a time
        b.drop(x, h3, x_out, x_dup, pred_x0, e_store)
        del x, h3, x_out, x_dup, pred_x0, e_store
        x2, h3b = b.put(arr["x"], off, "x (aliased run)"), b.put(arr["h3"], 0, "h3 (aliased run)")
        pred2 = b.out(n, off, "pred_x0 (aliased run)")
        ctx.op_plms_step(x2, eps, *args, x2, h1=h1, h2=h2, h3=h3b, e_store=h3b, pred_x0=pred2)
        b.check(written=[x2, h3b])
        for name, t in (("x_out", x2), ("e_store", h3b), ("pred_x0", pred2)):
            assert np.array_equal(_np(t).view(np.uint32), got[name].view(np.uint32)), f"{name}: the aliased run differs from the unaliased one"


@pytest.mark.parametrize("config", list(R.DDPM_CONFIGS))
@pytest.mark.parametrize("n,off,point", R.GRID, ids=R.GRID_IDS)
def test_ddpm_step_per_element_against_fp64(ctx, n, off, point, config):
    """ddpm_step_kernel is scalar only, as DDIM's.  nonzero = 0 with a noise operand must ignore it; the clamp decides at least a tenth of
    the elements on each side (test_step_ops_cpu.py asserts it on these inputs)."""
    clip, nonzero, temperature, _, in_place = R.DDPM_CONFIGS[config]
    arr, sc = R.ddpm_case(n, point, config)
    b = Bufs(ctx)
    x, eps, noise = b.put(arr["x"], off, "x"), b.put(arr["eps"], 0, "eps"), b.put(arr["noise"], 0, "noise")
    x_prev = x if in_place else b.out(n, off, "x_prev")
    ctx.op_ddpm_step(x, eps, noise, sc["sr"], sc["srm1"], sc["c1"], sc["c2"], sc["log_var"], clip, nonzero, temperature, x_prev)
    b.check(written=[x_prev])
    lines, _, margin = R.check("ddpm", arr, sc, {"x_prev": _np(x_prev)}, R.ddpm_misses(arr["noise"], clip, nonzero, temperature))
    _report("ddpm", f"{config} n={n} offset={off} t={R.DDPM_POINTS[point]}", lines, margin)


def test_device_expf_of_the_posterior_log_variances(ctx):
    """sd = expf(0.5 log_var) for the schedule's 1000 values against float64 exp: x = eps = 0 and noise = temperature = 1 make the kernel
    return sd itself.  The worst relative error is printed and held to R.SD_REL = max(4 x the recorded measurement, 4 ulp)."""
    lv = R.ddpm_arrays()["posterior_log_variance_clipped"]
    d = ctx.device
    zero, one, out = torch.zeros(1, device=d), torch.ones(1, device=d), torch.full((lv.shape[0],), float("nan"), device=d)
    for t in range(lv.shape[0]):
        ctx.op_ddpm_step(zero, zero, one, 0.0, 0.0, 0.0, 0.0, float(lv[t]), False, True, 1.0, out[t:t + 1])
    torch.cuda.synchronize()
    want = np.exp(0.5 * lv.astype(np.float64))
    rel = np.abs(_np(out).astype(np.float64) - want) / want
    t_worst = int(rel.argmax())
    print(f"[step ops] expf(0.5 log_var): worst relative error {rel.max():.4e} = {rel.max() / 2.0 ** -23:.3f} ulp at t = {t_worst} "
          f"(recorded {R.SD_MEASURED:.4e}, allowance {R.SD_REL:.4e})")
    assert rel.max() <= R.SD_REL


# ---- the seeded kernels against the unseeded ones
def LAST(B):
    """the last row0 check_noise_rows accepts for B rows: row0 + B <= 2^32 - 1"""
    return 2 ** 32 - 1 - B


SEEDED = [(3, 768, 0, 0), (3, 768, LAST(3), 3), (5, 12, 0, 3), (5, 12, LAST(5), 0), (4856, 432, LAST(4856), 3)]
SEEDED_IDS = ["b3x768_row0_step0", "b3x768_lastrows_step3", "b5x12_row0_step3", "b5x12_lastrows_step0", "b4856x432_second_trip_lastrows_step3"]


@pytest.mark.parametrize("kind", ["ddim_guided_all_outputs", "ddim_unguided_bare", "ddpm_clip"])
@pytest.mark.parametrize("B,per_row,row0,step", SEEDED, ids=SEEDED_IDS)
def test_seeded_step_equals_unseeded_on_randn_bitwise(ctx, B, per_row, row0, step, kind):
    """The kernel comments claim bit-identity with the unseeded form on rdm_op_randn(stream 1).  5 x 12: three blocks per row, so rows
    change inside a wavefront; 4856 x 432: n / 4 = 524 448 vectors on 2048 x 256 threads and 108 blocks per row, so a thread's second
    trip lands in another row and block than its first."""
    n = B * per_row
    b = Bufs(ctx)
    guided = kind == "ddim_guided_all_outputs"
    arr = R.inputs(n, 7 * n + step, ("x", "eps"), 2 if guided else 1)
    x, eps = b.put(arr["x"], 0, "x"), b.put(arr["eps"], 0, "eps")
    z = ctx.op_randn(SEED, B, per_row, row0=row0, step=step, stream=1).reshape(-1)
    outs = [[b.out(n, 0, f"{w} ({form})") for w in ("x_prev", "x_dup", "pred_x0")] for form in ("unseeded", "seeded")]
    if kind == "ddpm_clip":
        sc = R.ddpm_scalars(500)
        ctx.op_ddpm_step(x, eps, z, *sc, True, True, 0.7, outs[0][0])
        ctx.op_ddpm_step(x, eps, None, *sc, True, True, 0.7, outs[1][0], seed=SEED, row0=row0, per_row=per_row, step=step)
        used = 1
    else:
        _, a_t, a_prev, sigma_t, s1m = R.ddim_scalars(10, 5, 0.7)
        sc = (guided, 2.0 if guided else 1.0, a_t, a_prev, sigma_t, s1m, 0.7)
        opt = [dict(x_dup=o[1], pred_x0=o[2]) if guided else {} for o in outs]
        ctx.op_ddim_step(x, eps, z, *sc, outs[0][0], **opt[0])
        ctx.op_ddim_step(x, eps, None, *sc, outs[1][0], seed=SEED, row0=row0, per_row=per_row, step=step, **opt[1])
        used = 3 if guided else 1
    b.check()
    for u, s in list(zip(*outs))[:used]:
        assert not torch.isnan(s).any() and _same_bits(u, s)
    for u, s in list(zip(*outs))[used:]:
        assert bool((s.view(torch.int32) == SENTINEL).all()) and bool((u.view(torch.int32) == SENTINEL).all()), "an output that was not requested was written"


# ---- refusals
def test_step_op_refusals_leave_the_context_usable(ctx):
    """every refusal raises RdmError with its own message, leaves the output it was given as it was, and a following good call returns
    the bits it returned before"""
    from rdm_amd import _lib
    from rdm_amd._lib import Noise, RdmError
    lib, P = _lib.lib, _lib._ptr
    d = ctx.device
    n, per_row = 48, 12
    g = torch.Generator(device=d).manual_seed(3)
    v = lambda m=n: torch.randn(m, device=d, generator=g)
    x, eps2, e1, h1, h2, h3, nz = v(), v(2 * n), v(), v(), v(), v(), v()
    _, a_t, a_prev, sigma_t, s1m = R.ddim_scalars(10, 5, 0.7)
    dp = R.ddpm_scalars(500)
    odd = torch.randn(n + 4, device=d, generator=g)[1:n + 1]       # one float past alignment

    def good():
        outs = [torch.full((n,), float("nan"), device=d) for _ in range(8)]
        ctx.op_ddim_step(x, eps2, nz, True, 2.0, a_t, a_prev, sigma_t, s1m, 0.7, outs[0], pred_x0=outs[1])
        ctx.op_ddim_step(x, eps2, None, True, 2.0, a_t, a_prev, sigma_t, s1m, 0.7, outs[2], seed=SEED, row0=4, per_row=per_row, step=2)
        ctx.op_plms_step(x, eps2, True, 2.0, a_t, a_prev, s1m, R.PLMS_STEP, 3, outs[3], h1=h1, h2=h2, h3=h3, e_store=outs[4], pred_x0=outs[5])
        ctx.op_ddpm_step(x, eps2[:n], nz, *dp, True, True, 0.7, outs[6])
        ctx.op_ddpm_step(x, eps2[:n], None, *dp, True, True, 0.7, outs[7], seed=SEED, row0=4, per_row=per_row, step=2)
        torch.cuda.synchronize()
        assert all(not torch.isnan(o).any() for o in outs)
        return torch.stack(outs)

    base = good()
    o = torch.full((n,), SENTINEL, dtype=torch.int32, device=d).view(torch.float32)       # the output of every refused call: must stay as it is
    odd_before = odd.clone()
    ddim_raw = lambda x_, e_, o_, n_: ctx._check(lib.rdm_op_ddim_step(ctx._h, P(x_), P(e_), None, n_, 0, 1.0, a_t, a_prev, 0.0, s1m, 1.0, P(o_), None, None))
    seeded = lambda pr, row0, stack=None: C.byref(Noise(stack=P(stack), seeded=1, seed=1, row0=row0, per_row=pr, step=0))      # a filled rdm_noise
    ddim_seeded_raw = lambda x_, e_, o_, n_, pr, row0, stack=None: ctx._check(lib.rdm_op_ddim_step(ctx._h, P(x_), P(e_), seeded(pr, row0, stack), n_, 0, 1.0, a_t,
                                                                                                   a_prev, sigma_t, s1m, 1.0, P(o_), None, None))
    plms_raw = lambda x_, e_, o_, n_: ctx._check(lib.rdm_op_plms_step(ctx._h, P(x_), P(e_), None, None, None, None, n_, 0, 1.0, a_t, a_prev, s1m, 1, 0,
                                                                      P(o), P(o_), None, None))
    ddpm_raw = lambda x_, e_, z_, o_, n_, nonzero=1: ctx._check(lib.rdm_op_ddpm_step(ctx._h, P(x_), P(e_), C.byref(Noise(stack=P(z_))), n_, *dp, 1, nonzero, 1.0,
                                                                                     P(o_)))
    ddpm_seeded_raw = lambda x_, e_, o_, n_, pr, row0, stack=None: ctx._check(lib.rdm_op_ddpm_step(ctx._h, P(x_), P(e_), seeded(pr, row0, stack), n_, *dp, 1, 1,
                                                                                                   1.0, P(o_)))
    plms = lambda mode, order, **kw: ctx.op_plms_step(x, eps2, True, 2.0, a_t, a_prev, s1m, mode, order, o, **kw)
    e = eps2[:n]
    # each case has one fault, and the message says which refusal fired
    ARG, SHAPE, ROWS, COUNT = "bad argument", "multiple of 4 that divides n, and every operand 16-byte aligned", "row0 + B must fit 32 bits", "B and per_row must be >= 1"
    BOTH = "give a seed or a stack, not both"
    bad = [
        ("ddim: n = 0", "rdm_op_ddim_step: " + ARG, lambda: ddim_raw(x, e, o, 0)),
        ("ddim: null x", "rdm_op_ddim_step: " + ARG, lambda: ddim_raw(None, e, o, n)),
        ("ddim: null eps", "rdm_op_ddim_step: " + ARG, lambda: ddim_raw(x, None, o, n)),
        ("ddim: null x_prev", "rdm_op_ddim_step: " + ARG, lambda: ddim_raw(x, e, None, n)),
        ("ddim seeded: n = -4", "rdm_op_ddim_step: " + ARG, lambda: ddim_seeded_raw(x, e, o, -4, per_row, 0)),
        ("ddim seeded: null x_prev", "rdm_op_ddim_step: " + ARG, lambda: ddim_seeded_raw(x, e, None, n, per_row, 0)),
        ("ddim seeded: per_row % 4", "rdm_op_ddim_step (seeded): per_row must be a " + SHAPE, lambda: ddim_seeded_raw(x, e, o, n, 6, 0)),
        ("ddim seeded: n % per_row", "rdm_op_ddim_step (seeded): per_row must be a " + SHAPE, lambda: ddim_seeded_raw(x, e, o, 40, per_row, 0)),
        ("ddim seeded: misaligned x", "rdm_op_ddim_step (seeded): per_row must be a " + SHAPE, lambda: ddim_seeded_raw(odd, e, o, n, per_row, 0)),
        ("ddim seeded: misaligned x_prev", "rdm_op_ddim_step (seeded): per_row must be a " + SHAPE, lambda: ddim_seeded_raw(x, e, odd, n, per_row, 0)),
        ("ddim seeded: per_row 0", "rdm_op_ddim_step (seeded): " + COUNT, lambda: ddim_seeded_raw(x, e, o, n, 0, 0)),
        ("ddim seeded: row0 + B past 32 bits", "rdm_op_ddim_step (seeded): " + ROWS, lambda: ddim_seeded_raw(x, e, o, n, per_row, 2 ** 32 - n // per_row)),
        ("ddim seeded: negative row0", "rdm_op_ddim_step (seeded): " + ROWS, lambda: ddim_seeded_raw(x, e, o, n, per_row, -1)),
        ("ddim seeded: with a stack", "rdm_op_ddim_step: " + BOTH, lambda: ddim_seeded_raw(x, e, o, n, per_row, 0, stack=nz)),
        ("plms: n = 0", "rdm_op_plms_step: " + ARG, lambda: plms_raw(x, e, o, 0)),
        ("plms: null x", "rdm_op_plms_step: " + ARG, lambda: plms_raw(None, e, o, n)),
        ("plms: null eps", "rdm_op_plms_step: " + ARG, lambda: plms_raw(x, None, o, n)),
        ("plms: null x_out", "rdm_op_plms_step: " + ARG, lambda: plms_raw(x, e, None, n)),
        ("plms: mode 3", "mode 3 is none of", lambda: plms(3, 0, e_store=h1)),
        ("plms: mode -1", "mode -1 is none of", lambda: plms(-1, 0, e_store=h1)),
        ("plms: order 4", "order 4 outside 0..3", lambda: plms(R.PLMS_STEP, 4, h1=h1, h2=h2, h3=h3, e_store=e1)),
        ("plms: order -1", "order -1 outside 0..3", lambda: plms(R.PLMS_STEP, -1, e_store=e1)),
        ("plms: Euler B without e_prev", "Euler B reads e_prev, which is null", lambda: plms(R.PLMS_EULER_B, 0)),
        ("plms: order 1 without h1", "order 1 needs history operands that are null", lambda: plms(R.PLMS_STEP, 1, e_store=e1)),
        ("plms: order 2 without h2", "order 2 needs history operands that are null", lambda: plms(R.PLMS_STEP, 2, h1=h1, e_store=e1)),
        ("plms: order 3 without h3", "order 3 needs history operands that are null", lambda: plms(R.PLMS_STEP, 3, h1=h1, h2=h2, e_store=e1)),
        ("plms: step without e_store", "mode 0 writes e_store, which is null", lambda: plms(R.PLMS_STEP, 0)),
        ("plms: order 3 without e_store", "mode 0 writes e_store, which is null", lambda: plms(R.PLMS_STEP, 3, h1=h1, h2=h2, h3=h3)),
        ("plms: Euler A without e_store", "mode 1 writes e_store, which is null", lambda: plms(R.PLMS_EULER_A, 0)),
        ("ddpm: n = 0", "rdm_op_ddpm_step: " + ARG, lambda: ddpm_raw(x, e, nz, o, 0)),
        ("ddpm: null x", "rdm_op_ddpm_step: " + ARG, lambda: ddpm_raw(None, e, nz, o, n)),
        ("ddpm: null eps", "rdm_op_ddpm_step: " + ARG, lambda: ddpm_raw(x, None, nz, o, n)),
        ("ddpm: null x_prev", "rdm_op_ddpm_step: " + ARG, lambda: ddpm_raw(x, e, nz, None, n)),
        ("ddpm: nonzero with neither noise nor seed", "nonzero needs a noise operand", lambda: ctx.op_ddpm_step(x, e, None, *dp, True, True, 1.0, o)),
        ("ddpm seeded: null x", "rdm_op_ddpm_step: " + ARG, lambda: ddpm_seeded_raw(None, e, o, n, per_row, 0)),
        ("ddpm seeded: per_row % 4", "rdm_op_ddpm_step (seeded): per_row must be a " + SHAPE, lambda: ddpm_seeded_raw(x, e, o, n, 6, 0)),
        ("ddpm seeded: n % per_row", "rdm_op_ddpm_step (seeded): per_row must be a " + SHAPE, lambda: ddpm_seeded_raw(x, e, o, 40, per_row, 0)),
        ("ddpm seeded: misaligned eps", "rdm_op_ddpm_step (seeded): per_row must be a " + SHAPE, lambda: ddpm_seeded_raw(x, odd, o, n, per_row, 0)),
        ("ddpm seeded: misaligned x_prev", "rdm_op_ddpm_step (seeded): per_row must be a " + SHAPE, lambda: ddpm_seeded_raw(x, e, odd, n, per_row, 0)),
        ("ddpm seeded: row0 + B past 32 bits", "rdm_op_ddpm_step (seeded): " + ROWS, lambda: ddpm_seeded_raw(x, e, o, n, per_row, 2 ** 32 - n // per_row)),
        ("ddpm seeded: with a stack", "rdm_op_ddpm_step: " + BOTH, lambda: ddpm_seeded_raw(x, e, o, n, per_row, 0, stack=nz)),
    ]
    for what, message, call in bad:
        with pytest.raises(RdmError, match=re.escape(message)):
            call()
        torch.cuda.synchronize()
        assert bool((o.view(torch.int32) == SENTINEL).all()) and _same_bits(odd, odd_before), f"{what}: the refused call wrote its output"
        assert _same_bits(good(), base), f"after {what}"
    # what the last step of the loop does: nonzero = 0 needs no noise operand
    ddpm_raw(x, e, None, o, n, nonzero=0)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all()


# ---- the loops launch these kernels with the right scalars
B_LOOP, S_LOOP, HW, SCALE = 3, 6, 16, 2.0


def _loop_inputs(ctx, seed):
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(B_LOOP, 3, HW, HW, generator=g).to(ctx.device)
    cond = (torch.randn(B_LOOP, 4, 512, generator=g) * 0.45).to(ctx.device)
    return x_T, cond, torch.zeros_like(cond), g


@pytest.mark.parametrize("mode", ["eta07_t07_noise_stack", "eta07_t07_seeded", "eta0"])
def test_ddim_loop_steps_rebuilt_with_the_op_entry_bitwise(tiny, mode):
    """Deterministic mode, the tiny UNet, B = 3 at 16 x 16, CFG 2.0, S = 6 (7 timesteps), every step logged: step i rebuilt from
    x_inter[i-1] with ctx.unet_forward_guided and op_ddim_step on scalars this test computes from alphas_cumprod (R.ddim_scalars) must be
    x_inter[i] and pred_x0_inter[i] bit for bit."""
    ctx, _, _ = tiny
    x_T, cond, uncond, g = _loop_inputs(ctx, 41)
    eta, temperature = (0.0, 1.0) if mode == "eta0" else (0.7, 0.7)
    total = R.ddim_steps(S_LOOP)
    assert total == 7
    per_row = x_T[0].numel()
    kw = {}
    if mode == "eta07_t07_noise_stack":
        kw["noise"] = torch.randn(total, *x_T.shape, generator=g).to(ctx.device)
    elif mode == "eta07_t07_seeded":
        kw.update(seed=SEED, row0=9)
    ctx.set_deterministic(True)
    try:
        z, xi, pi = ctx.ddim_sample(S_LOOP, x_T, cond, uncond, R.ACP, eta=eta, scale=SCALE, log_every_t=1, temperature=temperature,
                                    want_intermediates=True, **kw)
        assert xi.shape[0] == pi.shape[0] == total and torch.equal(z, xi[-1])
        for i in range(total):
            t, a_t, a_prev, sigma_t, s1m = R.ddim_scalars(S_LOOP, total - 1 - i, eta)
            x = (x_T if i == 0 else xi[i - 1]).contiguous()
            eps = ctx.unet_forward_guided(x, t, cond, uncond)
            x_prev, pred = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
            step_kw = dict(seed=SEED, row0=9, per_row=per_row, step=i) if mode == "eta07_t07_seeded" else {}
            noise = kw["noise"][i].contiguous() if "noise" in kw else None
            ctx.op_ddim_step(x, eps, noise, True, SCALE, a_t, a_prev, sigma_t, s1m, temperature, x_prev, pred_x0=pred, **step_kw)
            torch.cuda.synchronize()
            assert _same_bits(x_prev, xi[i]), f"step {i} (t = {t}): x_inter differs, rel L2 {rel_l2(x_prev, xi[i]):.3e}"
            assert _same_bits(pred, pi[i]), f"step {i} (t = {t}): pred_x0 differs, rel L2 {rel_l2(pred, pi[i]):.3e}"
    finally:
        ctx.set_deterministic(False)


def test_plms_loop_steps_rebuilt_with_the_op_entry_bitwise(tiny):
    """All 7 steps of the S = 6 PLMS loop: the two Euler phases with the extra forward at t_next, then orders 1, 2, 3, 3 with the ring
    rotating by pointer (the newest e_t into the oldest slot once three are held)."""
    ctx, _, _ = tiny
    x_T, cond, uncond, _ = _loop_inputs(ctx, 42)
    total = R.ddim_steps(S_LOOP)
    orders = []
    ctx.set_deterministic(True)
    try:
        z, xi, pi = ctx.plms_sample(S_LOOP, x_T, cond, uncond, R.ACP, scale=SCALE, log_every_t=1, want_intermediates=True)
        assert xi.shape[0] == pi.shape[0] == total == 7 and torch.equal(z, xi[-1])
        hist = []                                        # newest first
        for i in range(total):
            index = total - 1 - i
            t, a_t, a_prev, _, s1m = R.ddim_scalars(S_LOOP, index, 0.0)
            sc = (True, SCALE, a_t, a_prev, s1m)
            x = (x_T if i == 0 else xi[i - 1]).contiguous()
            eps = ctx.unet_forward_guided(x, t, cond, uncond)
            x_out, pred = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
            if not hist:
                e_t, x_tmp = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
                ctx.op_plms_step(x, eps, *sc, R.PLMS_EULER_A, 0, x_tmp, e_store=e_t)
                t_next = R.ddim_scalars(S_LOOP, max(index - 1, 0), 0.0)[0]
                eps_next = ctx.unet_forward_guided(x_tmp, t_next, cond, uncond)
                ctx.op_plms_step(x, eps_next, *sc, R.PLMS_EULER_B, 0, x_out, e_prev=e_t, pred_x0=pred)
                hist = [e_t]
                orders.append("euler")
            else:
                order = len(hist)
                e_t = hist[2] if order == 3 else torch.full_like(x, float("nan"))
                h = hist + [None] * (3 - order)
                ctx.op_plms_step(x, eps, *sc, R.PLMS_STEP, order, x_out, h1=h[0], h2=h[1], h3=h[2], e_store=e_t, pred_x0=pred)
                hist = ([e_t] + hist)[:3]
                orders.append(order)
            torch.cuda.synchronize()
            assert _same_bits(x_out, xi[i]), f"step {i} ({orders[-1]}, t = {t}): x_inter differs, rel L2 {rel_l2(x_out, xi[i]):.3e}"
            assert _same_bits(pred, pi[i]), f"step {i} ({orders[-1]}, t = {t}): pred_x0 differs, rel L2 {rel_l2(pred, pi[i]):.3e}"
    finally:
        ctx.set_deterministic(False)
    assert orders == ["euler", 1, 2, 3, 3, 3, 3]


@pytest.mark.parametrize("mode", ["noise_stack", "seeded"])
def test_ddpm_chain_of_op_entries_against_the_loop(tiny, mode):
    """The DDPM loop logs nothing: 4 timesteps of ctx.unet_forward + op_ddpm_step with the caller's posterior arrays (clip on,
    temperature 0.7) against ctx.ddpm_sample's final latent, in deterministic mode.  The stand-alone unguided forward is the loop's
    forward bit for bit there, so the chain is held to bit equality like the guided loops."""
    ctx, _, _ = tiny
    x_T, cond, _, g = _loop_inputs(ctx, 43)
    T4 = 4
    arrays = R.ddpm_arrays()
    per_row = x_T[0].numel()
    ctx.set_deterministic(True)
    try:
        if mode == "noise_stack":
            noise = torch.randn(T4, *x_T.shape, generator=g).to(ctx.device)
            z = ctx.ddpm_sample(T4, x_T, cond, noise, arrays, clip_denoised=True, temperature=0.7)
        else:
            z = ctx.ddpm_sample(T4, x_T, cond, None, arrays, clip_denoised=True, temperature=0.7, seed=SEED, row0=11)
        x = x_T.clone()
        for n_, t in enumerate(reversed(range(T4))):
            eps = ctx.unet_forward(x, torch.full((B_LOOP,), t, dtype=torch.long, device=ctx.device), cond)
            nxt = torch.full_like(x, float("nan"))
            if mode == "noise_stack":
                ctx.op_ddpm_step(x, eps, noise[n_].contiguous(), *R.ddpm_scalars(t), True, t != 0, 0.7, nxt)
            elif t != 0:
                ctx.op_ddpm_step(x, eps, None, *R.ddpm_scalars(t), True, True, 0.7, nxt, seed=SEED, row0=11, per_row=per_row, step=n_)
            else:
                ctx.op_ddpm_step(x, eps, None, *R.ddpm_scalars(t), True, False, 0.7, nxt)
            x = nxt
        torch.cuda.synchronize()
    finally:
        ctx.set_deterministic(False)
    bitwise, err = _same_bits(x, z), rel_l2(x, z)
    print(f"[step ops] ddpm chain ({mode}): bitwise equal to the loop: {bitwise}; rel L2 {err:.3e}")
    assert bitwise, f"the chain differs from the loop: rel L2 {err:.3e}"
