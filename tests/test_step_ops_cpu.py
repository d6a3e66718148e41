"""The bounds test_gpu_step_ops.py holds the DDIM, PLMS and DDPM step kernels to, checked without a GPU: numpy fp32 emulations of the kernel
text (for the two kernels that allow FMA contraction both the uncontracted and the fully contracted form) stand in for the kernels at
the GPU file's inputs and must stay inside every per-element bound of tests/_step_ref.py, every near miss must fall outside, the
conditions on DDPM's clamp hold on the reference, the dirc bound holds over the schedules, the new symbols are in the header and the
library, and the bindings' size checks raise before any device is touched."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _step_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every (n, schedule point) of the GPU grid once: the inputs depend on n, the point and the configuration, not on the offset
CPU_GRID = sorted({(n, point) for n, _, point in R.GRID})
CPU_IDS = [f"n{n}_{'edge' if p else 'mid'}" for n, p in CPU_GRID]


@pytest.mark.parametrize("config", list(R.DDIM_CONFIGS))
@pytest.mark.parametrize("n,point", CPU_GRID, ids=CPU_IDS)
def test_ddim_emulation_within_bound_and_near_misses_outside(n, point, config):
    arr, sc = R.ddim_case(n, point, config)
    misses = R.ddim_misses(sc["cfg"], arr["noise"], sc["sigma_t"], sc["temperature"])
    for contracted in (False, True):
        xp, x0 = R.ddim_fp32(**arr, **sc, contracted=contracted)
        lines, worst, margin = R.check("ddim", arr, sc, {"x_prev": xp, "pred_x0": x0}, misses)
        print(f"[step ops] ddim {config} n={n} point={point} contracted={contracted}: " + "; ".join(lines) + f"; closest near miss {margin:.3g}")


@pytest.mark.parametrize("config", list(R.PLMS_CONFIGS))
@pytest.mark.parametrize("n,point", CPU_GRID, ids=CPU_IDS)
def test_plms_emulation_within_bound_and_near_misses_outside(n, point, config):
    arr, sc = R.plms_case(n, point, config)
    xo, x0, e = R.plms_fp32(**arr, **sc)
    got = {"x_out": xo, "pred_x0": x0}
    if sc["mode"] != R.PLMS_EULER_B:
        got["e_store"] = e
    lines, worst, margin = R.check("plms", arr, sc, got, R.plms_misses(sc["cfg"], sc["mode"], sc["order"]))
    print(f"[step ops] plms {config} n={n} point={point}: " + "; ".join(lines) + f"; closest near miss {margin:.3g}")


@pytest.mark.parametrize("config", list(R.DDPM_CONFIGS))
@pytest.mark.parametrize("n,point", CPU_GRID, ids=CPU_IDS)
def test_ddpm_emulation_within_bound_and_near_misses_outside(n, point, config):
    arr, sc = R.ddpm_case(n, point, config)
    misses = R.ddpm_misses(arr["noise"], sc["clip"], sc["nonzero"], sc["temperature"])
    for contracted in (False, True):
        got = {"x_prev": R.ddpm_fp32(**arr, **sc, contracted=contracted)}
        lines, worst, margin = R.check("ddpm", arr, sc, got, misses)
        print(f"[step ops] ddpm {config} n={n} point={point} contracted={contracted}: " + "; ".join(lines) + f"; closest near miss {margin:.3g}")


@pytest.mark.parametrize("config", [c for c, v in R.DDPM_CONFIGS.items() if v[0]])
@pytest.mark.parametrize("n,off,point", R.GRID, ids=R.GRID_IDS)
def test_ddpm_clamp_decides_elements_and_few_sit_on_the_boundary(n, off, point, config):
    """at every clipped GPU case: at least a tenth of the float64 x0 beyond +1 and a tenth beyond -1, at most 1e-3 of the elements within
    their own x0 tolerance of +-1 (those may take either branch)"""
    arr, sc = R.ddpm_case(n, point, config)
    ref = R.ddpm(**arr, **sc)
    above, below = ref["beyond"]
    print(f"[step ops] ddpm {config} n={n} t={R.DDPM_POINTS[point]}: x0 > 1 {above:.3f}, x0 < -1 {below:.3f}, boundary share {ref['boundary']:.2e}")
    assert above >= 0.1 and below >= 0.1
    assert ref["boundary"] <= 1e-3


def test_dirc_bound_over_the_schedules():
    worst = 0.0
    for S in (6, 10, 50):
        for eta in (0.0, 0.7, 1.0):
            for index in range(R.ddim_steps(S)):
                _, _, a_prev, sigma_t, _ = R.ddim_scalars(S, index, eta)
                exact = math.sqrt(1.0 - a_prev - sigma_t * sigma_t)
                for contracted in (False, True):
                    q = abs(float(R.dirc_fp32(a_prev, sigma_t, contracted)) - exact) / R.dirc_bound(a_prev, sigma_t)
                    worst = max(worst, q)
                    assert q <= 1.0, (S, eta, index, contracted, q)
    print(f"[step ops] dirc: the fp32 value uses at most {worst:.2f} of its bound over S in (6, 10, 50) x eta in (0, 0.7, 1)")


def test_counts_and_head_room():
    assert R.K(11) == 16 and R.K(10) == 15 and R.K(15) == 22 and R.K(5) == 8 and R.K(3) == 5 and R.K(7) == 11 and R.K(2) == 3
    assert R.SD_REL >= 4.0 * R.SD_MEASURED and R.SD_REL >= 4.0 * 2.0 ** -23


def test_step_op_symbols_in_header_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdm_hip.h")).read(), flags=re.S)
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    n_args = {"rdm_op_ddim_step": 15, "rdm_op_plms_step": 19, "rdm_op_ddpm_step": 14}
    for name, n in n_args.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib, name)
    for name in ("rdm_op_ddim_step_seeded", "rdm_op_ddpm_step_seeded"):      # the twins the one rdm_noise argument replaced
        assert not re.search(r"\b" + name + r"\b", src) and name not in _lib.SIGNATURES, name
    assert (_lib.PLMS_STEP, _lib.PLMS_EULER_A, _lib.PLMS_EULER_B) == (R.PLMS_STEP, R.PLMS_EULER_A, R.PLMS_EULER_B) == (0, 1, 2)


def test_step_op_bindings_check_sizes_before_any_device_call():
    """Every bad call must raise the binding's OWN message.  The context has no handle: a call that got past the Python checks reaches
    the library, which answers 'null context' -- also an RdmError, so each refusal is pinned by its text, and one well-formed call per
    entry is shown to reach the library."""
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._h = None
    v = lambda n: torch.zeros(n)
    x, out = v(8), v(8)
    SIZES, SEEDED, ROWS, COUNTERS = "operand sizes do not match x", "takes per_row and no noise operand", "must fit 32 bits", "per_row must be >= 1 and step"
    ddim = lambda eps, noise, cfg, x_prev, **kw: ctx.op_ddim_step(x, eps, noise, cfg, 2.0 if cfg else 1.0, .5, .6, .1, .7, 1., x_prev, **kw)
    plms = lambda eps, cfg, mode, order, x_out, **kw: ctx.op_plms_step(x, eps, cfg, 2.0 if cfg else 1.0, .5, .6, .7, mode, order, x_out, **kw)
    ddpm = lambda eps, noise, x_prev, **kw: ctx.op_ddpm_step(x, eps, noise, 1., .1, .5, .5, -3., True, True, 1., x_prev, **kw)
    bad = [
        ("ddim: eps of n under cfg", SIZES, lambda: ddim(v(8), None, True, out)),
        ("ddim: eps of 2n without cfg", SIZES, lambda: ddim(v(16), None, False, out)),
        ("ddim: short noise", SIZES, lambda: ddim(v(8), v(7), False, out)),
        ("ddim: short x_prev", SIZES, lambda: ddim(v(8), None, False, v(4))),
        ("ddim: long x_dup", SIZES, lambda: ddim(v(8), None, False, out, x_dup=v(9))),
        ("ddim: short pred_x0", SIZES, lambda: ddim(v(8), None, False, out, pred_x0=v(4))),
        ("ddim: short x_prev, seeded", SIZES, lambda: ddim(v(8), None, False, v(4), seed=1, per_row=4)),
        ("ddim: seed and noise", SEEDED, lambda: ddim(v(8), v(8), False, out, seed=1, per_row=4)),
        ("ddim: seed without per_row", SEEDED, lambda: ddim(v(8), None, False, out, seed=1)),
        ("ddim: rows past 32 bits", ROWS, lambda: ddim(v(8), None, False, out, seed=1, per_row=4, row0=2 ** 32 - 2)),
        ("ddim: negative row0", ROWS, lambda: ddim(v(8), None, False, out, seed=1, per_row=4, row0=-1)),
        ("ddim: step past 32 bits", COUNTERS, lambda: ddim(v(8), None, False, out, seed=1, per_row=4, step=2 ** 32)),
        ("ddim: per_row 0", COUNTERS, lambda: ddim(v(8), None, False, out, seed=1, per_row=0)),
        ("plms: eps of n under cfg", SIZES, lambda: plms(v(8), True, 0, 0, out, e_store=v(8))),
        ("plms: short h1", SIZES, lambda: plms(v(8), False, 0, 1, out, h1=v(4), e_store=v(8))),
        ("plms: short h2", SIZES, lambda: plms(v(8), False, 0, 2, out, h1=v(8), h2=v(4), e_store=v(8))),
        ("plms: short h3", SIZES, lambda: plms(v(8), False, 0, 3, out, h1=v(8), h2=v(8), h3=v(4), e_store=v(8))),
        ("plms: short e_prev", SIZES, lambda: plms(v(8), False, 2, 0, out, e_prev=v(4))),
        ("plms: short e_store", SIZES, lambda: plms(v(8), False, 1, 0, out, e_store=v(4))),
        ("plms: short x_out", SIZES, lambda: plms(v(8), False, 1, 0, v(4), e_store=v(8))),
        ("plms: long x_dup", SIZES, lambda: plms(v(8), False, 1, 0, out, e_store=v(8), x_dup=v(9))),
        ("plms: short pred_x0", SIZES, lambda: plms(v(8), False, 1, 0, out, e_store=v(8), pred_x0=v(4))),
        ("ddpm: long eps", SIZES, lambda: ddpm(v(16), v(8), out)),
        ("ddpm: short noise", SIZES, lambda: ddpm(v(8), v(4), out)),
        ("ddpm: short x_prev", SIZES, lambda: ddpm(v(8), v(8), v(4))),
        ("ddpm: seed and noise", SEEDED, lambda: ddpm(v(8), v(8), out, seed=1, per_row=4)),
        ("ddpm: seed without per_row", SEEDED, lambda: ddpm(v(8), None, out, seed=1)),
        ("ddpm: rows past 32 bits", ROWS, lambda: ddpm(v(8), None, out, seed=1, per_row=4, row0=2 ** 32 - 2)),
        ("ddpm: per_row 0", COUNTERS, lambda: ddpm(v(8), None, out, seed=1, per_row=0)),
        ("ddpm: step -1", COUNTERS, lambda: ddpm(v(8), None, out, seed=1, per_row=4, step=-1)),
    ]
    for what, message, call in bad:
        with pytest.raises(_lib.RdmError, match=re.escape(message)) as err:
            call()
        assert "null context" not in str(err.value), what
    # the same calls well formed get past the binding and are answered by the library: the bare context tells the two apart
    reach = [
        ("ddim", lambda: ddim(v(16), v(8), True, out, x_dup=v(8), pred_x0=v(8))),
        ("ddim seeded", lambda: ddim(v(8), None, False, out, seed=1, per_row=4, row0=2 ** 32 - 3, step=2 ** 32 - 1)),
        ("plms", lambda: plms(v(16), True, 0, 3, out, h1=v(8), h2=v(8), h3=v(8), e_store=v(8), x_dup=v(8), pred_x0=v(8))),
        ("ddpm", lambda: ddpm(v(8), v(8), out)),
        ("ddpm seeded", lambda: ddpm(v(8), None, out, seed=1, per_row=4)),
    ]
    for what, call in reach:
        with pytest.raises(_lib.RdmError, match="null context"):
            call()
