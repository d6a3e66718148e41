"""The inpainting blend (csrc/sampler_steps.hip: masked_blend_kernel<4|1>, masked_blend_seeded_kernel) restated: in float64 with the
per-element bound it is held to, and in numpy fp32 term for term, plain and with the near miss -- the inner sum contracted to an FMA.

    out = (sa x0 + s1m z) m + (1 - m) x            sa, s1m: fp32 scalars, taken as inputs;  m in [0, 1]

The float64 bound follows tests/_step_ref.py: tol = K(count) * 2^-24 * A with A the float64 sum of the absolute values of the terms
entering the element, A = (|sa x0| + |s1m z|) m + (1 - m) |x|, and count the fp32 roundings on the longest path from an input to the
output in the expression as the kernel text writes it:

    sa x0 (1), + s1m z (2), * m (3), + (1 - m) x (4)            K(4) = 6
    (the other path is shorter: 1 - m, * x, the last sum: 3)

An FMA contraction only REMOVES a rounding, so no tolerance against float64 can tell the contracted form from the kernel's: the
contracted form lies inside every bound the kernel's own form lies inside.  What tells them apart is the other bound the operation
count gives: the expression is six IEEE operations (three products, two sums, one difference), each correctly rounded and none of them
a library function, so the fp32 result has no freedom at all -- the kernel must equal the numpy fp32 evaluation of the same six
operations with ZERO differing elements.  The near miss (blend_fp32(contracted=True): fma(sa, x0, fp32(s1m z)) for the inner sum) must
fall outside that: it has to differ from the kernel's output on some element of every case, and check() asserts both."""
import numpy as np

from _step_ref import K, U, f64

COUNT = 4
K_BLEND = K(COUNT)

# (B, C, H, W): what each shape exercises
SHAPES = {
    "b3c3_8x8_float4_rows_and_channels": (3, 3, 8, 8),
    "b2c3_5x7_scalar_odd_plane": (2, 3, 5, 7),
    "b2c3_2x6_float4_plane_of_12": (2, 3, 2, 6),
}
SEEDED_STRADDLE = (2, 4, 3, 3)             # per_row = 36 (% 4 == 0), H W = 9: a Philox block straddles channel planes
SECOND_TRIP = (2, 3, 592, 592)             # 2 102 784 elements: just above 2048 blocks x 256 threads x 4, a second grid-stride trip
assert 2048 * 256 * 4 < int(np.prod(SECOND_TRIP)) < 2048 * 256 * 4 + 8192


def inputs(shape, mask_channels, soft, seed):
    """x, x0, z standard normal fp32 [B, C, H, W]; mask fp32 [B, mask_channels, H, W]: binary, or (soft) uniform in [0, 1] with exact
    0s and 1s mixed in."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    x, x0, z = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    mshape = (B, mask_channels, H, W)
    if soft:
        m = rng.random(mshape).astype(np.float32)
        pick = rng.random(mshape)
        m[pick < 0.15] = 0.0
        m[pick > 0.85] = 1.0
    else:
        m = (rng.random(mshape) > 0.5).astype(np.float32)
    return x, x0, z, m


def blend(x, x0, z, m, sa, s1m):
    """float64 -> (want, tol, A); m broadcasts over the channels"""
    X, X0, Z, M = f64(x), f64(x0), f64(z), f64(m)
    sa, s1m = float(np.float32(sa)), float(np.float32(s1m))
    want = (sa * X0 + s1m * Z) * M + (1.0 - M) * X
    A = (np.abs(sa * X0) + np.abs(s1m * Z)) * M + (1.0 - M) * np.abs(X)
    return want, K_BLEND * U * A, A


def blend_fp32(x, x0, z, m, sa, s1m, contracted=False):
    """The kernel's six operations in numpy fp32.  contracted: the near miss -- the inner sum takes its first product fused."""
    f = np.float32
    sa, s1m = f(sa), f(s1m)
    b = s1m * z
    q = (f64(sa) * f64(x0) + f64(b)).astype(np.float32) if contracted else sa * x0 + b
    known = q * m
    om = f(1.0) - m
    out = known + om * x
    assert out.dtype == np.float32
    return out


def check(got, x, x0, z, m, sa, s1m):
    """got (numpy fp32) against the float64 bound, the exact fp32 evaluation, and the near miss.  -> report line"""
    want, tol, A = blend(x, x0, z, m, sa, s1m)
    assert np.isfinite(got).all()
    err = np.abs(f64(got) - want)
    units = float(np.divide(err, U * A, out=np.zeros_like(err), where=err > 0).max())
    assert (err <= tol).all(), f"worst |got - ref| / (2^-24 A) = {units:.2f}, bound K = {K_BLEND}"
    exact = blend_fp32(x, x0, z, m, sa, s1m)
    differ = int((got != exact).sum())
    assert differ == 0, f"{differ} of {got.size} elements differ from the six fp32 operations"
    miss = blend_fp32(x, x0, z, m, sa, s1m, contracted=True)
    outside = int((got != miss).sum())
    assert outside > 0, "the FMA-contracted near miss is indistinguishable from the kernel's output"
    return (f"worst |got - fp64| / (2^-24 A) = {units:.2f} (K = {K_BLEND}); 0 elements off the fp32 evaluation; "
            f"FMA near miss differs on {outside} of {got.size}")


def schedule(acp, S):
    """(ts, a_t) of the S-step 'uniform' DDIM schedule from the fp32 alphas_cumprod"""
    acp = np.asarray(acp, dtype=np.float32)
    T = acp.shape[0]
    ts = np.asarray(list(range(0, T, T // S))) + 1
    return ts, acp[ts]


def level_scalars(a):
    """sqrt(a), sqrt(1 - a) in float64 from the fp32 alpha, rounded to fp32: what the loop hands the blend kernel"""
    a = float(np.float32(a))
    return float(np.float32(np.sqrt(a))), float(np.float32(np.sqrt(1.0 - a)))


def area_average(mask, f):
    """[B, f h, f w] -> [B, 1, h, w]: the mean of every f x f block in float64"""
    m = f64(mask)
    B, H, W = m.shape
    return m.reshape(B, H // f, f, W // f, f).mean(axis=(2, 4))[:, None]
