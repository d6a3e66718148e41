"""Float64 / integer restatements of the two weight-gradient ops (csrc/wgrad.hip and the transposed-copy fallbacks of csrc/backward.hip),
their cases and their near misses.  Shared by tests/test_gpu_training_ops.py (the HIP kernels) and tests/test_training_ops_cpu.py.  Same CASE
contract as tests/_train_ref.py: `make(**kw)`, `ref(inp, dt)`, `bound(inp, ref)`, `misses(inp)`.

    conv:    dW[n][ky][kx][c] = sum_{b, y, x} dY[b][y][x][n] X[b][y + ky - 1][x + kx - 1][c]      (zero outside the image)
    linear:  dW[n][k]         = sum_m dY[m][n] A[m][k]

Every case states its FORM = (path, Z, per_plane, remap), the answer of the host-only selector `_lib.wgrad_select` (the function the
library's own dispatch asks); the tests assert the selector gives exactly that, so a case cannot drift onto another kernel unnoticed.

EXACT cases: operands uniform in {-3 .. 3} (exact in bf16).  Every product is an integer of magnitude <= 9 and every partial sum, in any
order and any split over planes, an integer of magnitude <= sum |terms| < 2^24 -- exact in fp32.  dW must equal the integer reference bit
for bit; a dropped, doubled or misplaced term fails whatever M is.

ROUNDED cases: N(0, 1) operands rounded to bf16, one per path.  The bf16 MFMA is taken as one fp32 rounding per product accumulated along
the reduction (the convention of tests/_fwd_ref.py), so a plane is a chain of as many roundings as it has reduction positions
(chunks x max(32, W) pixels for the nine-tap kernel, rows for the per-tap kernel, padded K' positions for the fallbacks) and the fixed
order sum of the Z planes adds Z - 1:   |dW - ref| <= chain u sum |terms|,  chain = per-plane positions + Z - 1,  r = 0 (fp32 output).
The chain is written in the case and checked against the form.

Near misses (each built from the exact answer by adding or removing the terms the bug would):
  * corner: the bottom-right pixel of sample 0 missing from tap (0, 0) (linear: row 0 missing);
  * edge row: at the bottom image edge, the taps ky = 2 let in row 0 of the NEXT sample -- what the row ring holds there (B >= 2);
  * last chunk: the last (ragged) chunk of the reduction missing: max(32, W) pixels (nine-tap), the rows past the last multiple of 32
    (per-tap), the last sample's last image row (conv fallback), the rows past the last multiple of 64 (linear fallback);
  * plane: Z plane number Z - 2 missing (Z >= 2);
  * taps transposed (ky <-> kx)."""
import torch
import torch.nn.functional as F

from _train_ref import F64, U, bfr

CONV9 = {"conv9<4>": 16, "conv9<5>": 32, "conv9<6>": 64}


def _ints(shape, seed):
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).float()


def _gauss(shape, seed):
    return bfr(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


def chain_of(form):
    """roundings behind one element: the reduction positions of a plane, then Z - 1 plane additions"""
    path, Z, per_plane, _ = form
    return per_plane * max(32, CONV9[path]) + Z - 1 if path in CONV9 else per_plane + Z - 1


def _tap_sum(dy, x, mask=None):
    """dW [N, 3, 3, C] over the pixels where mask [B, H, W] is set (all when None)"""
    B, H, W, N = dy.shape
    C = x.shape[3]
    if mask is not None:
        dy = dy * mask[..., None].to(dy.dtype)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    d2 = dy.reshape(-1, N).t()
    out = torch.empty((N, 3, 3, C), dtype=dy.dtype)
    for ky in range(3):
        for kx in range(3):
            out[:, ky, kx] = d2 @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, C)
    return out


def _pixel_range_mask(B, H, W, lo, hi):
    m = torch.zeros(B * H * W, dtype=torch.bool)
    m[max(lo, 0):max(min(hi, B * H * W), 0)] = True
    return m.reshape(B, H, W)


class ConvWgrad:
    name = "conv3x3_wgrad"
    exact = False

    @staticmethod
    def make(B, H, W, C, N, form, exact, chain=None, seed=31):
        draw = _ints if exact else _gauss
        return {"x": draw((B, H, W, C), seed), "dy": draw((B, H, W, N), seed + 1), "form": form, "chain": chain}

    @staticmethod
    def ref(inp, dt):
        return {"dw": _tap_sum(inp["dy"].to(dt), inp["x"].to(dt))}

    @staticmethod
    def terms(inp):
        return _tap_sum(inp["dy"].double().abs(), inp["x"].double().abs())

    @staticmethod
    def bound(inp, ref):
        return {"dw": (0.0, inp["chain"] * U * ConvWgrad.terms(inp))}

    @staticmethod
    def plane_mask(inp, z):
        """the pixels plane z reduces over"""
        B, H, W, _ = inp["dy"].shape
        path, Z, per, _ = inp["form"]
        if path == "conv_fallback":                          # K' position of pixel (b, y, x): (b (H + 2) + y + 1) WP + x + 1
            WP = (W + 2 + 7) & ~7
            b, y, xx = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
            pos = (b * (H + 2) + y + 1) * WP + xx + 1
            return (pos >= z * per) & (pos < (z + 1) * per)
        unit = max(32, CONV9[path]) if path in CONV9 else 1
        return _pixel_range_mask(B, H, W, z * per * unit, (z + 1) * per * unit)

    @staticmethod
    def last_chunk_mask(inp):
        B, H, W, _ = inp["dy"].shape
        M = B * H * W
        path = inp["form"][0]
        if path in CONV9:
            return _pixel_range_mask(B, H, W, M - max(32, W), M)
        if path == "tn9":
            return _pixel_range_mask(B, H, W, (M - 1) // 32 * 32, M)
        return _pixel_range_mask(B, H, W, M - W, M)

    @staticmethod
    def misses(inp):
        dy, x = inp["dy"].double(), inp["x"].double()
        B, H, W, N = dy.shape
        ref = _tap_sum(dy, x)
        out = []
        m = ref.clone(); m[:, 0, 0] -= torch.outer(dy[0, H - 1, W - 1], x[0, H - 2, W - 2])
        out.append(("corner pixel of tap (0, 0) dropped", {"dw": m}))
        if B >= 2:
            m = ref.clone()
            xn = F.pad(x[1:, 0], (0, 0, 1, 1))                   # row 0 of the next sample, zero-bordered: [B - 1, W + 2, C]
            for kx in range(3):
                m[:, 2, kx] += dy[:-1, H - 1].reshape(-1, N).t() @ xn[:, kx:kx + W].reshape(-1, x.shape[3])
            out.append(("next sample's first row let in at the bottom edge", {"dw": m}))
        out.append(("last chunk dropped", {"dw": ref - _tap_sum(dy, x, ConvWgrad.last_chunk_mask(inp))}))
        if inp["form"][1] >= 2:
            out.append(("one Z plane skipped", {"dw": ref - _tap_sum(dy, x, ConvWgrad.plane_mask(inp, inp["form"][1] - 2))}))
        out.append(("taps transposed", {"dw": ref.transpose(1, 2).contiguous()}))
        return out


class ConvWgradExact(ConvWgrad):
    exact = True


class LinearWgrad:
    name = "linear_wgrad"
    exact = False

    @staticmethod
    def make(M, N, K, form, exact, chain=None, seed=41):
        draw = _ints if exact else _gauss
        return {"a": draw((M, K), seed), "dy": draw((M, N), seed + 1), "form": form, "chain": chain}

    @staticmethod
    def ref(inp, dt):
        return {"dw": inp["dy"].to(dt).t() @ inp["a"].to(dt)}

    @staticmethod
    def terms(inp):
        return inp["dy"].double().abs().t() @ inp["a"].double().abs()

    @staticmethod
    def bound(inp, ref):
        return {"dw": (0.0, inp["chain"] * U * LinearWgrad.terms(inp))}

    @staticmethod
    def _without(inp, lo, hi):
        dy, a = inp["dy"].double(), inp["a"].double()
        return {"dw": dy.t() @ a - dy[lo:hi].t() @ a[lo:hi]}

    @staticmethod
    def misses(inp):
        M = inp["dy"].shape[0]
        path, Z, per, _ = inp["form"]
        out = [("row 0 dropped", LinearWgrad._without(inp, 0, 1))]
        if M > 1:
            out.append(("last chunk dropped", LinearWgrad._without(inp, (M - 1) // (32 if path == "tn1" else 64) * (32 if path == "tn1" else 64), M)))
        if Z >= 2:
            out.append(("one Z plane skipped", LinearWgrad._without(inp, (Z - 2) * per, (Z - 1) * per)))
        return out


class LinearWgradExact(LinearWgrad):
    exact = True


def _conv(B, H, W, C, N, form, what, chain=None):
    exact = chain is None
    return (ConvWgradExact if exact else ConvWgrad, dict(B=B, H=H, W=W, C=C, N=N, form=form, exact=exact, chain=chain),
            f"{form[0]} Z={form[1]} remap={form[3]}: {what}" + ("" if exact else f" (rounded, chain {chain})"))


def _lin(M, N, K, form, what, chain=None):
    exact = chain is None
    return (LinearWgradExact if exact else LinearWgrad, dict(M=M, N=N, K=K, form=form, exact=exact, chain=chain),
            f"{form[0]} Z={form[1]} remap={form[3]}: {what}" + ("" if exact else f" (rounded, chain {chain})"))


# (case, kwargs, path description).  form = (path, Z, per_plane, remap) as _lib.wgrad_select answers on the shape.
CASES = [
    # ---- the nine-tap kernel
    _conv(8, 2, 16, 64, 64, ("conv9<4>", 1, 8, 0), "two-row images, RY = 2 rows per chunk, one plane"),
    _conv(1, 16, 16, 64, 64, ("conv9<4>", 1, 8, 0), "one sample, one plane"),
    _conv(5, 8, 16, 128, 128, ("conv9<4>", 2, 10, 0), "odd B, plane boundary inside a sample, 2 x 2 tiles, no remap"),
    _conv(8, 16, 16, 64, 64, ("conv9<4>", 8, 8, 8), "eight planes, all dealt to the XCDs"),
    _conv(9, 16, 16, 64, 64, ("conv9<4>", 9, 8, 8), "nine planes: eight remapped, a tail of one"),
    _conv(4, 2, 32, 64, 64, ("conv9<5>", 1, 8, 0), "two-row images, one plane"),
    _conv(13, 2, 32, 64, 64, ("conv9<5>", 3, 9, 0), "26 chunks in planes of 9: ragged last plane, plane boundaries inside a sample"),
    _conv(8, 8, 32, 64, 64, ("conv9<5>", 8, 8, 8), "eight planes, all remapped"),
    _conv(3, 32, 32, 128, 64, ("conv9<5>", 12, 8, 8), "twelve planes: eight remapped, a tail of four; two C tiles"),
    _conv(2, 2, 64, 64, 64, ("conv9<6>", 1, 4, 0), "two-row images, one plane"),
    _conv(3, 8, 64, 64, 128, ("conv9<6>", 3, 8, 0), "odd B, two N tiles, no remap"),
    _conv(9, 8, 64, 64, 64, ("conv9<6>", 9, 8, 8), "nine planes: eight remapped, a tail of one; odd B"),
    _conv(4, 32, 64, 64, 64, ("conv9<6>", 16, 8, 16), "sixteen planes, all remapped"),
    # ---- the per-tap kernel, nine taps
    _conv(8, 4, 8, 64, 64, ("tn9", 1, 256, 0), "W = 8, one plane, launch order"),
    _conv(8, 4, 8, 768, 384, ("tn9", 1, 256, 1), "one plane, 8 tiles: remapped"),
    _conv(33, 2, 4, 96, 224, ("tn9", 1, 288, 0), "M = 264 (no multiple of 32), C and N multiples of 32 only, masked column groups"),
    _conv(5, 16, 16, 96, 64, ("tn9", 5, 256, 0), "W = 16 with C no multiple of 64, five planes"),
    _conv(8, 16, 8, 256, 64, ("tn9", 4, 256, 1), "four planes x two tiles: remapped"),
    _conv(8, 32, 8, 64, 64, ("tn9", 8, 256, 1), "eight planes, remapped"),
    # ---- conv fallback (transposed zero-padded copies, implicit GEMM)
    _conv(1, 2, 16, 64, 64, ("conv_fallback", 1, 128, 0), "the 2 x 16 image (M = 32 < 256)"),
    _conv(2, 5, 7, 64, 34, ("conv_fallback", 1, 256, 0), "5 x 7 images, N = 34"),
    _conv(7, 12, 20, 34, 64, ("conv_fallback", 2, 1216, 0), "12 x 20 images, C = 34, two planes"),
    _conv(9, 55, 7, 64, 64, ("conv_fallback", 8, 1088, 0), "55 x 7 images, eight planes"),
    # ---- the per-tap kernel, one tap
    _lin(256, 64, 64, ("tn1", 1, 256, 0), "M = 256, the floor"),
    _lin(256, 1536, 384, ("tn1", 1, 256, 1), "one plane, 16 tiles: remapped"),
    _lin(1000, 320, 96, ("tn1", 3, 352, 0), "M ragged against 32 and against mz, partial 192 tiles"),
    _lin(512, 384, 384, ("tn1", 2, 256, 1), "two planes, 4 tiles: remapped"),
    _lin(2048, 64, 64, ("tn1", 8, 256, 1), "eight planes after the & ~7, remapped"),
    _lin(4097, 64, 224, ("tn1", 15, 288, 0), "fifteen planes, one row in the last chunk, masked column groups"),
    # ---- linear fallback
    _lin(1, 34, 64, ("linear_fallback", 1, 64, 0), "M = 1, N = 34"),
    _lin(64, 34, 64, ("linear_fallback", 1, 64, 0), "Mp == M: no memset"),
    _lin(255, 64, 36, ("linear_fallback", 1, 256, 0), "M = 255, K = 36"),
    _lin(1000, 34, 96, ("linear_fallback", 1, 1024, 0), "M = 1000, N = 34"),
    _lin(2500, 66, 34, ("linear_fallback", 3, 896, 0), "three planes"),
    # ---- one Gaussian case per path: chain = per-plane positions + Z - 1
    _conv(5, 8, 16, 128, 128, ("conv9<4>", 2, 10, 0), "odd B, 2 x 2 tiles", chain=321),
    _conv(13, 2, 32, 64, 64, ("conv9<5>", 3, 9, 0), "ragged last plane", chain=290),
    _conv(3, 8, 64, 64, 128, ("conv9<6>", 3, 8, 0), "odd B, two N tiles", chain=514),
    _conv(33, 2, 4, 96, 224, ("tn9", 1, 288, 0), "M = 264, masked column groups", chain=288),
    _conv(7, 12, 20, 34, 64, ("conv_fallback", 2, 1216, 0), "12 x 20 images, two planes", chain=1217),
    _lin(1000, 320, 96, ("tn1", 3, 352, 0), "ragged M, partial tiles", chain=354),
    _lin(1000, 34, 96, ("linear_fallback", 1, 1024, 0), "M = 1000, N = 34", chain=1024),
]

def exact_case(form):
    """the first integer case stated for this form"""
    return next(e for e in CASES if e[1]["exact"] and e[1]["form"] == form)


# a many-plane case, then a one-plane case of the same kernel on the same context: the planes of the first must not reach the second's dW
SCRATCH_REUSE = [(("conv9<4>", 9, 8, 8), ("conv9<4>", 1, 8, 0)), (("conv9<6>", 16, 8, 16), ("conv9<6>", 1, 4, 0)), (("tn9", 8, 256, 1), ("tn9", 1, 256, 0)),
                 (("conv_fallback", 8, 1088, 0), ("conv_fallback", 1, 128, 0)), (("tn1", 8, 256, 1), ("tn1", 1, 256, 0)),
                 (("linear_fallback", 3, 896, 0), ("linear_fallback", 1, 64, 0))]


def case_id(entry):
    case, kw, _ = entry
    shape = "x".join(str(kw[k]) for k in (("B", "H", "W", "C", "N") if "B" in kw else ("M", "N", "K")))
    return f"{case.name}-{'int' if kw['exact'] else 'gauss'}-{kw['form'][0]}-z{kw['form'][1]}-r{kw['form'][3]}-{shape}"


def answer_class(form):
    """what the enumeration tells apart: (path, Z = 1 / 2-7 / >= 8, remap form)"""
    path, Z, _, remap = form
    zc = "1" if Z == 1 else "2-7" if Z < 8 else ">=8"
    if path in CONV9:
        return (path, zc, "none" if remap == 0 else "all" if remap == Z else "tail")
    return (path, zc, "remap" if remap else "launch order")
