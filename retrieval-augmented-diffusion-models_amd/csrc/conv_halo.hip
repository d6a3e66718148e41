// Host side of the 3x3 convolution (pad 1, NHWC bf16; conv_nd(2, C, C', 3, padding=1) of ldm's ResBlock / Upsample / Downsample,
// reached from rdm/modules/diffusionmodules/openaimodel.py:144-305): the one statement of which kernel takes a conv, the K-split
// decision with its finisher, and the launch.  The kernels themselves: conv_halo4.hip (input-stationary, one wave per SIMD; its
// 64-column strip form for images wider than 64 pixels) and igemm.hip (the generic implicit GEMM, every other conv).

#include "kernels.h"

// out = bf16(sum of the ksplit fp32 partial planes + bias + time-embedding row + residual) -- one rounding --, 8 columns per thread
__global__ __launch_bounds__(256) void splitk_finish_kernel(IgemmParams p) {
    const long long nvec = (long long)p.M * (p.N >> 3);
    const long long plane = (long long)p.M * p.N;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long long)gridDim.x * 256) {
        const long long m = v / (p.N >> 3); const int n = (int)(v - m * (p.N >> 3)) * 8;
        float a[8];
        { const float4 b0 = p.bias ? *(const float4*)(p.bias + n) : make_float4(0, 0, 0, 0), b1 = p.bias ? *(const float4*)(p.bias + n + 4) : make_float4(0, 0, 0, 0);
          a[0] = b0.x; a[1] = b0.y; a[2] = b0.z; a[3] = b0.w; a[4] = b1.x; a[5] = b1.y; a[6] = b1.z; a[7] = b1.w; }
        for (int s = 0; s < p.ksplit; s++) {                  // fixed order: deterministic
            const float* w = p.ws + s * plane + m * p.N + n;
            const float4 w0 = *(const float4*)w, w1 = *(const float4*)(w + 4);
            a[0] += w0.x; a[1] += w0.y; a[2] += w0.z; a[3] += w0.w; a[4] += w1.x; a[5] += w1.y; a[6] += w1.z; a[7] += w1.w;
        }
        if (p.rowvec) {
            const float* rv = p.rowvec + (m / p.rows_per_sample) * p.rowvec_ld + n;
#pragma unroll
            for (int e = 0; e < 8; e++) a[e] += rv[e];
        }
        if (p.res_bf16) {     // the residual joins in fp32: ONE rounding, like conv_halo4's fused read-out (round 5: the finisher used to round
                              // the conv first -- which of the two a layer got depended on the batch through the K-split decision)
            const uint4 r4 = *(const uint4*)(p.res_bf16 + m * p.ldo + n);
            const uint32_t rr[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
            for (int e = 0; e < 4; e++) { a[2 * e] += __uint_as_float(rr[e] << 16); a[2 * e + 1] += __uint_as_float(rr[e] & 0xffff0000u); }
        }
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = cvt_pk_bf16(a[2 * e], a[2 * e + 1]);
        *(uint4*)(p.out_bf16 + m * p.ldo + n) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// Which kernel takes this conv: geometry and epilogue only -- whether the fragment-ordered weight copy the halo4 forms need
// exists is the caller's business (launch_conv3x3: without one, the implicit GEMM).
ConvKernel conv3x3_kernel(const IgemmParams& p) {
    const int W = p.Wout, H = p.Hout;
    if (p.stride != 1) return CONV_IGEMM;
    if (p.ups ? (p.Hout != 2 * p.Hin || p.Wout != 2 * p.Win) : (p.Hout != p.Hin || p.Wout != p.Win)) return CONV_IGEMM;
    if (p.M % 256 != 0 || p.C0 % 64 || p.C1 % 64 || p.ldo % 8 || p.K != 9 * (p.C0 + p.C1)) return CONV_IGEMM;
    if (p.alpha != 1.0f || p.act != ACT_NONE || !p.out_bf16 || p.out_f32 || p.res_f32) return CONV_IGEMM;
    if (p.rowvec && p.rows_per_sample % 32 != 0) return CONV_IGEMM;      // the read-out folds the per-sample row per 32-row fragment
    if ((long long)p.M * (p.C0 > p.C1 ? p.C0 : p.C1) >= 0x7fffffffLL) return CONV_IGEMM;
    if (W > 64) {      // 64-column strips (conv3x3_halo4_kernel<FN, STRIP>): the first-stage decoder's 128- / 256-pixel levels, the UNet's at latents wider than 64
        if (W % 64 || H % 4 || W > 4096 || H > 4096 || (p.N % 192 != 0 && p.N % 128 != 0) || (long long)p.M * p.ldo >= 0x7fffffffLL) return CONV_IGEMM;
        return CONV_HALO4_STRIP;
    }
    // a tile is 256 consecutive output pixels: whole rows of one image, or whole images
    if (W < 4 || 256 % W != 0 || (p.N % 192 != 0 && p.N % 128 != 0)) return CONV_IGEMM;
    const int HW = H * W;
    if (HW >= 256 ? (HW % 256 != 0 || H % (256 / W) != 0) : 256 % HW != 0) return CONV_IGEMM;
    const Halo4Geom g = halo4_geom(H, W);
    // the halo of a tile must fit the LDS buffer and the piece tables (three pieces per wave per tap-step, staged during taps 0..6):
    // this is what refuses 4-pixel-wide images (HBYTES = 71936 at 256+ pixels).  At most 400 halo positions: the retired 8-wave
    // kernel's bound, which alone keeps 32-wide, 4-high images on the implicit GEMM -- halo4 has never run them
    if (g.HBYTES > H4_HALO_MAX || g.NPT > 4 * 21 || g.NROW * g.HPW > 400) return CONV_IGEMM;
    // the kernel's multiply-shift divisions by NPR and RS + 2 must be exact over the ranges met
    const int mNPR = 65536 / g.NPR + 1, mRS2 = 65536 / (g.RS + 2) + 1;
    for (int x = 0; x < 4 * 36 + 4; x++) if (((x * mNPR) >> 16) != x / g.NPR) return CONV_IGEMM;
    for (int x = 0; x <= g.NROW + 36; x++) if (((x * mRS2) >> 16) != x / (g.RS + 2)) return CONV_IGEMM;
    return CONV_HALO4;
}

// K-split only pays when the MxN tiles leave most of the chip idle (the 8x8 level: 160 tiles on 256 CUs): S parts per tile
// turn one 62 %-occupied round into ceil(160 S / 256) rounds of 1/S the length
int conv_halo_ksplit(const IgemmParams& p) {
    if (conv3x3_kernel(p) != CONV_HALO4) return 1;       // neither the strip form nor the implicit GEMM knows ksplit / ws
    int dev = 0, ncu = 256; hipGetDevice(&dev); hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    const int bn = (p.N % 192 == 0) ? 192 : 128;
    const long long tiles = (long long)(p.M / 256) * (p.N / bn);
    const int nslice = (p.C0 + p.C1) / 64;
    if (tiles * 4 > (long long)ncu * 3 || p.N % 8 || p.ldo % 8) return 1;
    int best = 1; double bestc = 1.0;                       // cost = rounds / S (+6 % per extra plane for the fp32 round trip)
    for (int S = 2; S <= 3; S++) {
        if (nslice < 2 * S) continue;
        const double c = (double)((tiles * S + ncu - 1) / ncu) / S * (1.0 + 0.06 * (S - 1));
        if (c < bestc - 0.08) { bestc = c; best = S; }
    }
    return best;
}

hipError_t launch_conv3x3(const IgemmParams& p, hipStream_t st) {
    const ConvKernel k = p.Wfrag ? conv3x3_kernel(p) : CONV_IGEMM;
    // The implicit GEMM and the strip form know nothing of ksplit / ws and must never see ksplit > 1.  They cannot: conv_halo_ksplit
    // answers 1 unless the conv is CONV_HALO4's, and Ops::conv3 (dispatch.hip) asks it only once it holds the fragment copy.  A caller
    // that set ksplit some other way gets an error, not a conv missing its K-split parts
    if (p.ksplit > 1 && k != CONV_HALO4) return hipErrorInvalidValue;
    if (k == CONV_IGEMM) return launch_igemm(p, true, 1, st);
    const hipError_t e = launch_conv_halo4(p, k == CONV_HALO4_STRIP, st);
    if (e != hipSuccess || p.ksplit <= 1) return e;
    const long long nvec = (long long)p.M * (p.N >> 3);
    long long g = (nvec + 255) / 256; if (g > 4096) g = 4096;
    splitk_finish_kernel<<<dim3((unsigned)g), 256, 0, st>>>(p);
    return hipGetLastError();
}
