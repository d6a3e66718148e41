// Nearest-code search of a wide-latent VQ first stage (taming VectorQuantizer2 as reached from VQModel.encode; un-vendored, parity
// unpinned):  idx[m] = argmin_j ( |e_j|^2 - 2 z_m . e_j ),  first minimum on ties.  z fp32 [M, E] token-major, codebook fp32 [N, E].
// For the shipped VQGAN-f16 (N = 16384, E = 256) this is a 16384-code x 256-dim distance GEMM per token.
//
// Arithmetic: fp32-input MFMA (v_mfma_f32_32x32x2_f32), an exact fp32 fma chain over k -- neighbouring codes lie closer than bf16
// product error, and the result is a discrete index.  Every score is produced by the SAME instruction sequence wherever its code and
// its row land: the dot product starts from 0 and walks k in one fixed order (per 8-k step: k, k+4, k+1, k+5, ...: the lane halves
// of one MFMA hold k and k + 4, see the operand read below), then one fma with |e_j|^2.  The reductions (registers -> block ->
// code splits) only compare, with "lower index wins on equal score".  So an index is bitwise independent of M, of the split count
// and of the tile its code sits in; nothing here consults the deterministic switch, and no float atomics exist.
//
// Structure: a block owns 128 rows of z and walks a range of 128-code tiles; the codes are the MFMA's A operand (rows of the
// 32 x 32 result = registers) and z its B operand (columns = lanes), so the running (min, argmin) of a z row lives in ONE lane and is
// updated with two VALU ops per score, no cross-lane traffic until the block's last instruction.  When M is small the codebook is
// split over blockIdx.y; vq_nearest_merge_kernel folds the per-split pairs.
#include "common.h"
#include "kernels.h"

namespace {
constexpr int VC_T = 128;        // rows of z / codes per block tile
constexpr int VC_KC = 32;        // k per staged chunk
constexpr int VC_LD = 36;        // LDS row stride in floats: 144 B = 9 sixteen-byte slots (odd), every ds_read_b128 lane group lands on 16 distinct slots
constexpr int VC_SENTINEL = 0x7fffffff;

__device__ __forceinline__ bool vc_better(float s, int i, float bs, int bi) { return s < bs || (s == bs && i < bi); }

// |e_j|^2 in fp32, one fixed order (k ascending, one fma per element)
__global__ void vq_code_norms_kernel(const float* __restrict__ cb, float* __restrict__ norms, int N, int E) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const float4* row = (const float4*)(cb + (size_t)j * E);
    float n = 0.f;
    for (int k = 0; k < E / 4; k++) {
        const float4 v = row[k];
        n = fmaf(v.x, v.x, n); n = fmaf(v.y, v.y, n); n = fmaf(v.z, v.z, n); n = fmaf(v.w, v.w, n);
    }
    norms[j] = n;
}

__global__ __launch_bounds__(256) void vq_nearest_kernel(const float* __restrict__ z, const float* __restrict__ cb, const float* __restrict__ norms,
                                                         long long M, int N, int E, int tiles_per_split, float* __restrict__ ws_score,
                                                         int* __restrict__ ws_idx) {
    __shared__ __attribute__((aligned(16))) float sA[VC_T * VC_LD];      // codes [code][k]
    __shared__ __attribute__((aligned(16))) float sB[VC_T * VC_LD];      // z     [row][k]
    __shared__ float sN[VC_T];                                           // |e|^2 of the tile's codes, +inf for codes >= N: a padded code never wins
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wi = wave >> 1, wj = wave & 1, r = lane & 31, h = lane >> 5;
    const long long row0 = (long long)blockIdx.x * VC_T;
    const int ntiles = (N + VC_T - 1) / VC_T;
    const int tile_lo = blockIdx.y * tiles_per_split;
    const int tile_hi = min(ntiles, tile_lo + tiles_per_split);
    const int nkc = E / VC_KC, niter = (tile_hi - tile_lo) * nkc;

    // staging: thread t moves four 16-byte pieces of each operand per chunk: piece f = t + 256 i -> row f >> 3, floats 4 (f & 7) ..
    float4 ga[4], gb[4]; float gn = 0.f;
    auto fetch = [&](int it) {
        const int tile = tile_lo + it / nkc, k0 = (it % nkc) * VC_KC;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = t + 256 * i, row = f >> 3, c4 = (f & 7) * 4;
            const long long code = (long long)tile * VC_T + row, m = row0 + row;
            ga[i] = code < N ? *(const float4*)(cb + code * E + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            gb[i] = m < M ? *(const float4*)(z + m * E + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (k0 == 0 && t < VC_T) { const int code = tile * VC_T + t; gn = code < N ? norms[code] : __builtin_inff(); }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[a][b][q] = 0.f;
    float best[2] = {__builtin_inff(), __builtin_inff()};
    int bidx[2] = {VC_SENTINEL, VC_SENTINEL};

    if (niter > 0) fetch(0);
    for (int it = 0; it < niter; it++) {
        const int kc = it % nkc, tile = tile_lo + it / nkc;
        __syncthreads();                                  // the previous chunk's reads (and a finished tile's sN reads) are done
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = t + 256 * i, row = f >> 3, c4 = (f & 7) * 4;
            *(float4*)(sA + row * VC_LD + c4) = ga[i];
            *(float4*)(sB + row * VC_LD + c4) = gb[i];
        }
        if (kc == 0 && t < VC_T) sN[t] = gn;
        __syncthreads();
        if (it + 1 < niter) fetch(it + 1);                // in flight under this chunk's MFMAs
#pragma unroll
        for (int s = 0; s < VC_KC / 8; s++) {
            // lane (r, h) reads k = 8 s + 4 h .. + 3 of its operand row; MFMA u of the step sums k = 8 s + u (h = 0) then 8 s + 4 + u (h = 1)
            float4 a[2], b[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                a[q] = *(const float4*)(sA + (wi * 64 + q * 32 + r) * VC_LD + s * 8 + h * 4);
                b[q] = *(const float4*)(sB + (wj * 64 + q * 32 + r) * VC_LD + s * 8 + h * 4);
            }
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int tj = 0; tj < 2; tj++) {
                    acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti].x, b[tj].x, acc[ti][tj], 0, 0, 0);
                    acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti].y, b[tj].y, acc[ti][tj], 0, 0, 0);
                    acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti].z, b[tj].z, acc[ti][tj], 0, 0, 0);
                    acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti].w, b[tj].w, acc[ti][tj], 0, 0, 0);
                }
        }
        if (kc == nkc - 1) {
            // result register q of a 32 x 32 tile: code row (q & 3) + 8 (q >> 2) + 4 h, z row = lane column r.  Codes are visited in ascending
            // index order per lane, so the strict compare keeps the first minimum; NaN scores (non-finite z) never win
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    const int cl = wi * 64 + ti * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                    const float n = sN[cl];
                    const int code = tile * VC_T + cl;
#pragma unroll
                    for (int tj = 0; tj < 2; tj++) {
                        const float sc = fmaf(-2.f, acc[ti][tj][q], n);
                        if (sc < best[tj]) { best[tj] = sc; bidx[tj] = code; }
                        acc[ti][tj][q] = 0.f;
                    }
                }
        }
    }
    // block reduction: row (wj, tj, r) has four candidates (wi, h)
    __syncthreads();
    float* rs = sA; int* ri = (int*)sB;
#pragma unroll
    for (int tj = 0; tj < 2; tj++) {
        const int row = wj * 64 + tj * 32 + r;
        rs[row * 4 + wi * 2 + h] = best[tj]; ri[row * 4 + wi * 2 + h] = bidx[tj];
    }
    __syncthreads();
    if (t < VC_T && row0 + t < M) {
        float bs = rs[t * 4]; int bi = ri[t * 4];
#pragma unroll
        for (int q = 1; q < 4; q++) { const float s = rs[t * 4 + q]; const int i = ri[t * 4 + q]; if (vc_better(s, i, bs, bi)) { bs = s; bi = i; } }
        ws_score[(long long)blockIdx.y * M + row0 + t] = bs;
        ws_idx[(long long)blockIdx.y * M + row0 + t] = bi;
    }
}

// folds the per-split (score, index) pairs; an index that no finite score produced (non-finite z) becomes 0: the result indexes a gather
__global__ void vq_nearest_merge_kernel(const float* __restrict__ ws_score, const int* __restrict__ ws_idx, long long M, int N, int S,
                                        int* __restrict__ idx32, long long* __restrict__ idx64) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float bs = ws_score[m]; int bi = ws_idx[m];
    for (int s = 1; s < S; s++) {
        const float sc = ws_score[(long long)s * M + m]; const int i = ws_idx[(long long)s * M + m];
        if (vc_better(sc, i, bs, bi)) { bs = sc; bi = i; }
    }
    if ((unsigned)bi >= (unsigned)N) bi = 0;
    if (idx32) idx32[m] = bi;
    if (idx64) idx64[m] = bi;
}

// out f32 [B, E, HW] (NCHW) from token-major rows: row idx[token] of src (codebook rows) or, idx null, row `token` itself
__global__ void vq_rows_to_nchw_kernel(const float* __restrict__ src, const int* __restrict__ idx, float* __restrict__ out, int B, int HW, int E) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, p0 = blockIdx.x * 32, e0 = blockIdx.y * 32, tx = threadIdx.x, ty = threadIdx.y;
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i;
        if (p < HW) {
            const long long tok = (long long)b * HW + p, row = idx ? idx[tok] : tok;
            tile[i][tx] = src[row * E + e0 + tx];
        }
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + tx;
        if (p < HW) out[((long long)b * E + e0 + i) * HW + p] = tile[tx][i];
    }
}
}  // namespace

static void vq_nearest_grid(long long M, int N, long long* rowtiles, int* tps, int* S) {
    const int ntiles = (N + VC_T - 1) / VC_T;
    *rowtiles = (M + VC_T - 1) / VC_T;
    // two blocks per CU of a 256-CU device before the code range is left whole
    long long want = (512 + *rowtiles - 1) / *rowtiles;
    if (want < 1) want = 1;
    if (want > ntiles) want = ntiles;
    *tps = (ntiles + (int)want - 1) / (int)want;
    *S = (ntiles + *tps - 1) / *tps;
}

bool vq_nearest_supported(int E) { return E > 0 && E % 64 == 0 && E <= 512; }

size_t vq_nearest_ws_bytes(long long M, int N) {
    long long rt; int tps, S; vq_nearest_grid(M, N, &rt, &tps, &S);
    return (size_t)S * (size_t)M * 8;
}

hipError_t launch_vq_code_norms(const float* codebook, float* norms, int N, int E, hipStream_t st) {
    vq_code_norms_kernel<<<(N + 255) / 256, 256, 0, st>>>(codebook, norms, N, E);
    return hipGetLastError();
}

hipError_t launch_vq_nearest(const float* z, const float* codebook, const float* norms, long long M, int N, int E, char* ws, int* idx32,
                             long long* idx64, hipStream_t st) {
    if (!vq_nearest_supported(E) || M < 1 || N < 1) return hipErrorInvalidValue;
    long long rt; int tps, S; vq_nearest_grid(M, N, &rt, &tps, &S);
    if (rt > 0x7fffffffLL) return hipErrorInvalidValue;
    float* ws_score = (float*)ws; int* ws_idx = (int*)(ws + (size_t)S * (size_t)M * 4);
    vq_nearest_kernel<<<dim3((unsigned)rt, (unsigned)S), 256, 0, st>>>(z, codebook, norms, M, N, E, tps, ws_score, ws_idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    vq_nearest_merge_kernel<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(ws_score, ws_idx, M, N, S, idx32, idx64);
    return hipGetLastError();
}

hipError_t launch_vq_rows_to_nchw(const float* src, const int* idx, float* out, int B, int HW, int E, hipStream_t st) {
    vq_rows_to_nchw_kernel<<<dim3((HW + 31) / 32, E / 32, B), dim3(32, 8), 0, st>>>(src, idx, out, B, HW, E);
    return hipGetLastError();
}
