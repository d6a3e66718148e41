// Metric arithmetic on feature sets (f32 [n, d] row-major): the moments behind the Frechet distance, the streaming distance searches
// behind improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020), and the polynomial-kernel
// row sums behind KID (Binkowski et al. 2018).  Two launch groups; metric_dist is ONE kernel with five epilogues on the same dot products:
//   metric_moments   sum += SUM_i x_i,  outer += SUM_i x_i x_i^T            in fp64 (v_mfma_f64_16x16x4_f64)
//   metric_dist<0>   radius2[i] = k-th smallest d2(x_i, x_j) over j != i    (self left out BY INDEX: a duplicate is a neighbour at 0)
//   metric_dist<1>   hit[i]     = OR_j   d2(probe_i, ref_j) <= radius2[j]
//   metric_dist<2>   count[i]   = SUM_j  d2(probe_i, ref_j) <= radius2[j]   (int32; mode 1 with += for |=)
//   metric_dist<3>   nearest2[i] = MIN_j d2(probe_i, ref_j)                 (nothing left out)
//   metric_dist<4>   rowsum[g, i] = SUM_j (gamma (probe_gi . ref_gj) + coef0)^3   in fp64, optionally without j == i; no norms
//
// Distance arithmetic, shared by the four searches:  d2(a, b) = max(0, fma(-2, a.b, |a|^2 + |b|^2)), everything fp32.  The dot product and the
// two norms are the SAME two-level chain over k: inside a 32-wide chunk an fp32 fma chain from 0 in the order the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32) walks it (per 8 k: k, k+4, k+1, k+5, k+2, k+6, k+3, k+7: the lane halves of one MFMA hold k and k + 4),
// then the chunk sums are added in ascending chunk order.  metric_row_norms_kernel restates that chain on the VALU, so a.a from the
// matrix pipe equals |a|^2 bit for bit and two equal rows are at distance exactly 0.  (The chunk level keeps a norm's error, a sum of
// positive terms, at ~1e-7 |a|^2 for d = 512; one chain over all of k drifts to ~3e-7 rms.)  A pair's value is therefore produced by
// one instruction sequence wherever the pair lands: it does not depend on n, m, on the tile or lane either row sits in, nor on which of
// the two is the probe.  The reductions only compare.  Nothing here consults the deterministic switch; no atomics exist.
//
// The polynomial mode takes the SAME fp32 dot product (|dot - exact| <= 2.5e-7 (|a|^2 + |b|^2), the dot's half of the d2 budget) and does
// everything after it in fp64, per pair: convert, one fma (gamma dot + coef0), two multiplies (the cube), one add into the lane's running
// sum.  That is 5 fp64 VALU operations per pair against 2 d MFMA flops, negligible from d = 128 up: per tile a wave issues 2 d MFMAs of 64
// cycles and 320 fp64 operations of 4 (the vector fp64 rate is half the fp32 one), 8 % of the MFMA time at d = 128 and 2 % at d = 512,
// where a 50 000 x 50 000 product measures the same 34 ms in this mode as in the hit mode.  A lane's sum takes its
// reference rows in ascending tile order, then ascending result register; the four lanes of a probe are added in the order (wi, h)
// ascending.  A row sum therefore depends on the row, its group's reference rows and n alone: not on m, the group count or the block.
//
// Structure of metric_dist (the tiling of vqcode.hip, another reduction): a block owns 128 probe rows and walks all 128-row tiles of
// the reference set; the reference rows are the MFMA's A operand (result rows = registers) and the probes its B operand (columns =
// lanes), so a probe's running state -- its 8 smallest distances, its hit flag or count, its minimum, or its fp64 sum -- lives in ONE
// lane; four lanes per probe are merged through LDS at the end.  Nothing of size n x n is stored.  blockIdx.y is a GROUP: probe
// [G, M, D] and ref [G, N, D], group g's probes see group g's reference rows only (KID's subsets in one launch); all offsets are 64-bit.
// Only the polynomial mode is launched with G > 1 (the norms and radii of the other modes are not offset).
//
// metric_moments: a block owns a 32 x 32 tile of the d x d outer product (tiles on and above the diagonal only, mirrored on store) and
// a contiguous range of rows; each wave a 16 x 16 quarter in one f64 MFMA accumulator, rows taken four at a time in ascending order.
// Products of two floats are exact in fp64, so only the adds round.  When d is small the rows are split over blockIdx.z into partial
// planes that metric_moments_fold_kernel adds in split order: the order is fixed by (n, d) alone, so a call is reproducible;
// differently chunked calls differ by fp64 rounding only.
#include "common.h"
#include "kernels.h"

namespace {
typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int MT_T = 128;        // probe rows / reference rows per block tile
constexpr int MT_KC = 32;        // k per staged chunk = the inner chain's length
constexpr int MT_LD = 36;        // LDS row stride in floats (144 B: odd count of 16-byte slots, see vqcode.hip)
constexpr int MT_K = 8;          // neighbours kept per probe

// |x_i|^2 by the chain of the header (the VALU restatement of what the MFMAs of metric_dist_kernel do with a row against itself)
__global__ void metric_row_norms_kernel(const float* __restrict__ x, float* __restrict__ norms, int n, int d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4* row = (const float4*)(x + (size_t)i * d);
    float tot = 0.f;
    for (int c = 0; c < d / MT_KC; c++) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < MT_KC / 8; q++) {
            const float4 lo = row[c * 8 + 2 * q], hi = row[c * 8 + 2 * q + 1];
            s = fmaf(lo.x, lo.x, s); s = fmaf(hi.x, hi.x, s);
            s = fmaf(lo.y, lo.y, s); s = fmaf(hi.y, hi.y, s);
            s = fmaf(lo.z, lo.z, s); s = fmaf(hi.z, hi.z, s);
            s = fmaf(lo.w, lo.w, s); s = fmaf(hi.w, hi.w, s);
        }
        tot = tot + s;
    }
    norms[i] = tot;
}

// keeps top[0] <= ... <= top[7], the 8 smallest values seen
__device__ __forceinline__ void mt_insert(float (&top)[MT_K], float v) {
#pragma unroll
    for (int i = 0; i < MT_K; i++) {
        const float lo = fminf(top[i], v);
        v = fmaxf(top[i], v);
        top[i] = lo;
    }
}

enum { MT_RADIUS = 0, MT_HIT = 1, MT_COUNT = 2, MT_NEAREST = 3, MT_POLY = 4 };

// MODE 0: radius2 of the probes within their own set (probe == ref, M == N); 1 / 2: manifold hits / counts of the probes against
// (ref, rr2); 3: the nearest reference row's d2; 4: cubic-kernel row sums per group (pn, rn, rr2 unused and null).  out: f32 [M] (0, 3),
// uint8 [M] (1), int32 [M] (2), f64 [G, M] (4)
template <int MODE>
__global__ __launch_bounds__(256) void metric_dist_kernel(const float* __restrict__ probe, const float* __restrict__ pn, int M,
                                                          const float* __restrict__ ref, const float* __restrict__ rn,
                                                          const float* __restrict__ rr2, int N, int D, int kth, int excl, float gamma,
                                                          float coef0, void* __restrict__ out) {
    constexpr bool DIST = MODE != MT_POLY;                               // the modes on d2: they need the norms
    constexpr bool BALL = MODE == MT_HIT || MODE == MT_COUNT;            // the modes that compare with a radius per reference row
    __shared__ __attribute__((aligned(16))) float sA[MT_T * MT_LD];      // reference rows [row][k]
    __shared__ __attribute__((aligned(16))) float sB[MT_T * MT_LD];      // probe rows     [row][k]
    __shared__ float sN[MT_T];                                           // |ref|^2 of the tile, +inf for rows >= N: their distance is +inf
    __shared__ float sR[MT_T];                                           // MODE 1, 2: radius2 of the tile's rows (-1 for rows >= N)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wi = wave >> 1, wj = wave & 1, r = lane & 31, h = lane >> 5;
    const long long row0 = (long long)blockIdx.x * MT_T;
    probe += (long long)blockIdx.y * M * D;               // the group's rows
    ref += (long long)blockIdx.y * N * D;
    const int ntiles = (N + MT_T - 1) / MT_T;
    const int nkc = D / MT_KC;
    const long long niter = (long long)ntiles * nkc;

    float4 ga[4], gb[4]; float gn = 0.f, gr = 0.f;
    auto fetch = [&](long long it) {
        const int tile = (int)(it / nkc), k0 = (int)(it % nkc) * MT_KC;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = t + 256 * i, row = f >> 3, c4 = (f & 7) * 4;
            const long long j = (long long)tile * MT_T + row, m = row0 + row;
            ga[i] = j < N ? *(const float4*)(ref + j * D + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            gb[i] = m < M ? *(const float4*)(probe + m * D + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (DIST && k0 == 0 && t < MT_T) {
            const long long j = (long long)tile * MT_T + t;
            gn = j < N ? rn[j] : __builtin_inff();
            if (BALL) gr = j < N ? rr2[j] : -1.f;
        }
    };

    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int q = 0; q < 16; q++) { acc[a][b][q] = 0.f; tot[a][b][q] = 0.f; }
    // the lane's two probes
    long long prow[2]; float pnorm[2];
#pragma unroll
    for (int tj = 0; tj < 2; tj++) {
        prow[tj] = row0 + wj * 64 + tj * 32 + r;
        pnorm[tj] = DIST && prow[tj] < M ? pn[prow[tj]] : 0.f;
    }
    float top[2][MT_K];
#pragma unroll
    for (int tj = 0; tj < 2; tj++)
#pragma unroll
        for (int i = 0; i < MT_K; i++) top[tj][i] = __builtin_inff();
    int hit[2] = {0, 0};                                  // MODE 1: flag; MODE 2: count
    float best[2] = {__builtin_inff(), __builtin_inff()};
    double psum[2] = {0.0, 0.0};

    if (niter > 0) fetch(0);
    for (long long it = 0; it < niter; it++) {
        const int kc = (int)(it % nkc), tile = (int)(it / nkc);
        __syncthreads();                                  // the previous chunk's reads (and a finished tile's sN / sR reads) are done
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = t + 256 * i, row = f >> 3, c4 = (f & 7) * 4;
            *(float4*)(sA + row * MT_LD + c4) = ga[i];
            *(float4*)(sB + row * MT_LD + c4) = gb[i];
        }
        if (DIST && kc == 0 && t < MT_T) { sN[t] = gn; if (BALL) sR[t] = gr; }
        __syncthreads();
        if (it + 1 < niter) fetch(it + 1);                // in flight under this chunk's MFMAs
#pragma unroll
        for (int s = 0; s < MT_KC / 8; s++) {
            // lane (r, h) reads k = 8 s + 4 h .. + 3 of its operand row; MFMA u of the step sums k = 8 s + u (h = 0) then 8 s + 4 + u (h = 1)
            float4 a[2], b[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                a[q] = *(const float4*)(sA + (wi * 64 + q * 32 + r) * MT_LD + s * 8 + h * 4);
                b[q] = *(const float4*)(sB + (wj * 64 + q * 32 + r) * MT_LD + s * 8 + h * 4);
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
        // outer level of the chain: chunk sums in ascending chunk order
#pragma unroll
        for (int ti = 0; ti < 2; ti++)
#pragma unroll
            for (int tj = 0; tj < 2; tj++)
#pragma unroll
                for (int q = 0; q < 16; q++) { tot[ti][tj][q] = tot[ti][tj][q] + acc[ti][tj][q]; acc[ti][tj][q] = 0.f; }
        if (kc == nkc - 1) {
            // result register q of a 32 x 32 tile: reference row (q & 3) + 8 (q >> 2) + 4 h, probe = lane column r
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    const int cl = wi * 64 + ti * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                    const long long j = (long long)tile * MT_T + cl;
                    if (MODE == MT_POLY) {
                        // fp64 from here: k = gamma dot + coef0, k^3 into the lane's sum; rows past N and (excl) the pair j == i add nothing
#pragma unroll
                        for (int tj = 0; tj < 2; tj++) {
                            const double v = fma((double)gamma, (double)tot[ti][tj][q], (double)coef0);
                            tot[ti][tj][q] = 0.f;
                            const bool keep = j < N && !(excl && j == prow[tj]);
                            psum[tj] += keep ? (v * v) * v : 0.0;
                        }
                        continue;
                    }
                    const float n = sN[cl];
#pragma unroll
                    for (int tj = 0; tj < 2; tj++) {
                        float d2 = fmaxf(fmaf(-2.f, tot[ti][tj][q], pnorm[tj] + n), 0.f);
                        tot[ti][tj][q] = 0.f;
                        if (MODE == MT_RADIUS) {
                            if (j == prow[tj]) d2 = __builtin_inff();          // self, by index
                            mt_insert(top[tj], d2);
                        } else if (MODE == MT_HIT) {
                            hit[tj] |= d2 <= sR[cl] ? 1 : 0;
                        } else if (MODE == MT_COUNT) {
                            hit[tj] += d2 <= sR[cl] ? 1 : 0;
                        } else {
                            best[tj] = fminf(best[tj], d2);
                        }
                    }
                }
        }
    }
    // block reduction: probe (wj, tj, r) has four partial states (wi, h)
    __syncthreads();
    if (MODE == MT_RADIUS) {
        float* rs = sA;                                   // [128][4][8] floats = 16 KB of sA's 18
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int i = 0; i < MT_K; i++) rs[((wj * 64 + tj * 32 + r) * 4 + wi * 2 + h) * MT_K + i] = top[tj][i];
        __syncthreads();
        if (t < MT_T && row0 + t < M) {
            float best8[MT_K];
#pragma unroll
            for (int i = 0; i < MT_K; i++) best8[i] = rs[t * 4 * MT_K + i];
            for (int s = MT_K; s < 4 * MT_K; s++) mt_insert(best8, rs[t * 4 * MT_K + s]);
            float res = best8[0];
#pragma unroll
            for (int i = 1; i < MT_K; i++) res = (i == kth - 1) ? best8[i] : res;
            ((float*)out)[row0 + t] = res;
        }
    } else if (BALL) {
        int* rs = (int*)sA;
#pragma unroll
        for (int tj = 0; tj < 2; tj++) rs[(wj * 64 + tj * 32 + r) * 4 + wi * 2 + h] = hit[tj];
        __syncthreads();
        if (t < MT_T && row0 + t < M) {
            if (MODE == MT_HIT) ((unsigned char*)out)[row0 + t] = (unsigned char)((rs[t * 4] | rs[t * 4 + 1] | rs[t * 4 + 2] | rs[t * 4 + 3]) != 0);
            else ((int*)out)[row0 + t] = rs[t * 4] + rs[t * 4 + 1] + rs[t * 4 + 2] + rs[t * 4 + 3];
        }
    } else if (MODE == MT_NEAREST) {
        float* rs = sA;
#pragma unroll
        for (int tj = 0; tj < 2; tj++) rs[(wj * 64 + tj * 32 + r) * 4 + wi * 2 + h] = best[tj];
        __syncthreads();
        if (t < MT_T && row0 + t < M) ((float*)out)[row0 + t] = fminf(fminf(rs[t * 4], rs[t * 4 + 1]), fminf(rs[t * 4 + 2], rs[t * 4 + 3]));
    } else {
        double* rs = (double*)sA;                         // [128][4] doubles = 4 KB
#pragma unroll
        for (int tj = 0; tj < 2; tj++) rs[(wj * 64 + tj * 32 + r) * 4 + wi * 2 + h] = psum[tj];
        __syncthreads();
        // the four lanes of a probe in the order (wi, h) ascending
        if (t < MT_T && row0 + t < M) ((double*)out)[(long long)blockIdx.y * M + row0 + t] = ((rs[t * 4] + rs[t * 4 + 1]) + rs[t * 4 + 2]) + rs[t * 4 + 3];
    }
}

// ---- moments
constexpr int MM_T = 32;         // outer-product tile of a block: 2 x 2 waves of 16 x 16
constexpr int MM_ROWS = 128;     // fewest rows worth a split of their own

// the rows of split z of S: [lo, hi), multiples of 4 but for the last split's end
__device__ __forceinline__ void mm_range(int n, int S, int z, int* lo, int* hi) {
    const int per = (((n + S - 1) / S) + 3) & ~3;
    *lo = min(n, z * per); *hi = min(n, *lo + per);
}

// grid (d / 32, d / 32, S).  S == 1: outer += tile; else the tile goes to plane z of ws [S][d * d + d].  The outer product is symmetric:
// only the tiles on and above the diagonal are computed, each off-diagonal one stored twice (so both triangles are bitwise equal)
__global__ __launch_bounds__(256) void metric_outer_kernel(const float* __restrict__ x, int n, int d, int S, double* __restrict__ outer,
                                                           double* __restrict__ ws) {
    if (blockIdx.x > blockIdx.y) return;
    const bool mirror = blockIdx.x != blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a0 = blockIdx.x * MM_T + (wave >> 1) * 16, b0 = blockIdx.y * MM_T + (wave & 1) * 16;
    const int c = lane & 15, g = lane >> 4;               // operand lane: column c of the quarter, row g of the group of four
    int lo, hi; mm_range(n, S, blockIdx.z, &lo, &hi);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const float* xa = x + a0 + c; const float* xb = x + b0 + c;
    for (int i0 = lo; i0 < hi; i0 += 16) {
        float fa[4], fb[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + 4 * u + g;
            fa[u] = i < hi ? xa[(size_t)i * d] : 0.f;
            fb[u] = i < hi ? xb[(size_t)i * d] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fa[u], (double)fb[u], acc, 0, 0, 0);
    }
    // f64 C/D map: column = lane & 15, row = (lane >> 4) + 4 * register
    double* dst = S == 1 ? outer : ws + (size_t)blockIdx.z * ((size_t)d * d + d);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const size_t e = (size_t)(a0 + g + 4 * q) * d + b0 + c, et = (size_t)(b0 + c) * d + a0 + g + 4 * q;
        dst[e] = S == 1 ? dst[e] + acc[q] : acc[q];
        if (mirror) dst[et] = S == 1 ? dst[et] + acc[q] : acc[q];
    }
}

// grid (d / 32, S), 256 threads = 8 row lanes x 32 columns: column sums of the split's rows, row lane by row lane, then the 8 in order
__global__ __launch_bounds__(256) void metric_sum_kernel(const float* __restrict__ x, int n, int d, int S, double* __restrict__ sum,
                                                         double* __restrict__ ws) {
    __shared__ double part[8][MM_T];
    const int c = threadIdx.x & 31, rl = threadIdx.x >> 5, col = blockIdx.x * MM_T + c;
    int lo, hi; mm_range(n, S, blockIdx.y, &lo, &hi);
    double s = 0.0;
    for (int i = lo + rl; i < hi; i += 8) s += (double)x[(size_t)i * d + col];
    part[rl][c] = s;
    __syncthreads();
    if (rl == 0) {
        double tsum = part[0][c];
#pragma unroll
        for (int q = 1; q < 8; q++) tsum += part[q][c];
        if (S == 1) sum[col] = sum[col] + tsum;
        else ws[(size_t)blockIdx.y * ((size_t)d * d + d) + (size_t)d * d + col] = tsum;
    }
}

// outer, sum += the S planes in split order
__global__ void metric_moments_fold_kernel(const double* __restrict__ ws, int d, int S, double* __restrict__ outer, double* __restrict__ sum) {
    const size_t per = (size_t)d * d + d, e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= per) return;
    double tsum = ws[e];
    for (int s = 1; s < S; s++) tsum += ws[(size_t)s * per + e];
    double* dst = e < (size_t)d * d ? outer + e : sum + (e - (size_t)d * d);
    *dst = *dst + tsum;
}
}  // namespace

bool metric_dim_supported(int d) { return d >= 32 && d <= 4096 && d % 32 == 0; }

// row splits of the moments: two blocks per CU of a 256-CU device before the rows are left whole, MM_ROWS rows a split at the least
static int metric_moments_splits(int n, int d) {
    const long long tiles = (long long)(d / MM_T) * (d / MM_T + 1) / 2;          // on and above the diagonal
    long long want = (512 + tiles - 1) / tiles, cap = (n + MM_ROWS - 1) / MM_ROWS;
    if (want > cap) want = cap;
    return want < 1 ? 1 : (int)want;
}

size_t metric_moments_ws_bytes(int n, int d) {
    const int S = metric_moments_splits(n, d);
    return S == 1 ? 0 : (size_t)S * ((size_t)d * d + d) * sizeof(double);
}

hipError_t launch_metric_row_norms(const float* x, float* norms, int n, int d, hipStream_t st) {
    if (!metric_dim_supported(d) || n < 1) return hipErrorInvalidValue;
    metric_row_norms_kernel<<<(n + 127) / 128, 128, 0, st>>>(x, norms, n, d);
    return hipGetLastError();
}

hipError_t launch_metric_knn_radius(const float* x, const float* norms, int n, int d, int k, float* radius2, hipStream_t st) {
    if (!metric_dim_supported(d) || k < 1 || k > MT_K || k >= n) return hipErrorInvalidValue;
    metric_dist_kernel<MT_RADIUS><<<(n + MT_T - 1) / MT_T, 256, 0, st>>>(x, norms, n, x, norms, nullptr, n, d, k, 0, 0.f, 0.f, radius2);
    return hipGetLastError();
}

hipError_t launch_metric_manifold_hits(const float* probe, const float* pnorms, int m, const float* ref, const float* rnorms, const float* ref_radius2,
                                       int n, int d, unsigned char* hit, hipStream_t st) {
    if (!metric_dim_supported(d) || m < 1 || n < 1) return hipErrorInvalidValue;
    metric_dist_kernel<MT_HIT><<<(m + MT_T - 1) / MT_T, 256, 0, st>>>(probe, pnorms, m, ref, rnorms, ref_radius2, n, d, 0, 0, 0.f, 0.f, hit);
    return hipGetLastError();
}

hipError_t launch_metric_manifold_counts(const float* probe, const float* pnorms, int m, const float* ref, const float* rnorms, const float* ref_radius2,
                                         int n, int d, int* count, hipStream_t st) {
    if (!metric_dim_supported(d) || m < 1 || n < 1) return hipErrorInvalidValue;
    metric_dist_kernel<MT_COUNT><<<(m + MT_T - 1) / MT_T, 256, 0, st>>>(probe, pnorms, m, ref, rnorms, ref_radius2, n, d, 0, 0, 0.f, 0.f, count);
    return hipGetLastError();
}

hipError_t launch_metric_nearest_d2(const float* probe, const float* pnorms, int m, const float* ref, const float* rnorms, int n, int d, float* d2,
                                    hipStream_t st) {
    if (!metric_dim_supported(d) || m < 1 || n < 1) return hipErrorInvalidValue;
    metric_dist_kernel<MT_NEAREST><<<(m + MT_T - 1) / MT_T, 256, 0, st>>>(probe, pnorms, m, ref, rnorms, nullptr, n, d, 0, 0, 0.f, 0.f, d2);
    return hipGetLastError();
}

hipError_t launch_metric_poly3_rowsums(const float* probe, int m, const float* ref, int n, int d, int groups, int exclude_same_index, float gamma,
                                       float coef0, double* rowsum, hipStream_t st) {
    if (!metric_dim_supported(d) || m < 1 || n < 1 || groups < 1 || groups > METRIC_MAX_GROUPS) return hipErrorInvalidValue;
    metric_dist_kernel<MT_POLY><<<dim3((m + MT_T - 1) / MT_T, groups), 256, 0, st>>>(probe, nullptr, m, ref, nullptr, nullptr, n, d, 0,
                                                                                     exclude_same_index ? 1 : 0, gamma, coef0, rowsum);
    return hipGetLastError();
}

hipError_t launch_metric_moments(const float* x, int n, int d, double* sum, double* outer, char* ws, hipStream_t st) {
    if (!metric_dim_supported(d) || n < 1) return hipErrorInvalidValue;
    const int S = metric_moments_splits(n, d);
    if (S > 1 && !ws) return hipErrorInvalidValue;
    metric_outer_kernel<<<dim3(d / MM_T, d / MM_T, S), 256, 0, st>>>(x, n, d, S, outer, (double*)ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    metric_sum_kernel<<<dim3(d / MM_T, S), 256, 0, st>>>(x, n, d, S, sum, (double*)ws);
    e = hipGetLastError();
    if (e != hipSuccess || S == 1) return e;
    const size_t per = (size_t)d * d + d;
    metric_moments_fold_kernel<<<(unsigned)((per + 255) / 256), 256, 0, st>>>((const double*)ws, d, S, outer, sum);
    return hipGetLastError();
}
