// Streaming single-head attention for the first stage's AttnBlock (gfx950).
// Replaces, beyond 4096 tokens, the materialised chain of ldm / taming AttnBlock.forward (q k^T * C^-1/2 -> softmax -> . v, one head of
// d = C channels over the n = H W latent pixels): out[b] = softmax(q[b] k[b]^T scale) v[b] + bias_v for token-major bf16
// q, k, v [B, n, C] with row strides, any n >= 1, C = 128 NCB <= 512.  No n x n tensor ever reaches memory.
//
// The arithmetic is the chain's (oracle/vq_emul.py): fp32 scores from bf16 operands scaled in fp32, p = __expf(s - max) * (1 / sum)
// against the exact row maximum, the NORMALISED p rounded to bf16 as the P.V operand, fp32 accumulation, + bias_v, one bf16 rounding.
// Rounding the normalised probability rules the online-softmax recurrence out (it rounds unnormalised ones and rescales O), so a block
// walks the keys TWICE: sweep 1 forms the scores and keeps the running row maximum and sum, sweep 2 forms the same scores again (the
// same MFMA sequence: bit-identical, so the maximum is exact), turns them into bf16 p and accumulates P.V.  Three GEMM-sized products
// instead of two, no rescale of the 128 accumulator registers and no statistics exchange inside sweep 2.
//
// A block = 4 waves = 64 query rows of one sample; the keys go by in groups of 128.
//   scores: the swapped product S^T = K . Q^T on 32x32x16 bf16 MFMAs (flash_d32's form): wave w takes keys 32 w .. 32 w + 31 of the
//           group against all 64 queries, K rows straight from global memory in operand layout (nobody else in the block reads them),
//           the Q tile from LDS (loaded once per block).  A lane then holds 16 scores of ONE query per 32-query half, so the
//           statistics are lane-local; the two lane halves and the four waves meet once, after sweep 1.
//   P.V:    wave w leaves its [64 queries][32 keys] of p in LDS (bf16, double-buffered by group); after a barrier every wave
//           accumulates O^T[its C/4 channels][64 queries] = V^T . P^T over the group's 128 keys.  V arrives token-major: each wave
//           copies its own [32 keys][C/4] slice into a private LDS region and reads the operand (8 consecutive keys of one channel per
//           lane) back through ds_read_b64_tr_b16, as flash_d32_lds_kernel<true> does.  No V^T GEMM.
// Ragged sizes: key and query rows beyond n are redirected to row n - 1 on the way in; the padding keys get probability exactly 0
// and enter neither the maximum nor the sum; stores of padding queries are dropped.  No atomics, no key split across blocks: a
// sample's result does not depend on the batch or on its place in it.
#include "kernels.h"

namespace {
constexpr int QB = 64;                       // query rows per block
constexpr int KG = 128;                      // keys per group (32 per wave)
constexpr int PSTR = KG * 2 + 16;            // bytes per query row of the p image (the 16: conflict-free ds_read_b128 at one row per lane)
constexpr float M_NONE = -3.0e38f;           // "no valid key yet": finite, so that M_NONE - M_NONE = 0 and no NaN can form

template <int NCB> struct Lay {              // NCB = C / 128 = 32-channel blocks of O per wave
    static constexpr int C = 128 * NCB, CW = 32 * NCB;
    static constexpr int QSTR = C * 2 + 16;                  // bytes per row of the Q tile
    static constexpr int VSTR = CW * 2 + 64;                 // bytes per key row of a wave's V slice: 4 rows of a transpose read 64 bytes apart mod 256
    static constexpr int Q_OFF = 0, P_OFF = QB * QSTR, V_OFF = P_OFF + 2 * QB * PSTR, S_OFF = V_OFF + 4 * 32 * VSTR, BYTES = S_OFF + 4 * QB * 8;
};
}

template <int NCB>
__global__ __launch_bounds__(256) void vq_attn_stream_kernel(VqAttnParams p) {
    using L = Lay<NCB>;
    constexpr int C = L::C, CW = L::CW, NKS = C / 16;
    extern __shared__ __attribute__((aligned(16))) char vsm[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = p.n, nlast = n - 1;
    const int nqb = (n + QB - 1) / QB;
    const int b = blockIdx.x / nqb, q0 = (blockIdx.x - b * nqb) * QB;
    const long long tok0 = (long long)b * n;

    // ---- the Q tile: 16-byte pieces, consecutive threads along a row; rows beyond n repeat row n - 1
    for (int id = tid; id < QB * (C / 8); id += 256) {
        const int row = id / (C / 8), pc = id - row * (C / 8);
        const int qr = min(q0 + row, nlast);
        *(uint4*)(vsm + L::Q_OFF + row * L::QSTR + pc * 16) = *(const uint4*)(p.q + (tok0 + qr) * p.ldq + pc * 8);
    }
    __syncthreads();

    // scores of this wave's 32 keys of the group at kg0 against the two 32-query halves: register r of a lane = key 8 (r >> 2) + 4 hf + (r & 3)
    // of the wave's 32, query l31 of the half
    const char* qlds = vsm + L::Q_OFF + l31 * L::QSTR + hf * 16;
    auto scores = [&](int kg0, f32x16 (&s)[2]) __attribute__((always_inline)) {
        const int key = min(kg0 + 32 * w + l31, nlast);
        const bf16_t* kp = p.k + (tok0 + key) * p.ldk + hf * 8;
#pragma unroll
        for (int r = 0; r < 16; r++) { s[0][r] = 0.f; s[1][r] = 0.f; }
#pragma unroll
        for (int kb = 0; kb < NKS; kb += 8) {
            bf16x8 kf[8];
#pragma unroll
            for (int u = 0; u < 8; u++) kf[u] = *(const bf16x8*)(kp + (kb + u) * 16);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const bf16x8 qa = *(const bf16x8*)(qlds + (kb + u) * 32);
                const bf16x8 qb = *(const bf16x8*)(qlds + 32 * L::QSTR + (kb + u) * 32);
                s[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[u], qa, s[0], 0, 0, 0);
                s[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[u], qb, s[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; r++) { s[0][r] *= p.scale; s[1][r] *= p.scale; }
    };

    // ---- sweep 1: row maximum and sum over the valid keys (running, lane-local)
    const int ngrp = (n + KG - 1) / KG;
    float m[2] = {M_NONE, M_NONE}, l[2] = {0.f, 0.f};
    for (int g = 0; g < ngrp; g++) {
        f32x16 s[2];
        scores(g * KG, s);
        const int kv0 = g * KG + 32 * w + 4 * hf;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            float mx = M_NONE;
#pragma unroll
            for (int r = 0; r < 16; r++) mx = fmaxf(mx, kv0 + 8 * (r >> 2) + (r & 3) < n ? s[h][r] : M_NONE);
            const float mn = fmaxf(m[h], mx);
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) sum += kv0 + 8 * (r >> 2) + (r & 3) < n ? __expf(s[h][r] - mn) : 0.f;
            l[h] = l[h] * __expf(m[h] - mn) + sum;
            m[h] = mn;
        }
    }
    // the two lane halves, then the four waves: every lane ends with the maximum and 1 / sum of its two queries
    float inv[2];
    {
        float2* st = (float2*)(vsm + L::S_OFF);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float mo = __shfl_xor(m[h], 32), lo = __shfl_xor(l[h], 32);
            const float mn = fmaxf(m[h], mo);
            l[h] = l[h] * __expf(m[h] - mn) + lo * __expf(mo - mn);
            m[h] = mn;
            if (hf == 0) st[w * QB + 32 * h + l31] = make_float2(m[h], l[h]);
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; h++) {
            float2 a[4];
#pragma unroll
            for (int ww = 0; ww < 4; ww++) a[ww] = st[ww * QB + 32 * h + l31];
            const float mn = fmaxf(fmaxf(a[0].x, a[1].x), fmaxf(a[2].x, a[3].x));
            float sum = 0.f;
#pragma unroll
            for (int ww = 0; ww < 4; ww++) sum += a[ww].y * __expf(a[ww].x - mn);
            m[h] = mn; inv[h] = 1.f / sum;
        }
    }

    // ---- sweep 2: p = bf16(exp(s - max) / sum) through LDS, O^T += V^T . P^T
    f32x16 o[2][NCB];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int cb = 0; cb < NCB; cb++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[h][cb][r] = 0.f;
    // this wave's V slice of a 32-key chunk: [32 keys][CW channels], NVL 16-byte pieces per lane
    constexpr int PPR = CW / 8, NVL = 2 * NCB;
    char* vl = vsm + L::V_OFF + w * 32 * L::VSTR;
    const bf16_t* vg[NVL];                                 // this lane's pieces: source at key row 0 of the sample, and the row inside the chunk
    int vrow[NVL]; char* vdst[NVL];
#pragma unroll
    for (int it = 0; it < NVL; it++) {
        const int id = it * 64 + lane, pc = id % PPR;
        vrow[it] = id / PPR;
        vg[it] = p.v + tok0 * p.ldv + CW * w + pc * 8;
        vdst[it] = vl + vrow[it] * L::VSTR + pc * 16;
    }
    bf16x8 vr[NVL];
#define VQA_VLOAD(key0) _Pragma("unroll") for (int it = 0; it < NVL; it++) vr[it] = *(const bf16x8*)(vg[it] + (long long)min((key0) + vrow[it], nlast) * p.ldv)
    // transpose read (ds_read_b64_tr_b16): a 16-lane group reads [4 keys][16 channels], lane i the 4 channels 4 (i & 3) .. of key i >> 2, and lane
    // j receives channel j of the 4 keys: lane (channel l31, half hf) gets keys 8 hf .. 8 hf + 3 of a 16-key step, and + 4 rows the other four
    const uint32_t vtr = (8 * hf + ((lane & 15) >> 2)) * L::VSTR + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    typedef __attribute__((ext_vector_type(4))) short s16x4;

    for (int g = 0; g < ngrp; g++) {
        const int kg0 = g * KG;
        VQA_VLOAD(kg0);                                       // chunk 0 travels behind the scores
        f32x16 s[2];
        scores(kg0, s);
        char* P = vsm + L::P_OFF + (g & 1) * QB * PSTR;
        const int kv0 = kg0 + 32 * w + 4 * hf;
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; j++) e[j] = kv0 + 8 * gg + j < n ? __expf(s[h][4 * gg + j] - m[h]) * inv[h] : 0.f;
                uint2 wv;
                wv.x = cvt_pk_bf16(e[0], e[1]); wv.y = cvt_pk_bf16(e[2], e[3]);
                *(uint2*)(P + (32 * h + l31) * PSTR + (32 * w + 8 * gg + 4 * hf) * 2) = wv;
            }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the slice is rewritten only after the reads of the chunk before (one wave: LDS runs in order)
#pragma unroll
            for (int it = 0; it < NVL; it++) *(bf16x8*)vdst[it] = vr[it];
            if (c < 3) { VQA_VLOAD(kg0 + 32 * (c + 1)); }
            __syncthreads();                                  // c == 0: the group's p from all four waves; every c: this wave's V slice
#pragma unroll
            for (int kk = 0; kk < 2; kk++) {
                const int kstep = 2 * c + kk;
                const bf16x8 pa = *(const bf16x8*)(P + l31 * PSTR + kstep * 32 + hf * 16);
                const bf16x8 pb = *(const bf16x8*)(P + (32 + l31) * PSTR + kstep * 32 + hf * 16);
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) {
                    const LDS_AS char* vb = (const LDS_AS char*)(vl + vtr + kk * 16 * L::VSTR + cb * 64);
                    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(vb));
                    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(vb + 4 * L::VSTR));
                    const bf16x8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                    o[0][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pa, o[0][cb], 0, 0, 0);
                    o[1][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb, o[1][cb], 0, 0, 0);
                }
            }
        }
    }

    // ---- out = bf16(O + bias_v): register r of a lane = channel 8 (r >> 2) + 4 hf + (r & 3) of the 32-block, query l31 of the half
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int row = q0 + 32 * h + l31;
        if (row >= n) continue;
        bf16_t* op = p.out + (tok0 + row) * p.ldo + CW * w + 4 * hf;
#pragma unroll
        for (int cb = 0; cb < NCB; cb++)
#pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                const int ch = 32 * cb + 8 * gg;
                float bv[4] = {0.f, 0.f, 0.f, 0.f};
                if (p.bias) {
#pragma unroll
                    for (int j = 0; j < 4; j++) bv[j] = p.bias[CW * w + 4 * hf + ch + j];
                }
                uint2 wv;
                wv.x = cvt_pk_bf16(o[h][cb][4 * gg] + bv[0], o[h][cb][4 * gg + 1] + bv[1]);
                wv.y = cvt_pk_bf16(o[h][cb][4 * gg + 2] + bv[2], o[h][cb][4 * gg + 3] + bv[3]);
                *(uint2*)(op + ch) = wv;
            }
    }
}

#undef VQA_VLOAD

bool vq_attn_stream_supported(int C) { return C >= 128 && C <= 512 && C % 128 == 0; }

template <int NCB>
static hipError_t launch_vq_attn_t(const VqAttnParams& p, int B, hipStream_t st) {
    static bool attr_dev[RDM_MAX_DEVICES] = {false};
    bool& attr = attr_dev[rdm_cur_device()];
    if (!attr) {
        hipError_t e = hipFuncSetAttribute((const void*)vq_attn_stream_kernel<NCB>, hipFuncAttributeMaxDynamicSharedMemorySize, Lay<NCB>::BYTES);
        if (e != hipSuccess) return e;
        attr = true;
    }
    const long long blocks = (long long)B * ((p.n + QB - 1) / QB);
    vq_attn_stream_kernel<NCB><<<(unsigned)blocks, 256, Lay<NCB>::BYTES, st>>>(p);
    return hipGetLastError();
}

hipError_t launch_vq_attn_stream(const VqAttnParams& p, int B, hipStream_t st) {
    if (!vq_attn_stream_supported(p.C) || B < 1 || p.n < 1 || (long long)B * ((p.n + QB - 1) / QB) > 0x7fffffffLL) return hipErrorInvalidValue;
    if (p.ldq % 8 || p.ldk % 8 || p.ldv % 8 || p.ldo % 4 || p.ldq < p.C || p.ldk < p.C || p.ldv < p.C || p.ldo < p.C) return hipErrorInvalidValue;
    switch (p.C / 128) {
        case 1: return launch_vq_attn_t<1>(p, B, st);
        case 2: return launch_vq_attn_t<2>(p, B, st);
        case 3: return launch_vq_attn_t<3>(p, B, st);
        default: return launch_vq_attn_t<4>(p, B, st);
    }
}
