// Kernels of the RARM (retrieval-augmented autoregressive) sampling path on gfx950:
//   LatentImageRETRO.sample              rdm/models/autoregression/transformer.py:224-294
//   RetrievalPatchTransformer.forward    rdm/modules/attention.py:199-272 (continuous=False: token embedding + positional
//                                        encoding, 18 causal BasicTransformerBlocks with cross-attention to the k neighbours)
//   top_k_logits / softmax / multinomial transformer.py:256-270 (taming Net2NetTransformer.top_k_logits)
// The reference re-runs the transformer over the WHOLE prefix for each of the 256 new tokens (:241-248, 32 896 token-forwards
// per image); here every step processes one token per sequence against a K/V cache.  A decode step is M = B' (<= 128) rows, so
// the linear layers are weight-bandwidth-bound launches of the shared GEMM (igemm.hip); what is new is below.
//
// The step index lives in DEVICE memory (`pos`): every kernel of a step reads it, the sampler increments it — so the launches
// of all steps are identical and nothing on the host depends on the step.
#include "kernels.h"

// Sum of one value per thread over the block of 256 in a FIXED order: xor butterfly inside each wave (every lane ends with the same
// bits), then (w0 + w1) + (w2 + w3) of the four wave sums.  `slot` is four floats the caller alternates between rounds: one barrier.
__device__ __forceinline__ float rarm_block_sum_fixed(float v, float* slot, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) slot[tid >> 6] = v;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

// ---------------------------------------------------------------- token embedding + positional encoding
// x[b, :] = proj_in.weight[token[b]] + positional_encoding[:, pos]   (attention.py:252-258), fp32 residual stream
__global__ __launch_bounds__(256) void rarm_embed_kernel(const long long* tokens, const float* emb, const float* pos_t /*[L][C]*/,
                                                         const int* pos, float* x, int B, int C, int vocab) {
    const int b = blockIdx.x, t = *pos;
    long long tok = tokens[b];
    if (tok < 0 || tok >= vocab) tok = 0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) x[(long long)b * C + c] = emb[tok * C + c] + pos_t[(long long)t * C + c];
}
hipError_t launch_rarm_embed(const long long* tokens, const float* emb, const float* pos_t, const int* pos, float* x, int B, int C,
                             int vocab, hipStream_t st) {
    rarm_embed_kernel<<<B, 256, 0, st>>>(tokens, emb, pos_t, pos, x, B, C, vocab);
    return hipGetLastError();
}

// The same for ALL positions of a range of sequences (the whole-sequence pass, rarm_exec.hip: rarm_seq_body): row r of x is position r % t
// of sequence r / t.  Token rows wrap at tok_rows: the unconditional half of a guided batch reads the conditional half's tokens.
__global__ __launch_bounds__(256) void rarm_embed_seq_kernel(const long long* tokens, int tok_ld, int tok_rows, int seq0, const float* emb,
                                                             const float* pos_t /*[L][C]*/, float* x, int t, int C, int vocab) {
    const long long r = blockIdx.x;
    const int s = (int)(r / t), i = (int)(r - (long long)s * t);
    long long tok = tokens[(long long)((seq0 + s) % tok_rows) * tok_ld + i];
    if (tok < 0 || tok >= vocab) tok = 0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) x[r * C + c] = emb[tok * C + c] + pos_t[(long long)i * C + c];
}
hipError_t launch_rarm_embed_seq(const long long* tokens, int tok_ld, int tok_rows, int seq0, const float* emb, const float* pos_t, float* x, long long rows,
                                 int t, int C, int vocab, hipStream_t st) {
    if (rows < 1 || rows > 0x7fffffffLL || t < 1 || tok_rows < 1) return hipErrorInvalidValue;
    rarm_embed_seq_kernel<<<(unsigned)rows, 256, 0, st>>>(tokens, tok_ld, tok_rows, seq0, emb, pos_t, x, t, C, vocab);
    return hipGetLastError();
}

// ---------------------------------------------------------------- token negative log-likelihood from logits
// nll[r] = logsumexp(logits[r, :]) - logits[r, target[r]]: F.cross_entropy(reduction='none') of LatentImageRETRO.compute_loss
// (rdm/models/autoregression/transformer.py:62-70), all in fp32.  One block per row, two passes over the row (maximum, then the sum of
// exponentials; the second pass finds the row in L2).  16-byte loads: V is even, so a row starts 0 or 8 bytes past a 16-byte boundary and
// the (at most two) elements before the first boundary and after the last are taken one by one.  Fixed order, no atomics: a thread adds
// its elements in index order, the wave sums by butterfly, the four wave sums are added as (w0 + w1) + (w2 + w3).
// A target outside [0, V) gives NaN (the callers check the ids first).
__global__ __launch_bounds__(256) void rarm_nll_kernel(const float* logits, int V, const long long* targets, float* nll_out) {
    __shared__ float red[8];
    const long long r = blockIdx.x;
    const int tid = threadIdx.x;
    const float* row = logits + r * V;
    int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);        // elements before the first 16-byte boundary
    if (head > V) head = V;
    const int nv = (V - head) >> 2, tail0 = head + nv * 4;
    const float4* rv = (const float4*)(row + head);
    float m = -INFINITY;
    for (int i = tid; i < nv; i += 256) { const float4 v = rv[i]; m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); }
    if (tid < head) m = fmaxf(m, row[tid]);
    if (tail0 + tid < V) m = fmaxf(m, row[tail0 + tid]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int i = tid; i < nv; i += 256) { const float4 v = rv[i]; s += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m)); }
    if (tid < head) s += expf(row[tid] - m);
    if (tail0 + tid < V) s += expf(row[tail0 + tid] - m);
    s = rarm_block_sum_fixed(s, red + 4, tid);
    if (tid == 0) {
        const long long tg = targets[r];
        nll_out[r] = (tg >= 0 && tg < V) ? (m + logf(s)) - row[tg] : NAN;
    }
}
hipError_t launch_rarm_nll(const float* logits, long long rows, int vocab, const long long* targets, float* nll_out, hipStream_t st) {
    if (rows < 1 || rows > 0x7fffffffLL || vocab < 1 || ((uintptr_t)logits & 7)) return hipErrorInvalidValue;
    rarm_nll_kernel<<<(unsigned)rows, 256, 0, st>>>(logits, vocab, targets, nll_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- gradient of the mean token NLL w.r.t. the logits
// dlogits[r, j] = gscale (softmax(logits[r])[j] - [j == target[r]]): the backward of F.cross_entropy in LatentImageRETRO.compute_loss
// (transformer.py:46-48; gscale = 1 / rows for its mean).  The maximum and the sum of exponentials are formed exactly as in
// rarm_nll_kernel (same loads, same order), so the optional nll_out is bit for bit that kernel's.  The third pass walks the row in pairs
// (V is even: 8-byte loads, 4-byte bf16x2 stores at any row): exp(x - max) / sum and the subtraction in fp32, one rounding to bf16.
// A target outside [0, V) gives NaN in the whole row.
__global__ __launch_bounds__(256) void rarm_nll_bwd_kernel(const float* logits, int V, const long long* targets, float gscale, bf16_t* dlogits, float* nll_out) {
    __shared__ float red[8];
    const long long r = blockIdx.x;
    const int tid = threadIdx.x;
    const float* row = logits + r * V;
    int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);
    if (head > V) head = V;
    const int nv = (V - head) >> 2, tail0 = head + nv * 4;
    const float4* rv = (const float4*)(row + head);
    float m = -INFINITY;
    for (int i = tid; i < nv; i += 256) { const float4 v = rv[i]; m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); }
    if (tid < head) m = fmaxf(m, row[tid]);
    if (tail0 + tid < V) m = fmaxf(m, row[tail0 + tid]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int i = tid; i < nv; i += 256) { const float4 v = rv[i]; s += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m)); }
    if (tid < head) s += expf(row[tid] - m);
    if (tail0 + tid < V) s += expf(row[tail0 + tid] - m);
    s = rarm_block_sum_fixed(s, red + 4, tid);
    const long long tg = targets[r];
    const bool ok = tg >= 0 && tg < V;
    if (tid == 0 && nll_out) nll_out[r] = ok ? (m + logf(s)) - row[tg] : NAN;
    const float inv = ok ? 1.f / s : NAN;
    const float2* rp = (const float2*)row;
    uint32_t* dp = (uint32_t*)(dlogits + r * V);
    const int tpair = ok ? (int)(tg >> 1) : -1;
    for (int i = tid; i < (V >> 1); i += 256) {
        const float2 v = rp[i];
        float p0 = expf(v.x - m) * inv, p1 = expf(v.y - m) * inv;
        if (i == tpair) { if (tg & 1) p1 -= 1.f; else p0 -= 1.f; }
        dp[i] = pack2bf(p0 * gscale, p1 * gscale);
    }
}
hipError_t launch_rarm_nll_bwd(const float* logits, long long rows, int vocab, const long long* targets, float gscale, bf16_t* dlogits, float* nll_out,
                               hipStream_t st) {
    if (rows < 1 || rows > 0x7fffffffLL || vocab < 2 || vocab % 2 || ((uintptr_t)logits & 7) || ((uintptr_t)dlogits & 3)) return hipErrorInvalidValue;
    rarm_nll_bwd_kernel<<<(unsigned)rows, 256, 0, st>>>(logits, vocab, targets, gscale, dlogits, nll_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- gradient of the token embedding
// dw[v, :] = sum over m with tokens[m] == v of dy[m, :] (the backward of nn.Embedding proj_in, attention.py:252): fp32 [V, C], every row
// written -- zero where no token has the id -- so the caller does not clear dw.  No atomics and a fixed order: a block owns VB consecutive
// ids and keeps their fp32 rows in LDS, each (row, column) touched by ONE thread; it walks the tokens in chunks of 2048, a thread looking
// at 8 consecutive ones, and adds the matching dy rows in ascending m (thread order through the waves' match masks, then the thread's
// own positions in order).  Almost every chunk has no token of the block's ids and costs one barrier.  Ids outside [0, V) match no row.
__global__ __launch_bounds__(256) void embedding_grad_kernel(const long long* __restrict__ tokens, const bf16_t* __restrict__ dy, int M, int C, int V, int VB,
                                                             float* __restrict__ dw) {
    extern __shared__ float eg_acc[];                       // [VB][C]
    __shared__ unsigned long long hit[4];
    __shared__ int found[256][8], nfound[256];
    const int tid = threadIdx.x, v0 = blockIdx.x * VB, nv = min(VB, V - v0);
    for (int i = tid; i < VB * C; i += 256) eg_acc[i] = 0.f;
    for (int m0 = 0; m0 < M; m0 += 2048) {
        int cnt = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int m = m0 + tid * 8 + e;
            if (m < M) {
                const long long d = tokens[m] - v0;
                if (d >= 0 && d < nv) found[tid][cnt++] = (e << 8) | (int)d;
            }
        }
        nfound[tid] = cnt;
        const unsigned long long mask = __ballot(cnt > 0);
        if (__syncthreads_or(cnt) == 0) continue;           // also orders the LDS clear before the first accumulation
        if ((tid & 63) == 0) hit[tid >> 6] = mask;
        __syncthreads();
        for (int w = 0; w < 4; w++) {
            unsigned long long left = hit[w];
            while (left) {
                const int t = w * 64 + __ffsll((long long)left) - 1;
                left &= left - 1;
                const int nf = nfound[t];
                for (int i = 0; i < nf; i++) {
                    const int f = found[t][i];
                    const int e = f >> 8, d = f & 255;
                    const bf16_t* src = dy + (long long)(m0 + t * 8 + e) * C;
                    for (int c = tid; c < C; c += 256) eg_acc[d * C + c] += bf2f(src[c]);
                }
            }
        }
        __syncthreads();                                    // found / nfound / hit are rewritten by the next chunk
    }
    __syncthreads();
    for (int i = tid; i < nv * C; i += 256) dw[(long long)v0 * C + i] = eg_acc[i];
}
static int embedding_grad_vb(int C) { int vb = 12288 / C; return vb > 16 ? 16 : vb; }      // <= 48 KB of fp32 rows per block
hipError_t launch_embedding_grad(const long long* tokens, const bf16_t* dy, int M, int C, int V, float* dw, hipStream_t st) {
    if (M < 1 || C < 1 || C > 12288 || V < 1) return hipErrorInvalidValue;
    const int VB = embedding_grad_vb(C);
    embedding_grad_kernel<<<(V + VB - 1) / VB, 256, (size_t)VB * C * sizeof(float), st>>>(tokens, dy, M, C, V, VB, dw);
    return hipGetLastError();
}

// One BLOCK of four waves per (head, sequence) (round 4; one wave before: its 2 x 8 chunk loops were 16 serialised round trips to
// the cache, 12.8 us at 256 cached rows -- four waves take every fourth 32-row chunk, and a wave's first K and V chunks are requested
// together before anything is computed).  Self-attention (attn1, causal): the new token's k / v rows are appended to the cache at
// position *pos and the query attends to rows 0..*pos.  Cross-attention (attn2): k_new == null, the cache holds the projected
// neighbours and all nkv rows are attended.  Phase 1: scores of the wave's chunks into LDS; block-wide maximum and sum; phase 2: the
// wave's chunks of sum_j p_j V[j][:], the four partial rows meet in LDS and are added in wave order.  CrossAttention.forward,
// attention.py:42-74.
// NW: waves per block = 32-row chunks in flight at once.  Eight waves (all 256 cached rows of a (head, sequence) requested in ONE round
// trip) measured SLOWER, round 5: 419 / 578 / 683 -> 406 / 552 / 644 img/s at 256 / 512 / 1024 sequences
// (profiles/r05e_rarm_attn_8wave_sweep.log) -- averaged over the 256 positions the launch is a fixed ~6.5 us + the cache bytes at ~5.5 TB/s
// already; the bigger blocks raise the fixed part (idle waves at short prefixes, wider barriers).  Four waves; the eight-wave path is removed.
template <int NW>
__global__ __launch_bounds__(64 * NW) void rarm_decode_attention_kernel(RarmAttnParams p) {
    // Eight lanes per cache row (16 bytes each), eight rows per load instruction: an instruction touches 8 cache lines.  (One lane
    // per key row -- 64 rows, 64 lines per instruction -- in the score phase and one 128-byte row per instruction in the value
    // phase made this launch 11.5 us of mostly address traffic.)
    constexpr int D = 64;
    __shared__ float sc[1024];
    __shared__ float red[2 * NW];
    __shared__ float part[NW][D];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int jr = lane >> 3, c8 = (lane & 7) * 8;
    const int t = p.pos ? *p.pos : 0;
    const int n = p.k_new ? t + 1 : p.nkv;
    const int nc = p.k_new ? t : n;                     // rows read from the cache by the value phase
    const long long hs = p.head_stride > 0 ? p.head_stride : D;
    bf16_t* Kc = p.Kc + (long long)b * p.batch_stride + h * hs;
    bf16_t* Vc = p.Vc + (long long)b * p.batch_stride + h * hs;
    const bf16_t* knew = p.k_new ? p.k_new + (long long)b * p.ldq + h * D : nullptr;
    const bf16_t* vnew = p.k_new ? p.v_new + (long long)b * p.ldq + h * D : nullptr;
    float qv[8];
    {
        const bf16x8 qq = *(const bf16x8*)(p.q + (long long)b * p.ldq + h * D + c8);
#pragma unroll
        for (int e = 0; e < 8; e++) qv[e] = bf2f((bf16_t)qq[e]) * p.scale;
    }
    if (p.k_new && w == 0 && jr == 0) {       // append the new row (read back from the projection output below, never through the cache)
        *(bf16x8*)(Kc + (long long)t * p.row_stride + c8) = *(const bf16x8*)(knew + c8);
        *(bf16x8*)(Vc + (long long)t * p.row_stride + c8) = *(const bf16x8*)(vnew + c8);
    }
    // ---- the wave's first chunk of keys AND values in one batch of requests (the values do not depend on the scores)
    bf16x8 kk[4], vv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int j = w * 32 + u * 8 + jr;
        const bf16_t* kr = (p.k_new && j == t) ? knew : Kc + (long long)(j < n ? j : 0) * p.row_stride;
        kk[u] = *(const bf16x8*)(kr + c8);
        vv[u] = *(const bf16x8*)(Vc + (long long)(j < nc ? j : 0) * p.row_stride + c8);
    }
    // ---- scores: rows j0 + 8 u + jr of chunks w, w + 4, ...
    float m = -INFINITY;
    for (int j0 = w * 32; j0 < n; j0 += 32 * NW) {
        if (j0 != w * 32) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + u * 8 + jr;
                const bf16_t* kr = (p.k_new && j == t) ? knew : Kc + (long long)(j < n ? j : 0) * p.row_stride;
                kk[u] = *(const bf16x8*)(kr + c8);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + u * 8 + jr;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) s += qv[e] * bf2f((bf16_t)kk[u][e]);
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
            if (j < n) { if ((lane & 7) == 0) sc[j] = s; m = fmaxf(m, s); }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red[w] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int u = 1; u < NW; u++) m = fmaxf(m, red[u]);
    float l = 0.f;
    for (int j = tid; j < n; j += 64 * NW) { const float e = __expf(sc[j] - m); sc[j] = e; l += e; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o);
    if (lane == 0) red[NW + w] = l;
    __syncthreads();
    l = (red[NW] + red[NW + 1]) + (red[NW + 2] + red[NW + 3]);
    if constexpr (NW == 8) l += (red[NW + 4] + red[NW + 5]) + (red[NW + 6] + red[NW + 7]);
    // ---- values: the wave's chunks of the cached rows
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j0 = w * 32; j0 < nc; j0 += 32 * NW) {
        if (j0 != w * 32) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + u * 8 + jr;
                vv[u] = *(const bf16x8*)(Vc + (long long)(j < nc ? j : 0) * p.row_stride + c8);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + u * 8 + jr;
            const float pj = j < nc ? sc[j] : 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += pj * bf2f((bf16_t)vv[u][e]);
        }
    }
    if (p.k_new && w == 0 && jr == 0) {                   // ... and the new token's row straight from the projection output
        const bf16x8 vn = *(const bf16x8*)(vnew + c8);
        const float pt = sc[t];
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] += pt * bf2f((bf16_t)vn[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; e++) { acc[e] += __shfl_xor(acc[e], 8); acc[e] += __shfl_xor(acc[e], 16); acc[e] += __shfl_xor(acc[e], 32); }
    if (jr == 0) {
#pragma unroll
        for (int e = 0; e < 8; e++) part[w][c8 + e] = acc[e];
    }
    __syncthreads();
    if (tid < D / 2) {                                    // fixed order over the waves: deterministic
        const int c = tid * 2;
        const float inv = 1.f / l;
        float o0 = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
        float o1 = (part[0][c + 1] + part[1][c + 1]) + (part[2][c + 1] + part[3][c + 1]);
        if constexpr (NW == 8) {
            o0 += (part[4][c] + part[5][c]) + (part[6][c] + part[7][c]);
            o1 += (part[4][c + 1] + part[5][c + 1]) + (part[6][c + 1] + part[7][c + 1]);
        }
        o0 *= inv; o1 *= inv;
        *(uint32_t*)(p.out + (long long)b * p.ldo + h * D + c) = pack2bf(o0, o1);
    }
}
// Cross-attention over <= 8 projected neighbours (the GEMM-form decode step of big batches, round 5): ONE block per sequence, a wave per
// head in turn (heads w, w + 4, ..): a wave instruction reads the head's eight 128-byte key rows (eight lanes per row), the eight partial dot
// products of a row meet by three lane exchanges, the softmax over the eight keys by three more, the values likewise -- the launch above
// spends a 256-thread block with two LDS exchanges on each of heads x sequences eight-key problems (17 us at 512 sequences).
__global__ __launch_bounds__(256) void rarm_fewkey_attention_kernel(RarmAttnParams p, int heads) {
    constexpr int D = 64;
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane >> 3, c8 = (lane & 7) * 8;
    const bool live = j < p.nkv;
    for (int h = w; h < heads; h += 4) {
        const bf16_t* Kr = p.Kc + (long long)b * p.batch_stride + (long long)(live ? j : 0) * p.row_stride + h * D + c8;
        const bf16_t* Vr = p.Vc + (long long)b * p.batch_stride + (long long)(live ? j : 0) * p.row_stride + h * D + c8;
        const bf16x8 qq = *(const bf16x8*)(p.q + (long long)b * p.ldq + h * D + c8);
        const bf16x8 kk = *(const bf16x8*)Kr, vv = *(const bf16x8*)Vr;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) s += bf2f((bf16_t)qq[e]) * p.scale * bf2f((bf16_t)kk[e]);
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
        s = live ? s : -INFINITY;
        float m = s;
        m = fmaxf(m, __shfl_xor(m, 8)); m = fmaxf(m, __shfl_xor(m, 16)); m = fmaxf(m, __shfl_xor(m, 32));
        const float e_ = live ? __expf(s - m) : 0.f;
        float l = e_;
        l += __shfl_xor(l, 8); l += __shfl_xor(l, 16); l += __shfl_xor(l, 32);
        const float pj = e_ / l;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            o[e] = pj * bf2f((bf16_t)vv[e]);
            o[e] += __shfl_xor(o[e], 8); o[e] += __shfl_xor(o[e], 16); o[e] += __shfl_xor(o[e], 32);
        }
        if (j == 0)
            *(uint4*)(p.out + (long long)b * p.ldo + h * D + c8) = make_uint4(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7]));
    }
}
hipError_t launch_rarm_decode_attention(const RarmAttnParams& p, int heads, int batch, hipStream_t st) {
    if (p.nkv > 1024) return hipErrorInvalidValue;
    if (!p.k_new && !p.pos && p.nkv >= 1 && p.nkv <= 8 && batch >= 128) {       // cross-attention over few keys at big batches
        rarm_fewkey_attention_kernel<<<batch, 256, 0, st>>>(p, heads);
        return hipGetLastError();
    }
    rarm_decode_attention_kernel<4><<<dim3(heads, batch), 256, 0, st>>>(p);
    return hipGetLastError();
}

// ---------------------------------------------------------------- decode-step cross-attention, one launch
// norm2 + to_q + attention over the k neighbours + to_out + residual (RetrievalPatchTransformer block, rdm/modules/attention.py:238)
// for ONE new token per sequence.  With the neighbours fixed for the whole sampling call, softmax(q K^T / sqrt d) V W_o^T is
// re-associated per sequence (rarm_exec.hip: rarm_prepare): scores = LN(x) G_b^T, out = P UT_b -- two matrix-vector products against 2 x
// heads*k x C bf16 per sequence instead of two C x C projections and an attention launch (3 launches of ~9 us each, all latency).
// One block per sequence: LayerNorm by block reduction (two-pass, rounded to bf16 as the GEMM operand was), a wave per group of
// score rows (coalesced 16-byte pieces, wave reduction), per-head softmax, then 4 output channels per thread over the heads*k rows.
// LayerNorm of ONE row spread one channel per thread over NW waves (two-pass, fp32), rounded to bf16: y[c] = (x - mean) rstd g[c] + b[c].
// red: >= 2 NW floats of LDS.  Every thread of the block must call it.
template <int NW>
__device__ __forceinline__ void rarm_emit_ln(float xv, bool live, int c, int C, const float* g, const float* bta, float eps, bf16_t* y, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float s = live ? xv : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __syncthreads();                                   // red may still be read by the caller's previous phase
    if (lane == 0) red[w] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < NW; i++) tot += red[i];
    const float mean = tot / C;
    const float d = live ? xv - mean : 0.f;
    float q = d * d;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if (lane == 0) red[NW + w] = q;
    __syncthreads();
    tot = 0.f;
#pragma unroll
    for (int i = 0; i < NW; i++) tot += red[NW + i];
    const float rstd = rsqrtf(tot / C + eps);
    if (live) y[c] = f2bf(d * rstd * g[c] + bta[c]);
}
__global__ __launch_bounds__(1024) void rarm_xattn_decode_kernel(RarmXattnParams p) {
    // 16 waves per sequence: the two matrix-vector products are one batch of loads each (every row of G / UT a thread needs is
    // requested before the first one is used) -- with 4 waves and batches of 4 - 8 rows the kernel was 15 dependent HBM round trips
    __shared__ float xn[1024];            // LayerNorm(x), C <= 1024
    __shared__ float sc[128];             // scores -> probabilities
    __shared__ float red[32];
    __shared__ __attribute__((aligned(16))) float part[4 * 1024];        // output partials [row group][C]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, C = p.C;
    float* xr = p.x + (long long)b * C;
    if (b >= p.Bc) {                      // zero neighbours: K = V = 0 -> the attention output is 0, to_out leaves its bias
        float xv = 0.f;
        if (tid < C) { xv = xr[tid] + p.bias[tid]; xr[tid] = xv; }
        if (p.ln3_out) rarm_emit_ln<16>(xv, tid < C, tid, C, p.ln3_g, p.ln3_b, p.ln_eps, p.ln3_out + (long long)b * C, red);
        return;
    }
    // ---- LayerNorm (one channel per thread)
    const float v = tid < C ? xr[tid] : 0.f;
    float s = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) red[w] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) tot += red[i];
    const float mean = tot / C;
    const float d = tid < C ? v - mean : 0.f;
    float q = d * d;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if (lane == 0) red[16 + w] = q;
    __syncthreads();
    tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) tot += red[16 + i];
    const float rstd = rsqrtf(tot / C + p.ln_eps);
    if (tid < C) xn[tid] = bf2f(f2bf(d * rstd * p.ln_g[tid] + p.ln_b[tid]));
    __syncthreads();
    // ---- scores: wave w takes rows w, w + 16, ... (<= 8 rows); a row = C/8 16-byte pieces over the lanes (two rounds)
    const int nrow = p.heads * p.k, npc = C >> 3;
    const bf16_t* Gb = p.G + (long long)b * p.NP * C;
    {
        bf16x8 g[8][2];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int j = w + 16 * u;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int pc = lane + 64 * h;
                g[u][h] = (j < nrow && pc < npc) ? *(const bf16x8*)(Gb + (long long)j * C + pc * 8) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int j = w + 16 * u;
            float a = 0.f;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int pc = lane + 64 * h;
                if (pc < npc) {
#pragma unroll
                    for (int e = 0; e < 8; e++) a += bf2f((bf16_t)g[u][h][e]) * xn[pc * 8 + e];
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
            if (lane == 0 && j < nrow) sc[j] = a;
        }
    }
    __syncthreads();
    // ---- softmax over each head's k columns
    float pr = 0.f;
    if (tid < nrow) {
        const int h0 = (tid / p.k) * p.k;
        float m = -INFINITY;
        for (int i = 0; i < p.k; i++) m = fmaxf(m, sc[h0 + i]);
        float sum = 0.f;
        for (int i = 0; i < p.k; i++) sum += __expf(sc[h0 + i] - m);
        pr = __expf(sc[tid] - m) / sum;
    }
    __syncthreads();
    if (tid < nrow) sc[tid] = pr;
    __syncthreads();
    // ---- output: thread = (4 channels, row group); NG = 4 row groups, each thread <= 32 rows, all requested at once
    const bf16_t* Ub = p.UT + (long long)b * p.NP * C;
    const int nc4 = C >> 2, c4 = tid % nc4, jg = tid / nc4;      // nc4 <= 256 -> at least 4 groups among the 1024 threads
    if (jg < 4) {
        uint2 u[32];
#pragma unroll
        for (int i = 0; i < 32; i++) { const int j = jg + 4 * i; u[i] = j < nrow ? *(const uint2*)(Ub + (long long)j * C + c4 * 4) : make_uint2(0u, 0u); }
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int j = jg + 4 * i;
            const float pj = j < nrow ? sc[j] : 0.f;
            a0 += pj * __uint_as_float(u[i].x << 16); a1 += pj * __uint_as_float(u[i].x & 0xffff0000u);
            a2 += pj * __uint_as_float(u[i].y << 16); a3 += pj * __uint_as_float(u[i].y & 0xffff0000u);
        }
        *(float4*)(part + jg * 1024 + c4 * 4) = make_float4(a0, a1, a2, a3);
    }
    __syncthreads();
    if (tid < nc4) {
        float4 xo = *(float4*)(xr + tid * 4);
        const float4 bb = *(const float4*)(p.bias + tid * 4);
        float4 acc = bb;
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) { const float4 t = *(const float4*)(part + g4 * 1024 + tid * 4); acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w; }
        xo.x += acc.x; xo.y += acc.y; xo.z += acc.z; xo.w += acc.w;
        *(float4*)(xr + tid * 4) = xo;
        if (p.ln3_out) *(float4*)(xn + tid * 4) = xo;          // the finished row, for norm3 below (xn is free: the scores are done)
    }
    if (p.ln3_out) {       // the block holds the finished row: norm3 of the feed-forward that follows leaves with it (bf16 GEMM operand)
        __syncthreads();
        rarm_emit_ln<16>(tid < C ? xn[tid] : 0.f, tid < C, tid, C, p.ln3_g, p.ln3_b, p.ln_eps, p.ln3_out + (long long)b * C, red);
    }
}
hipError_t launch_rarm_xattn_decode(const RarmXattnParams& p, hipStream_t st) {
    if (p.C % 8 || p.C > 1024 || p.heads * p.k > 128 || p.heads * p.k > p.NP || p.k < 1) return hipErrorInvalidValue;
    // (A four-blocks-per-sequence form -- a quarter of the heads per block, the partial rows handed over in global memory -- was
    // measured SLOWER than one block per sequence in round 6 (64 sequences 198.0 vs 199.4 img/s, 128: 284.5 vs 290.6;
    // profiles/r06_rarm_split_ab.log) and removed.)
    rarm_xattn_decode_kernel<<<p.B2, 1024, 0, st>>>(p);
    return hipGetLastError();
}

// ---------------------------------------------------------------- CFG + temperature + top-k filter + softmax + multinomial
// transformer.py:250-270.  One block per sequence: logits = l_u + s (l_c - l_u) (rows b and b + B of the doubled batch),
// / temperature, values below the k-th largest -> -inf (taming top_k_logits keeps ties with the k-th), softmax, then ONE draw by
// inverse CDF with the caller's uniform u in [0,1): the smallest index whose cumulative probability exceeds u * total, in
// vocabulary order (torch.multinomial's device-specific random stream has no cross-device definition; the uniform is an input
// so that the draw is reproducible and checkable).  The k-th largest value is found by a 32-round bit-wise threshold search on the
// order-preserving integer image of the floats (keys in registers).  Writes the token to out[b, *pos], to the next-step token buffer (both CFG
// halves), and — last block — advances *pos.
__device__ __forceinline__ uint32_t f2ord(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }


// NUCLEUS: the top-p filter after the top-k one (below).  COUNT: p.kept_out[b] receives the number of kept tokens.  Both are
// compile-time variants: rarm_sample_kernel<false, false>, the top_p == 1 path of every older entry, carries none of their code.
template <bool NUCLEUS, bool COUNT>
__global__ __launch_bounds__(256) void rarm_sample_kernel(RarmSampleParams p) {
    __shared__ uint32_t hist[256];
    __shared__ float red[256];
    __shared__ int chosen;
    const int b = blockIdx.x, tid = threadIdx.x, V = p.vocab;
    const int t = *p.pos;
    const float* lc = p.logits + (long long)b * V;
    const float* lu = p.cfg ? p.logits + (long long)(b + p.B) * V : nullptr;
    const float inv_t = 1.0f / p.temperature;
    auto logit_g = [&](int i) { const float c = lc[i]; return (lu ? lu[i] + p.scale * (c - lu[i]) : c) * inv_t; };
    // The guided, temperature-scaled logits are formed ONCE (coalesced reads) and kept in LDS: the select's four passes, the max,
    // the partial sums and the final scan had each gone back to global memory, the last two one strided / dependent element at a
    // time (117 us per step).  Element i lives at i + (i >> 6): a thread's contiguous 64-element chunk then spreads over the banks.
    extern __shared__ float lg[];
    for (int i0 = tid; i0 < V; i0 += 256 * 16) {              // sixteen independent (pairs of) loads in flight per thread
        float tmp[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { const int i = i0 + u * 256; tmp[u] = i < V ? logit_g(i) : 0.f; }
#pragma unroll
        for (int u = 0; u < 16; u++) { const int i = i0 + u * 256; if (i < V) lg[i + (i >> 6)] = tmp[u]; }
    }
    __syncthreads();
    auto logit = [&](int i) { return lg[i + (i >> 6)]; };
    // ---- the top_k-th largest value: bit-by-bit search for the largest threshold that at least top_k keys reach.  Keys (the
    // order-preserving integer image of the logits) sit in registers, a round is 64 compares per thread + one block-wide count:
    // 32 rounds.  (The 4-pass radix select it replaces spent its time in wave-aggregated LDS-atomic histogram updates: ~180 us.)
    const int remaining0 = p.top_k < V ? p.top_k : V;
    constexpr int KPT = 64;                                   // keys per thread: vocabularies up to 16 384; longer ones loop below
    uint32_t prefix = 0;
    [[maybe_unused]] uint32_t theta = 0;                      // NUCLEUS: order image of the smallest logit of the nucleus
    if (V <= 256 * KPT) {
        uint32_t key[KPT];
#pragma unroll
        for (int u = 0; u < KPT; u++) { const int i = tid + u * 256; key[u] = i < V ? f2ord(logit(i)) : 0u; }      // 0 is below every real key
        // TWO bits per round (round 4): a round is a block-wide count + one barrier whatever it counts, so three thresholds per round
        // (prefix | 01, 10, 11 at the bit pair) halve the 32 rounds; counts of 01 / 10 ride in one register (<= 4096 per wave each)
        for (int bit = 30; bit >= 0; bit -= 2) {
            const uint32_t c1 = prefix | (1u << bit), c2 = prefix | (2u << bit), c3 = prefix | (3u << bit);
            uint32_t n12 = 0, n3 = 0;
#pragma unroll
            for (int u = 0; u < KPT; u++) { n12 += (key[u] >= c1 ? 1u : 0u) + (key[u] >= c2 ? 0x10000u : 0u); n3 += key[u] >= c3 ? 1u : 0u; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { n12 += __shfl_xor(n12, o); n3 += __shfl_xor(n3, o); }
            const int slot = ((bit >> 1) & 1) * 8;                                       // two alternating slots: one barrier per round
            if ((tid & 63) == 0) { hist[slot + (tid >> 6) * 2] = n12; hist[slot + (tid >> 6) * 2 + 1] = n3; }
            __syncthreads();
            const uint32_t t12 = hist[slot] + hist[slot + 2] + hist[slot + 4] + hist[slot + 6];          // <= 16384 per field
            const int tot3 = (int)(hist[slot + 1] + hist[slot + 3] + hist[slot + 5] + hist[slot + 7]);
            const int tot1 = (int)(t12 & 0xffffu), tot2 = (int)(t12 >> 16);
            if (tot3 >= remaining0) prefix = c3; else if (tot2 >= remaining0) prefix = c2; else if (tot1 >= remaining0) prefix = c1;
        }
        if constexpr (NUCLEUS) {
            // ---- top-p among the top-k survivors K = {key >= prefix}: M(theta) = sum over K of exp(g - max) with key >= theta never grows
            // with theta, so the largest threshold whose mass still reaches top_p * M(k-th) is found by the same bit-wise search, a round
            // SUMMING the exponentials at or above the candidates where the top-k round counted keys.  The 64 exponentials sit in
            // registers beside the keys (0 for the tokens top-k dropped).  Every mass is added in one fixed order -- four chains of 16
            // per thread, (a0 + a1) + (a2 + a3), the wave butterfly, (w0 + w1) + (w2 + w3): 26 additions deep -- and dropping a term
            // only replaces it by 0, so the rounded M is still monotone and depends on neither the batch nor the launch.
            float ex[KPT];
            float m = -INFINITY;
#pragma unroll
            for (int u = 0; u < KPT; u++) { const int i = tid + u * 256; ex[u] = i < V ? logit(i) : -INFINITY; m = fmaxf(m, ex[u]); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if ((tid & 63) == 0) red[40 + (tid >> 6)] = m;
            __syncthreads();
            m = fmaxf(fmaxf(red[40], red[41]), fmaxf(red[42], red[43]));           // the arg-max always survives top-k: the max of K
#pragma unroll
            for (int u = 0; u < KPT; u++) ex[u] = key[u] >= prefix ? __expf(ex[u] - m) : 0.f;
            float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < KPT; u++) a[u & 3] += ex[u];
            const float need = p.top_p * rarm_block_sum_fixed((a[0] + a[1]) + (a[2] + a[3]), red + 32, tid);
            uint32_t th = 0;
            for (int bit = 30; bit >= 0; bit -= 2) {
                const uint32_t c1 = th | (1u << bit), c2 = th | (2u << bit), c3 = th | (3u << bit);
                float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, s3[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < KPT; u++) {
                    s1[u & 3] += key[u] >= c1 ? ex[u] : 0.f; s2[u & 3] += key[u] >= c2 ? ex[u] : 0.f; s3[u & 3] += key[u] >= c3 ? ex[u] : 0.f;
                }
                float m1 = (s1[0] + s1[1]) + (s1[2] + s1[3]), m2 = (s2[0] + s2[1]) + (s2[2] + s2[3]), m3 = (s3[0] + s3[1]) + (s3[2] + s3[3]);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { m1 += __shfl_xor(m1, o); m2 += __shfl_xor(m2, o); m3 += __shfl_xor(m3, o); }
                float* slot = red + ((bit >> 1) & 1) * 16;                                   // two alternating slots: one barrier per round
                if ((tid & 63) == 0) { slot[tid >> 6] = m1; slot[4 + (tid >> 6)] = m2; slot[8 + (tid >> 6)] = m3; }
                __syncthreads();
                m1 = (slot[0] + slot[1]) + (slot[2] + slot[3]); m2 = (slot[4] + slot[5]) + (slot[6] + slot[7]); m3 = (slot[8] + slot[9]) + (slot[10] + slot[11]);
                if (m3 >= need) th = c3; else if (m2 >= need) th = c2; else if (m1 >= need) th = c1;
            }
            theta = th;
        }
    } else {
        for (int bit = 31; bit >= 0; bit--) {
            const uint32_t cand = prefix | (1u << bit);
            int cnt = 0;
            for (int i = tid; i < V; i += 256) cnt += f2ord(logit(i)) >= cand ? 1 : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
            if ((tid & 63) == 0) hist[(bit & 1) * 4 + (tid >> 6)] = (uint32_t)cnt;
            __syncthreads();
            const int tot = (int)(hist[(bit & 1) * 4] + hist[(bit & 1) * 4 + 1] + hist[(bit & 1) * 4 + 2] + hist[(bit & 1) * 4 + 3]);
            if (tot >= remaining0) prefix = cand;
        }
        if constexpr (NUCLEUS) {          // the same search from LDS, one bit a round, the exponentials formed again every round: slow, as the loop above
            float m = -INFINITY;
            for (int i = tid; i < V; i += 256) m = fmaxf(m, logit(i));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if ((tid & 63) == 0) red[40 + (tid >> 6)] = m;
            __syncthreads();
            m = fmaxf(fmaxf(red[40], red[41]), fmaxf(red[42], red[43]));
            auto mass = [&](uint32_t cand, float* slot) {        // per thread: four chains over its strided elements, then the fixed reduction
                float a[4] = {0.f, 0.f, 0.f, 0.f};
                int j = 0;
                for (int i = tid; i < V; i += 256, j++) { const float v = logit(i); const uint32_t o = f2ord(v); a[j & 3] += (o >= prefix && o >= cand) ? __expf(v - m) : 0.f; }
                return rarm_block_sum_fixed((a[0] + a[1]) + (a[2] + a[3]), slot, tid);
            };
            const float need = p.top_p * mass(prefix, red + 32);
            uint32_t th = 0;
            for (int bit = 31; bit >= 0; bit--) {
                const uint32_t cand = th | (1u << bit);
                if (mass(cand, red + (bit & 1) * 16) >= need) th = cand;
            }
            theta = th;
        }
    }
    __syncthreads();
    const uint32_t kth = NUCLEUS ? (theta > prefix ? theta : prefix) : prefix;     // order image of the k-th largest logit (of the nucleus edge, if higher): keep o >= kth
    // ---- max, then per-thread partial sums over a CONTIGUOUS chunk (vocabulary order), block scan, locate the draw
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 256) { const float v = logit(i); if (f2ord(v) >= kth) mx = fmaxf(mx, v); }
    red[tid] = mx; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]); __syncthreads(); }
    mx = red[0]; __syncthreads();
    if constexpr (COUNT) {                                    // the kept-token count of the row (a read-out for callers and tests)
        if (p.kept_out) {
            int cnt = 0;
            for (int i = tid; i < V; i += 256) cnt += f2ord(logit(i)) >= kth ? 1 : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
            if ((tid & 63) == 0) hist[32 + (tid >> 6)] = (uint32_t)cnt;
            __syncthreads();
            if (tid == 0) p.kept_out[b] = (int)(hist[32] + hist[33] + hist[34] + hist[35]);
        }
    }
    const int chunk = (V + 255) / 256, i0 = tid * chunk, i1 = min(V, i0 + chunk);
    // (round 4) the three scans below add in EXACTLY the order they always did -- the draw is defined by it -- but no longer wait for one
    // LDS read / one exponential per addition: loads and exponentials are issued in batches of 16, the additions then run out of registers
    // (the serial forms were ~30 of the kernel's 77 us: 256 + 64 + 64 dependent LDS round trips)
    float part = 0.f;
    for (int i = i0; i < i1; i += 16) {
        float e[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { const float v = (i + u < i1) ? logit(i + u) : 0.f; e[u] = (i + u < i1 && f2ord(v) >= kth) ? __expf(v - mx) : -1.f; }
#pragma unroll
        for (int u = 0; u < 16; u++) if (e[u] >= 0.f) part += e[u];
    }
    red[tid] = part; __syncthreads();
    if (tid == 0) {
        float total = 0.f;
        for (int j = 0; j < 256; j += 16) {
            float r[16];
#pragma unroll
            for (int u = 0; u < 16; u++) r[u] = red[j + u];
#pragma unroll
            for (int u = 0; u < 16; u++) total += r[u];
        }
        const float target = p.uniforms[(long long)(t - p.pos0) * p.B + b] * total;
        float run = 0.f; int c = -1;
        for (int j = 0; j < 256; j += 16) {
            float r[16];
#pragma unroll
            for (int u = 0; u < 16; u++) r[u] = red[j + u];
#pragma unroll
            for (int u = 0; u < 16; u++) { const float nr = run + r[u]; if (c < 0) { if (nr > target) c = j + u; else run = nr; } }
        }
        if (c < 0) c = 255;
        // (if rounding pushed the target past the total, fall into the last non-empty chunk)
        while (c > 0 && red[c] == 0.f) c--;
        chosen = c; red[0] = run; red[1] = target;
    }
    __syncthreads();
    if (tid == chosen) {
        float run = red[0]; const float target = red[1];
        int pick = -1, last = -1;
        for (int i = i0; i < i1 && pick < 0; i += 16) {
            float e[16];
#pragma unroll
            for (int u = 0; u < 16; u++) { const float v = (i + u < i1) ? logit(i + u) : 0.f; e[u] = (i + u < i1 && f2ord(v) >= kth) ? __expf(v - mx) : -1.f; }
#pragma unroll
            for (int u = 0; u < 16; u++) {
                if (e[u] >= 0.f && pick < 0) { last = i + u; run += e[u]; if (run > target) pick = i + u; }
            }
        }
        if (pick < 0) pick = last;
        p.tokens_out[(long long)b * p.steps + (t - p.pos0)] = pick;
        p.next_tokens[b] = pick;
        if (p.cfg) p.next_tokens[b + p.B] = pick;
        __threadfence();
        if (atomicAdd(p.done, 1) == p.B - 1) { *p.done = 0; *p.pos = t + 1; }     // last sequence of the step advances the clock
    }
}
hipError_t launch_rarm_sample(const RarmSampleParams& p, hipStream_t st) {
    const size_t sm = ((size_t)p.vocab + (p.vocab >> 6) + 64) * sizeof(float);
    if (sm > 150 * 1024) return hipErrorInvalidValue;          // vocabulary beyond ~37 k entries: not an RARM configuration
    if (!(p.top_p > 0.f && p.top_p <= 1.f)) return hipErrorInvalidValue;
    // top_p == 1 is the kernel without a nucleus (a nucleus of mass 1 would not be the same thing: in fp32 the tail's mass can round away)
    const int which = p.top_p < 1.f ? 2 : (p.kept_out ? 1 : 0);
    void (*const kern[3])(RarmSampleParams) = {rarm_sample_kernel<false, false>, rarm_sample_kernel<false, true>, rarm_sample_kernel<true, true>};
    static bool attr_dev[RDM_MAX_DEVICES][3] = {};
    bool& attr = attr_dev[rdm_cur_device()][which];
    if (!attr && sm > 32 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern[which], hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        if (e != hipSuccess) return e;
        attr = true;
    }
    kern[which]<<<p.B, 256, sm, st>>>(p);
    return hipGetLastError();
}

// ---------------------------------------------------------------- VQGAN codebook lookup (taming VectorQuantizer2.get_codebook_entry)
// indices [B*HW] -> bf16 token-major [B*HW, E] (== NHWC), the layout post_quant_conv (1x1) reads as a GEMM operand
__global__ __launch_bounds__(256) void codebook_gather_kernel(const long long* idx, const float* codebook, int n_embed, int E, long long n,
                                                              bf16_t* out) {
    const long long total = n * E;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / E; const int c = (int)(i - r * E);
        long long id = idx[r]; if (id < 0 || id >= n_embed) id = 0;
        out[i] = f2bf(codebook[id * E + c]);
    }
}
hipError_t launch_codebook_gather(const long long* idx, const float* codebook, int n_embed, int E, long long n, bf16_t* out, hipStream_t st) {
    const long long total = n * E;
    int grid = (int)((total + 255) / 256); if (grid > 4096) grid = 4096; if (grid < 1) grid = 1;
    codebook_gather_kernel<<<grid, 256, 0, st>>>(idx, codebook, n_embed, E, n, out);
    return hipGetLastError();
}
// f32 [rows, C] += nothing; bf16 copy of the fp32 residual stream for the logits GEMM is launch_cast_f32_bf16 (misc.hip)
__global__ void set_int_kernel(int* p, int v) { *p = v; }
hipError_t launch_set_int(int* p, int v, hipStream_t st) { set_int_kernel<<<1, 1, 0, st>>>(p, v); return hipGetLastError(); }
