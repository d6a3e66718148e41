// Internal kernel-launch interface of librdm_hip (host side). All launches are asynchronous on `st`.
#pragma once
#include "common.h"
#include "../../include/rdm_hip.h"

struct GnParams {
    const bf16_t* x0; const bf16_t* x1;   // [B, HW, C0], [B, HW, C1] (x1 may be null)
    int C0, C1, HW, B, groups;
    int L0, L1;                           // logical channels of x0 / x1 (<= C0 / C1: the tails are zero padding, build_unet); 0 = C0 / C1
    int nchunk;                           // pixel chunks per sample
    float* partial;                       // [B, nchunk, groups, 2] (sum, sumsq)
    const float* gamma; const float* beta;
    float eps; int silu;
    bf16_t* out;                          // [B, HW, C0+C1]
    int x1_bmod;                          // > 0: x1 holds only x1_bmod samples and sample b reads b % x1_bmod (a shared-prefix skip tensor whose second half was never materialised)
    int x0_bmod;                          // the same for x0 (round 5: the activation leaving the shared guidance prefix is not duplicated either)
};

hipError_t launch_gn_stats(GnParams p, hipStream_t st);          // the statistics pass alone (p.partial), for consumers that apply the norm themselves

// GroupNorm-apply + SiLU + 3x3 conv to a few output channels in one kernel (the UNet's `out` head, the VQ decoder's conv_out)
struct HeadParams {
    const bf16_t* x; int B, H, W, C;                  // NHWC bf16, raw (pre-norm) when partial is given
    const float* partial; int nchunk, groups;         // GroupNorm statistics from launch_gn_stats ([B][nchunk][groups][2]) or null: x is used as is
    const float* gamma; const float* beta; float eps;
    const float* w;                                   // [Cout][C][3][3] fp32
    bf16_t* wp;                                       // scratch for the packed weights: head_conv_wp_bytes(C)
    const float* bias; float* out; int Cout;          // out NCHW fp32
};
size_t head_conv_wp_bytes(int C);
bool head_conv_supported(const HeadParams& p);
hipError_t launch_head_conv(const HeadParams& p, hipStream_t st);

struct FlashParams {
    const bf16_t* q; int ldq;        // q[(b*n + i)*ldq + h*32 + d]
    const bf16_t* k; int ldk;        // k[(b*n + j)*ldk + h*32 + d]
    const bf16_t* vt;                // vt[((b*C) + h*32 + d)*n + j]   (V transposed per sample), or null with:
    const bf16_t* v; int ldv;        // v[(b*n + j)*ldv + h*32 + d]     (token-major V, n % 64 == 0 only: read through ds_read_b64_tr_b16)
    bf16_t* out; int ldo;            // out[(b*n + i)*ldo + h*32 + d]
    int n, C;                        // tokens, channels (= heads*32)
    float scale_log2e;               // d^-0.5 * log2(e)
};

// cross-attention over k retrieved neighbours in the re-associated form (unet_exec.hip: unet_compute_xattn): per sample b
//   out = softmax_groups(x G_b^T) U_b^T + bias + res      x [rows][C], G_b [NP][C], U_b [C][NP]  (all bf16, row-major)
struct XattnParams {
    const bf16_t* x; const bf16_t* G; const bf16_t* U;
    const float* bias; const bf16_t* res; bf16_t* out;
    int rows, n, C, NP;              // rows = samples * n (n rows per sample, n % 32 == 0); NP = row count of G (128)
    int ncols, group;                // heads * k used score columns; softmax over groups of `group` (1, 2, 4) adjacent columns
    const float* ln_g; const float* ln_b; float ln_eps;   // given: x holds the RAW rows, the scores are taken on LayerNorm(x) and the residual is x itself (res unused)
    // LN-fused form only: out may alias x (a block reads its 32 rows before it writes them); ln3_out given: LayerNorm(out rows; ln3_g,
    // ln3_b, ln_eps) -- norm3 of BasicTransformerBlock (attention.py:239) -- leaves with the finished tile as the next GEMM's operand
    const float* ln3_g; const float* ln3_b; bf16_t* ln3_out;
    // neighbour bias (rdm_hip.h: rdm_set_neighbour_bias): fp32 [samples][group], added to every head's score of neighbour j of the block's
    // sample before the group softmax; -inf removes the neighbour.  Null: the unbiased instantiations run (the bias is a template parameter)
    const float* key_bias;
};
bool xattn_fused_supported(const XattnParams& p);
hipError_t launch_xattn_fused(const XattnParams& p, hipStream_t st);        // G / U: FRAGMENT-ORDERED images, written by:
hipError_t launch_xattn_pack(const bf16_t* G, const bf16_t* U, bf16_t* Gp, bf16_t* Up, int B, int NP, int C, hipStream_t st);

struct SmallAttnParams {
    const bf16_t* q; int ldq;        // q[(b*nq + i)*ldq + h*D + d]
    const bf16_t* k; int ldk; const bf16_t* v; int ldv;   // k[(b*nkv + j)*ldk + h*D + d]
    bf16_t* out; int ldo;
    int nq, nkv, causal;
    float scale;
    const float* key_bias;           // optional fp32 [B][nkv], added to every head's scaled score of key j; -inf keys are skipped (not with causal)
};

// causal self-attention over all query positions, d_head = 64 (attention.hip: causal_d64_kernel); q | k | v are the thirds of the fused
// projection output, head h in columns h*64 .. h*64+63 of each third
struct CausalD64Params {
    const bf16_t* qkv; int ldq;      // q[(b*n + i)*ldq + h*64 + d], k at + C, v at + 2C  (C = heads*64)
    bf16_t* out; int ldo;            // out[(b*n + i)*ldo + h*64 + d]
    int n, C;                        // tokens per sequence (any 1 <= n <= 1024), channels
    float scale_log2e;               // scale * log2(e)
    bf16_t* kcache; bf16_t* vcache;  // optional (both or neither): head-major decode caches [B][heads][L][64]; rows 0 .. n-1 receive the K / V columns of qkv
    int L;
};

// streaming single-head attention of the first stage's AttnBlock (vq_attn.hip): out[b] = softmax(q[b] k[b]^T scale) v[b] + bias
struct VqAttnParams {
    const bf16_t* q; int ldq;        // q[(b*n + i)*ldq + d]   (row strides in elements, multiples of 8)
    const bf16_t* k; int ldk;        // k[(b*n + j)*ldk + d]
    const bf16_t* v; int ldv;        // v[(b*n + j)*ldv + d]   (token-major)
    const float* bias;               // [C] added after P.V (rows of P sum to 1), or null
    bf16_t* out; int ldo;            // out[(b*n + i)*ldo + d]  (ldo a multiple of 4)
    int n, C;                        // tokens per sample (any n >= 1), channels (a multiple of 128, <= 512)
    float scale;
};

struct DdimStepParams {
    const float* x; const float* eps; const float* noise;   // noise may be null (eta == 0)
    float* x_prev; float* pred_x0;                           // pred_x0 may be null
    float* x_dup;                                            // second copy of x_prev (the CFG-doubled batch) or null
    long long n_per_batch;                                   // B*C*H*W
    float a_t, a_prev, sigma_t, sqrt_one_minus_at, scale, temperature;
    int cfg;
};

// One PLMS step (ldm PLMSSampler.p_sample_plms, eta = 0).  mode PLMS_STEP: e_t = CFG(eps) -> e_store, e' from `order` history
// tensors (h1 = o[-1], h2 = o[-2], h3 = o[-3]; e_store may alias h3: each element is read before it is written), x_out = update(x, e').
// mode PLMS_EULER_A (first step, before the t_next forward): e_t -> e_store, x_out = update(x, e_t) (x_tmp; no pred_x0).
// mode PLMS_EULER_B (after it): e' = (e_prev + CFG(eps)) / 2, x_out = update(x, e').  x_dup: second half of the CFG-doubled batch or null.
enum { PLMS_STEP = 0, PLMS_EULER_A = 1, PLMS_EULER_B = 2 };
struct PlmsStepParams {
    const float* x; const float* eps;                        // eps: [n] rows (scale == 1) or [2n] (cond | uncond)
    const float* e_prev;                                     // PLMS_EULER_B: the step's stored e_t
    const float* h1; const float* h2; const float* h3;       // PLMS_STEP history (order of them are read)
    float* e_store; float* x_out; float* x_dup; float* pred_x0;
    long long n;                                             // B*C*H*W
    float a_t, a_prev, sqrt_one_minus_at, scale;
    int cfg, mode, order;
};

// One DPM-Solver++ step, ODE or SDE (Lu et al. 2022, multistep data prediction, "dpmsolver++" / "sde-dpmsolver++"; ldm
// models/diffusion/dpm_solver): e = CFG(eps), m0 = (x - sqrt_one_minus_a_s e) / sqrt_a_s -> m_store, pred_x0;
// x_out = ((c_x x + c_0 m0) + c_1 m_prev) + c_n z.  The host flattens the solver's D = (1 + 1/(2r)) m0 - (1/(2r)) m_prev into c_0, c_1
// (first-order step: m_prev null, c_1 unused).  noise null: the ODE step, no fourth term (c_n unused); else z = noise[i] (the stack form),
// or the normal of StepRngParams drawn in registers (the seeded launch: noise unused).  m_store may be the very slot m_prev points to:
// each thread reads its elements of m_prev before it writes m_store, so ONE history slot serves the whole loop.
struct DpmppStepParams {
    const float* x; const float* eps;                        // eps: [n] rows (cfg == 0) or [2n] (cond | uncond)
    const float* m_prev;                                     // the previous step's m0, or null
    const float* noise;                                      // z_j, n elements (SDE stack form), or null
    float* x_out; float* x_dup; float* m_store; float* pred_x0;     // x_dup, m_store, pred_x0 may be null
    long long n;                                             // B*C*H*W
    float sqrt_a_s, sqrt_one_minus_a_s, scale, c_x, c_0, c_1, c_n;
    int cfg;
};

// One UniPC pass (Zhao et al. 2023, data prediction, multistep), run after the forward at node j: e = CFG(eps), m = (u - sigma e) / alpha
// -> m_store, pred_x0; the correction of the kept iterate xc = a_x xc_prev + a_t m + a_1 h1 + a_2 h2 + a_3 h3 with order_c history terms
// (order_c == 0: xc = u, xc_prev unused) -> xc_out; the prediction u_next = b_x xc + b_0 m + b_1 h1 + b_2 h2 with order_p - 1 history
// terms -> u_next, x_dup.  h1, h2, h3 = m_{j-1}, m_{j-2}, m_{j-3}; a slot the pass does not read is null.  Every input element is read
// before any output element is written, by the same thread: u_next may be u, xc_out may be xc_prev, m_store may be h3 (or any slot).
struct UnipcStepParams {
    const float* u; const float* eps;                        // eps: [n] rows (cfg == 0) or [2n] (cond | uncond)
    const float* xc_prev; const float* h1; const float* h2; const float* h3;
    float* xc_out; float* u_next; float* x_dup; float* m_store; float* pred_x0;     // all but u_next may be null
    long long n;                                             // B*C*H*W
    float alpha, sigma, scale, a_x, a_t, a_1, a_2, a_3, b_x, b_0, b_1, b_2;
    int cfg, order_c, order_p;                               // order_c 0..3, order_p 1..3
};

// One step of deterministic DDIM inversion (rdm_ddim_encode), from the level whose sqrt(alpha), sqrt(1 - alpha) are sa_c, s1m_c UP to the
// level of sa_n, s1m_n: e = CFG(eps), pred_x0 = (x - s1m_c e) / sa_c, x_out = sa_n pred_x0 + s1m_n e.  The four scalars are the host's
// float64 values rounded to fp32.  x_out may be x: a thread reads its elements of x before it writes them.
struct DdimInverseStepParams {
    const float* x; const float* eps;                        // eps: [n] rows (cfg == 0) or [2n] (cond | uncond)
    float* x_out; float* x_dup; float* pred_x0;              // x_dup, pred_x0 may be null
    long long n;                                             // B*C*H*W
    float sa_c, s1m_c, sa_n, s1m_n, scale;
    int cfg;
};

// The forward process with the noise generated in registers (rdm_op_q_sample_seeded): out = sqrt_a x0 + sqrt_1ma z, z the normals of
// (seed, stream 0, step 0, row0 + b) -- a seeded sampling call's starting latent.  rows x per_row elements, per_row % 4 == 0.
struct QSampleSeededParams {
    const float* x0; float* out; unsigned long long seed; long long rows, per_row; uint32_t row0; float sqrt_a, sqrt_1ma;
};

struct DdpmStepParams {
    const float* x; const float* eps; const float* noise; float* x_prev; long long n;
    float sqrt_recip, sqrt_recipm1, coef1, coef2, log_var; int clip, nonzero; float temperature;
};

// Device noise (philox.h).  StepRngParams: what a seeded step kernel adds to the step's own parameters -- the noise of element e of row b
// is the normal of (seed, stream 1, step, row0 + b, e), per_row = C*H*W elements per sample row.  RngFillParams: rows x per_row words or
// normals of one (step, stream) into out.
struct StepRngParams { unsigned long long seed; long long per_row; uint32_t row0, step; };
struct RngFillParams { unsigned long long seed; long long rows, per_row; uint32_t row0, step, stream; uint32_t* out; };

// The inpainting blend of the DDIM loop (rdm_op_masked_blend, rdm_ddim_inpaint; ldm's img_orig * mask + (1 - mask) * img with
// img_orig = q_sample(x0, t)): out = (sqrt_a x0 + sqrt_1ma z) m + (1 - m) x over [B, C, H, W], m = mask [B, mask_channels, H, W] with
// mask_channels 1 (one plane for every channel) or C; 1 keeps the known latent x0.  The two scalars are the host's float64 square roots
// rounded to fp32.  z: the known region's noise, read from memory (null: zeros) -- the seeded kernel draws it instead, the normals of
// (seed, stream 0, StepRngParams::step, row0 + b).  out may be x: a thread reads its elements of x before it writes them.
struct MaskedBlendParams {
    const float* x; const float* x0; const float* mask; const float* z;
    float* out; float* x_dup;                                // x_dup: second copy of out (the CFG-doubled batch) or null
    long long n, chw, hw;                                    // B*C*H*W, C*H*W, H*W
    int mask_channels;                                       // 1 | C
    int mask_vec;                                            // the seeded kernel: hw % 4 == 0 and mask 16-byte aligned, so a block's four elements share one mask quad
    float sqrt_a, sqrt_1ma;
};

// RARM decode step (rarm.hip)
struct RarmAttnParams {
    const bf16_t* q; int ldq;                 // q[b*ldq + h*64 + d]; k_new / v_new share ldq (one fused qkv row per sequence)
    const bf16_t* k_new; const bf16_t* v_new; // self-attention: the new token's rows (appended to the cache at *pos); null for cross-attention
    bf16_t* Kc; bf16_t* Vc;                   // cache [B][rows][row_stride]
    long long batch_stride; int row_stride;
    long long head_stride;                    // elements between the heads of a cache row set: 0 / 64 = heads side by side inside a row (row_stride = C); rows * 64 = head-major [B][head][rows][64] (row_stride = 64)
    int nkv;                                  // cross-attention: rows to attend; self-attention: capacity (<= 1024)
    const int* pos;                           // device step counter (self-attention attends rows 0..*pos)
    float scale; bf16_t* out; int ldo;
};
// decode-step cross-attention over the k neighbours with the per-sequence operands re-associated once per sampling call (as the UNet's
// xattn kernels): x += softmax_heads(LN(x) G_b^T) UT_b + bias for sequences b < Bc; x += bias for the others (zero neighbours)
struct RarmXattnParams {
    float* x;                                  // [B2][C] fp32 residual stream, updated in place
    const float* ln_g; const float* ln_b; float ln_eps;
    const bf16_t* G; const bf16_t* UT;         // [Bc][NP][C] each: G row h*k + j = scale * (key j restricted to head h) W_q;  UT row h*k + j = W_o (value j restricted to head h)
    const float* bias;                         // [C]
    int B2, Bc, C, NP, heads, k;
    const float* ln3_g; const float* ln3_b; bf16_t* ln3_out;   // given: LayerNorm (gamma, beta) of the FINISHED rows leaves with them as bf16 [B2][C] (norm3: the operand of the feed-forward's first GEMM)
};
hipError_t launch_rarm_xattn_decode(const RarmXattnParams& p, hipStream_t st);

struct RarmSampleParams {
    const float* logits; int vocab; int B; int cfg; float scale, temperature; int top_k;
    const float* uniforms;                    // [steps][B], row = *pos - pos0
    int* pos; int pos0; int steps;            // tokens_out[b*steps + (*pos - pos0)]
    long long* tokens_out; long long* next_tokens; int* done;
    float top_p = 1.0f;                       // in (0, 1]; < 1: nucleus filter among the top-k survivors (the nucleus instantiation)
    int* kept_out = nullptr;                  // optional [B]: tokens each row kept
};
hipError_t launch_rarm_embed(const long long* tokens, const float* emb, const float* pos_t, const int* pos, float* x, int B, int C,
                             int vocab, hipStream_t st);
hipError_t launch_rarm_decode_attention(const RarmAttnParams& p, int heads, int batch, hipStream_t st);
hipError_t launch_rarm_sample(const RarmSampleParams& p, hipStream_t st);
// whole-sequence pass (rarm.hip): row r of x is position r % t of sequence r / t, whose tokens are row (seq0 + r / t) % tok_rows of tokens [tok_rows][tok_ld]
hipError_t launch_rarm_embed_seq(const long long* tokens, int tok_ld, int tok_rows, int seq0, const float* emb, const float* pos_t, float* x, long long rows,
                                 int t, int C, int vocab, hipStream_t st);
hipError_t launch_rarm_nll(const float* logits, long long rows, int vocab, const long long* targets, float* nll_out, hipStream_t st);
// training (rarm.hip): gradient of the mean NLL w.r.t. the logits (bf16; nll_out optional, bitwise launch_rarm_nll's), gradient of the token embedding
hipError_t launch_rarm_nll_bwd(const float* logits, long long rows, int vocab, const long long* targets, float gscale, bf16_t* dlogits, float* nll_out,
                               hipStream_t st);
hipError_t launch_embedding_grad(const long long* tokens, const bf16_t* dy, int M, int C, int V, float* dw, hipStream_t st);
hipError_t launch_codebook_gather(const long long* idx, const float* codebook, int n_embed, int E, long long n, bf16_t* out, hipStream_t st);
hipError_t launch_set_int(int* p, int v, hipStream_t st);

// skinny GEMM, M <= 128 rows (sgemm.hip): out[M, N(/2 for GEGLU)] = act(A W^T + bias) (+ res)
struct SgemmParams {
    const bf16_t* A; int lda; const bf16_t* W; int M, N, K;     // W [N][K]; GEGLU: N = 2 x outputs, rows interleaved in blocks of 32
    const float* bias; int act; const float* res_f32; const bf16_t* res_bf16; float* out_f32; bf16_t* out_bf16; int ldo;
    const float* ln_x; const float* ln_g; const float* ln_b; float ln_eps;      // A = LayerNorm(ln_x [M][K] fp32) formed in the kernel (A ignored)
    int fixed_split;          // deterministic mode (rdm_set_deterministic): a row's fp32 summation order must not follow the batch -- always the four-wave K split
                              // (K / 4 per wave, partial tiles added in wave order), never the eight-wave / folded / LayerNorm-in-tile forms that start at 384 rows
};
bool sgemm_supported(const SgemmParams& p);
// the sgemm_kernel<MA, NB, GEGLU, U, LN, NW> instantiation launch_sgemm runs for a supported p (host only: reads M, N, K, act, ln_x, fixed_split)
struct SgemmForm { int ma, nb, u, nw, ln, geglu; };
SgemmForm sgemm_form(const SgemmParams& p);
bool sgemm_form_compiled(const SgemmForm& f);
hipError_t launch_sgemm(const SgemmParams& p, hipStream_t st);
// mid-size GEMM (mgemm.hip): one-row-per-sequence operands at 1024+ rows, LDS-staged BM x 64 tiles, fp32 / bf16 residual and output
bool mgemm_supported(const SgemmParams& p);
hipError_t launch_mgemm(const SgemmParams& p, hipStream_t st);
hipError_t launch_igemm(const IgemmParams& p, bool conv, int batch, hipStream_t st);
// 3x3 conv (conv_halo.hip): the one statement of which kernel takes a conv -- geometry and epilogue only, not whether p.Wfrag exists
enum ConvKernel { CONV_IGEMM, CONV_HALO4, CONV_HALO4_STRIP };     // igemm.hip | conv_halo4.hip | its 64-column strip form (output wider than 64 pixels)
ConvKernel conv3x3_kernel(const IgemmParams& p);
int conv_halo_ksplit(const IgemmParams& p);                // K-split factor worth using for this conv (1 = none, and always unless CONV_HALO4); needs p.ws of ksplit*M*N floats
// launches conv3x3_kernel's choice when p.Wfrag (the fragment-ordered weight copy) is given, plus the K-split finisher when p.ksplit > 1; without p.Wfrag the implicit GEMM
hipError_t launch_conv3x3(const IgemmParams& p, hipStream_t st);
hipError_t launch_conv_halo4(const IgemmParams& p, bool strip, hipStream_t st);      // conv_halo4.hip; launch_conv3x3 is its caller
// one-wave-per-SIMD linear GEMM (lin4.hip): needs p.Wfrag = the fragment-ordered copy of W built by launch_lin_w_fragpack
bool lin4_supported(const IgemmParams& p, int batch);
hipError_t launch_lin4(const IgemmParams& p, hipStream_t st);
hipError_t launch_lin_w_fragpack(const bf16_t* W, bf16_t* dst, int N, int K, int ldw, int geglu, hipStream_t st, const float* gamma = nullptr);       // dst: N*K elements; geglu: W rows in packing.py's _geglu_perm order; gamma: dst = bf16(gamma[k] W[n][k]) (LayerNorm fold)
hipError_t launch_lin_ln_sb(const bf16_t* W, const float* gamma, const float* beta, const float* bias, float* sb, int N, int K, hipStream_t st);   // sb[n] = (sum_k bf16(gamma W), bias + sum_k beta W), n = stored row
hipError_t launch_conv_w_fragpack(const bf16_t* W, bf16_t* dst, int N, int Cin, hipStream_t st);   // dst: N*9*Cin elements
hipError_t launch_conv_phase_weights(const bf16_t* W, bf16_t* Wp, int N, int C, hipStream_t st);     // igemm.hip: [N][3][3][C] -> [4 phases][N][2][2][C]
// ---- backward pieces (backward.hip)
hipError_t launch_conv_w_dgrad(const bf16_t* w, bf16_t* wd, int N, int C, hipStream_t st);             // [N][9][C] -> flipped [C][9][N]
size_t conv_wgrad_scratch_bytes(int B, int H, int W, int C, int N, int* WP, int* PR, int* Kc, int* Z, int* margin);
hipError_t launch_conv_wgrad(const bf16_t* x, const bf16_t* dy, float* dw, int B, int H, int W, int C, int N, char* scratch, const void* zero_page,
                             hipStream_t st);
hipError_t launch_reduce_planes(const float* parts, float* out, long long n, int Z, hipStream_t st);
hipError_t launch_add_bf16(const bf16_t* a, const bf16_t* b, bf16_t* out, long long n, hipStream_t st);
// GEGLU on an unpermuted pre-activation [M, 2F] ([x | gate]): dh null -> out [M, F] = x gelu(gate); else out [M, 2F] = [dx | dgate]
hipError_t launch_geglu(const bf16_t* pre, const bf16_t* dh, bf16_t* out, long long M, int F, hipStream_t st);
hipError_t launch_colsum(const bf16_t* x, float* out, long long M, int N, hipStream_t st, float* scratch = nullptr);     // scratch: colsum_scratch_bytes(M, N)
size_t colsum_scratch_bytes(long long M, int N);
// dW [N][K] fp32 = dy^T a for dy [M, N], a [M, K] bf16 (Linear weight gradient): K-split over the M rows, fp32 planes summed in fixed order
size_t linear_wgrad_scratch_bytes(long long M, int N, int K);
// wgrad.hip: dW = dY^T X read in the activation layout (no transposes), taps = 1 (linear) or 9 (conv3x3 over [B][H][W] images)
bool wgrad_tn_supported(long long M, int N, int K, int lda, int ldb);
bool conv_wgrad_tn_supported(int B, int H, int W, int C, int N);
size_t wgrad_tn_scratch_bytes(long long M, int N, int K, int taps);
size_t conv_wgrad_tn_scratch_bytes(int B, int H, int W, int C, int N);
// which kernel takes a weight gradient and its split (wgrad.hip): the public rdm_wgrad_form of rdm_hip.h (path = RDM_WGRAD_*, Z planes of per_plane
// chunks / rows / K' positions each, remap); *_args_ok: the shapes rdm_op_conv3x3_wgrad / rdm_op_linear_wgrad and rdm_wgrad_select accept
bool conv_wgrad_args_ok(int B, int H, int W, int C, int N);
bool linear_wgrad_args_ok(long long M, int N, int K);
rdm_wgrad_form conv_wgrad_plan(int B, int H, int W, int C, int N);
rdm_wgrad_form linear_wgrad_plan(long long M, int N, int K);
void linear_wgrad_geom(long long M, int* Z, long long* Kc);
hipError_t launch_wgrad_tn(const bf16_t* dy, const bf16_t* x, float* dw, long long M, int N, int K, int taps, int H, int W, char* scratch,
                           const void* zero_page, hipStream_t st);
hipError_t launch_linear_wgrad(const bf16_t* dy, const bf16_t* a, float* dw, long long M, int N, int K, char* scratch, const void* zero_page, hipStream_t st);
size_t groupnorm_bwd_scratch_bytes(int B, int HW, int C, int groups);
hipError_t launch_groupnorm_bwd(const bf16_t* x, const bf16_t* dy, const float* gamma, const float* beta, int B, int HW, int C, int groups,
                                float eps, int silu, float* scratch, bf16_t* dx, float* dgamma, float* dbeta, hipStream_t st, const bf16_t* residual = nullptr);    // residual: dx = gradient + residual
hipError_t launch_layernorm_bwd(const bf16_t* x, const bf16_t* dy, const float* gamma, int M, int C, float eps, float* scratch, int* nb_out,
                                bf16_t* dx, float* dgamma, float* dbeta, hipStream_t st, const bf16_t* residual = nullptr);
hipError_t launch_groupnorm(GnParams p, hipStream_t st);
hipError_t launch_layernorm(const void* x, int in_is_f32, const float* gamma, const float* beta, void* out, int out_is_f32,
                            int M, int C, float eps, hipStream_t st, int Clog = -1);   // Clog: logical width of zero-padded rows (statistics over Clog)
hipError_t launch_flash_d32(const FlashParams& p, int heads, int batch, hipStream_t st);
hipError_t launch_small_attention(const SmallAttnParams& p, int D, int heads, int batch, hipStream_t st);
hipError_t launch_causal_d64(const CausalD64Params& p, int heads, int batch, hipStream_t st);
bool vq_attn_stream_supported(int C);                     // C % 128 == 0, C <= 512
hipError_t launch_vq_attn_stream(const VqAttnParams& p, int batch, hipStream_t st);
size_t small_attention_bwd_scratch_bytes(int B, int heads, int nq, int nkv);
hipError_t launch_small_attention_bwd(const bf16_t* q, int ldq, const bf16_t* k, const bf16_t* v, int ldkv, const bf16_t* dout, int ldo, int B, int nq, int nkv,
                                      int heads, float scale, bf16_t* dq, bf16_t* dk, bf16_t* dv, char* scratch, hipStream_t st);    // backward.hip: d_head 32, nkv <= 32
hipError_t launch_conv_in(const float* x, const float* w, const float* bias, bf16_t* out, int B, int Cin, int H, int W,
                          int Cout, hipStream_t st);
hipError_t launch_conv_out(const bf16_t* x, const float* w, const float* bias, float* out, int B, int H, int W, int Cin,
                           int Cout, hipStream_t st);
hipError_t launch_timestep_embedding(const long long* t, bf16_t* out, int B, int dim, int ld, hipStream_t st);   // rows of ld >= dim, tail zeroed
hipError_t launch_cast_f32_bf16(const float* x, bf16_t* y, long long n, hipStream_t st);
hipError_t launch_transpose_bf16(const bf16_t* x, bf16_t* y, int rows, int cols, hipStream_t st, int batch = 1, int ldy = 0);       // y[c][r] = x[r][c] (batch contiguous matrices)
hipError_t launch_multi_tensor(int n, float* const* p, const float* const* g, float* const* m, float* const* v, void* const* pb, const long long* numel, int ema,
                               double lr, double b1, double b2, double eps, double wd, int step, float omd, hipStream_t st);      // AdamW / LitEma over a list of tensors, 48 per launch
hipError_t launch_adamw(float* p, const float* g, float* m, float* v, bf16_t* pb, long long n, double lr, double b1, double b2, double eps, double wd, int step,
                        hipStream_t st);
hipError_t launch_ema(float* shadow, const float* p, long long n, float one_minus_decay, hipStream_t st);
hipError_t launch_silu(const float* x, const float* dy, bf16_t* ob, float* of, long long n, hipStream_t st);
// training-step glue (backward.hip, end): q_sample, squared-error loss + gradient, conditioning switch, scaling, per-sample column sums, 2x expansions
hipError_t launch_q_sample(const float* x0, const float* noise, const float* a, const float* b, float* out, bf16_t* out_nhwc, int B, int C, int HW, int cpad, hipStream_t st);
hipError_t launch_mse_loss(const bf16_t* eps, const float* target, const float* coef, float* se, bf16_t* deps, int B, int C, int HW, int ldc, hipStream_t st);
hipError_t launch_where_rows(const unsigned char* mask, const float* a, const float* x, float* out, long long rows, long long n, hipStream_t st);
hipError_t launch_scale_f32(float* x, long long n, float s, hipStream_t st);
size_t colsum_samples_scratch_bytes(int B, int HW, int N);
hipError_t launch_colsum_samples(const bf16_t* x, bf16_t* out, int B, int HW, int N, hipStream_t st, float* scratch = nullptr);
hipError_t launch_expand2(const bf16_t* x, bf16_t* out, int B, int H, int W, int C, int mode, hipStream_t st);
hipError_t launch_sumpool2(const bf16_t* x, bf16_t* out, int B, int H, int W, int C, hipStream_t st);
// fused attention backward, d_head = 32 (backward.hip): no score matrix in memory
size_t attn_bwd_scratch_bytes(int B, int H, int n, int m);
hipError_t launch_attention_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, const bf16_t* o, const bf16_t* dout, int B, int n, int m, int H,
                                bf16_t* dq, bf16_t* dk, bf16_t* dv, char* scratch, hipStream_t st);
// fused backward of the causal d_head = 64 attention (backward.hip) on the fused q | k | v projection: dqkv = dq | dk | dv
size_t causal_attention_d64_bwd_scratch_bytes(int B, int H, int n);
hipError_t launch_causal_attention_d64_bwd(const bf16_t* qkv, int ldq, const bf16_t* o, int ldo, const bf16_t* dout, int lddo, int B, int n, int H, float scale,
                                           bf16_t* dqkv, int ldd, char* scratch, hipStream_t st);
// attention backward helpers (backward.hip)
hipError_t launch_heads(const bf16_t* x, bf16_t* out, int B, int n, int H, int D, int ldx, int mode, hipStream_t st);
hipError_t launch_softmax_bwd(const bf16_t* P, const float* dP, bf16_t* dS, long long rows, int n, hipStream_t st);
hipError_t launch_expand_heads(const bf16_t* kv, int ld, int B, int k, int heads, int hd, int NP, float scale, bf16_t* out, hipStream_t st);
hipError_t launch_add_bias_rows(const bf16_t* x, const float* bias, bf16_t* out, long long rows, int C, hipStream_t st);
hipError_t launch_row_nonzero(const float* x, int rows, long long n, int* flag, hipStream_t st);   // flag[r] = row r has a non-zero element
// rng null: the kernel reads p.noise / p.z from memory; else the seeded kernel draws it (p.noise / p.z unused), which has no scalar form --
// hipErrorInvalidValue unless n and per_row are multiples of 4, per_row divides n and every operand is 16-byte aligned
hipError_t launch_ddim_step(const DdimStepParams& p, const StepRngParams* rng, hipStream_t st);
hipError_t launch_ddpm_step(const DdpmStepParams& p, const StepRngParams* rng, hipStream_t st);
hipError_t launch_rng_fill(const RngFillParams& p, bool normal, hipStream_t st);
hipError_t launch_plms_step(const PlmsStepParams& p, hipStream_t st);
hipError_t launch_dpmpp_step(const DpmppStepParams& p, const StepRngParams* rng, hipStream_t st);      // rng and p.noise null: the ODE step; else the SDE step
hipError_t launch_unipc_step(const UnipcStepParams& p, hipStream_t st);
hipError_t launch_ddim_inverse_step(const DdimInverseStepParams& p, hipStream_t st);
hipError_t launch_q_sample_seeded(const QSampleSeededParams& p, hipStream_t st);     // hipErrorInvalidValue: per_row % 4 or an operand not 16-byte aligned
// rng null: float4 form when n % 4 == 0, hw % 4 == 0 and every operand is 16-byte aligned, else scalar; rng: hipErrorInvalidValue for chw % 4 or x / x0 / out / x_dup not 16-byte aligned
hipError_t launch_masked_blend(const MaskedBlendParams& p, const StepRngParams* rng, hipStream_t st);
hipError_t launch_vq_quantize(const float* z, const float* codebook, int n_embed, const float* pq_w, const float* pq_b,
                              float* out, int* idx_out, int B, int HW, int quantize, hipStream_t st);
// nearest-code search of a wide-latent VQ first stage (vqcode.hip): idx[m] = argmin_j |e_j|^2 - 2 z_m . e_j on fp32-input MFMAs, first minimum on ties
bool vq_nearest_supported(int E);                         // E % 64 == 0, E <= 512
size_t vq_nearest_ws_bytes(long long M, int N);           // per-split (score, index) planes
hipError_t launch_vq_code_norms(const float* codebook, float* norms, int N, int E, hipStream_t st);
hipError_t launch_vq_nearest(const float* z, const float* codebook, const float* norms, long long M, int N, int E, char* ws, int* idx32,
                             long long* idx64, hipStream_t st);       // idx32 / idx64: either may be null
hipError_t launch_vq_rows_to_nchw(const float* src, const int* idx, float* out, int B, int HW, int E, hipStream_t st);      // out [B,E,HW] = rows idx[token] (null: token) of src [.,E]; E % 32 == 0
// metric arithmetic on feature sets f32 [n, d] (metrics.hip): fp64 moments, and the two streaming searches over d2(a, b) = |a|^2 + |b|^2 - 2 a.b
// in fp32 (norms from launch_metric_row_norms: the same chain as the MFMA dot product, so equal rows are at distance exactly 0)
bool metric_dim_supported(int d);                         // d % 32 == 0, 32 <= d <= 4096
size_t metric_moments_ws_bytes(int n, int d);             // partial planes of the row splits; 0: none needed
hipError_t launch_metric_moments(const float* x, int n, int d, double* sum, double* outer, char* ws, hipStream_t st);   // sum [d], outer [d, d]: accumulated into
hipError_t launch_metric_row_norms(const float* x, float* norms, int n, int d, hipStream_t st);
hipError_t launch_metric_knn_radius(const float* x, const float* norms, int n, int d, int k, float* radius2, hipStream_t st);   // 1 <= k <= 8, k < n
hipError_t launch_metric_manifold_hits(const float* probe, const float* pnorms, int m, const float* ref, const float* rnorms, const float* ref_radius2,
                                       int n, int d, unsigned char* hit, hipStream_t st);
// the same kernel's other epilogues: count [m] = # of the balls probe i lies in; d2 [m] = the nearest ref row's d2; and, on the dot products
// alone (no norms), rowsum f64 [groups, m] = SUM_j (gamma probe_gi . ref_gj + coef0)^3, group g = blockIdx.y, optionally without j == i
constexpr int METRIC_MAX_GROUPS = 65535;                  // gridDim.y
hipError_t launch_metric_manifold_counts(const float* probe, const float* pnorms, int m, const float* ref, const float* rnorms, const float* ref_radius2,
                                         int n, int d, int* count, hipStream_t st);
hipError_t launch_metric_nearest_d2(const float* probe, const float* pnorms, int m, const float* ref, const float* rnorms, int n, int d, float* d2,
                                    hipStream_t st);
hipError_t launch_metric_poly3_rowsums(const float* probe, int m, const float* ref, int n, int d, int groups, int exclude_same_index, float gamma,
                                       float coef0, double* rowsum, hipStream_t st);
hipError_t launch_softmax_rows(const float* s, bf16_t* p, long long rows, int n, hipStream_t st, int n_valid = 0);   // columns >= n_valid: probability 0
hipError_t launch_clip_embed(const long long* tokens, const float* tok_emb, const float* pos_emb, float* out, int B, int L,
                             int Wd, hipStream_t st);
hipError_t launch_clip_gather_eot(const long long* tokens, const float* x, float* out, int B, int L, int Wd, hipStream_t st);
hipError_t launch_clip_patchify(const float* img, bf16_t* out, int B, int R, int P, hipStream_t st);
// bicubic resize (align_corners) + (x+1)/2 + CLIP mean/std: into f32 [B,3,R,R] (out_patch null) or the bf16 patch matrix
hipError_t launch_clip_preprocess(const float* img, int B, int H, int W, int R, int P, float* out_f32, bf16_t* out_patch, hipStream_t st);
hipError_t launch_clip_vit_assemble(const float* patch, const float* cls, const float* pos, float* out, int B, int GG, int Wd,
                                    hipStream_t st);
hipError_t launch_gather_rows_f32(const float* x, float* out, int B, long long row_stride, int Wd, hipStream_t st);
hipError_t launch_to_uint8_hwc(const float* x, unsigned char* out, int B, int C, int H, int W, hipStream_t st);

// box calibration probes (calib.hip): a fixed MFMA stream on random bf16 operands and a fixed HBM copy, timed on `st`
hipError_t run_calib_probes(void* buf, double mfma_ms, size_t stream_bytes, int stream_reps, double* mfma_tflops, double* stream_gbps, hipStream_t st);
