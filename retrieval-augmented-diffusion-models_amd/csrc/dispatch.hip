// Kernel selection of librdm_hip: which kernel runs an op, with which parameters.  The row-count rules of the linear ops
// (skinny / mid-size / tiled), the bodies of the Ops methods that every model executor and every rdm_op_* entry goes through, and
// rdm_linear_rows_select, which reports the linear rule to the tests.  Host only; the kernels are in the files kernels.h lists.
#include "host.h"

// ------------------------------------------------------------------------------------ op helpers
static int gn_chunks(int HW) { const int n = HW / 64; return n < 1 ? 1 : n > 32 ? 32 : n; }      // GroupNorm statistics: pixel chunks per sample

// Which kernel takes a linear op that the skinny kernels may run (one bf16 operand, no row vector, alpha 1), and whether the LayerNorm-in-
// kernel form takes a LayerNorm + projection: the ONE statement of both choices, shared by Ops::linear / Ops::linear_ln (every executor
// and op entry) and by rdm_linear_rows_select, which reports it.  Host only: reads q's shape, activation and which pointers are set.
static bool skinny_rows(bool deterministic, bool single_row, int M, int single_max) {
    return deterministic ? single_row : (M <= 128 || (single_row && M <= single_max));
}
static int linear_kernel(SgemmParams& q, bool deterministic, bool single_row) {
    // one-row-per-sample operands beyond these row counts take the tiled kernels
    constexpr int SGEMM_MAX_ROWS = 4096;          // (2048 sequences: 716 -> 780 img/s against the tiled kernels, round 5)
    // (round 5, same box: the GEGLU projection of the RARM decode step through the tiled kernel from ~200 rows on: 397.8 -> 409.5 img/s at 256
    //  sequences, 487.0 -> 514.8 at 512; the plain projections through it: 221 / 305 -- their N = 768 gives the tiled kernel 16-24 tiles)
    constexpr int SGEMM_GEGLU_MAX_ROWS = 192;
    if (skinny_rows(deterministic, single_row, q.M, q.act == ACT_GEGLU ? SGEMM_GEGLU_MAX_ROWS : SGEMM_MAX_ROWS)) {
        // 1536+ rows: LDS-staged 64 x 64 tiles (mgemm.hip) -- the skinny kernel's per-wave operand fetch is 75 MB through the L2 -> CU
        // fabric for a [2048 x 768] x [768 x 768] product (33.6 us; 15.5 there).  Not in deterministic mode (the kernel choice would follow the batch).
        static const int mg_from = rdm_env_int(getenv("RDM_MGEMM_FROM"), 1536);     // (tests move it)
        if (!deterministic && single_row && mg_from > 0 && q.M >= mg_from && q.act != ACT_GEGLU && mgemm_supported(q)) return RDM_LINEAR_ROWS_MGEMM;
        q.fixed_split = deterministic ? 1 : 0;
        if (sgemm_supported(q)) return RDM_LINEAR_ROWS_SGEMM;
    }
    static const int mg_any = rdm_env_int(getenv("RDM_MGEMM_ANY"), 0);      // tests: operands of >= mg_any rows that are not single_row
    if (!single_row && mg_any > 0 && q.M >= mg_any && q.act != ACT_GEGLU && mgemm_supported(q)) return RDM_LINEAR_ROWS_MGEMM;
    return RDM_LINEAR_ROWS_TILED;
}
static bool linear_ln_takes(SgemmParams& q, bool deterministic, bool single_row) {
    // (from ~200 rows on a separate LayerNorm pass + the 64 x 64-tile GEMM beats the LayerNorm-fused 32-row tiles: sgemm.hip)
    constexpr int SGEMM_LN_MAX_ROWS = 192;
    if (!deterministic && q.M > SGEMM_LN_MAX_ROWS) return false;
    q.fixed_split = deterministic ? 1 : 0;
    return skinny_rows(deterministic, single_row, q.M, 1024) && sgemm_supported(q);
}

// ------------------------------------------------------------------------------------ Ops (declared in host.h)
const bf16_t* Ops::derived(const bf16_t* W, int N, int K, int kind) {
    if (const_weights) return c->cached_derived(W, N, K, kind);
    if (ensure_bytes(c, &c->wfrag_tmp, &c->wfrag_tmp_bytes, rdm_ctx::derived_bytes(kind, N, K)) != 0) return nullptr;
    bf16_t* d = (bf16_t*)c->wfrag_tmp;
    return c->pack_derived(kind, W, d, N, K) == hipSuccess ? d : nullptr;
}

// The skinny (weight-streaming) kernels take decode-sized operands (skinny_rows).  Fast mode: whenever M <= 128, and for `single_row`
// operands up to a per-form row count.  Deterministic mode: exactly for the ops with ONE row per sample (`single_row`: time embedding,
// RARM decode step, CLIP projection), at any batch (one-row-per-sample operands of bigger batches -- RARM decode at 128+ sequences per
// GPU -- keep the skinny kernel: its row blocks scale with M, while the tiled kernels would run a dozen 256-row tiles)
static SgemmParams skinny_params(const LinearOp& op) {      // the op as the skinny / mid-size kernels take it (one bf16 operand, or LayerNorm(ln_x))
    SgemmParams q{}; q.A = op.A0; q.lda = op.C0; q.W = op.W; q.M = op.M; q.N = op.N; q.K = op.C0; q.bias = op.bias;
    q.act = op.act; q.res_f32 = op.res_f32; q.res_bf16 = op.res_bf16; q.out_f32 = op.out_f32; q.out_bf16 = op.out_bf16;
    q.ldo = op.act == ACT_GEGLU ? op.N / 2 : op.N;
    return q;
}
bool Ops::lin4_takes(const LinearOp& op) {
    if (c->deterministic) return false;
    IgemmParams t = base(op.M, op.N, op.C0 + op.C1);
    t.C0 = op.C0; t.C1 = op.C1; t.W = (const bf16_t*)blob; t.Wfrag = t.W; t.out_bf16 = (bf16_t*)blob;
    t.a0_wrap_rows = op.a0_wrap_rows; t.a1_wrap_rows = op.a1_wrap_rows;
    if (op.rowvec) { t.rowvec = op.rowvec; t.rowvec_ld = op.rowvec_ld; t.rows_per_sample = op.rows_per_sample; }
    if (op.res_wrap_rows > 0) { t.res_bf16 = (const bf16_t*)blob; t.res_wrap_rows = op.res_wrap_rows; }
    return lin4_supported(t, 1);
}
void Ops::linear(const LinearOp& op) {
    if (plan) return;
    const int M = op.M, N = op.N, K = op.C0 + op.C1;
    if (!op.A1 && op.C1 == 0 && !op.rowvec && op.alpha == 1.f && op.a0_wrap_rows == 0 && op.res_wrap_rows == 0) {         // N/32 x ceil(M/32) blocks (sgemm.hip), 64 x 64 tiles (mgemm.hip)
        SgemmParams q = skinny_params(op);
        if (op.choice_rows > M) q.M = op.choice_rows;
        const int kernel = linear_kernel(q, c->deterministic, op.single_row);
        q.M = M;
        if (kernel != RDM_LINEAR_ROWS_TILED) {
            const bool mid = kernel == RDM_LINEAR_ROWS_MGEMM;
            prof_begin(RDM_PROF_LINEAR, 2.0 * M * N * (double)K, M, N, K);
            check(mid ? launch_mgemm(q, c->stream) : launch_sgemm(q, c->stream), mid ? "mid-size linear" : "skinny linear");
            prof_end();
            return;
        }
    }
    IgemmParams p = base(M, N, K);
    p.A0 = op.A0; p.A1 = op.A1; p.C0 = op.C0; p.C1 = op.C1; p.W = op.W; p.bias = op.bias; p.alpha = op.alpha;
    p.act = op.act; p.res_bf16 = op.res_bf16; p.res_f32 = op.res_f32; p.out_bf16 = op.out_bf16; p.out_f32 = op.out_f32;
    p.a0_wrap_rows = op.a0_wrap_rows; p.a1_wrap_rows = op.a1_wrap_rows; p.res_wrap_rows = op.res_wrap_rows; p.choice_rows = op.choice_rows;
    if (op.rowvec) { p.rowvec = op.rowvec; p.rowvec_ld = op.rowvec_ld; p.rows_per_sample = op.rows_per_sample; }
    if (op.act == ACT_GEGLU) p.ldo = N / 2;
    // one-wave-per-SIMD kernel for the big-M projections (its tile choice follows M, so not in deterministic mode)
    // (deterministic mode: its use must not follow the batch -- exactly when the rows of ONE sample (op.sample_rows) fill whole
    //  128 / 256-row tiles, at any tile count; a row's sum order is the same in every tile position)
    {
        IgemmParams t = p; t.Wfrag = p.W;
        const int tile_rows = (N % 384 == 0) ? 128 : 256;
        const bool det_ok = op.sample_rows > 0 && op.sample_rows % tile_rows == 0;
        if (c->deterministic) t.l4_any_tiles = p.l4_any_tiles = 1;
        if ((!c->deterministic || det_ok) && lin4_supported(t, 1)) p.Wfrag = derived(p.W, N, K, op.act == ACT_GEGLU ? 2 : 1);
    }
    prof_begin(RDM_PROF_LINEAR, 2.0 * M * N * (double)K, M, N, K);
    check(launch_igemm(p, false, 1, c->stream), "linear");
    prof_end();
}
// out = act(LayerNorm(ln_x; ln_g, ln_b) W^T + bias), bf16, with the LayerNorm formed inside the skinny GEMM (sgemm.hip): decode-sized
// operands only.  false = not available for this shape (the caller runs layernorm + linear)
bool Ops::linear_ln(const LinearOp& op) {
    SgemmParams q = skinny_params(op);
    q.ln_x = op.ln_x; q.ln_g = op.ln_g; q.ln_b = op.ln_b; q.ln_eps = 1e-5f;
    if (!linear_ln_takes(q, c->deterministic, op.single_row)) return false;
    if (plan) return true;
    prof_begin(RDM_PROF_LINEAR, 2.0 * op.M * op.N * (double)op.C0, op.M, op.N, op.C0);
    check(launch_sgemm(q, c->stream), "skinny linear on a LayerNorm");
    prof_end();
    return true;
}
void Ops::conv3(const Conv3Op& op) {
    if (plan) return;
    const bf16_t* A0 = op.A0; const bf16_t* A1 = op.A1; const bf16_t* W = op.W; const float* bias = op.bias;
    const int C0 = op.C0, C1 = op.C1, B = op.B, Hin = op.Hin, Win = op.Win, N = op.N, stride = op.stride, ups = op.ups;
    const float* rowvec = op.rowvec; const bf16_t* res = op.res_bf16; bf16_t* out = op.out_bf16;
    const int Hout = ups ? Hin * 2 : (stride == 2 ? Hin / 2 : Hin), Wout = ups ? Win * 2 : (stride == 2 ? Win / 2 : Win);
    IgemmParams p = base(B * Hout * Wout, N, 9 * (C0 + C1));
    p.asym = op.asym;
    p.A0 = A0; p.A1 = A1; p.C0 = C0; p.C1 = C1; p.W = W; p.bias = bias;
    p.Hin = Hin; p.Win = Win; p.Hout = Hout; p.Wout = Wout; p.stride = stride; p.ups = ups;
    p.rowvec = rowvec; p.rowvec_ld = op.rowvec_ld; p.rows_per_sample = Hout * Wout; p.res_bf16 = res; p.out_bf16 = out;
    // deterministic mode: the halo kernels need whole 256-pixel tiles, which at < 256 pixels per sample exist only for batches
    // that are multiples of 256 / HW -- there the generic implicit GEMM (another summation order) runs for EVERY batch; and no
    // split-K (its factor follows the tile count, i.e. the batch)
    // Upsample's conv by output phase: four 2 x 2-tap convs at source resolution on pre-summed weights, 2.25 x fewer FLOPs than the
    // nine taps at output resolution (igemm.hip CONV == 3)
    if (ups && !A1 && C1 == 0 && C0 % 64 == 0 && N % 8 == 0 && !rowvec && !res && stride == 1) {
        const bf16_t* wp = derived(W, N, C0, 5);
        if (wp) {
            IgemmParams q = base(B * Hin * Win, N, 4 * C0);
            q.A0 = A0; q.C0 = C0; q.W = wp; q.bias = bias; q.out_bf16 = out; q.phase2 = 1;
            q.Hin = Hin; q.Win = Win; q.Hout = Hout; q.Wout = Wout; q.stride = 1; q.rows_per_sample = Hin * Win;
            q.sA = 0; q.sW = (long long)N * 4 * C0; q.sO = 0;
            prof_begin(RDM_PROF_UPSCONV, 2.0 * 4.0 * q.M * N * (double)q.K, 4 * q.M, N, q.K);
            check(launch_igemm(q, true, 4, c->stream), "conv3x3 on a 2x upsample, by phase");
            prof_end();
            return;
        }
    }
    const bool det_generic = c->deterministic && ((Hout * Wout) % 256 != 0);
    if (!det_generic && conv3x3_kernel(p) != CONV_IGEMM) p.Wfrag = derived(W, N, C0 + C1, 0);
    // the K-split is chosen only with the fragment copy in hand: without one the conv runs on the implicit GEMM, which knows nothing of ksplit / ws
    const int ks = (p.Wfrag && !c->deterministic) ? conv_halo_ksplit(p) : 1;
    if (ks > 1 && ensure_bytes(c, &c->splitk_ws, &c->splitk_ws_bytes, (size_t)ks * p.M * N * 4) == 0) { p.ksplit = ks; p.ws = (float*)c->splitk_ws; }
    prof_begin(RDM_PROF_CONV3X3, 2.0 * p.M * N * (double)p.K, p.M, N, p.K);
    check(launch_conv3x3(p, c->stream), "conv3x3");      // no p.Wfrag (det_generic, no halo geometry, no memory for the copy): the implicit GEMM
    prof_end();
}
// (Round 6, wave quantisation: a conv of q full rounds of the CUs plus a partial round -- the 16 x 16 level of a guided batch of 64 is 384
//  tiles on 256 CUs -- was run as full rounds + a K-split remainder in three forms: tail rows on a second stream, halves handed out inside
//  one launch, two launches on tile sub-ranges.  All parity-exact, all SLOWER (-1.0 .. -1.4 % on the headline), and the launch trace says
//  why: under the package power cap a half-empty round is nearly half price -- 256 tiles take 140 us, 384 tiles 213 us: the 128
//  remainder tiles cost 73 us on a chip that clocks up when half its CUs idle -- while 256 K halves + their fp32 planes and finisher cost
//  118 us.  The code is in the history (commits "conv tail split", "conv_halo4 TAIL variant", "conv remainder split"), the numbers in
//  profiles/r06_conv_tail_split_*.log, r06_conv_remainder_split_*.)
// twice: the stage ran on the first half of a guided batch only (unet_body's shared prefix inside the first transformer) and ptr holds
// those nbytes; the tap shows the LOGICAL tensor, both halves, the second a copy of the first
void Ops::tap(int stage, const void* ptr, size_t nbytes, bool twice, size_t offset) {      // rdm_debug_tap: stage `stage` of layer cur_layer of block cur_block
    if (plan || !c->tap_buf || c->tap_block != cur_block || c->tap_sub != cur_layer * 16 + stage || offset >= c->tap_bytes) return;
    char* dst = (char*)c->tap_buf + offset; const size_t room = c->tap_bytes - offset;
    const size_t n0 = nbytes > room ? room : nbytes;
    check(hipMemcpyAsync(dst, ptr, n0, hipMemcpyDeviceToDevice, c->stream), "debug tap");
    if (!twice || room <= nbytes) return;
    const size_t n1 = room - nbytes < nbytes ? room - nbytes : nbytes;
    check(hipMemcpyAsync(dst + nbytes, ptr, n1, hipMemcpyDeviceToDevice, c->stream), "debug tap");
}
void Ops::prof_begin(int kind, double work, int d0, int d1, int d2) {       // work: FLOPs (GEMM-class kinds) or bytes (bandwidth-class kinds)
    prof_open = (c->prof >> kind) & 1u;
    if (!prof_open) return;
    rdm_ctx::ProfRec r; r.a = c->prof_event(); r.b = c->prof_event(); r.kind = kind; r.flops = work; r.tag = tag; r.d0 = d0; r.d1 = d1; r.d2 = d2;
    hipEventRecord(r.a, c->stream); c->prof_recs.push_back(r);
}
void Ops::prof_end() { if (prof_open) hipEventRecord(c->prof_recs.back().b, c->stream); prof_open = false; }
// (gn_partial must hold B samples' statistics: ensure_gn_partial)
// the caller names x0 (x1), C0 (C1), HW, B, gamma, beta, eps, silu, out, and L0 / L1 (logical channels of zero-padded sources; 0 = all)
// and x1_bmod / x0_bmod where they apply; the statistics' geometry is the dispatch's
void Ops::groupnorm(GnParams p) {
    if (plan) return;
    p.groups = 32; p.nchunk = gn_chunks(p.HW); p.partial = c->gn_partial;
    if (p.L0 <= 0) p.L0 = p.C0;
    if (p.L1 <= 0) p.L1 = p.C1;
    prof_begin(RDM_PROF_GROUPNORM, (double)p.B * p.HW * (p.C0 + p.C1) * 4.0, p.B * p.HW, p.C0 + p.C1, p.silu);       // ALGORITHMIC bytes: one read + one write of the bf16 tensor (round 5: the one-pass kernel moves exactly these; the two-pass form of the 64 x 64 level reads twice)
    check(launch_groupnorm(p, c->stream), "groupnorm");
    prof_end();
}
// GroupNorm + SiLU + 3x3 conv to a few channels (UNet `out`, VQ decoder conv_out): one statistics pass + the fused MFMA head kernel
// (misc.hip), or GroupNorm-apply into `tmp` + the VALU head conv where the fused kernel does not apply.  gamma == null: no GroupNorm
// (the fused kernel only).  The caller names x, B, H, W, C, gamma, beta, eps, w, wp, bias, out, Cout.
HeadParams Ops::head_params(HeadParams hp) const {
    hp.groups = 32;
    if (hp.gamma) { hp.partial = c->gn_partial; hp.nchunk = gn_chunks(hp.H * hp.W); }
    return hp;
}
void Ops::head(HeadParams hp, int Clog, bf16_t* tmp) {
    if (plan) return;
    hp = head_params(hp);
    const int B = hp.B, H = hp.H, W = hp.W, C = hp.C;
    if ((Clog <= 0 || Clog == C) && head_conv_supported(hp)) {
        if (hp.gamma) {
            GnParams p{}; p.x0 = hp.x; p.C0 = C; p.HW = H * W; p.B = B; p.groups = 32; p.L0 = C; p.nchunk = hp.nchunk; p.partial = c->gn_partial;
            prof_begin(RDM_PROF_GROUPNORM, (double)B * H * W * C * 2.0, B * H * W, C, 2);
            check(launch_gn_stats(p, c->stream), "head groupnorm statistics");
            prof_end();
        }
        check(launch_head_conv(hp, c->stream), "head conv");
        return;
    }
    groupnorm({.x0 = hp.x, .C0 = C, .HW = H * W, .B = B, .L0 = Clog, .gamma = hp.gamma, .beta = hp.beta, .eps = hp.eps, .silu = 1, .out = tmp});
    check(launch_conv_out(tmp, hp.w, hp.bias, hp.out, B, H, W, C, hp.Cout, c->stream), "conv_out");
}
void Ops::vq_nearest(const VqNearestOp& op) {
    if (plan) return;
    check(launch_vq_nearest(op.z, op.codebook, op.norms, op.M, op.N, op.E, op.ws, op.idx32, op.idx64, c->stream), "vq nearest code");
}
void Ops::layernorm(const LayerNormOp& op) {
    if (plan) return;
    const bool in_f32 = op.x_f32 != nullptr, out_f32 = op.out_f32 != nullptr;
    prof_begin(RDM_PROF_LAYERNORM, (double)op.M * op.C * ((in_f32 ? 4.0 : 2.0) + (out_f32 ? 4.0 : 2.0)), op.M, op.C, 0);
    check(launch_layernorm(in_f32 ? (const void*)op.x_f32 : op.x_bf16, in_f32, op.gamma, op.beta, out_f32 ? (void*)op.out_f32 : op.out_bf16, out_f32,
                           op.M, op.C, op.eps, c->stream, op.Clog < 0 ? op.C : op.Clog), "layernorm");
    prof_end();
}
// d = 32 flash attention over n tokens (attention.hip): q / k (= q + C) token-major at row stride ldq; V either token-major at the
// same stride (v: the fused q | k | v projection, n % 64 == 0) or V^T per sample [B][C][n] (vt).  The caller names q, ldq, v or vt, out, n.
void Ops::flash_d32(FlashParams f, int heads, int B) {
    if (plan) return;
    const int C = heads * 32, n = f.n;
    f.k = f.q + C; f.ldk = f.ldq; f.ldv = f.v ? f.ldq : 0; f.ldo = C; f.C = C;
    f.scale_log2e = (1.0f / sqrtf(32.f)) * 1.4426950408889634f;
    prof_begin(RDM_PROF_ATTENTION, 4.0 * B * heads * (double)n * n * 32, B, n, C);
    check(launch_flash_d32(f, heads, B, c->stream), "flash attention");
    prof_end();
}
// causal self-attention at d_head 64 over all n positions of B sequences (attention.hip): qkv = the fused q | k | v projection rows;
// kcache / vcache: optional head-major decode caches [B][heads][L][64] that receive rows 0 .. n-1.  The caller names all but C and scale_log2e.
void Ops::causal_d64(CausalD64Params f, int heads, int B, float scale) {
    if (plan) return;
    const int n = f.n;
    f.C = heads * 64; f.scale_log2e = scale * 1.4426950408889634f;
    prof_begin(RDM_PROF_ATTENTION, 2.0 * B * heads * (double)n * n * 64, B, n, f.C);
    check(launch_causal_d64(f, heads, B, c->stream), "causal attention");
    prof_end();
}
// the first stage's AttnBlock without its n x n scores (vq_attn.hip): one head of C channels over n tokens, any n
void Ops::vq_attention(const VqAttnParams& f, int B) {
    if (plan) return;
    prof_begin(RDM_PROF_ATTENTION, 6.0 * B * (double)f.n * f.n * f.C, B, f.n, f.C);      // the scores twice (vq_attn.hip) and P.V
    check(launch_vq_attn_stream(f, B, c->stream), "vq attention");
    prof_end();
}
// attention over a few keys / short sequences (attention.hip): head dim D, nq queries and nkv keys per sample
void Ops::small_attention(const SmallAttnParams& p, int D, int heads, int B, const char* what) {
    if (plan) return;
    check(launch_small_attention(p, D, heads, B, c->stream), what);
}
// cross-attention over k neighbours in one launch (attention.hip): scores against G, softmax, P U, bias and residual; G / U are the
// fragment-ordered images of launch_xattn_pack.  ln_g given: x holds the raw rows, the scores are taken on LayerNorm(x) and the residual
// is x itself (res null); ln3_out given: LayerNorm(out rows; ln3_g, ln3_b) leaves with the finished rows
void Ops::xattn_fused(const XattnParams& q) {
    if (plan) return;
    prof_begin(RDM_PROF_LINEAR, 4.0 * q.rows * q.NP * (double)q.C, q.rows, q.NP, q.C);
    check(launch_xattn_fused(q, c->stream), "fused cross attention");
    prof_end();
}

int rdm_linear_rows_select(int M, int N, int K, int act, int ln, int deterministic, rdm_linear_rows_form* out) {
    if (!out || M < 1 || N < 1 || K < 1 || act < ACT_NONE || act > ACT_SILU) return -1;
    *out = rdm_linear_rows_form{};
    static const float some = 0.f;                        // the choice reads which operands are given, never their values
    SgemmParams q{}; q.M = M; q.N = N; q.K = K; q.lda = K; q.act = act; q.ldo = act == ACT_GEGLU ? N / 2 : N;
    if (ln) { q.ln_x = &some; q.ln_g = &some; q.ln_b = &some; q.ln_eps = 1e-5f; }
    out->kernel = ln ? (linear_ln_takes(q, deterministic != 0, true) ? RDM_LINEAR_ROWS_SGEMM : RDM_LINEAR_ROWS_REFUSED) : linear_kernel(q, deterministic != 0, true);
    if (out->kernel == RDM_LINEAR_ROWS_SGEMM) {
        const SgemmForm f = sgemm_form(q);
        if (!sgemm_form_compiled(f)) return -3;
        out->ma = f.ma; out->nb = f.nb; out->u = f.u; out->nw = f.nw; out->ln = f.ln; out->geglu = f.geglu;
    }
    return 0;
}
