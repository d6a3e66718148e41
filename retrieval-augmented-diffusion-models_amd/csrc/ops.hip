// The operator-level entries of librdm_hip (rdm_op_*: parity tests, op benchmarks, the training path) and rdm_wgrad_select: forward
// ops, backward ops, the token sampler, the RARM decode-step ops.  Calls only host.h: the Ops methods (dispatch.hip) and the
// launch_* of kernels.h; no executor of the other host files.
#include "host.h"

// ---- operator-level entries (parity tests, op benchmarks, the training path): argument checks, then the executors' dispatch (Ops) on
// caller-owned weights.  Their derived copies are packed per call, unless RDM_OP_FRAG_CACHE=1: the caller promises constant weights (op benchmarks).
static Ops op_exec(rdm_ctx* c) {
    static const bool cache = rdm_env_int(getenv("RDM_OP_FRAG_CACHE"), 0) != 0;
    Ops o{c, nullptr, nullptr, /*plan=*/false};
    o.const_weights = cache;
    return o;
}
int rdm_op_linear(rdm_ctx* c, const void* a, const void* w, const float* bias, const void* res, void* out, float* out_f32,
                  int M, int N, int K, int act, float alpha) {
    RDM_ENTER(c);
    Ops o = op_exec(c);
    o.linear({.A0 = (const bf16_t*)a, .C0 = K, .W = (const bf16_t*)w, .bias = bias, .M = M, .N = N, .act = act, .res_bf16 = (const bf16_t*)res,
              .out_bf16 = (bf16_t*)out, .out_f32 = out_f32, .alpha = alpha});
    return o.rc;
}
int rdm_op_linear_rowvec(rdm_ctx* c, const void* a, const void* w, const float* bias, const float* rowvec, int rows_per_group, const void* res,
                         void* out, int M, int N, int K) {      // rows_per_group: LinearOp's (and IgemmParams') rows_per_sample
    RDM_ENTER(c);
    if (!rowvec || rows_per_group < 1) return c->fail(-1, "rdm_op_linear_rowvec: rowvec and rows_per_group >= 1 required");
    Ops o = op_exec(c);
    o.linear({.A0 = (const bf16_t*)a, .C0 = K, .W = (const bf16_t*)w, .bias = bias, .M = M, .N = N, .res_bf16 = (const bf16_t*)res, .out_bf16 = (bf16_t*)out,
              .rowvec = rowvec, .rowvec_ld = N, .rows_per_sample = rows_per_group});
    return o.rc;
}
int rdm_op_linear_ln(rdm_ctx* c, const void* x, const void* w, const float* bias, const float* gamma, const float* beta, void* out,
                     int M, int N, int K, int act, float eps) {
    RDM_ENTER(c);
    if (!x || !w || !gamma || !beta || !out) return c->fail(-1, "rdm_op_linear_ln: null argument");
    IgemmParams p = igemm_plain(M, N, K, c->zero_page);
    if (act == ACT_GEGLU) p.ldo = N / 2;
    p.A0 = (const bf16_t*)x; p.C0 = K; p.W = (const bf16_t*)w; p.out_bf16 = (bf16_t*)out; p.act = act; p.l4_any_tiles = 1;
    p.ln_inv_c = 1.0f / (float)K; p.ln_eps = eps;
    IgemmParams t = p; t.Wfrag = p.W; t.ln_sb = gamma;
    if (!lin4_supported(t, 1)) return c->fail(-5, "rdm_op_linear_ln: shape not taken by the folded-LayerNorm kernel (M %% 128/256, N %% 384/192, K %% 64, K >= 128)");
    // caller-owned weights: packed per call into the scratch copy [fragments | (s, b') table]
    const size_t wbytes = ((size_t)N * K * 2 + 255) & ~(size_t)255;
    RDM_TRY(ensure_bytes(c, &c->wfrag_tmp, &c->wfrag_tmp_bytes, wbytes + (size_t)N * 8));
    float* sb = (float*)(c->wfrag_tmp + wbytes);
    RDM_CHECK_HIP(c, launch_lin_w_fragpack(p.W, (bf16_t*)c->wfrag_tmp, N, K, K, act == ACT_GEGLU, c->stream, gamma));
    RDM_CHECK_HIP(c, launch_lin_ln_sb(p.W, gamma, beta, bias, sb, N, K, c->stream));
    p.Wfrag = (const bf16_t*)c->wfrag_tmp; p.ln_sb = sb;
    RDM_CHECK_HIP(c, launch_lin4(p, c->stream));
    return 0;
}
int rdm_op_conv3x3(rdm_ctx* c, const void* x0, const void* x1, int C0, int C1, const void* w, const float* bias,
                   const float* rowvec, int rowvec_ld, const void* res, void* out, int B, int Hin, int Win, int N, int stride,
                   int ups) {
    RDM_ENTER(c);
    Ops o = op_exec(c);
    o.conv3({.A0 = (const bf16_t*)x0, .A1 = (const bf16_t*)x1, .C0 = C0, .C1 = C1, .W = (const bf16_t*)w, .bias = bias, .B = B, .Hin = Hin, .Win = Win, .N = N,
             .stride = stride, .ups = ups, .res_bf16 = (const bf16_t*)res, .out_bf16 = (bf16_t*)out, .rowvec = rowvec, .rowvec_ld = rowvec_ld});
    return o.rc;
}
// the first-stage encoder's Downsample conv (vqenc_body's call): F.pad(x, (0, 1, 0, 1)) + Conv2d(3, stride 2, padding 0) on the generic implicit GEMM
int rdm_op_conv3x3_down(rdm_ctx* c, const void* x, int C, const void* w, const float* bias, void* out, int B, int Hin, int Win, int N) {
    RDM_ENTER(c);
    if (!x || !w || !out || B < 1 || Hin < 2 || Win < 2 || C < 64 || C % 64 || N < 2 || N % 2 || (long long)B * Hin * Win > 0x7fffffffLL)
        return c->fail(-1, "rdm_op_conv3x3_down: bad argument (null pointer, or B %d Hin %d Win %d C %d N %d: C %% 64 == 0, N even)", B, Hin, Win, C, N);
    if (Hin % 2 || Win % 2) return c->fail(-1, "rdm_op_conv3x3_down: Hin and Win must be even (a Downsample halves exactly), got %d x %d", Hin, Win);
    Ops o = op_exec(c);
    o.conv3({.A0 = (const bf16_t*)x, .C0 = C, .W = (const bf16_t*)w, .bias = bias, .B = B, .Hin = Hin, .Win = Win, .N = N, .stride = 2, .out_bf16 = (bf16_t*)out, .asym = 1});
    return o.rc;
}
// the nearest-code kernel alone on caller-given operands (vqcode.hip): |e|^2 and the split planes live in the sampler scratch
int rdm_op_vq_nearest_code(rdm_ctx* c, const float* z, const float* codebook, long long M, int N, int E, int32_t* idx_out) {
    RDM_ENTER(c);
    if (!z || !codebook || !idx_out || M < 1 || N < 1) return c->fail(-1, "rdm_op_vq_nearest_code: null argument or M, N < 1");
    if (!vq_nearest_supported(E)) return c->fail(-1, "rdm_op_vq_nearest_code: E = %d; the kernel takes multiples of 64 up to 512", E);
    const size_t nbytes = ((size_t)N * 4 + 255) & ~(size_t)255;
    RDM_TRY(ensure_bytes(c, &c->samp, &c->samp_bytes, nbytes + vq_nearest_ws_bytes(M, N)));
    float* norms = (float*)c->samp;
    RDM_CHECK_HIP(c, launch_vq_code_norms(codebook, norms, N, E, c->stream));
    Ops o = op_exec(c);
    o.vq_nearest({.z = z, .codebook = codebook, .norms = norms, .M = M, .N = N, .E = E, .ws = c->samp + nbytes, .idx32 = idx_out});
    return o.rc;
}
// ---- metric arithmetic on feature sets (kernels in metrics.hip); norms and split planes live in the sampler scratch
static int metric_dim_check(rdm_ctx* c, const char* op, int d) {
    if (!metric_dim_supported(d)) return c->fail(-1, "%s: d = %d; the kernels take multiples of 32 from 32 to 4096", op, d);
    return 0;
}
// |probe_i|^2 [m] and |ref_j|^2 [n] into the sampler scratch, for the modes of metric_dist_kernel that work on d2
static int metric_pair_norms(rdm_ctx* c, const float* probe, int m, const float* ref, int n, int d, float** pn, float** rn) {
    const size_t mb = ((size_t)m * 4 + 255) & ~(size_t)255;
    RDM_TRY(ensure_bytes(c, &c->samp, &c->samp_bytes, mb + (size_t)n * 4));
    *pn = (float*)c->samp; *rn = (float*)(c->samp + mb);
    RDM_CHECK_HIP(c, launch_metric_row_norms(probe, *pn, m, d, c->stream));
    RDM_CHECK_HIP(c, launch_metric_row_norms(ref, *rn, n, d, c->stream));
    return 0;
}
// Frechet distance (Heusel et al. 2017): the sufficient statistics of mu = sum / n and Sigma = (outer - n mu mu^T) / (n - 1)
int rdm_op_moments_f64(rdm_ctx* c, const float* x, int n, int d, double* sum, double* outer) {
    RDM_ENTER(c);
    if (n < 1) return c->fail(-1, "rdm_op_moments_f64: n = %d; at least one row", n);
    if (!x || !sum || !outer) return c->fail(-1, "rdm_op_moments_f64: null argument");
    RDM_TRY(metric_dim_check(c, "rdm_op_moments_f64", d));
    const size_t ws = metric_moments_ws_bytes(n, d);
    if (ws) RDM_TRY(ensure_bytes(c, &c->samp, &c->samp_bytes, ws));
    RDM_CHECK_HIP(c, launch_metric_moments(x, n, d, sum, outer, ws ? c->samp : nullptr, c->stream));
    return 0;
}
// improved precision / recall (Kynkaanniemi et al. 2019, eq. 3): the radius of row i's k-NN ball, NN_k(x_i, X \ {x_i}), squared
int rdm_op_knn_radius(rdm_ctx* c, const float* x, int n, int d, int k, float* radius2_out) {
    RDM_ENTER(c);
    if (n < 1) return c->fail(-1, "rdm_op_knn_radius: n = %d; at least one row", n);
    if (!x || !radius2_out) return c->fail(-1, "rdm_op_knn_radius: null argument");
    RDM_TRY(metric_dim_check(c, "rdm_op_knn_radius", d));
    if (k < 1 || k > 8) return c->fail(-1, "rdm_op_knn_radius: k = %d; the kernel keeps 1 to 8 neighbours", k);
    if (k >= n) return c->fail(-1, "rdm_op_knn_radius: k = %d needs more than n = %d rows (self is no neighbour)", k, n);
    RDM_TRY(ensure_bytes(c, &c->samp, &c->samp_bytes, (size_t)n * 4));
    float* norms = (float*)c->samp;
    RDM_CHECK_HIP(c, launch_metric_row_norms(x, norms, n, d, c->stream));
    RDM_CHECK_HIP(c, launch_metric_knn_radius(x, norms, n, d, k, radius2_out, c->stream));
    return 0;
}
// the same paper's f(probe_i, Ref) (eq. 3): 1 iff probe_i lies in the k-NN ball of some reference row
int rdm_op_manifold_hits(rdm_ctx* c, const float* probe, int m, const float* ref, const float* ref_radius2, int n, int d, unsigned char* hit_out) {
    RDM_ENTER(c);
    if (m < 1 || n < 1) return c->fail(-1, "rdm_op_manifold_hits: m = %d, n = %d; at least one row each", m, n);
    if (!probe || !ref || !ref_radius2 || !hit_out) return c->fail(-1, "rdm_op_manifold_hits: null argument");
    RDM_TRY(metric_dim_check(c, "rdm_op_manifold_hits", d));
    float *pn, *rn;
    RDM_TRY(metric_pair_norms(c, probe, m, ref, n, d, &pn, &rn));
    RDM_CHECK_HIP(c, launch_metric_manifold_hits(probe, pn, m, ref, rn, ref_radius2, n, d, hit_out, c->stream));
    return 0;
}
// density (Naeem et al. 2020, eq. 7): 1 / (k M) SUM_j SUM_i 1[Y_j in B(X_i, NND_k(X_i))]; the inner sum over the real rows i is count[j]
int rdm_op_manifold_counts(rdm_ctx* c, const float* probe, int m, const float* ref, const float* ref_radius2, int n, int d, int32_t* count_out) {
    RDM_ENTER(c);
    if (m < 1 || n < 1) return c->fail(-1, "rdm_op_manifold_counts: m = %d, n = %d; at least one row each", m, n);
    if (!probe || !ref || !ref_radius2 || !count_out) return c->fail(-1, "rdm_op_manifold_counts: null argument");
    RDM_TRY(metric_dim_check(c, "rdm_op_manifold_counts", d));
    float *pn, *rn;
    RDM_TRY(metric_pair_norms(c, probe, m, ref, n, d, &pn, &rn));
    RDM_CHECK_HIP(c, launch_metric_manifold_counts(probe, pn, m, ref, rn, ref_radius2, n, d, count_out, c->stream));
    return 0;
}
// coverage (the same paper, eq. 9): 1 / N SUM_i 1[exists j: Y_j in B(X_i, NND_k(X_i))] = mean_i [min_j d2(X_i, Y_j) <= r2_i]; the minimum
int rdm_op_nearest_d2(rdm_ctx* c, const float* probe, int m, const float* ref, int n, int d, float* d2_out) {
    RDM_ENTER(c);
    if (m < 1 || n < 1) return c->fail(-1, "rdm_op_nearest_d2: m = %d, n = %d; at least one row each", m, n);
    if (!probe || !ref || !d2_out) return c->fail(-1, "rdm_op_nearest_d2: null argument");
    RDM_TRY(metric_dim_check(c, "rdm_op_nearest_d2", d));
    float *pn, *rn;
    RDM_TRY(metric_pair_norms(c, probe, m, ref, n, d, &pn, &rn));
    RDM_CHECK_HIP(c, launch_metric_nearest_d2(probe, pn, m, ref, rn, n, d, d2_out, c->stream));
    return 0;
}
// KID (Binkowski et al. 2018, eq. 4 with k(x, y) = (x.y / d + 1)^3): the row sums of the three kernel matrices of the unbiased MMD^2, one
// group per subset.  No norms, no scratch
int rdm_op_poly3_rowsums(rdm_ctx* c, const float* probe, int m, const float* ref, int n, int d, int groups, int exclude_same_index, float gamma,
                         float coef0, double* rowsum_out) {
    RDM_ENTER(c);
    if (m < 1 || n < 1) return c->fail(-1, "rdm_op_poly3_rowsums: m = %d, n = %d; at least one row each", m, n);
    if (groups < 1 || groups > METRIC_MAX_GROUPS)
        return c->fail(-1, "rdm_op_poly3_rowsums: groups = %d; one launch takes 1 to %d groups", groups, METRIC_MAX_GROUPS);
    if (!probe || !ref || !rowsum_out) return c->fail(-1, "rdm_op_poly3_rowsums: null argument");
    RDM_TRY(metric_dim_check(c, "rdm_op_poly3_rowsums", d));
    if ((long long)groups * (m > n ? m : n) > 2147483647LL)
        return c->fail(-1, "rdm_op_poly3_rowsums: groups = %d times max(m, n) = %d rows does not fit an int", groups, m > n ? m : n);
    RDM_CHECK_HIP(c, launch_metric_poly3_rowsums(probe, m, ref, n, d, groups, exclude_same_index, gamma, coef0, rowsum_out, c->stream));
    return 0;
}
// ---- backward ops (kernels in backward.hip)
int rdm_op_conv3x3_dgrad(rdm_ctx* c, const void* dy, const void* w, void* dx, int B, int H, int W, int C, int N) {
    RDM_ENTER(c);
    if (!dy || !w || !dx || C % 64 || N % 64) return c->fail(-1, "rdm_op_conv3x3_dgrad: null argument or channel counts not multiples of 64");
    // dX = conv3x3(dY, W~): the flipped, transposed filter through the FORWARD kernel (input channels N, output channels C)
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, (size_t)N * 9 * C * 2));
    RDM_CHECK_HIP(c, launch_conv_w_dgrad((const bf16_t*)w, (bf16_t*)c->bwd_tmp, N, C, c->stream));
    return rdm_op_conv3x3(c, dy, nullptr, N, 0, c->bwd_tmp, nullptr, nullptr, 0, nullptr, dx, B, H, W, C, 1, 0);
}
int rdm_op_conv3x3_wgrad(rdm_ctx* c, const void* x, const void* dy, float* dw, int B, int H, int W, int C, int N) {
    RDM_ENTER(c);
    if (!x || !dy || !dw || !conv_wgrad_args_ok(B, H, W, C, N)) return c->fail(-1, "rdm_op_conv3x3_wgrad: bad arguments (B, H, W, N >= 1, C even)");
    if (conv_wgrad_plan(B, H, W, C, N).path != RDM_WGRAD_CONV_FALLBACK) {
        RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, conv_wgrad_tn_scratch_bytes(B, H, W, C, N) + 256));
        RDM_CHECK_HIP(c, launch_wgrad_tn((const bf16_t*)dy, (const bf16_t*)x, dw, (long long)B * H * W, N, C, 9, H, W, c->bwd_tmp, c->zero_page, c->stream));
        return 0;
    }
    const size_t need = conv_wgrad_scratch_bytes(B, H, W, C, N, nullptr, nullptr, nullptr, nullptr, nullptr);
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, need));
    RDM_CHECK_HIP(c, launch_conv_wgrad((const bf16_t*)x, (const bf16_t*)dy, dw, B, H, W, C, N, c->bwd_tmp, c->zero_page, c->stream));
    return 0;
}
int rdm_op_groupnorm_bwd_add(rdm_ctx* c, const void* x, const void* dy, const float* gamma, const float* beta, int B, int HW, int C, float eps, int silu,
                             const void* residual, void* dx, float* dgamma, float* dbeta) {
    RDM_ENTER(c);
    if (!x || !dy || !gamma || !beta || !dx || !dgamma || !dbeta || C % 32) return c->fail(-1, "rdm_op_groupnorm_bwd: bad arguments");
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, groupnorm_bwd_scratch_bytes(B, HW, C, 32)));
    RDM_CHECK_HIP(c, launch_groupnorm_bwd((const bf16_t*)x, (const bf16_t*)dy, gamma, beta, B, HW, C, 32, eps, silu, (float*)c->bwd_tmp, (bf16_t*)dx,
                                          dgamma, dbeta, c->stream, (const bf16_t*)residual));
    return 0;
}
int rdm_op_groupnorm_bwd(rdm_ctx* c, const void* x, const void* dy, const float* gamma, const float* beta, int B, int HW, int C, float eps, int silu,
                         void* dx, float* dgamma, float* dbeta) {
    return rdm_op_groupnorm_bwd_add(c, x, dy, gamma, beta, B, HW, C, eps, silu, nullptr, dx, dgamma, dbeta);
}
int rdm_op_layernorm_bwd_add(rdm_ctx* c, const void* x, const void* dy, const float* gamma, int M, int C, float eps, const void* residual, void* dx,
                             float* dgamma, float* dbeta) {
    RDM_ENTER(c);
    if (!x || !dy || !gamma || !dx || !dgamma || !dbeta) return c->fail(-1, "rdm_op_layernorm_bwd: null argument");
    if (M < 1 || C < 1) return c->fail(-1, "rdm_op_layernorm_bwd: M and C must be positive");
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, (size_t)2 * ((M + 15) / 16) * C * 4));
    RDM_CHECK_HIP(c, launch_layernorm_bwd((const bf16_t*)x, (const bf16_t*)dy, gamma, M, C, eps, (float*)c->bwd_tmp, nullptr, (bf16_t*)dx, dgamma, dbeta,
                                          c->stream, (const bf16_t*)residual));
    return 0;
}
int rdm_op_layernorm_bwd(rdm_ctx* c, const void* x, const void* dy, const float* gamma, int M, int C, float eps, void* dx, float* dgamma, float* dbeta) {
    return rdm_op_layernorm_bwd_add(c, x, dy, gamma, M, C, eps, nullptr, dx, dgamma, dbeta);
}
int rdm_op_linear_wgrad(rdm_ctx* c, const void* dy, const void* a, float* dw, long long M, int N, int K) {
    RDM_ENTER(c);
    if (!dy || !a || !dw || !linear_wgrad_args_ok(M, N, K)) return c->fail(-1, "rdm_op_linear_wgrad: bad argument (N, K even)");
    if (linear_wgrad_plan(M, N, K).path != RDM_WGRAD_LINEAR_FALLBACK) {
        RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, wgrad_tn_scratch_bytes(M, N, K, 1) + 256));
        RDM_CHECK_HIP(c, launch_wgrad_tn((const bf16_t*)dy, (const bf16_t*)a, dw, M, N, K, 1, 1, 1, c->bwd_tmp, c->zero_page, c->stream));
        return 0;
    }
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, linear_wgrad_scratch_bytes(M, N, K)));
    RDM_CHECK_HIP(c, launch_linear_wgrad((const bf16_t*)dy, (const bf16_t*)a, dw, M, N, K, c->bwd_tmp, c->zero_page, c->stream));
    return 0;
}
// host only: the plan the two entry points above dispatch on, behind the shape checks they make
int rdm_wgrad_select(int conv, int B, int H, int W, int C, int N, long long M, int K, rdm_wgrad_form* out) {
    if (!out) return -1;
    *out = rdm_wgrad_form{};
    if (conv ? !conv_wgrad_args_ok(B, H, W, C, N) : !linear_wgrad_args_ok(M, N, K)) return -1;
    *out = conv ? conv_wgrad_plan(B, H, W, C, N) : linear_wgrad_plan(M, N, K);
    return 0;
}
int rdm_op_colsum(rdm_ctx* c, const void* x, float* out, long long M, int N) {
    RDM_ENTER(c);
    if (!x || !out) return c->fail(-1, "rdm_op_colsum: null argument");
    if (M < 1 || N < 1) return c->fail(-1, "rdm_op_colsum: M and N must be positive");
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, colsum_scratch_bytes(M, N) + 256));
    RDM_CHECK_HIP(c, launch_colsum((const bf16_t*)x, out, M, N, c->stream, (float*)c->bwd_tmp));
    return 0;
}
int rdm_op_transpose(rdm_ctx* c, const void* x, void* y, int rows, int cols) {
    RDM_ENTER(c);
    if (!x || !y) return c->fail(-1, "rdm_op_transpose: null argument");
    if (rows < 1 || cols < 1) return c->fail(-1, "rdm_op_transpose: rows and cols must be positive");
    RDM_CHECK_HIP(c, launch_transpose_bf16((const bf16_t*)x, (bf16_t*)y, rows, cols, c->stream));
    return 0;
}
int rdm_op_add(rdm_ctx* c, const void* a, const void* b, void* out, long long n) {
    RDM_ENTER(c);
    if (!a || !b || !out) return c->fail(-1, "rdm_op_add: null argument");
    if (n < 1) return c->fail(-1, "rdm_op_add: n must be positive");
    RDM_CHECK_HIP(c, launch_add_bf16((const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out, n, c->stream));
    return 0;
}
int rdm_op_ema(rdm_ctx* c, float* shadow, const float* p, long long n, float one_minus_decay) {
    RDM_ENTER(c);
    if (!shadow || !p || n < 1) return c->fail(-1, "rdm_op_ema: bad argument");
    RDM_CHECK_HIP(c, launch_ema(shadow, p, n, one_minus_decay, c->stream));
    return 0;
}
int rdm_op_silu(rdm_ctx* c, const float* x, const float* dy, void* out, long long n) {
    RDM_ENTER(c);
    if (!x || !out || n < 1) return c->fail(-1, "rdm_op_silu: bad argument");
    RDM_CHECK_HIP(c, launch_silu(x, dy, dy ? nullptr : (bf16_t*)out, dy ? (float*)out : nullptr, n, c->stream));
    return 0;
}
int rdm_op_q_sample(rdm_ctx* c, const float* x0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac, float* out, void* out_nhwc, int B, int C,
                    int H, int W, int cpad) {
    RDM_ENTER(c);
    if (!x0 || !noise || !sqrt_ac || !sqrt_1mac || (!out && !out_nhwc) || B < 1 || C < 1 || H < 1 || W < 1) return c->fail(-1, "rdm_op_q_sample: bad argument");
    RDM_CHECK_HIP(c, launch_q_sample(x0, noise, sqrt_ac, sqrt_1mac, out, (bf16_t*)out_nhwc, B, C, H * W, cpad, c->stream));
    return 0;
}
int rdm_op_mse_loss(rdm_ctx* c, const void* eps_nhwc, const float* target, const float* coef, float* se, void* deps_nhwc, int B, int C, int H, int W, int ldc) {
    RDM_ENTER(c);
    if (!eps_nhwc || !target || !se || (deps_nhwc && !coef) || B < 1 || C < 1 || ldc < C) return c->fail(-1, "rdm_op_mse_loss: bad argument");
    RDM_CHECK_HIP(c, launch_mse_loss((const bf16_t*)eps_nhwc, target, coef, se, (bf16_t*)deps_nhwc, B, C, H * W, ldc, c->stream));
    return 0;
}
int rdm_op_where_rows(rdm_ctx* c, const unsigned char* mask, const float* a, const float* x, float* out, long long rows, long long n) {
    RDM_ENTER(c);
    if (!mask || !a || !x || !out || rows < 1 || n < 1) return c->fail(-1, "rdm_op_where_rows: bad argument");
    RDM_CHECK_HIP(c, launch_where_rows(mask, a, x, out, rows, n, c->stream));
    return 0;
}
int rdm_op_timestep_embedding(rdm_ctx* c, const int64_t* t, void* out_bf16, int B, int dim, int ld) {
    RDM_ENTER(c);
    if (!t || !out_bf16 || B < 1 || dim < 2 || dim % 2 || ld < dim) return c->fail(-1, "rdm_op_timestep_embedding: bad argument");
    RDM_CHECK_HIP(c, launch_timestep_embedding((const long long*)t, (bf16_t*)out_bf16, B, dim, ld, c->stream));
    return 0;
}
int rdm_op_colsum_samples(rdm_ctx* c, const void* x, void* out, int B, int HW, int N) {
    RDM_ENTER(c);
    if (!x || !out || B < 1 || HW < 1 || N < 1) return c->fail(-1, "rdm_op_colsum_samples: bad argument");
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, colsum_samples_scratch_bytes(B, HW, N)));
    RDM_CHECK_HIP(c, launch_colsum_samples((const bf16_t*)x, (bf16_t*)out, B, HW, N, c->stream, (float*)c->bwd_tmp));
    return 0;
}
int rdm_op_expand2(rdm_ctx* c, const void* x, void* out, int B, int H, int W, int C, int mode) {
    RDM_ENTER(c);
    if (!x || !out || B < 1 || H < 1 || W < 1 || C < 8 || C % 8 || (mode != 0 && mode != 1)) return c->fail(-1, "rdm_op_expand2: bad argument (C %% 8 == 0, mode 0 / 1)");
    RDM_CHECK_HIP(c, launch_expand2((const bf16_t*)x, (bf16_t*)out, B, H, W, C, mode, c->stream));
    return 0;
}
int rdm_op_sumpool2(rdm_ctx* c, const void* x, void* out, int B, int H, int W, int C) {
    RDM_ENTER(c);
    if (!x || !out || B < 1 || H < 1 || W < 1 || C < 8 || C % 8) return c->fail(-1, "rdm_op_sumpool2: bad argument (C must be a multiple of 8)");
    RDM_CHECK_HIP(c, launch_sumpool2((const bf16_t*)x, (bf16_t*)out, B, H, W, C, c->stream));
    return 0;
}
int rdm_op_adamw(rdm_ctx* c, float* p, const float* g, float* m, float* v, void* p_bf16, long long n, double lr, double beta1, double beta2, double eps,
                 double weight_decay, int step) {
    RDM_ENTER(c);
    if (!p || !g || !m || !v || n < 1 || step < 1) return c->fail(-1, "rdm_op_adamw: bad argument");
    RDM_CHECK_HIP(c, launch_adamw(p, g, m, v, (bf16_t*)p_bf16, n, lr, beta1, beta2, eps, weight_decay, step, c->stream));
    return 0;
}
int rdm_op_adamw_multi(rdm_ctx* c, int n, float* const* p, const float* const* g, float* const* m, float* const* v, void* const* p_bf16, const long long* numel,
                       double lr, double beta1, double beta2, double eps, double weight_decay, int step) {
    RDM_ENTER(c);
    if (n < 1 || !p || !g || !m || !v || !numel || step < 1) return c->fail(-1, "rdm_op_adamw_multi: bad argument");
    for (int i = 0; i < n; i++) if (!p[i] || !g[i] || !m[i] || !v[i] || numel[i] < 1) return c->fail(-1, "rdm_op_adamw_multi: null tensor in the list");
    RDM_CHECK_HIP(c, launch_multi_tensor(n, p, g, m, v, p_bf16, numel, 0, lr, beta1, beta2, eps, weight_decay, step, 0.f, c->stream));
    return 0;
}
int rdm_op_ema_multi(rdm_ctx* c, int n, float* const* shadow, const float* const* param, const long long* numel, float one_minus_decay) {
    RDM_ENTER(c);
    if (n < 1 || !shadow || !param || !numel) return c->fail(-1, "rdm_op_ema_multi: bad argument");
    for (int i = 0; i < n; i++) if (!shadow[i] || !param[i] || numel[i] < 1) return c->fail(-1, "rdm_op_ema_multi: null tensor in the list");
    RDM_CHECK_HIP(c, launch_multi_tensor(n, shadow, param, nullptr, nullptr, nullptr, numel, 1, 0.0, 0.0, 0.0, 0.0, 0.0, 1, one_minus_decay, c->stream));
    return 0;
}
int rdm_op_attention_bwd(rdm_ctx* c, const void* q, const void* k, const void* v, const void* o, const void* dout, int B, int n, int m, int heads,
                         void* dq, void* dk, void* dv) {
    RDM_ENTER(c);
    if (!q || !k || !v || !o || !dout || !dq || !dk || !dv || B < 1 || heads < 1 || n < 32 || m < 32 || n % 32 || m % 32)
        return c->fail(-1, "rdm_op_attention_bwd: bad argument (d_head = 32; n and m multiples of 32)");
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, attn_bwd_scratch_bytes(B, heads, n, m)));
    RDM_CHECK_HIP(c, launch_attention_bwd((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)o, (const bf16_t*)dout, B, n, m, heads,
                                          (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, c->bwd_tmp, c->stream));
    return 0;
}
int rdm_op_small_attention_bwd(rdm_ctx* c, const void* q, int ldq, const void* k, const void* v, int ldkv, const void* dout, int ldo, int B, int nq, int nkv,
                               int heads, float scale, void* dq, void* dk, void* dv) {
    RDM_ENTER(c);
    if (!q || !k || !v || !dout || !dq || !dk || !dv || B < 1 || heads < 1 || nq < 1 || nkv < 1 || nkv > 32)
        return c->fail(-1, "rdm_op_small_attention_bwd: bad argument (d_head = 32, 1..32 keys)");
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, small_attention_bwd_scratch_bytes(B, heads, nq, nkv)));
    RDM_CHECK_HIP(c, launch_small_attention_bwd((const bf16_t*)q, ldq, (const bf16_t*)k, (const bf16_t*)v, ldkv, (const bf16_t*)dout, ldo, B, nq, nkv, heads, scale,
                                                (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, c->bwd_tmp, c->stream));
    return 0;
}
int rdm_op_bmm(rdm_ctx* c, const void* a, const void* w, void* out_bf16, float* out_f32, int batch, int M, int N, int K, float alpha) {
    RDM_ENTER(c);
    if (!a || !w || (!out_bf16 && !out_f32) || batch < 1 || M < 1 || N < 2 || K < 64 || K % 64 || N % 2)
        return c->fail(-1, "rdm_op_bmm: bad argument (K must be a multiple of 64, N even)");
    IgemmParams p = igemm_plain(M, N, K, c->zero_page);
    p.alpha = alpha; p.A0 = (const bf16_t*)a; p.C0 = K; p.W = (const bf16_t*)w; p.out_bf16 = (bf16_t*)out_bf16; p.out_f32 = out_f32;
    p.sA = (long long)M * K; p.sW = (long long)N * K; p.sO = (long long)M * N;
    RDM_CHECK_HIP(c, launch_igemm(p, false, batch, c->stream));
    return 0;
}
int rdm_op_heads(rdm_ctx* c, const void* x, void* out, int B, int n, int H, int D, int ldx, int mode) {
    RDM_ENTER(c);
    if (!x || !out || B < 1 || n < 1 || H < 1) return c->fail(-1, "rdm_op_heads: bad argument");
    if (D < 1 || D > 64) return c->fail(-1, "rdm_op_heads: D must be in 1..64");
    if (mode < 0 || mode > 2) return c->fail(-1, "rdm_op_heads: mode must be 0, 1 or 2");
    if (mode != 2 && (long long)ldx < (long long)H * D) return c->fail(-1, "rdm_op_heads: ldx must be at least H * D");
    RDM_CHECK_HIP(c, launch_heads((const bf16_t*)x, (bf16_t*)out, B, n, H, D, ldx, mode, c->stream));
    return 0;
}
int rdm_op_transpose_batched(rdm_ctx* c, const void* x, void* y, int batch, int rows, int cols) {
    RDM_ENTER(c);
    if (!x || !y || batch < 1 || batch > 65535) return c->fail(-1, "rdm_op_transpose_batched: bad argument");
    if (rows < 1 || cols < 1) return c->fail(-1, "rdm_op_transpose_batched: rows and cols must be positive");
    RDM_CHECK_HIP(c, launch_transpose_bf16((const bf16_t*)x, (bf16_t*)y, rows, cols, c->stream, batch));
    return 0;
}
int rdm_op_softmax(rdm_ctx* c, const float* s, void* p_bf16, long long rows, int n, int n_valid) {
    RDM_ENTER(c);
    if (!s || !p_bf16 || n % 4) return c->fail(-1, "rdm_op_softmax: bad argument (n must be a multiple of 4)");
    if (rows < 1 || n < 4) return c->fail(-1, "rdm_op_softmax: rows and n must be positive");
    if (n_valid < 0 || n_valid > n) return c->fail(-1, "rdm_op_softmax: n_valid must be in 0..n (0: all columns valid)");
    RDM_CHECK_HIP(c, launch_softmax_rows(s, (bf16_t*)p_bf16, rows, n, c->stream, n_valid));
    return 0;
}
int rdm_op_softmax_bwd(rdm_ctx* c, const void* p_bf16, const float* dp, void* ds_bf16, long long rows, int n) {
    RDM_ENTER(c);
    if (!p_bf16 || !dp || !ds_bf16 || n % 4) return c->fail(-1, "rdm_op_softmax_bwd: bad argument (n must be a multiple of 4)");
    RDM_CHECK_HIP(c, launch_softmax_bwd((const bf16_t*)p_bf16, dp, (bf16_t*)ds_bf16, rows, n, c->stream));
    return 0;
}
int rdm_op_geglu(rdm_ctx* c, const void* pre, const void* dh, void* out, long long M, int F) {
    RDM_ENTER(c);
    if (!pre || !out || M < 1 || F < 8 || F % 8) return c->fail(-1, "rdm_op_geglu: bad argument (F must be a positive multiple of 8)");
    RDM_CHECK_HIP(c, launch_geglu((const bf16_t*)pre, (const bf16_t*)dh, (bf16_t*)out, M, F, c->stream));
    return 0;
}
int rdm_op_groupnorm(rdm_ctx* c, const void* x0, const void* x1, int C0, int C1, int B, int HW, const float* gamma,
                     const float* beta, float eps, int silu, void* out) {
    RDM_ENTER(c);
    RDM_TRY(ensure_gn_partial(c, B));
    Ops o = op_exec(c);
    o.groupnorm({.x0 = (const bf16_t*)x0, .x1 = (const bf16_t*)x1, .C0 = C0, .C1 = C1, .HW = HW, .B = B, .gamma = gamma, .beta = beta, .eps = eps, .silu = silu,
                 .out = (bf16_t*)out});
    return o.rc;
}
int rdm_op_layernorm(rdm_ctx* c, const void* x, int in_is_f32, const float* gamma, const float* beta, int M, int C, float eps,
                     void* out) {
    RDM_ENTER(c);
    Ops o = op_exec(c);
    o.layernorm({.x_f32 = in_is_f32 ? (const float*)x : nullptr, .x_bf16 = in_is_f32 ? nullptr : (const bf16_t*)x, .gamma = gamma, .beta = beta, .M = M, .C = C,
                 .out_bf16 = (bf16_t*)out, .eps = eps});
    return o.rc;
}
// the CLIP towers' forms (first_stage.hip clip_tower / clip_image_body): fp32 rows normalised to fp32 (visual.ln_pre), and a projection
// added into the fp32 residual stream (x += out_proj(attn), x += c_proj(h): out_f32 may be res_f32 itself)
int rdm_op_layernorm_f32(rdm_ctx* c, const float* x, const float* gamma, const float* beta, int M, int C, float eps, float* out) {
    RDM_ENTER(c);
    if (!x || !gamma || !beta || !out || M < 1 || C < 2) return c->fail(-1, "rdm_op_layernorm_f32: null argument or M < 1, C < 2");
    Ops o = op_exec(c);
    o.layernorm({.x_f32 = x, .gamma = gamma, .beta = beta, .M = M, .C = C, .out_f32 = out, .eps = eps});
    return o.rc;
}
int rdm_op_linear_res_f32(rdm_ctx* c, const void* a, const void* w, const float* bias, const float* res_f32, float* out_f32, int M, int N, int K, int act) {
    RDM_ENTER(c);
    if (!a || !w || !out_f32) return c->fail(-1, "rdm_op_linear_res_f32: a, w and out_f32 required");
    if (M < 1 || N < 2 || N % 2 || K < 64 || K % 64 || (act != ACT_NONE && act != ACT_QUICKGELU && act != ACT_SILU))
        return c->fail(-1, "rdm_op_linear_res_f32: bad shape M=%d N=%d K=%d act=%d (N even, K a multiple of 64; no activation, QuickGELU or SiLU)", M, N, K, act);
    Ops o = op_exec(c);
    o.linear({.A0 = (const bf16_t*)a, .C0 = K, .W = (const bf16_t*)w, .bias = bias, .M = M, .N = N, .act = act, .res_f32 = res_f32, .out_f32 = out_f32});
    return o.rc;
}
int rdm_op_self_attention(rdm_ctx* c, const void* qk, const void* vt, int B, int n, int heads, void* out) {
    RDM_ENTER(c);
    Ops o = op_exec(c);
    o.flash_d32({.q = (const bf16_t*)qk, .ldq = 2 * heads * 32, .vt = (const bf16_t*)vt, .out = (bf16_t*)out, .n = n}, heads, B);
    return o.rc;
}
int rdm_op_self_attention_qkv(rdm_ctx* c, const void* qkv, int B, int n, int heads, void* out) {
    RDM_ENTER(c);
    if (n % 64 != 0) return c->fail(-3, "rdm_op_self_attention_qkv: n = %d must be a multiple of 64 (token-major V is read by the LDS-shared kernel only)", n);
    Ops o = op_exec(c);
    o.flash_d32({.q = (const bf16_t*)qkv, .ldq = 3 * heads * 32, .v = (const bf16_t*)qkv + 2 * heads * 32, .out = (bf16_t*)out, .n = n}, heads, B);
    return o.rc;
}
// G / U arrive in their natural layout: their fragment-ordered images are packed per call into bwd_tmp
static int op_xattn_fused(rdm_ctx* c, XattnParams q, int B) {      // q.G / q.U: the natural layout
    const size_t img = (size_t)B * q.NP * q.C;
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, 2 * img * 2));
    bf16_t* Gp = (bf16_t*)c->bwd_tmp; bf16_t* Up = Gp + img;
    Ops o = op_exec(c);
    o.check(launch_xattn_pack(q.G, q.U, Gp, Up, B, q.NP, q.C, c->stream), "xattn pack");
    q.G = Gp; q.U = Up;
    o.xattn_fused(q);
    return o.rc;
}
int rdm_op_xattn_fused(rdm_ctx* c, const void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G, const void* U,
                       const float* bias, const void* res, int B, int n, int C, int NP, int ncols, int group, void* out) {
    RDM_ENTER(c);
    if ((ln_gamma != nullptr) != (ln_beta != nullptr) || (ln_gamma && res)) return c->fail(-3, "rdm_op_xattn_fused: LayerNorm needs gamma and beta, and then the residual is x itself (res must be null)");
    const XattnParams q{.x = (const bf16_t*)x, .G = (const bf16_t*)G, .U = (const bf16_t*)U, .bias = bias, .res = (const bf16_t*)res, .out = (bf16_t*)out,
                        .rows = B * n, .n = n, .C = C, .NP = NP, .ncols = ncols, .group = group, .ln_g = ln_gamma, .ln_b = ln_beta, .ln_eps = ln_eps};
    if (!xattn_fused_supported(q)) return c->fail(-3, "rdm_op_xattn_fused: unsupported shape (n %% 32, C %% 64, NP %% 32, ncols <= min(NP, 128), group 1 / 2 / 4): n %d C %d NP %d ncols %d group %d", n, C, NP, ncols, group);
    return op_xattn_fused(c, q, B);
}
int rdm_op_xattn_fused_ln3(rdm_ctx* c, void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G, const void* U,
                           const float* bias, int B, int n, int C, int NP, int ncols, int group, const float* ln3_gamma, const float* ln3_beta, void* ln3_out) {
    RDM_ENTER(c);
    if (!x || !ln_gamma || !ln_beta || !ln3_gamma || !ln3_beta || !ln3_out) return c->fail(-1, "rdm_op_xattn_fused_ln3: null argument");
    const XattnParams q{.x = (const bf16_t*)x, .G = (const bf16_t*)G, .U = (const bf16_t*)U, .bias = bias, .out = (bf16_t*)x,
                        .rows = B * n, .n = n, .C = C, .NP = NP, .ncols = ncols, .group = group, .ln_g = ln_gamma, .ln_b = ln_beta, .ln_eps = ln_eps,
                        .ln3_g = ln3_gamma, .ln3_b = ln3_beta, .ln3_out = (bf16_t*)ln3_out};
    if (!xattn_fused_supported(q)) return c->fail(-3, "rdm_op_xattn_fused_ln3: unsupported shape: n %d C %d NP %d ncols %d group %d", n, C, NP, ncols, group);
    return op_xattn_fused(c, q, B);
}
int rdm_op_xattn_fused_biased(rdm_ctx* c, void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G, const void* U,
                              const float* bias, const void* res, int B, int n, int C, int NP, int ncols, int group, void* out,
                              const float* ln3_gamma, const float* ln3_beta, void* ln3_out, const float* key_bias) {
    RDM_ENTER(c);
    if (!key_bias) return c->fail(-1, "rdm_op_xattn_fused_biased: key_bias is null (the unbiased entries are rdm_op_xattn_fused / _ln3)");
    if ((ln_gamma != nullptr) != (ln_beta != nullptr) || (ln_gamma && res)) return c->fail(-3, "rdm_op_xattn_fused_biased: LayerNorm needs gamma and beta, and then the residual is x itself (res must be null)");
    if (ln3_out && (!x || !ln_gamma || !ln3_gamma || !ln3_beta || (out && out != x)))
        return c->fail(-1, "rdm_op_xattn_fused_biased: the norm3 form runs in place on x with ln_gamma, ln_beta, ln3_gamma and ln3_beta given (out: x or null)");
    if (!ln3_out && !out) return c->fail(-1, "rdm_op_xattn_fused_biased: out is null");
    const XattnParams q{.x = (const bf16_t*)x, .G = (const bf16_t*)G, .U = (const bf16_t*)U, .bias = bias, .res = (const bf16_t*)res,
                        .out = ln3_out ? (bf16_t*)x : (bf16_t*)out, .rows = B * n, .n = n, .C = C, .NP = NP, .ncols = ncols, .group = group,
                        .ln_g = ln_gamma, .ln_b = ln_beta, .ln_eps = ln_eps, .ln3_g = ln3_out ? ln3_gamma : nullptr, .ln3_b = ln3_out ? ln3_beta : nullptr,
                        .ln3_out = (bf16_t*)ln3_out, .key_bias = key_bias};
    if (!xattn_fused_supported(q)) return c->fail(-3, "rdm_op_xattn_fused_biased: unsupported shape (n %% 32, C %% 64, NP %% 32, ncols <= min(NP, 128), group 1 / 2 / 4): n %d C %d NP %d ncols %d group %d", n, C, NP, ncols, group);
    return op_xattn_fused(c, q, B);
}
int rdm_op_head_conv(rdm_ctx* c, const void* x, const float* gn_gamma, const float* gn_beta, float gn_eps, const float* w, const float* bias,
                     int B, int H, int W, int C, int Cout, float* out) {
    RDM_ENTER(c);
    if ((gn_gamma != nullptr) != (gn_beta != nullptr)) return c->fail(-3, "rdm_op_head_conv: GroupNorm needs gamma and beta");
    if (gn_gamma) RDM_TRY(ensure_gn_partial(c, B));
    Ops o = op_exec(c);
    HeadParams hp{.x = (const bf16_t*)x, .B = B, .H = H, .W = W, .C = C, .gamma = gn_gamma, .beta = gn_beta, .eps = gn_eps, .w = w, .bias = bias, .out = out, .Cout = Cout};
    if (!head_conv_supported(o.head_params(hp)))
        return c->fail(-3, "rdm_op_head_conv: unsupported shape (C %% 32, C <= 240, W %% 32, H %% 2, Cout <= 8, C %% 32 groups): C %d H %d W %d Cout %d", C, H, W, Cout);
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, head_conv_wp_bytes(C)));
    hp.wp = (bf16_t*)c->bwd_tmp;
    o.head(hp);             // (the fused kernel takes it: no GroupNorm-apply scratch)
    return o.rc;
}
int rdm_op_causal_attention_d64(rdm_ctx* c, const void* qkv, int ldq, int B, int n, int heads, float scale, void* out, int ldo, void* kcache,
                                void* vcache, int L) {
    RDM_ENTER(c);
    if (!qkv || !out) return c->fail(-1, "rdm_op_causal_attention_d64: null argument");
    if (B < 1 || n < 1 || n > 1024 || heads < 1) return c->fail(-1, "rdm_op_causal_attention_d64: bad shape B=%d n=%d heads=%d (1 <= n <= 1024)", B, n, heads);
    if ((kcache != nullptr) != (vcache != nullptr) || (kcache && L < n))
        return c->fail(-1, "rdm_op_causal_attention_d64: kcache and vcache come together, with L >= n (L=%d, n=%d)", L, n);
    Ops o = op_exec(c);
    o.causal_d64({.qkv = (const bf16_t*)qkv, .ldq = ldq, .out = (bf16_t*)out, .ldo = ldo, .n = n, .kcache = (bf16_t*)kcache, .vcache = (bf16_t*)vcache, .L = L},
                 heads, B, scale);
    return o.rc;
}
int rdm_op_vq_attention(rdm_ctx* c, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* bias_v, int B, int n, int C, float scale,
                        void* out, int ldo) {
    RDM_ENTER(c);
    if (B < 1 || n < 1) return c->fail(-1, "rdm_op_vq_attention: bad shape B=%d n=%d (B >= 1, n >= 1)", B, n);
    if (!q || !k || !v || !out) return c->fail(-1, "rdm_op_vq_attention: null argument");
    if (!vq_attn_stream_supported(C)) return c->fail(-1, "rdm_op_vq_attention: C=%d must be a multiple of 128, at most 512", C);
    if (ldq % 8 || ldq < C || ldk % 8 || ldk < C || ldv % 8 || ldv < C || ldo % 4 || ldo < C)
        return c->fail(-1, "rdm_op_vq_attention: bad row pitch (ldq=%d, ldk=%d, ldv=%d: multiples of 8; ldo=%d: a multiple of 4; each at least C=%d)", ldq, ldk, ldv, ldo, C);
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 || (uintptr_t)out % 8)
        return c->fail(-1, "rdm_op_vq_attention: q, k and v must be 16-byte aligned, out 8-byte aligned");
    if ((long long)B * ((n + 63) / 64) > 0x7fffffffLL) return c->fail(-1, "rdm_op_vq_attention: B=%d x n=%d is more than one launch takes", B, n);
    Ops o = op_exec(c);
    o.vq_attention({.q = (const bf16_t*)q, .ldq = ldq, .k = (const bf16_t*)k, .ldk = ldk, .v = (const bf16_t*)v, .ldv = ldv, .bias = bias_v, .out = (bf16_t*)out, .ldo = ldo,
                    .n = n, .C = C, .scale = scale}, B);
    return o.rc;
}
int rdm_op_causal_attention_d64_bwd(rdm_ctx* c, const void* qkv, int ldq, const void* out, int ldo, const void* dout, int lddo, int B, int n, int heads,
                                    float scale, void* dqkv, int ldd) {
    RDM_ENTER(c);
    if (!qkv || !out || !dout || !dqkv) return c->fail(-1, "rdm_op_causal_attention_d64_bwd: null argument");
    if (B < 1 || n < 1 || n > 1024 || heads < 1) return c->fail(-1, "rdm_op_causal_attention_d64_bwd: bad shape B=%d n=%d heads=%d (1 <= n <= 1024)", B, n, heads);
    const int C = heads * 64;
    if (ldq % 8 || ldq < 3 * C || lddo % 8 || lddo < C || ldo % 4 || ldo < C || ldd % 4 || ldd < 3 * C)
        return c->fail(-1, "rdm_op_causal_attention_d64_bwd: bad row pitch (ldq=%d, lddo=%d: multiples of 8; ldo=%d, ldd=%d: multiples of 4; each at least its %d or %d columns)",
                       ldq, lddo, ldo, ldd, C, 3 * C);
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, causal_attention_d64_bwd_scratch_bytes(B, heads, n)));
    RDM_CHECK_HIP(c, launch_causal_attention_d64_bwd((const bf16_t*)qkv, ldq, (const bf16_t*)out, ldo, (const bf16_t*)dout, lddo, B, n, heads, scale, (bf16_t*)dqkv, ldd,
                                                     c->bwd_tmp, c->stream));
    return 0;
}
int rdm_op_embedding_grad(rdm_ctx* c, const int64_t* tokens, const void* dy, int M, int C, int V, float* dw) {
    RDM_ENTER(c);
    if (!tokens || !dy || !dw) return c->fail(-1, "rdm_op_embedding_grad: null argument");
    if (M < 1 || C < 1 || C > 12288 || V < 1) return c->fail(-1, "rdm_op_embedding_grad: bad shape M=%d C=%d V=%d (M, V >= 1; 1 <= C <= 12288)", M, C, V);
    RDM_CHECK_HIP(c, launch_embedding_grad((const long long*)tokens, (const bf16_t*)dy, M, C, V, dw, c->stream));
    return 0;
}
int rdm_op_small_attention(rdm_ctx* c, const void* q, int ldq, const void* k, const void* v, int ldkv, int B, int nq, int nkv,
                           int heads, int D, int causal, float scale, void* out, int ldo) {
    RDM_ENTER(c);
    Ops o = op_exec(c);
    o.small_attention({.q = (const bf16_t*)q, .ldq = ldq, .k = (const bf16_t*)k, .ldk = ldkv, .v = (const bf16_t*)v, .ldv = ldkv, .out = (bf16_t*)out, .ldo = ldo,
                       .nq = nq, .nkv = nkv, .causal = causal, .scale = scale}, D, heads, B, "small attention");
    return o.rc;
}
int rdm_op_small_attention_biased(rdm_ctx* c, const void* q, int ldq, const void* k, const void* v, int ldkv, int B, int nq, int nkv,
                                  int heads, int D, int causal, float scale, void* out, int ldo, const float* key_bias) {
    RDM_ENTER(c);
    if (!key_bias) return c->fail(-1, "rdm_op_small_attention_biased: key_bias is null (the unbiased entry is rdm_op_small_attention)");
    if (causal) return c->fail(-1, "rdm_op_small_attention_biased: a key bias does not combine with the causal mask");
    Ops o = op_exec(c);
    o.small_attention({.q = (const bf16_t*)q, .ldq = ldq, .k = (const bf16_t*)k, .ldk = ldkv, .v = (const bf16_t*)v, .ldv = ldkv, .out = (bf16_t*)out, .ldo = ldo,
                       .nq = nq, .nkv = nkv, .causal = 0, .scale = scale, .key_bias = key_bias}, D, heads, B, "small attention (biased)");
    return o.rc;
}
int rdm_op_conv_in(rdm_ctx* c, const float* x, const float* w, const float* bias, int B, int Cin, int H, int W, int Cout, void* out) {
    RDM_ENTER(c);
    if (!x || !w || !bias || !out) return c->fail(-1, "rdm_op_conv_in: null argument");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W * 5 >= (1ll << 30) || Cin < 1 || Cin > 4 || Cout < 8 || Cout % 8 || ((Cin <= 3 ? 3 : 4) * 9 + 1) * (long long)Cout * 4 > 96 * 1024)
        return c->fail(-3, "rdm_op_conv_in: unsupported shape (1 <= Cin <= 4, Cout %% 8, weights + bias within 96 KB of LDS): B %d Cin %d H %d W %d Cout %d", B, Cin, H, W, Cout);
    RDM_CHECK_HIP(c, launch_conv_in(x, w, bias, (bf16_t*)out, B, Cin, H, W, Cout, c->stream));
    return 0;
}
int rdm_op_conv_out(rdm_ctx* c, const void* x, const float* w, const float* bias, int B, int H, int W, int Cin, int Cout, float* out) {
    RDM_ENTER(c);
    if (!x || !w || !bias || !out) return c->fail(-1, "rdm_op_conv_out: null argument");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W >= (1ll << 31) || Cin < 64 || Cin % 64 || Cout < 1 || Cout > 4 || (long long)Cout * 9 * Cin * 4 > 64 * 1024)
        return c->fail(-3, "rdm_op_conv_out: unsupported shape (Cin %% 64, 1 <= Cout <= 4, weights within 64 KB of LDS): B %d H %d W %d Cin %d Cout %d", B, H, W, Cin, Cout);
    RDM_CHECK_HIP(c, launch_conv_out((const bf16_t*)x, w, bias, (float*)out, B, H, W, Cin, Cout, c->stream));
    return 0;
}

// ---- the token sampler alone
static int op_rarm_sampler_run(rdm_ctx* c, const float* logits, int b, int vocab, int cfg, float guidance_scale, float temperature, int top_k,
                               float top_p, const float* uniforms, int64_t* tokens_out, int32_t* kept_out) {
    RDM_ENTER(c);
    if (!logits || !uniforms || !tokens_out || b < 1 || vocab < 1) return c->fail(-1, "rdm_op_rarm_sampler: bad arguments");
    if (!(temperature > 0.f)) return c->fail(-1, "rdm_op_rarm_sampler: temperature must be positive");
    RDM_TRY(ensure_bytes(c, &c->samp, &c->samp_bytes, (size_t)b * 8 + 64));
    int* pos = (int*)c->samp; int* done = pos + 1; long long* next = (long long*)(c->samp + 64);
    RDM_CHECK_HIP(c, launch_set_int(pos, 0, c->stream));
    RDM_CHECK_HIP(c, launch_set_int(done, 0, c->stream));
    RarmSampleParams sp{}; sp.logits = logits; sp.vocab = vocab; sp.B = b; sp.cfg = cfg ? 1 : 0; sp.scale = guidance_scale; sp.temperature = temperature;
    sp.top_k = top_k > 0 ? top_k : vocab; sp.uniforms = uniforms; sp.pos = pos; sp.pos0 = 0; sp.steps = 1; sp.tokens_out = (long long*)tokens_out;
    sp.next_tokens = next; sp.done = done; sp.top_p = top_p; sp.kept_out = kept_out;
    RDM_CHECK_HIP(c, launch_rarm_sample(sp, c->stream));
    return 0;
}
int rdm_op_rarm_sampler(rdm_ctx* c, const float* logits, int b, int vocab, int cfg, float guidance_scale, float temperature, int top_k,
                        const float* uniforms, int64_t* tokens_out) {
    return op_rarm_sampler_run(c, logits, b, vocab, cfg, guidance_scale, temperature, top_k, 1.0f, uniforms, tokens_out, nullptr);
}
int rdm_op_rarm_sampler_top_p(rdm_ctx* c, const float* logits, int b, int vocab, int cfg, float guidance_scale, float temperature, int top_k,
                              float top_p, const float* uniforms, int64_t* tokens_out, int32_t* kept_out) {
    RDM_ENTER(c);
    if (!(top_p > 0.f && top_p <= 1.f)) return c->fail(-1, "rdm_op_rarm_sampler_top_p: top_p must lie in (0, 1], got %g", (double)top_p);
    return op_rarm_sampler_run(c, logits, b, vocab, cfg, guidance_scale, temperature, top_k, top_p, uniforms, tokens_out, kept_out);
}
// ---- the decode step's kernels one at a time (tests/test_gpu_decode_ops.py): argument checks, then the launch rarm_step makes
int rdm_op_linear_rows(rdm_ctx* c, const void* a, const float* ln_x, const float* gamma, const float* beta, const void* w, const float* bias,
                       const float* res_f32, void* out_bf16, float* out_f32, int M, int N, int K, int act) {
    RDM_ENTER(c);
    if (!w || (a != nullptr) == (ln_x != nullptr) || (!out_bf16 && !out_f32)) return c->fail(-1, "rdm_op_linear_rows: w, exactly one of a / ln_x and an output required");
    if (M < 1 || N < 1 || K < 8 || K % 8 || act < ACT_NONE || act > ACT_SILU || (act == ACT_GEGLU && N % 2))
        return c->fail(-1, "rdm_op_linear_rows: bad shape M=%d N=%d K=%d act=%d (K a multiple of 8; GEGLU: N even)", M, N, K, act);
    Ops o = op_exec(c);
    const LinearOp op{.A0 = (const bf16_t*)a, .C0 = K, .ln_x = ln_x, .ln_g = gamma, .ln_b = beta, .W = (const bf16_t*)w, .bias = bias, .M = M, .N = N, .act = act,
                      .res_f32 = res_f32, .out_bf16 = (bf16_t*)out_bf16, .out_f32 = out_f32, .single_row = true};
    if (ln_x) {
        if (!gamma || !beta || !out_bf16 || out_f32 || res_f32) return c->fail(-1, "rdm_op_linear_rows: the LayerNorm form takes gamma, beta and a bf16 output, no residual");
        if (!o.linear_ln(op))
            return c->fail(-5, "rdm_op_linear_rows: shape not taken by the LayerNorm-in-kernel form (M=%d N=%d K=%d act=%d, %s mode)", M, N, K, act,
                           c->deterministic ? "deterministic" : "fast");
        return o.rc;
    }
    o.linear(op);
    return o.rc;
}
static int op_pos_slot(rdm_ctx* c, int pos, int** slot) {      // the device step counter of the decode kernels, set on the stream
    RDM_TRY(ensure_bytes(c, &c->samp, &c->samp_bytes, 64));
    *slot = (int*)c->samp;
    RDM_CHECK_HIP(c, launch_set_int(*slot, pos, c->stream));
    return 0;
}
int rdm_op_rarm_decode_attention(rdm_ctx* c, const void* q, int ldq, const void* k_new, const void* v_new, void* kcache, void* vcache, long long batch_stride,
                                 int row_stride, long long head_stride, int nkv, int pos, float scale, void* out, int ldo, int heads, int batch) {
    RDM_ENTER(c);
    if (!q || !kcache || !vcache || !out) return c->fail(-1, "rdm_op_rarm_decode_attention: null argument");
    if ((k_new != nullptr) != (v_new != nullptr)) return c->fail(-1, "rdm_op_rarm_decode_attention: k_new and v_new come together");
    if (heads < 1 || batch < 1 || batch > 65535 || nkv < 1 || nkv > 1024)
        return c->fail(-1, "rdm_op_rarm_decode_attention: bad shape heads=%d batch=%d nkv=%d (1 <= nkv <= 1024, batch <= 65535)", heads, batch, nkv);
    if (k_new ? (pos < 0 || pos >= nkv) : pos < -1)
        return c->fail(-1, "rdm_op_rarm_decode_attention: pos=%d: 0 <= pos < nkv=%d with k_new / v_new, -1 or more without", pos, nkv);
    if (ldq % 8 || ldq < heads * 64 || ldo % 8 || ldo < heads * 64 || row_stride % 8 || row_stride < 64 || batch_stride % 8 || head_stride % 8 || head_stride < 0)
        return c->fail(-1, "rdm_op_rarm_decode_attention: bad stride (ldq=%d, ldo=%d: multiples of 8, at least %d; row_stride=%d, batch_stride=%lld, head_stride=%lld: multiples of 8)",
                       ldq, ldo, heads * 64, row_stride, batch_stride, head_stride);
    if (((uintptr_t)q | (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)out) % 16)
        return c->fail(-1, "rdm_op_rarm_decode_attention: pointers must be 16-byte aligned");
    RarmAttnParams p{}; p.q = (const bf16_t*)q; p.ldq = ldq; p.k_new = (const bf16_t*)k_new; p.v_new = (const bf16_t*)v_new;
    p.Kc = (bf16_t*)kcache; p.Vc = (bf16_t*)vcache; p.batch_stride = batch_stride; p.row_stride = row_stride; p.head_stride = head_stride;
    p.nkv = nkv; p.scale = scale; p.out = (bf16_t*)out; p.ldo = ldo;
    if (pos >= 0) { int* slot = nullptr; RDM_TRY(op_pos_slot(c, pos, &slot)); p.pos = slot; }
    RDM_CHECK_HIP(c, launch_rarm_decode_attention(p, heads, batch, c->stream));
    return 0;
}
int rdm_op_rarm_xattn_decode(rdm_ctx* c, float* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G, const void* UT, const float* bias,
                             int B2, int Bc, int C, int NP, int heads, int k, const float* ln3_gamma, const float* ln3_beta, void* ln3_out) {
    RDM_ENTER(c);
    if (!x || !ln_gamma || !ln_beta || !bias || (Bc > 0 && (!G || !UT))) return c->fail(-1, "rdm_op_rarm_xattn_decode: null argument");
    if ((ln3_gamma != nullptr) != (ln3_out != nullptr) || (ln3_beta != nullptr) != (ln3_out != nullptr))
        return c->fail(-1, "rdm_op_rarm_xattn_decode: ln3_gamma, ln3_beta and ln3_out come together");
    if (B2 < 1 || Bc < 0 || Bc > B2 || C < 8 || C % 8 || C > 1024 || heads < 1 || k < 1 || heads * k > 128 || heads * k > NP)
        return c->fail(-1, "rdm_op_rarm_xattn_decode: bad shape B2=%d Bc=%d C=%d NP=%d heads=%d k=%d (Bc <= B2; C a multiple of 8 up to 1024; heads * k <= min(128, NP))",
                       B2, Bc, C, NP, heads, k);
    if (((uintptr_t)x | (uintptr_t)G | (uintptr_t)UT | (uintptr_t)bias) % 16) return c->fail(-1, "rdm_op_rarm_xattn_decode: x, G, UT and bias must be 16-byte aligned");
    RarmXattnParams p{}; p.x = x; p.ln_g = ln_gamma; p.ln_b = ln_beta; p.ln_eps = ln_eps; p.G = (const bf16_t*)G; p.UT = (const bf16_t*)UT; p.bias = bias;
    p.B2 = B2; p.Bc = Bc; p.C = C; p.NP = NP; p.heads = heads; p.k = k; p.ln3_g = ln3_gamma; p.ln3_b = ln3_beta; p.ln3_out = (bf16_t*)ln3_out;
    RDM_CHECK_HIP(c, launch_rarm_xattn_decode(p, c->stream));
    return 0;
}
int rdm_op_rarm_embed(rdm_ctx* c, const int64_t* tokens, int tok_ld, int tok_rows, int seq0, const float* emb, const float* pos_t, float* x, long long rows, int t,
                      int C, int vocab, int L, int pos) {
    RDM_ENTER(c);
    if (!tokens || !emb || !pos_t || !x) return c->fail(-1, "rdm_op_rarm_embed: null argument");
    if (rows < 1 || rows > 0x7fffffffLL || C < 1 || vocab < 1 || L < 1 || t < 1 || t > L || pos < -1 || pos >= L)
        return c->fail(-1, "rdm_op_rarm_embed: bad shape rows=%lld t=%d C=%d vocab=%d L=%d pos=%d (1 <= t <= L, -1 <= pos < L)", rows, t, C, vocab, L, pos);
    if (pos >= 0) {
        if (t != 1) return c->fail(-1, "rdm_op_rarm_embed: the decode-step form (pos >= 0) is one row per sequence: t = 1, got %d", t);
        int* slot = nullptr; RDM_TRY(op_pos_slot(c, pos, &slot));
        RDM_CHECK_HIP(c, launch_rarm_embed((const long long*)tokens, emb, pos_t, slot, x, (int)rows, C, vocab, c->stream));
        return 0;
    }
    if (tok_rows < 1 || tok_ld < t || seq0 < 0 || rows % t) return c->fail(-1, "rdm_op_rarm_embed: tok_rows >= 1, tok_ld >= t, seq0 >= 0 and whole sequences required (tok_rows=%d tok_ld=%d seq0=%d)", tok_rows, tok_ld, seq0);
    RDM_CHECK_HIP(c, launch_rarm_embed_seq((const long long*)tokens, tok_ld, tok_rows, seq0, emb, pos_t, x, rows, t, C, vocab, c->stream));
    return 0;
}
int rdm_op_rarm_nll(rdm_ctx* c, const float* logits, long long rows, int vocab, const int64_t* targets, float* nll_out) {
    RDM_ENTER(c);
    if (!logits || !targets || !nll_out) return c->fail(-1, "rdm_op_rarm_nll: null argument");
    if (rows < 1 || vocab < 2 || vocab % 2) return c->fail(-1, "rdm_op_rarm_nll: rows >= 1 and an even vocabulary required (rows=%lld, vocab=%d)", rows, vocab);
    RDM_CHECK_HIP(c, launch_rarm_nll(logits, rows, vocab, (const long long*)targets, nll_out, c->stream));
    return 0;
}
int rdm_op_rarm_nll_bwd(rdm_ctx* c, const float* logits, long long rows, int vocab, const int64_t* targets, float gscale, void* dlogits, float* nll_out) {
    RDM_ENTER(c);
    if (!logits || !targets || !dlogits) return c->fail(-1, "rdm_op_rarm_nll_bwd: null argument");
    if (rows < 1 || vocab < 2 || vocab % 2) return c->fail(-1, "rdm_op_rarm_nll_bwd: rows >= 1 and an even vocabulary required (rows=%lld, vocab=%d)", rows, vocab);
    RDM_CHECK_HIP(c, launch_rarm_nll_bwd(logits, rows, vocab, (const long long*)targets, gscale, (bf16_t*)dlogits, nll_out, c->stream));
    return 0;
}
