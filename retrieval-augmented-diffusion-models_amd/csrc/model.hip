// Host-side executors of librdm_hip: the UNet, first-stage / CLIP and RARM graph walkers, the five samplers and the
// operator-level entries (rdm_op_*) of the C ABI declared in include/rdm_hip.h.  What they share is in host.h; model
// descriptions and loaders are in describe.hip, kernel selection (the Ops methods) in dispatch.hip, the context in context.hip.
//
// The executors mirror the reference's module graphs
//   UNetModel.__init__/forward      rdm/modules/diffusionmodules/openaimodel.py:66-371
//   SpatialTransformer / BasicTransformerBlock / CrossAttention   rdm/modules/attention.py:20-196
//   DDIMSampler                     rdm/models/diffusion/ddim.py:27-268
//   CLIP                            rdm/modules/custom_clip/model.py:152-336
//   [ldm, un-vendored] ResBlock, Down/Upsample, VQModelInterface.decode, p_sample_loop
// but are laid out for the hardware: NHWC bf16 activations (a 1x1 conv, a Linear and a token
// sequence are the same [M,C] matrix), fused epilogues (bias, time-embedding add, residual, GEGLU,
// SiLU), no materialised skip-concat, cross-attention K/V and all 22 emb_layers projections batched
// into one GEMM each, K/V of the retrieved neighbours computed once per sample() call instead of
// once per step per layer.
#include "host.h"
#include "philox.h"

// ------------------------------------------------------------------------------------ UNet forward
// kv: bf16 [B*k, kv_total] cross-attention keys/values for every SpatialTransformer (rdm_unet_forward: per call; the samplers: prepare_kv)
static void unet_compute_kv(Ops& o, UNet& u, const float* context, int B, int k, bf16_t* kv_out) {
    const int cd = u.cfg.context_dim;
    bf16_t* cb = o.abf((size_t)B * k * cd);
    if (!o.plan) o.check(launch_cast_f32_bf16(context, cb, (long long)B * k * cd, o.c->stream), "cast ctx");
    o.linear(cb, nullptr, cd, 0, o.w<bf16_t>(u.kvw), nullptr, B * k, u.kv_total, ACT_NONE, nullptr, kv_out);
}

// ---- cross-attention over k neighbours as two skinny GEMMs.  softmax(q K^T / sqrt d) V W_o^T with q = x W_q^T is re-associated
// per sample:  scores = x G_b^T with G_b[(h,j), :] = (K_bj restricted to head h) W_q / sqrt d   -> [heads*k <= 128 columns]
//              out    = P U_b^T  with U_b[:, (h,j)] = W_o (V_bj restricted to head h)            -> K = 128
// G_b and U_b depend only on the conditioning (computed once per sampling call next to the K/V cache).  The per-forward work
// drops from two C x C projections + an attention kernel (9 tensor passes) to N = 128 / K = 128 GEMMs (3.3 passes); identical
// in exact arithmetic to rdm/modules/attention.py:52-72 (CrossAttention.forward).
static bool xattn_skinny_ok(const UNet& u, int k) {
    if (!(k == 1 || k == 2 || k == 4)) return false;
    for (const StW& s : u.st) if (s.heads * k > XA_NP || s.c != s.heads * 32) return false;
    return !u.st.empty();
}
static void unet_compute_xattn(Ops& o, UNet& u, const bf16_t* kv, int B, int k, bf16_t* xa) {
    int cmax = 0;
    for (const StW& s : u.st) cmax = s.c > cmax ? s.c : cmax;
    bf16_t* kexp = o.abf((size_t)B * XA_NP * cmax);
    bf16_t* vexp = o.abf((size_t)B * XA_NP * cmax);
    bf16_t* wqt = o.abf((size_t)cmax * cmax);
    if (o.plan) return;
    for (const StW& s : u.st) {
        const int C = s.c;
        bf16_t* G = xa + (size_t)B * s.xa_unit;                       // [B][NP][C]
        bf16_t* U = G + (size_t)B * XA_NP * C;                        // [B][C][NP]
        o.check(launch_expand_heads(kv + s.kv_off, u.kv_total, B, k, s.heads, 32, XA_NP, 1.0f / sqrtf(32.f), kexp, o.c->stream), "expand K");
        o.check(launch_expand_heads(kv + s.kv_off + C, u.kv_total, B, k, s.heads, 32, XA_NP, 1.0f, vexp, o.c->stream), "expand V");
        o.check(launch_transpose_bf16(o.w<bf16_t>(s.wq2), wqt, C, C, o.c->stream), "transpose Wq");
        {   // G = Kexp . Wq   (contract over Wq's ROW index: weights operand = Wq^T)
            IgemmParams p = o.base(B * XA_NP, C, C);
            p.A0 = kexp; p.C0 = C; p.W = wqt; p.out_bf16 = G;
            o.check(launch_igemm(p, false, 1, o.c->stream), "xattn G");
        }
        {   // U_b = Wo . Vexp_b^T  per sample (A shared)
            IgemmParams p = o.base(C, XA_NP, C);
            p.A0 = o.w<bf16_t>(s.wo2); p.C0 = C; p.W = vexp; p.sA = 0; p.sW = (long long)XA_NP * C; p.sO = (long long)C * XA_NP;
            p.out_bf16 = U; p.ldo = XA_NP;
            o.check(launch_igemm(p, false, B, o.c->stream), "xattn U");
        }
        o.check(launch_xattn_pack(G, U, U + (size_t)B * C * XA_NP, U + (size_t)B * C * XA_NP + (size_t)B * XA_NP * C, B, XA_NP, C, o.c->stream), "xattn pack");
    }
}

// time embedding (openaimodel.py:352-353) and all 22 ResBlock emb_layers of it as ONE row of u.emb_total floats per timestep row:
// emb is only ever consumed through SiLU (ResBlock.emb_layers[0]), so SiLU is folded into the two MLP outputs
static void unet_time_rows(Ops& o, UNet& u, const long long* t, int B, float* emb_all) {
    const int mcl = u.cfg.model_channels, mc = pad64(mcl), ted = mcl * 4;
    bf16_t* temb = o.abf((size_t)B * mc);
    if (!o.plan) o.check(launch_timestep_embedding(t, temb, B, mcl, mc, o.c->stream), "timestep_embedding");
    bf16_t* e1 = o.abf((size_t)B * ted);
    o.single_row = true;                                  // one row per sample (see Ops::linear)
    o.tag = "time_embed";
    o.linear(temb, nullptr, mc, 0, o.w<bf16_t>(u.te0w), o.w<float>(u.te0b), B, ted, ACT_SILU, nullptr, e1);
    bf16_t* semb = o.abf((size_t)B * ted);
    o.linear(e1, nullptr, ted, 0, o.w<bf16_t>(u.te2w), o.w<float>(u.te2b), B, ted, ACT_SILU, nullptr, semb);
    o.linear(semb, nullptr, ted, 0, o.w<bf16_t>(u.embw), o.w<float>(u.embb), B, u.emb_total, ACT_NONE, nullptr, nullptr, emb_all);      // all 22 emb_layers in one GEMM
    o.single_row = false;
}

// emb_row: the batch shares ONE timestep whose emb row was computed ahead of the sampling loop (rdm_ddim_sample: a table of the S rows, one
// launch set per call instead of three GEMMs per forward); null: the rows are formed here from t
static void unet_body(Ops& o, UNet& u, const float* x, const long long* t, const bf16_t* kv, const bf16_t* xa, const int Bfull, int k, int H, int W,
                      float* eps_out, int Bx /* samples [Bx, Bfull) have all-zero context */, int Bshared /* Bfull, or Bfull/2: see below */,
                      const float* emb_row = nullptr) {
    int B = Bfull;               // the batch the CURRENT layer runs on (Bshared inside the guidance prefix)
    const rdm_unet_cfg& c = u.cfg;
    const int mcl = c.model_channels, mc = pad64(mcl);        // mc: padded width of the base level (see build_unet)
    const float* emb_all = emb_row;
    const int emb_ld = emb_row ? 0 : u.emb_total;           // row stride per sample: 0 = every sample reads the same row
    if (!emb_row) {
        float* e = o.af32((size_t)B * u.emb_total);
        unet_time_rows(o, u, t, B, e);
        emb_all = e;
    }

    struct Act { bf16_t* p; int C, H, W, L; bool half = false; };          // C: padded channels (row stride), L: logical channels; half: only samples [0, Bfull/2) exist (a shared-prefix skip tensor read with a batch wrap)
    std::vector<Act> hs;
    Act h{nullptr, 0, H, W, 0};
    // Shared guidance prefix: with classifier-free guidance the batch is [x | x] with the SAME x and t in both halves and different
    // contexts (ddim.py:229-234), so every layer before the first SpatialTransformer (conv_in, the 64x64 ResBlocks, the first
    // Downsample, the first 32x32 ResBlock: 12 % of the conv FLOPs, 17 % of the GroupNorm bytes) computes identical values for the two
    // halves.  They run once on Bfull/2 samples; the activations (and the skip tensors already pushed) are duplicated right before the
    // first context-dependent layer.  B below is the batch the CURRENT layer runs on.
    B = (Bshared > 0 && Bshared * 2 == Bfull) ? Bshared : Bfull;
    // (block outputs produced inside the prefix are allocated for Bfull samples and written into the first half, so leaving the
    //  prefix costs one copy of B samples per tensor: first half -> second half)
    auto expand = [&](Act& a) {        // [B, H, W, C] in a [2B, H, W, C] allocation -> second half = copy of the first
        const size_t n = (size_t)(Bfull / 2) * a.H * a.W * a.C;
        if (!o.plan) o.check(hipMemcpyAsync(a.p + n, a.p, n * 2, hipMemcpyDeviceToDevice, o.c->stream), "expand prefix");
        a.half = false;
    };
    // Skip tensors pushed inside the prefix are NOT duplicated when their readers can wrap the batch index instead (GroupNorm's and the
    // skip_connection GEMM's second source: 4 of the 5 copies, 0.24 ms of a 34.5 ms forward); resblock() materialises one on demand.

    auto resblock = [&](const ResW& r, const Act& a, Act* skip) -> Act {
        const int C0 = a.C, C1 = skip ? skip->C : 0, HW = a.H * a.W, M = B * HW;
        o.rows_hint = HW;
        int wrap_b = 0;                                    // > 0: the skip tensor holds Bfull/2 samples, read with a batch wrap
        if (skip && skip->half) {
            if (B == Bfull && r.skip && o.lin4_takes(M, r.cout, C0, C1, (Bfull / 2) * HW)) wrap_b = Bfull / 2;
            else expand(*skip);
        }
        const bf16_t* x1 = skip ? skip->p : nullptr;
        // skip_connection first: it needs the block's input only.  (Issuing it on a second stream, to fill the CUs the conv kernels leave
        // idle in their last round, measured + 0.45 % on one box and - 0.25 % on another in round 6 (profiles/r06_skip_overlap_ab*.log): removed.)
        const bf16_t* res = a.p;
        bf16_t* sk = nullptr;
        if (r.skip) {
            sk = o.abf((size_t)M * r.cout);
            o.tag = "res.skip";
            o.linear(a.p, x1, C0, C1, o.w<bf16_t>(r.wsk), o.w<float>(r.bsk), M, r.cout, ACT_NONE, nullptr, sk, nullptr, nullptr, wrap_b * HW);
            res = sk;
        }
        bf16_t* n1 = o.abf((size_t)M * r.cin);
        o.tag = "res.gn1";
        o.groupnorm(a.p, x1, C0, C1, B, HW, o.w<float>(r.gn1g), o.w<float>(r.gn1b), 1e-5f, 1, n1, a.L, skip ? skip->L : 0, wrap_b);
        o.tap(1, n1, (size_t)M * r.cin * 2);
        bf16_t* h1 = o.abf((size_t)M * r.cout);
        o.tag = "res.conv1";
        o.conv3(n1, nullptr, r.cin, 0, o.w<bf16_t>(r.w1), o.w<float>(r.b1), B, a.H, a.W, r.cout, 1, 0, emb_all + r.emb_off, emb_ld, nullptr, h1);
        o.tap(2, h1, (size_t)M * r.cout * 2);
        bf16_t* n2 = o.abf((size_t)M * r.cout);
        o.tag = "res.gn2";
        o.groupnorm(h1, nullptr, r.cout, 0, B, HW, o.w<float>(r.gn2g), o.w<float>(r.gn2b), 1e-5f, 1, n2, r.lout, 0);
        o.tap(3, n2, (size_t)M * r.cout * 2);
        if (r.skip) o.tap(4, sk, (size_t)M * r.cout * 2);
        bf16_t* out = o.abf((size_t)Bfull * HW * r.cout);           // Bfull: see expand()
        o.tag = "res.conv2";
        o.conv3(n2, nullptr, r.cout, 0, o.w<bf16_t>(r.w2), o.w<float>(r.b2), B, a.H, a.W, r.cout, 1, 0, nullptr, 0, res, out);
        o.tap(5, out, (size_t)M * r.cout * 2);
        return Act{out, r.cout, a.H, a.W, r.lout};
    };
    auto transformer = [&](const StW& s, const Act& a) -> Act {
        const int C = s.c, n = a.H * a.W, M = B * n;
        o.rows_hint = n;
        // a.half: the input left the shared guidance prefix and only its first Bfull / 2 samples exist: its two readers -- the entry GroupNorm and
        // the residual of ff.net.2 x proj_out -- wrap the batch index (round 5: no 50 MB duplication pass per forward)
        const int in_wrap = a.half ? Bfull / 2 : 0;
        bf16_t* xn = o.abf((size_t)M * C);
        o.tag = "st.gn";
        o.groupnorm(a.p, nullptr, C, 0, B, n, o.w<float>(s.gng), o.w<float>(s.gnb), 1e-6f, 0, xn, s.lc, 0, 0, in_wrap);
        o.tap(1, xn, (size_t)M * C * 2);
        bf16_t* t0 = o.abf((size_t)M * C);
        o.tag = "st.proj_in";
        o.linear(xn, nullptr, C, 0, o.w<bf16_t>(s.win), o.w<float>(s.bin), M, C, ACT_NONE, nullptr, t0);
        o.tap(2, t0, (size_t)M * C * 2);
        // --- attn1 (self)
        bf16_t* l1 = o.abf((size_t)M * C);
        // n % 64 == 0: q | k | v in ONE projection (to_v's rows follow to_q | to_k in the blob, asserted in build_unet); the flash kernel
        // reads the token-major V block through transpose reads, so no per-layer V^T GEMM (6.8 % of the forward as a batched
        // weights-as-A GEMM at 380 TFLOP/s)
        const bool vrow = (n % 64 == 0) && s.v_follows;
        const int QW = vrow ? 3 * C : 2 * C;
        bf16_t* qk = o.abf((size_t)M * QW);
        o.tag = "st.norm1+qkv";
        o.layernorm(t0, 0, o.w<float>(s.ln1g), o.w<float>(s.ln1b), l1, 0, M, C, s.lc);
        o.tap(3, l1, (size_t)M * C * 2);
        o.linear(l1, nullptr, C, 0, o.w<bf16_t>(s.wqk), nullptr, M, QW, ACT_NONE, nullptr, qk);
        o.tap(4, qk, (size_t)M * QW * 2);
        bf16_t* ao = o.abf((size_t)M * C);
        o.tag = "st.self_attention";
        if (vrow) {
            o.flash_d32(qk, QW, qk + 2 * C, nullptr, ao, B, n, s.heads);
        } else if (n % 32 == 0) {
            bf16_t* vt = o.abf((size_t)M * C);      // V^T per sample: [B][C][n] via swapped-operand GEMM
            if (!o.plan) {
                IgemmParams p = o.base(C, n, C);
                p.A0 = o.w<bf16_t>(s.wv); p.C0 = C; p.W = l1; p.sA = 0; p.sW = (long long)n * C; p.sO = (long long)C * n;
                p.out_bf16 = vt; p.ldo = n;
                o.check(launch_igemm(p, false, B, o.c->stream), "v^T gemm");
            }
            o.flash_d32(qk, 2 * C, nullptr, vt, ao, B, n, s.heads);
        } else {
            bf16_t* v = o.abf((size_t)M * C);
            o.linear(l1, nullptr, C, 0, o.w<bf16_t>(s.wv), nullptr, M, C, ACT_NONE, nullptr, v);
            o.small_attention(qk, 2 * C, qk + C, 2 * C, v, C, ao, C, B, n, n, s.heads, 32, 0, 1.0f / sqrtf(32.f), "small self attention");
        }
        o.tap(5, ao, (size_t)M * C * 2);
        bf16_t* t1 = o.abf((size_t)M * C);
        // --- attn2 (cross over the k neighbours); samples >= Bx have all-zero neighbours: t2 = t1 + b_o exactly (see add_bias_rows_kernel)
        const int Mx = Bx * n;
        // norm2 + attn2 + residual in one kernel when the neighbours' operands are cached (xa), norm2 too when no channel is padding
        const bool xfused = xa && Mx > 0 && xattn_fused_supported(Ops::xattn_params(Mx, n, C, XA_NP, s.heads * k, k));
        const bool xln = xfused && s.lc == C && C <= 2048;
        // Round 5: in a guided batch [conditional | unconditional] (Bx = B / 2) with the LayerNorm-fused cross-attention kernel,
        //   * the unconditional rows' t2 = attn1.to_out(...) + t0 + b_o2 leaves attn1.to_out's GEMM directly (b_o2 rides in the start
        //     values of those rows: Ops::linear's rowvec; one rounding less than t1 -> + b_o2), no add_bias_rows pass;
        //   * the cross-attention kernel runs IN PLACE on the conditional rows (t2 aliases t1) and emits norm3 of its finished rows, so
        //     the separate LayerNorm-3 pass only covers the unconditional rows.
        const bool xfold_shape = xln && !o.c->deterministic;
        const bool bias_fold = xfold_shape && Bx * 2 == B;             // the unconditional half exists and is exactly the second half
        o.tag = "st.attn1.to_out";
        if (bias_fold) {
            const float* zb = o.plan ? nullptr : o.c->zero_bias_pair(o.w<float>(s.bo2), C);
            if (!o.plan && !zb && o.rc == 0) o.rc = o.c->fail(-2, "out of memory for a bias table");
            o.linear(ao, nullptr, C, 0, o.w<bf16_t>(s.wo1), o.w<float>(s.bo1), M, C, ACT_NONE, t0, t1, nullptr, nullptr, 0, zb, C, Mx);
        } else {
            o.linear(ao, nullptr, C, 0, o.w<bf16_t>(s.wo1), o.w<float>(s.bo1), M, C, ACT_NONE, t0, t1);
        }
        o.tap(6, t1, (size_t)M * C * 2);          // (with the bias fold: the unconditional rows already hold t2)
        o.tag = "st.norm2+attn2";
        bf16_t* l2 = o.abf((size_t)M * C);
        if (Mx > 0 && !xln) o.layernorm(t1, 0, o.w<float>(s.ln2g), o.w<float>(s.ln2b), l2, 0, Mx, C, s.lc);
        bf16_t* t2 = xfold_shape ? t1 : o.abf((size_t)M * C);
        bf16_t* l3 = o.abf((size_t)M * C);
        if (Bx < B && !bias_fold && !o.plan)
            o.check(launch_add_bias_rows(t1 + (size_t)Mx * C, o.w<float>(s.bo2), t2 + (size_t)Mx * C, (long long)(M - Mx), C, o.c->stream), "zero-context cross attention");
        if (Mx == 0) {
        } else if (xa) {       // two skinny per-sample GEMMs (see unet_compute_xattn)
            bf16_t* P = o.abf((size_t)M * XA_NP);
            const bf16_t* G = xa + (size_t)B * s.xa_unit; const bf16_t* U = G + (size_t)B * XA_NP * C;
            const bf16_t* Gp = U + (size_t)B * C * XA_NP; const bf16_t* Up = Gp + (size_t)B * XA_NP * C;     // their packed images
            if (xln)            // both GEMMs, the softmax, the residual and norm2 (and norm3) in one launch
                o.xattn_fused(t1, o.w<float>(s.ln2g), o.w<float>(s.ln2b), 1e-5f, Gp, Up, o.w<float>(s.bo2), nullptr, t2, Mx, n, C, XA_NP, s.heads * k, k,
                              xfold_shape ? o.w<float>(s.ln3g) : nullptr, xfold_shape ? o.w<float>(s.ln3b) : nullptr, xfold_shape ? l3 : nullptr);
            else if (xfused)    // on the LayerNorm'd rows
                o.xattn_fused(l2, nullptr, nullptr, 0.f, Gp, Up, o.w<float>(s.bo2), t1, t2, Mx, n, C, XA_NP, s.heads * k, k);
            else if (!o.plan) {
                IgemmParams p = o.base(n, XA_NP, C);
                p.A0 = l2; p.C0 = C; p.sA = (long long)n * C; p.W = G; p.sW = (long long)XA_NP * C; p.out_bf16 = P; p.sO = (long long)n * XA_NP;
                p.act = ACT_SOFTMAXG; p.sm_group = k;
                o.prof_begin(RDM_PROF_LINEAR, 2.0 * Mx * XA_NP * (double)C);
                o.check(launch_igemm(p, false, Bx, o.c->stream), "xattn scores");
                o.prof_end();
                IgemmParams q = o.base(n, C, XA_NP);
                q.A0 = P; q.C0 = XA_NP; q.sA = (long long)n * XA_NP; q.W = U; q.sW = (long long)C * XA_NP; q.bias = o.w<float>(s.bo2);
                q.res_bf16 = t1; q.out_bf16 = t2; q.sO = (long long)n * C;
                o.prof_begin(RDM_PROF_LINEAR, 2.0 * Mx * C * (double)XA_NP);
                o.check(launch_igemm(q, false, Bx, o.c->stream), "xattn out");
                o.prof_end();
            }
        } else {
            bf16_t* q2 = o.abf((size_t)M * C);
            o.linear(l2, nullptr, C, 0, o.w<bf16_t>(s.wq2), nullptr, Mx, C, ACT_NONE, nullptr, q2);
            bf16_t* ao2 = o.abf((size_t)M * C);
            o.small_attention(q2, C, kv + s.kv_off, u.kv_total, kv + s.kv_off + C, u.kv_total, ao2, C, Bx, n, k, s.heads, 32, 0, 1.0f / sqrtf(32.f),
                              "cross attention");
            o.linear(ao2, nullptr, C, 0, o.w<bf16_t>(s.wo2), o.w<float>(s.bo2), Mx, C, ACT_NONE, t1, t2);
        }
        o.tap(7, t2, (size_t)M * C * 2);
        // --- GEGLU feed-forward
        o.tag = "st.norm3+geglu";
        const int FI = 4 * s.lc;                     // GEGLU hidden width: 4 x the LOGICAL channels (a multiple of 128, never padded)
        bf16_t* ff = o.abf((size_t)M * FI);
        if (xfold_shape) {       // norm3 of the conditional rows left the cross-attention kernel; the unconditional rows' here
            if (M > Mx) o.layernorm(t2 + (size_t)Mx * C, 0, o.w<float>(s.ln3g), o.w<float>(s.ln3b), l3 + (size_t)Mx * C, 0, M - Mx, C, s.lc);
            o.linear(l3, nullptr, C, 0, o.w<bf16_t>(s.wff1), o.w<float>(s.bff1), M, 2 * FI, ACT_GEGLU, nullptr, ff);
        } else {
            o.layernorm(t2, 0, o.w<float>(s.ln3g), o.w<float>(s.ln3b), l3, 0, M, C, s.lc);
            o.linear(l3, nullptr, C, 0, o.w<bf16_t>(s.wff1), o.w<float>(s.bff1), M, 2 * FI, ACT_GEGLU, nullptr, ff);
        }
        o.tap(8, l3, (size_t)M * C * 2);
        o.tap(9, ff, (size_t)M * FI * 2);
        bf16_t* out = o.abf((size_t)M * C);
        o.tag = "st.ff2*proj_out";
        // t3 = ff W_2^T + b_2 + t2 and out = t3 W_out^T + b_out + x are one GEMM over the K-concatenated operand [ff | t2]
        // (dual-source A) with the product weights built by the packer: t3 never exists (2 of 9 tensor passes, one launch)
        o.linear(ff, t2, FI, C, o.w<bf16_t>(s.wfo), o.w<float>(s.bfo), M, C, ACT_NONE, a.p, out, nullptr, nullptr, 0, nullptr, 0, 1, in_wrap * n);
        o.tap(10, out, (size_t)M * C * 2);
        return Act{out, C, a.H, a.W, s.lc};
    };

    for (const UBlock& blk : u.blocks) {
        Act* skip = nullptr; Act sk{};
        if (blk.where == 2) { sk = hs.back(); hs.pop_back(); skip = &sk; }
        bool first = true;
        o.cur_block = (int)(&blk - &u.blocks[0]); o.cur_layer = 0;
        for (const ULayer& L : blk.layers) {
            switch (L.kind) {
                case 0: {
                    bf16_t* out = o.abf((size_t)Bfull * H * W * mc);
                    if (!o.plan) o.check(launch_conv_in(x, o.w<float>(u.cinw), o.w<float>(u.cinb), out, B, c.in_channels, H, W, mc, o.c->stream), "conv_in");
                    h = Act{out, mc, H, W, mcl};
                } break;
                case 1: h = resblock(u.res[L.idx], h, (first && skip) ? skip : nullptr); break;
                case 2:
                    if (B < Bfull) {       // first context-dependent layer: leave the shared prefix
                        {   // the activation itself is duplicated only where its readers cannot wrap the batch index instead (transformer())
                            const StW& s0 = u.st[L.idx];
                            const int n0 = h.H * h.W, Mfull = Bfull * n0;
                            if (!o.c->deterministic && o.lin4_takes(Mfull, s0.c, 4 * s0.lc, s0.c, 0, (Bfull / 2) * n0)) h.half = true;
                            else expand(h);
                        }
                        for (Act& a : hs) { if (o.c->deterministic) expand(a); else a.half = true; }
                        B = Bfull;
                    }
                    h = transformer(u.st[L.idx], h); break;
                case 3: {
                    const ConvW& d = u.down[L.idx];
                    bf16_t* out = o.abf((size_t)Bfull * (h.H / 2) * (h.W / 2) * d.c);
                    o.tag = "downsample";
                    o.conv3(h.p, nullptr, d.c, 0, o.w<bf16_t>(d.w), o.w<float>(d.b), B, h.H, h.W, d.c, 2, 0, nullptr, 0, nullptr, out);
                    h = Act{out, d.c, h.H / 2, h.W / 2, d.lc};
                } break;
                case 4: {
                    const ConvW& d = u.up[L.idx];
                    bf16_t* out = o.abf((size_t)Bfull * (h.H * 2) * (h.W * 2) * d.c);
                    o.tag = "upsample";
                    o.conv3(h.p, nullptr, d.c, 0, o.w<bf16_t>(d.w), o.w<float>(d.b), B, h.H, h.W, d.c, 1, 1, nullptr, 0, nullptr, out);
                    h = Act{out, d.c, h.H * 2, h.W * 2, d.lc};
                } break;
            }
            first = false;
            o.cur_layer++;
        }
        if (blk.where == 0) hs.push_back(h);
        if (!o.plan && o.c->tap_buf && o.c->tap_sub == 0 && o.c->tap_block == (int)(&blk - &u.blocks[0])) {       // (inside the shared guidance prefix: B < Bfull samples exist)
            size_t nb = (size_t)B * h.H * h.W * h.C * 2; if (nb > o.c->tap_bytes) nb = o.c->tap_bytes;
            o.check(hipMemcpyAsync(o.c->tap_buf, h.p, nb, hipMemcpyDeviceToDevice, o.c->stream), "debug tap");
        }
    }
    if (B < Bfull) { expand(h); B = Bfull; }          // (a UNet without attention: the whole network was shared)
    bf16_t* no = o.abf((size_t)B * H * W * mc);
    bf16_t* hwp = o.abf(head_conv_wp_bytes(mc) / 2);
    o.tag = "out_head";
    o.head(h.p, B, H, W, mc, mcl, o.w<float>(u.outg), o.w<float>(u.outb), 1e-5f, o.w<float>(u.outw), o.w<float>(u.outbias), c.out_channels, eps_out, no, hwp);
}

static int unet_forward_impl(rdm_ctx* c, const float* x, const int64_t* t, const float* context, const bf16_t* kv_cached,
                             int b, int k, int H, int W, float* eps_out, int ctx_rows = -1, int shared_half = 0, const float* emb_row = nullptr) {
    UNet& u = c->unet;
    if (!u.loaded) return c->fail(-1, "unet weights not loaded");
    const int down = 1 << (u.cfg.n_channel_mult - 1);
    if (b < 1 || k < 1 || H % down || W % down) return c->fail(-1, "bad unet_forward shape b=%d k=%d H=%d W=%d", b, k, H, W);
    if (k > 256) return c->fail(-1, "k=%d neighbours exceeds the cross-attention kernel limit (256)", k);
    RDM_TRY(ensure_gn_partial(c, b));
    return run_with_arena(c, u.arena, u.blob, [&](Ops& o) {
        const bf16_t* kv = kv_cached;
        const bf16_t* xa = (kv_cached && xattn_skinny_ok(u, k)) ? u.xa_cache : nullptr;
        if (!kv) {
            bf16_t* kvb = o.abf((size_t)b * k * u.kv_total);
            unet_compute_kv(o, u, context, b, k, kvb);
            kv = kvb;
            if (xattn_skinny_ok(u, k)) {
                bf16_t* xab = o.abf((size_t)b * u.xa_total);
                unet_compute_xattn(o, u, kv, b, k, xab);
                xa = xab;
            }
        }
        unet_body(o, u, x, (const long long*)t, kv, xa, b, k, H, W, eps_out, (ctx_rows >= 0 && ctx_rows <= b) ? ctx_rows : b, shared_half, emb_row);
    });
}

int rdm_unet_forward(rdm_ctx* c, const float* x, const int64_t* t, const float* context, int b, int k, int H, int W,
                     float* eps_out) {
    RDM_ENTER(c);
    if (!c || !x || !t || !context || !eps_out) return c ? c->fail(-1, "null argument") : -1;
    return unet_forward_impl(c, x, t, context, nullptr, b, k, H, W, eps_out);
}

int rdm_debug_tap(rdm_ctx* c, void* buf, size_t nbytes, int block, int sub) {
    if (!c) return -1;
    c->tap_buf = buf; c->tap_bytes = buf ? nbytes : 0; c->tap_block = buf ? block : -1; c->tap_sub = buf ? sub : 0;
    return 0;
}

// ------------------------------------------------------------------------------------ VQ decode / encode
// ldm / taming ResnetBlock (no time embedding): GroupNorm + SiLU + 3x3 conv twice, 1x1 skip when the width changes
static bf16_t* vq_res(Ops& o, const VqRes& r, bf16_t* x, int B, int H, int W) {
    const int HW = H * W, M = B * HW;
    bf16_t* n1 = o.abf((size_t)M * r.cin);
    o.groupnorm(x, nullptr, r.cin, 0, B, HW, o.w<float>(r.n1g), o.w<float>(r.n1b), 1e-6f, 1, n1);
    bf16_t* h1 = o.abf((size_t)M * r.cout);
    o.conv3(n1, nullptr, r.cin, 0, o.w<bf16_t>(r.w1), o.w<float>(r.b1), B, H, W, r.cout, 1, 0, nullptr, 0, nullptr, h1);
    bf16_t* n2 = o.abf((size_t)M * r.cout);
    o.groupnorm(h1, nullptr, r.cout, 0, B, HW, o.w<float>(r.n2g), o.w<float>(r.n2b), 1e-6f, 1, n2);
    const bf16_t* rs = x;
    if (r.skip) { bf16_t* s = o.abf((size_t)M * r.cout); o.linear(x, nullptr, r.cin, 0, o.w<bf16_t>(r.wsk), o.w<float>(r.bsk), M, r.cout, ACT_NONE, nullptr, s); rs = s; }
    bf16_t* out = o.abf((size_t)M * r.cout);
    o.conv3(n2, nullptr, r.cout, 0, o.w<bf16_t>(r.w2), o.w<float>(r.b2), B, H, W, r.cout, 1, 0, nullptr, 0, rs, out);
    return out;
}
// An AttnBlock over more than VQ_ATTN_STREAM_N tokens runs on the streaming kernel (vq_attn.hip) when that kernel takes its width; up to there
// -- the shipped 64 x 64 decode, VQGAN-f16's 256 tokens, the padded small sizes -- and at every other width it materialises its scores.
constexpr int VQ_ATTN_STREAM_N = 4096;
static bool vq_attn_streams(long long n, int C) { return n > VQ_ATTN_STREAM_N && vq_attn_stream_supported(C); }
// ldm / taming AttnBlock: single head over H*W tokens, scale C^-1/2
static bf16_t* vq_attn(Ops& o, const VqAttn& a, bf16_t* x, int B, int H, int W) {
    const int C = a.c, n = H * W, M = B * n;
    if (vq_attn_streams(n, C)) {
        // beyond VQ_ATTN_STREAM_N tokens: token-major q, k, v (b_v after P.V, as below) and the two-sweep kernel of vq_attn.hip -- the chain's
        // arithmetic with no scores, no probabilities and no padded copies in memory, at any n
        bf16_t* hn = o.abf((size_t)M * C);
        o.groupnorm(x, nullptr, C, 0, B, n, o.w<float>(a.ng), o.w<float>(a.nb), 1e-6f, 0, hn);
        bf16_t* q = o.abf((size_t)M * C); bf16_t* kk = o.abf((size_t)M * C); bf16_t* v = o.abf((size_t)M * C);
        o.linear(hn, nullptr, C, 0, o.w<bf16_t>(a.wq), o.w<float>(a.bq), M, C, ACT_NONE, nullptr, q);
        o.linear(hn, nullptr, C, 0, o.w<bf16_t>(a.wk), o.w<float>(a.bk), M, C, ACT_NONE, nullptr, kk);
        o.linear(hn, nullptr, C, 0, o.w<bf16_t>(a.wv), nullptr, M, C, ACT_NONE, nullptr, v);
        bf16_t* ao = o.abf((size_t)M * C);
        o.vq_attention(q, C, kk, C, v, C, o.w<float>(a.bv), ao, C, B, n, C, 1.0f / sqrtf((float)C));
        bf16_t* out = o.abf((size_t)M * C);
        o.linear(ao, nullptr, C, 0, o.w<bf16_t>(a.wo), o.w<float>(a.bo), M, C, ACT_NONE, x, out);
        return out;
    }
    // The score and P.V GEMMs contract over tokens in 64-slices and write column pairs: a token count that is no multiple of 64 (a 5 x 7
    // latent) runs on np = n rounded up to 64 tokens per sample -- the normalised rows are copied into a zeroed [B][np][C] image, the padding
    // KEYS get probability 0 in the softmax (n_valid), the padding QUERIES' rows are computed and never read -- and the real rows copied back.
    // A correctness fallback for small odd sizes, not a fast path: one memset, two strided copies and the padding queries' q / k / scores per
    // AttnBlock on top of the materialised n x n matrix.
    const int np = (n + 63) & ~63, Mp = B * np;
    const bool padn = np != n;
    const size_t rowb = (size_t)n * C * 2, prowb = (size_t)np * C * 2;
    bf16_t* hn = o.abf((size_t)M * C);
    o.groupnorm(x, nullptr, C, 0, B, n, o.w<float>(a.ng), o.w<float>(a.nb), 1e-6f, 0, hn);
    if (padn) {
        bf16_t* hp = o.abf((size_t)Mp * C);
        if (!o.plan) {
            o.check(hipMemsetAsync(hp, 0, (size_t)Mp * C * 2, o.c->stream), "vq attention padding");
            o.check(hipMemcpy2DAsync(hp, prowb, hn, rowb, rowb, B, hipMemcpyDeviceToDevice, o.c->stream), "vq attention padding");
        }
        hn = hp;
    }
    bf16_t* q = o.abf((size_t)Mp * C); bf16_t* kk = o.abf((size_t)Mp * C); bf16_t* vt = o.abf((size_t)Mp * C);
    o.linear(hn, nullptr, C, 0, o.w<bf16_t>(a.wq), o.w<float>(a.bq), Mp, C, ACT_NONE, nullptr, q);
    o.linear(hn, nullptr, C, 0, o.w<bf16_t>(a.wk), o.w<float>(a.bk), Mp, C, ACT_NONE, nullptr, kk);
    float* S = o.af32((size_t)B * np * np); bf16_t* P = o.abf((size_t)B * np * np); bf16_t* ao = o.abf((size_t)Mp * C);
    if (!o.plan) {
        IgemmParams p = o.base(C, np, C);    // V^T[b] = Wv . hn[b]^T   (bias b_v folded in after P.V: rows of P sum to 1)
        p.A0 = o.w<bf16_t>(a.wv); p.C0 = C; p.W = hn; p.sW = (long long)np * C; p.sO = (long long)C * np; p.out_bf16 = vt; p.ldo = np;
        o.check(launch_igemm(p, false, B, o.c->stream), "vq v^T");
        IgemmParams s = o.base(np, np, C);   // S[b] = q[b] k[b]^T * C^-1/2  (fp32 scores)
        s.A0 = q; s.C0 = C; s.W = kk; s.sA = (long long)np * C; s.sW = (long long)np * C; s.sO = (long long)np * np; s.out_f32 = S; s.ldo = np;
        s.alpha = 1.0f / sqrtf((float)C);
        o.check(launch_igemm(s, false, B, o.c->stream), "vq qk^T");
        o.check(launch_softmax_rows(S, P, (long long)B * np, np, o.c->stream, n), "vq softmax");
        IgemmParams pv = o.base(np, C, np);  // O[b] = P[b] V[b] + b_v
        pv.A0 = P; pv.C0 = np; pv.W = vt; pv.sA = (long long)np * np; pv.sW = (long long)C * np; pv.sO = (long long)np * C; pv.out_bf16 = ao; pv.ldo = C;
        pv.bias = o.w<float>(a.bv);
        o.check(launch_igemm(pv, false, B, o.c->stream), "vq pv");
    }
    if (padn) {
        bf16_t* aoc = o.abf((size_t)M * C);
        if (!o.plan) o.check(hipMemcpy2DAsync(aoc, rowb, ao, prowb, rowb, B, hipMemcpyDeviceToDevice, o.c->stream), "vq attention padding");
        ao = aoc;
    }
    bf16_t* out = o.abf((size_t)M * C);
    o.linear(ao, nullptr, C, 0, o.w<bf16_t>(a.wo), o.w<float>(a.bo), M, C, ACT_NONE, x, out);
    return out;
}

// debug tap (rdm_debug_tap): first-stage decoder layers are blocks 1000, 1001, ... in execution order (conv_in's output = 1000).
// tapi: the decoder's running block number; null (the encoder): no taps
static void vq_tap(Ops& o, int* tapi, const bf16_t* t, int B, int H, int W, int ch) {
    if (!tapi) return;
    o.cur_block = (*tapi)++; o.cur_layer = 0;
    if (!o.plan && o.c->tap_buf && o.c->tap_sub == 0 && o.c->tap_block == o.cur_block) {
        size_t nb = (size_t)B * H * W * ch * 2; if (nb > o.c->tap_bytes) nb = o.c->tap_bytes;
        o.check(hipMemcpyAsync(o.c->tap_buf, t, nb, hipMemcpyDeviceToDevice, o.c->stream), "debug tap");
    }
}
// the ResnetBlocks (+ AttnBlocks) of one level (ch: the running width) and the middle, for the decoder and the encoder
static bf16_t* vq_blocks(Ops& o, const VqLevel& L, bf16_t* h, int B, int H, int W, int& ch, int* tapi) {
    for (size_t i = 0; i < L.blocks.size(); i++) {
        h = vq_res(o, L.blocks[i], h, B, H, W); ch = L.blocks[i].cout; vq_tap(o, tapi, h, B, H, W, ch);
        if (i < L.attn.size()) { h = vq_attn(o, L.attn[i], h, B, H, W); vq_tap(o, tapi, h, B, H, W, ch); }
    }
    return h;
}
static bf16_t* vq_mid(Ops& o, const VqMid& m, bf16_t* h, int B, int H, int W, int* tapi) {
    const int ch = m.res1.cout;
    h = vq_res(o, m.res1, h, B, H, W); vq_tap(o, tapi, h, B, H, W, ch);
    if (m.has_attn) { h = vq_attn(o, m.attn, h, B, H, W); vq_tap(o, tapi, h, B, H, W, ch); }
    h = vq_res(o, m.res2, h, B, H, W); vq_tap(o, tapi, h, B, H, W, ch);
    return h;
}

// decoder trunk shared by the VQ-f4 (ldm) and VQGAN-f16 (taming) first stages: ResnetBlocks, AttnBlocks, nearest-2x upsample convs
static void vq_trunk(Ops& o, VqModel& v, bf16_t* h, int B, int H, int W, float* img) {
    const rdm_vq_cfg& c = v.cfg;
    int bin = c.ch * c.ch_mult[c.n_ch_mult - 1], tapi = 1000;
    vq_tap(o, &tapi, h, B, H, W, bin);
    h = vq_mid(o, v.mid, h, B, H, W, &tapi);
    for (int lvl = c.n_ch_mult - 1; lvl >= 0; lvl--) {
        h = vq_blocks(o, v.levels[lvl], h, B, H, W, bin, &tapi);
        if (lvl != 0) {
            const ConvW& u = v.levels[lvl].resample;
            bf16_t* out = o.abf((size_t)B * (H * 2) * (W * 2) * u.c);
            o.conv3(h, nullptr, u.c, 0, o.w<bf16_t>(u.w), o.w<float>(u.b), B, H, W, u.c, 1, 1, nullptr, 0, nullptr, out);
            h = out; H *= 2; W *= 2;
            vq_tap(o, &tapi, h, B, H, W, u.c);
        }
    }
    bf16_t* no = o.abf((size_t)B * H * W * bin);
    bf16_t* hwp = o.abf(head_conv_wp_bytes(bin) / 2);
    o.head(h, B, H, W, bin, bin, o.w<float>(v.noutg), o.w<float>(v.noutb), 1e-6f, o.w<float>(v.coutw), o.w<float>(v.coutb), c.out_ch, img, no, hwp);
}

// VQ-f4 (3-channel latent [B, 3, h0, w0]: any size, the decoder is conv-only): quantise (or not) + post_quant_conv + conv_in as tiny fp32 stem
// kernels, then the trunk
static void vq_body(Ops& o, VqModel& v, const float* z, int B, int h0, int w0, int force_not_quantize, float* img, int* idx_out) {
    const rdm_vq_cfg& c = v.cfg;
    const int HW0 = h0 * w0;
    float* zq = o.af32((size_t)B * c.z_channels * HW0);
    const int quant = (!c.kl && !force_not_quantize) ? 1 : 0;
    if (!o.plan)
        o.check(launch_vq_quantize(z, c.kl ? nullptr : o.w<float>(v.codebook), c.kl ? 0 : c.n_embed, o.w<float>(v.pqw), o.w<float>(v.pqb),
                                   zq, idx_out, B, HW0, quant, o.c->stream), "vq_quantize");
    const int bin = c.ch * c.ch_mult[c.n_ch_mult - 1];
    bf16_t* h = o.abf((size_t)B * HW0 * bin);
    if (!o.plan) o.check(launch_conv_in(zq, o.w<float>(v.cinw), o.w<float>(v.cinb), h, B, c.z_channels, h0, w0, bin, o.c->stream), "vq conv_in");
    vq_trunk(o, v, h, B, h0, w0, img);
}

// VQGAN-f16 (wide latent): decode_to_img from code indices (taming Net2NetTransformer.decode_to_img -> quantize.get_codebook_entry ->
// VQModel.decode = post_quant_conv + Decoder; reached from transformer.py:296-312): codebook rows gathered straight into bf16
// NHWC tokens, post_quant_conv (1x1) as a GEMM, conv_in as a 3x3 halo conv.
static void vq_wide_body(Ops& o, VqModel& v, const long long* indices, int B, float* img) {
    const rdm_vq_cfg& c = v.cfg;
    const int zr = c.resolution >> (c.n_ch_mult - 1), HW0 = zr * zr, M = B * HW0;
    bf16_t* zq = o.abf((size_t)M * c.embed_dim);
    if (!o.plan) o.check(launch_codebook_gather(indices, o.w<float>(v.codebook), c.n_embed, c.embed_dim, M, zq, o.c->stream), "codebook gather");
    bf16_t* h0 = o.abf((size_t)M * c.z_channels);
    o.linear(zq, nullptr, c.embed_dim, 0, o.w<bf16_t>(v.pqw), o.w<float>(v.pqb), M, c.z_channels, ACT_NONE, nullptr, h0);
    const int bin = c.ch * c.ch_mult[c.n_ch_mult - 1];
    bf16_t* h = o.abf((size_t)M * bin);
    o.conv3(h0, nullptr, c.z_channels, 0, o.w<bf16_t>(v.cinw), o.w<float>(v.cinb), B, zr, zr, bin, 1, 0, nullptr, 0, nullptr, h);
    vq_trunk(o, v, h, B, zr, zr, img);
}

// first-stage encode: image f32 [B, out_ch, H, W] (H, W multiples of f = 2^(levels-1)) -> z f32 [B, embed_dim, H / f, W / f]  (VQModelInterface.encode:
// no quantisation here).
// Wide latents (taming VQGAN-f16; un-vendored, parity unpinned): norm_out + swish as a GroupNorm pass, conv_out as a 3x3 conv, quant_conv as
// a GEMM whose fp32 output stays token-major [B h w, embed_dim] (returned; what the nearest-code search reads); z (NCHW) may then be null.
static float* vqenc_body(Ops& o, VqEncModel& v, const float* img, int B, int H, int W, float* z) {
    const rdm_vq_cfg& c = v.cfg;
    bf16_t* h = o.abf((size_t)B * H * W * c.ch);
    if (!o.plan) o.check(launch_conv_in(img, o.w<float>(v.cinw), o.w<float>(v.cinb), h, B, c.out_ch, H, W, c.ch, o.c->stream), "encoder conv_in");
    int bin = c.ch;
    for (int lvl = 0; lvl < c.n_ch_mult; lvl++) {
        h = vq_blocks(o, v.levels[lvl], h, B, H, W, bin, nullptr);
        if (lvl != c.n_ch_mult - 1) {      // F.pad(x, (0, 1, 0, 1)) + Conv2d(stride 2, padding 0): window rows 2 oy .. 2 oy + 2, zero beyond the last row / column
            const ConvW& d = v.levels[lvl].resample;
            bf16_t* out = o.abf((size_t)B * (H / 2) * (W / 2) * d.c);
            o.conv3(h, nullptr, d.c, 0, o.w<bf16_t>(d.w), o.w<float>(d.b), B, H, W, d.c, 2, 0, nullptr, 0, nullptr, out, /*asym=*/1);
            h = out; H /= 2; W /= 2;
        }
    }
    h = vq_mid(o, v.mid, h, B, H, W, nullptr);
    bf16_t* no = o.abf((size_t)B * H * W * bin);
    if (v.wide) {
        const int M = B * H * W;
        o.groupnorm(h, nullptr, bin, 0, B, H * W, o.w<float>(v.noutg), o.w<float>(v.noutb), 1e-6f, 1, no);
        bf16_t* ze = o.abf((size_t)M * c.z_channels);
        o.conv3(no, nullptr, bin, 0, o.w<bf16_t>(v.coutw), o.w<float>(v.coutb), B, H, W, c.z_channels, 1, 0, nullptr, 0, nullptr, ze);
        float* zt = o.af32((size_t)M * c.embed_dim);
        o.linear(ze, nullptr, c.z_channels, 0, o.w<bf16_t>(v.qw), o.w<float>(v.qb), M, c.embed_dim, ACT_NONE, nullptr, nullptr, zt);
        if (z && !o.plan) o.check(launch_vq_rows_to_nchw(zt, nullptr, z, B, H * W, c.embed_dim, o.c->stream), "latent to NCHW");
        return zt;
    }
    bf16_t* hwp = o.abf(head_conv_wp_bytes(bin) / 2);
    float* ze = o.af32((size_t)B * c.z_channels * H * W);
    o.head(h, B, H, W, bin, bin, o.w<float>(v.noutg), o.w<float>(v.noutb), 1e-6f, o.w<float>(v.coutw), o.w<float>(v.coutb), c.z_channels, ze, no, hwp);
    if (!o.plan) o.check(launch_vq_quantize(ze, nullptr, 0, o.w<float>(v.qw), o.w<float>(v.qb), z, nullptr, B, H * W, 0, o.c->stream), "quant_conv");
    return nullptr;
}

// Samples per decoder (or encoder: the same levels, mirrored) pass at an h x w latent.  Decoding is per sample (GroupNorm statistics included), so a
// batch may be walked in ranges; a range is sized so that the decoder's largest activation stays below 2^30 elements (2 GiB of bf16): the halo
// convs address an operand through 32-bit offsets and leave bigger tensors to the generic implicit GEMM (RARM at 512 sequences per GPU: the
// seven 128-channel convs of the 256 x 256 level on an 8.6 GB activation ran there at 0.30 of peak, 94 of the step's 933 ms).
// An AttnBlock of at most VQ_ATTN_STREAM_N pixels (or of a width the streaming kernel does not take) materialises its scores and probabilities,
// n^2 fp32 + n^2 bf16 per sample over the n pixels of its level: they are bounded in BYTES, VQ_SCORE_BYTES per pass -- 8 GiB, which the shipped
// batch of 64 at the training size (n = 4096: 6.4 GB) stays under, so that size is walked as it always was.  Larger levels stream (vq_attn.hip)
// and count for nothing here: a 128 x 128 latent goes 16 images per pass, what the activation count allows.  Returns 0 when ONE sample is beyond
// what the kernels index (an activation of 2^30 elements; a materialised score matrix of 2^31, which only a width outside the streaming kernel's
// can still reach).  RDM_VQ_RANGE overrides the range (tests).
constexpr long long VQ_SCORE_BYTES = 8LL << 30;
template <typename M>
static int vq_range(const M& m, int b, int h, int w) {
    static const int env = rdm_env_int(getenv("RDM_VQ_RANGE"), 0);
    const rdm_vq_cfg& c = m.cfg;
    const int top = c.n_ch_mult - 1;
    long long per = 1, score = 0;
    for (int l = 0; l <= top; l++) {
        const long long px = ((long long)h << (top - l)) * ((long long)w << (top - l)), e = px * c.ch * c.ch_mult[l];
        if (e > per) per = e;
        // the level's Upsample output (and the first convs' input at the next finer level) keeps THIS level's channel count at twice the
        // resolution -- the decoder's largest activation (VQ-f4: 256 x 256 x 256 per image, twice the level maximum): a range sized without
        // it reached exactly 2^31 elements and pushed those convs off the 32-bit-offset halo kernels (advisor, round 5)
        if (l >= 1 && 4 * e > per) per = 4 * e;
        const bool attn = !m.levels[l].attn.empty() || (l == top && m.mid.has_attn);
        const long long np = (px + 63) & ~63LL;
        if (attn && !vq_attn_streams(px, c.ch * c.ch_mult[l]) && np * np > score) score = np * np;
    }
    if (per > (1LL << 30) || score >= (1LL << 31)) return 0;
    if (env > 0) return env < b ? env : b;
    long long n = (1LL << 30) / per;
    if (score > 0 && VQ_SCORE_BYTES / (6 * score) < n) n = VQ_SCORE_BYTES / (6 * score);
    if (n < 1) n = 1;
    return n < b ? (int)n : b;
}
// a first-stage pass over a batch of h x w latents: body(o, b0, n) runs samples [b0, b0 + n) -- in ranges of vq_range(), or the whole batch at once
template <typename M, typename F>
static int vq_walk(rdm_ctx* c, M& m, int b, int h, int w, bool in_ranges, F&& body) {
    const int nr = vq_range(m, b, h, w);
    if (nr < 1) return c->fail(-1, "first stage: a %d x %d latent is beyond what one pass can index (largest activation of one sample 2^30 elements; an AttnBlock whose width is not a multiple of 128 up to 512 materialises its scores: 46336 pixels)", h, w);
    const int nb = in_ranges ? nr : b;
    RDM_TRY(ensure_gn_partial(c, nb));
    for (int b0 = 0; b0 < b; b0 += nb)
        RDM_TRY(run_with_arena(c, m.arena, m.blob, [&](Ops& o) { body(o, b0, b - b0 < nb ? b - b0 : nb); }));
    return 0;
}

// ------------------------------------------------------------------------------------ CLIP
static void clip_tower(Ops& o, const std::vector<ClipBlk>& blks, float* x, int B, int L, int Wd, int heads, int causal) {
    const int M = B * L;
    bf16_t* ln = o.abf((size_t)M * Wd); bf16_t* qkv = o.abf((size_t)M * 3 * Wd); bf16_t* ao = o.abf((size_t)M * Wd);
    bf16_t* hid = o.abf((size_t)M * 4 * Wd);
    for (const ClipBlk& k : blks) {
        o.layernorm(x, 1, o.w<float>(k.ln1g), o.w<float>(k.ln1b), ln, 0, M, Wd);
        o.linear(ln, nullptr, Wd, 0, o.w<bf16_t>(k.wqkv), o.w<float>(k.bqkv), M, 3 * Wd, ACT_NONE, nullptr, qkv);
        o.small_attention(qkv, 3 * Wd, qkv + Wd, 3 * Wd, qkv + 2 * Wd, 3 * Wd, ao, Wd, B, L, L, heads, Wd / heads, causal, 1.0f / sqrtf((float)(Wd / heads)),
                          "clip attention");
        o.linear(ao, nullptr, Wd, 0, o.w<bf16_t>(k.wo), o.w<float>(k.bo), M, Wd, ACT_NONE, nullptr, nullptr, x, x);        // x += out_proj(attn)
        o.layernorm(x, 1, o.w<float>(k.ln2g), o.w<float>(k.ln2b), ln, 0, M, Wd);
        o.linear(ln, nullptr, Wd, 0, o.w<bf16_t>(k.wfc), o.w<float>(k.bfc), M, 4 * Wd, ACT_QUICKGELU, nullptr, hid);
        o.linear(hid, nullptr, 4 * Wd, 0, o.w<bf16_t>(k.wpj), o.w<float>(k.bpj), M, Wd, ACT_NONE, nullptr, nullptr, x, x);  // x += mlp
    }
}
static void clip_text_body(Ops& o, ClipModel& m, const long long* tokens, int B, float* out) {
    const rdm_clip_cfg& c = m.cfg; const int L = c.context_length, Wd = c.transformer_width;
    float* x = o.af32((size_t)B * L * Wd);
    if (!o.plan) o.check(launch_clip_embed(tokens, o.w<float>(m.tok), o.w<float>(m.pos), x, B, L, Wd, o.c->stream), "clip embed");
    clip_tower(o, m.text, x, B, L, Wd, c.transformer_heads, 1);
    float* eot = o.af32((size_t)B * Wd); bf16_t* ln = o.abf((size_t)B * Wd);
    if (!o.plan) o.check(launch_clip_gather_eot(tokens, x, eot, B, L, Wd, o.c->stream), "gather eot");
    o.layernorm(eot, 1, o.w<float>(m.lnfg), o.w<float>(m.lnfb), ln, 0, B, Wd);
    o.single_row = true;                                  // the pooled token: one row per sample
    o.linear(ln, nullptr, Wd, 0, o.w<bf16_t>(m.tproj), nullptr, B, c.embed_dim, ACT_NONE, nullptr, nullptr, out);
    o.single_row = false;
}
// raw_h > 0: `img` is the un-preprocessed [B,3,raw_h,raw_w] image in [-1,1]; the bicubic resize + normalisation of
// ClipImageRetriever.preprocess (rdm/modules/retrievers.py:83-91) is fused into the patch gather
static void clip_image_body(Ops& o, ClipModel& m, const float* img, int B, float* out, int raw_h = 0, int raw_w = 0) {
    const rdm_clip_cfg& c = m.cfg; const int P = c.vision_patch_size, G = c.image_resolution / P, Wd = c.vision_width;
    const int K = 3 * P * P, L = G * G + 1;
    bf16_t* patches = o.abf((size_t)B * G * G * K); float* pe = o.af32((size_t)B * G * G * Wd);
    if (!o.plan) {
        if (raw_h > 0) o.check(launch_clip_preprocess(img, B, raw_h, raw_w, c.image_resolution, P, nullptr, patches, o.c->stream), "preprocess+patchify");
        else o.check(launch_clip_patchify(img, patches, B, c.image_resolution, P, o.c->stream), "patchify");
    }
    o.linear(patches, nullptr, K, 0, o.w<bf16_t>(m.conv1), nullptr, B * G * G, Wd, ACT_NONE, nullptr, nullptr, pe);
    float* x0 = o.af32((size_t)B * L * Wd); float* x = o.af32((size_t)B * L * Wd);
    if (!o.plan) o.check(launch_clip_vit_assemble(pe, o.w<float>(m.cls), o.w<float>(m.vpos), x0, B, G * G, Wd, o.c->stream), "vit assemble");
    o.layernorm(x0, 1, o.w<float>(m.lnpreg), o.w<float>(m.lnpreb), x, 1, B * L, Wd);
    clip_tower(o, m.vis, x, B, L, Wd, Wd / 64, 0);
    float* cls = o.af32((size_t)B * Wd); bf16_t* ln = o.abf((size_t)B * Wd);
    if (!o.plan) o.check(launch_gather_rows_f32(x, cls, B, L, Wd, o.c->stream), "gather cls");
    o.layernorm(cls, 1, o.w<float>(m.lnpostg), o.w<float>(m.lnpostb), ln, 0, B, Wd);
    o.single_row = true;                                  // the pooled token: one row per sample
    o.linear(ln, nullptr, Wd, 0, o.w<bf16_t>(m.vproj), nullptr, B, c.embed_dim, ACT_NONE, nullptr, nullptr, out);
    o.single_row = false;
}

// img [b, out_ch, H, W] -> z_out [b, embed_dim, H / f, W / f]; `what`: the entry's name in messages
static int vq_encode_impl(rdm_ctx* c, const char* what, const float* img, int b, int H, int W, float* z_out) {
    if (!img || !z_out || b < 1) return c->fail(-1, "%s: bad argument", what);
    if (!c->vqenc.loaded) return c->fail(-1, "first-stage encoder weights not loaded (rdm_load_vqenc)");
    const rdm_vq_cfg& q = c->vqenc.cfg;
    const int f = 1 << (q.n_ch_mult - 1);
    if (H < f || W < f || H % f || W % f) return c->fail(-1, "%s: image height and width must be positive multiples of %d (every Downsample halves exactly), got %d x %d", what, f, H, W);
    const int h = H / f, w = W / f;
    return vq_walk(c, c->vqenc, b, h, w, c->vqenc.wide, [&](Ops& o, int b0, int n) {      // wide latents: walked in ranges as rdm_vq_decode* is
        vqenc_body(o, c->vqenc, img + (size_t)b0 * q.out_ch * H * W, n, H, W, z_out + (size_t)b0 * q.embed_dim * h * w);
    });
}
int rdm_vq_encode(rdm_ctx* c, const float* img, int b, float* z_out) {
    RDM_ENTER(c);
    const int R = c->vqenc.loaded ? c->vqenc.cfg.resolution : 1;      // (not loaded: refused before R is used)
    return vq_encode_impl(c, "rdm_vq_encode", img, b, R, R, z_out);
}
int rdm_vq_encode_hw(rdm_ctx* c, const float* img, int b, int H, int W, float* z_out) {
    RDM_ENTER(c);
    if (c->vqenc.loaded && c->vqenc.wide) return c->fail(-1, "rdm_vq_encode_hw: a first stage with a wide latent (VQGAN-f16) runs at its own resolution only (rdm_vq_encode)");
    return vq_encode_impl(c, "rdm_vq_encode_hw", img, b, H, W, z_out);
}
// taming VQModel.encode as reached from Net2NetTransformer.encode_to_z (un-vendored, parity unpinned): quant_z, _, info =
// first_stage_model.encode(x); indices = info[2].view(b, -1).  The token-major fp32 latent of the encoder goes straight into the
// nearest-code search; quant_out = the chosen codebook rows as [b, embed_dim, h, w].
int rdm_vq_encode_indices(rdm_ctx* c, const float* img, int b, int64_t* indices_out, float* quant_out) {
    RDM_ENTER(c);
    if (!img || !indices_out || b < 1) return c->fail(-1, "rdm_vq_encode_indices: bad argument");
    if (!c->vqenc.loaded) return c->fail(-1, "first-stage encoder weights not loaded (rdm_load_vqenc)");
    if (!c->vq.loaded) return c->fail(-1, "rdm_vq_encode_indices: the codebook comes with the first-stage decoder weights (rdm_load_vq), which are not loaded");
    const rdm_vq_cfg& q = c->vqenc.cfg; const rdm_vq_cfg& d = c->vq.cfg;
    if (!c->vqenc.wide || !c->vq.wide || d.kl) return c->fail(-1, "rdm_vq_encode_indices needs a VQGAN first stage with a wide latent (embed_dim %% 64 == 0); VQ-f4 latents are quantised by rdm_vq_quantize");
    if (q.embed_dim != d.embed_dim || q.z_channels != d.z_channels || q.resolution != d.resolution || q.n_ch_mult != d.n_ch_mult || q.out_ch != d.out_ch)
        return c->fail(-1, "rdm_vq_encode_indices: encoder and decoder were loaded with different cfgs (embed_dim %d / %d, resolution %d / %d)", q.embed_dim, d.embed_dim, q.resolution, d.resolution);
    if (!vq_nearest_supported(q.embed_dim)) return c->fail(-1, "rdm_vq_encode_indices: embed_dim %d not taken by the nearest-code kernel (multiples of 64 up to 512)", q.embed_dim);
    const float* cb = (const float*)(c->vq.blob + c->vq.codebook);
    if (!c->vq.code_norms) {
        RDM_CHECK_HIP(c, hipMalloc((void**)&c->vq.code_norms, (size_t)d.n_embed * sizeof(float)));
        const hipError_t e = launch_vq_code_norms(cb, c->vq.code_norms, d.n_embed, d.embed_dim, c->stream);
        if (e != hipSuccess) { (void)hipFree(c->vq.code_norms); c->vq.code_norms = nullptr; return c->fail(-2, "codebook norms: %s", hipGetErrorString(e)); }
    }
    const int zr = q.resolution >> (q.n_ch_mult - 1), HW = zr * zr;
    return vq_walk(c, c->vqenc, b, zr, zr, true, [&](Ops& o, int b0, int n) {
        const float* zt = vqenc_body(o, c->vqenc, img + (size_t)b0 * q.out_ch * q.resolution * q.resolution, n, q.resolution, q.resolution, nullptr);
        const long long M = (long long)n * HW;
        char* ws = (char*)o.ar->alloc(vq_nearest_ws_bytes(M, d.n_embed));
        int* idx32 = (int*)o.ar->alloc((size_t)M * 4);
        o.vq_nearest(zt, cb, c->vq.code_norms, M, d.n_embed, d.embed_dim, ws, idx32, (long long*)indices_out + (size_t)b0 * HW);
        if (quant_out && !o.plan)
            o.check(launch_vq_rows_to_nchw(cb, idx32, quant_out + (size_t)b0 * d.embed_dim * HW, n, HW, d.embed_dim, o.c->stream), "codebook rows to NCHW");
    });
}

// z [b, z_channels, h, w] -> img_out [b, out_ch, f h, f w], indices_out [b, h w] or null
static int vq_decode_impl(rdm_ctx* c, const float* z, int b, int h, int w, int force_not_quantize, float* img_out, int32_t* indices_out) {
    if (!z || !img_out) return c->fail(-1, "null argument");
    if (!c->vq.loaded) return c->fail(-1, "vq weights not loaded");
    if (c->vq.wide) return c->fail(-1, "this first stage has a wide latent (VQGAN-f16): decode from code indices with rdm_vq_decode_indices");
    if (b < 1 || h < 1 || w < 1) return c->fail(-1, "vq decode: bad shape b=%d h=%d w=%d", b, h, w);
    const rdm_vq_cfg& q = c->vq.cfg;
    const int f = 1 << (q.n_ch_mult - 1);
    const size_t zper = (size_t)q.z_channels * h * w, iper = (size_t)q.out_ch * (f * h) * ((size_t)f * w);
    return vq_walk(c, c->vq, b, h, w, true, [&](Ops& o, int b0, int n) {
        vq_body(o, c->vq, z + b0 * zper, n, h, w, force_not_quantize, img_out + b0 * iper, indices_out ? indices_out + (size_t)b0 * h * w : nullptr);
    });
}
int rdm_vq_decode(rdm_ctx* c, const float* z, int b, int force_not_quantize, float* img_out, int32_t* indices_out) {
    RDM_ENTER(c);
    const int zr = c->vq.loaded ? c->vq.cfg.resolution >> (c->vq.cfg.n_ch_mult - 1) : 1;      // (not loaded: refused before zr is used)
    return vq_decode_impl(c, z, b, zr, zr, force_not_quantize, img_out, indices_out);
}
int rdm_vq_decode_hw(rdm_ctx* c, const float* z, int b, int h, int w, int force_not_quantize, float* img_out, int32_t* indices_out) {
    RDM_ENTER(c);
    return vq_decode_impl(c, z, b, h, w, force_not_quantize, img_out, indices_out);
}
static int vq_quantize_impl(rdm_ctx* c, const char* what, const float* z, int b, int h, int w, float* zq_out, int32_t* indices_out) {
    if (!z || !zq_out || b < 1 || h < 1 || w < 1 || (long long)h * w > 0x7fffffffLL / b) return c->fail(-1, "%s: bad argument", what);
    VqModel& v = c->vq;
    if (!v.loaded) return c->fail(-1, "vq weights not loaded");
    if (v.wide || v.cfg.kl || v.cfg.embed_dim != 3) return c->fail(-1, "%s: needs a VQ first stage with a 3-channel latent (VQ-f4)", what);
    if (!c->eye3) {       // the quantiser kernel ends in a 3 x 3 map (post_quant_conv in decode): identity + zero bias here
        const float e[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
        RDM_CHECK_HIP(c, hipMalloc((void**)&c->eye3, sizeof e));
        RDM_CHECK_HIP(c, hipMemcpy(c->eye3, e, sizeof e, hipMemcpyHostToDevice));
    }
    RDM_CHECK_HIP(c, launch_vq_quantize(z, (const float*)(v.blob + v.codebook), v.cfg.n_embed, c->eye3, c->eye3 + 9, zq_out, indices_out, b, h * w, 1, c->stream));
    return 0;
}
int rdm_vq_quantize(rdm_ctx* c, const float* z, int b, float* zq_out, int32_t* indices_out) {
    RDM_ENTER(c);
    const int zr = c->vq.loaded ? c->vq.cfg.resolution >> (c->vq.cfg.n_ch_mult - 1) : 1;
    return vq_quantize_impl(c, "rdm_vq_quantize", z, b, zr, zr, zq_out, indices_out);
}
int rdm_vq_quantize_hw(rdm_ctx* c, const float* z, int b, int h, int w, float* zq_out, int32_t* indices_out) {
    RDM_ENTER(c);
    return vq_quantize_impl(c, "rdm_vq_quantize_hw", z, b, h, w, zq_out, indices_out);
}
int rdm_vq_decode_indices(rdm_ctx* c, const int64_t* indices, int b, float* img_out) {
    RDM_ENTER(c);
    if (!indices || !img_out || b < 1) return c->fail(-1, "bad argument");
    if (!c->vq.loaded) return c->fail(-1, "vq weights not loaded");
    if (!c->vq.wide || c->vq.cfg.kl) return c->fail(-1, "rdm_vq_decode_indices needs a VQGAN first stage with a wide latent (z_channels %% 64 == 0)");
    const rdm_vq_cfg& q = c->vq.cfg;
    const int zr = q.resolution >> (q.n_ch_mult - 1);
    return vq_walk(c, c->vq, b, zr, zr, true, [&](Ops& o, int b0, int n) {
        vq_wide_body(o, c->vq, (const long long*)indices + (size_t)b0 * zr * zr, n, img_out + (size_t)b0 * q.out_ch * q.resolution * q.resolution);
    });
}

int rdm_to_uint8(rdm_ctx* c, const float* img, int b, int ch, int h, int w, uint8_t* out) {
    RDM_ENTER(c);
    if (!c || !img || !out) return -1;
    RDM_CHECK_HIP(c, launch_to_uint8_hwc(img, out, b, ch, h, w, c->stream));
    return 0;
}

int rdm_clip_encode_text(rdm_ctx* c, const int64_t* tokens, int b, float* out) {
    RDM_ENTER(c);
    if (!c || !tokens || !out) return c ? c->fail(-1, "null argument") : -1;
    if (!c->clip.loaded) return c->fail(-1, "clip weights not loaded");
    return run_with_arena(c, c->clip.arena, c->clip.blob, [&](Ops& o) { clip_text_body(o, c->clip, (const long long*)tokens, b, out); });
}
int rdm_clip_encode_image(rdm_ctx* c, const float* image, int b, float* out) {
    RDM_ENTER(c);
    if (!c || !image || !out) return c ? c->fail(-1, "null argument") : -1;
    if (!c->clip.loaded) return c->fail(-1, "clip weights not loaded");
    return run_with_arena(c, c->clip.arena, c->clip.blob, [&](Ops& o) { clip_image_body(o, c->clip, image, b, out); });
}

int rdm_clip_preprocess(rdm_ctx* c, const float* image, int b, int h, int w, float* out) {
    RDM_ENTER(c);
    if (!image || !out || b < 1 || h < 1 || w < 1) return c->fail(-1, "bad argument");
    if (!c->clip.loaded) return c->fail(-1, "clip weights not loaded (the target resolution comes from the clip cfg)");
    RDM_CHECK_HIP(c, launch_clip_preprocess(image, b, h, w, c->clip.cfg.image_resolution, c->clip.cfg.vision_patch_size, out, nullptr, c->stream));
    return 0;
}
int rdm_clip_encode_image_raw(rdm_ctx* c, const float* image, int b, int h, int w, float* out) {
    RDM_ENTER(c);
    if (!image || !out || b < 1 || h < 1 || w < 1) return c->fail(-1, "bad argument");
    if (!c->clip.loaded) return c->fail(-1, "clip weights not loaded");
    return run_with_arena(c, c->clip.arena, c->clip.blob, [&](Ops& o) { clip_image_body(o, c->clip, image, b, out, h, w); });
}

// ---- samplers
int rdm_ddim_num_intermediates(int S, int log_every_t) {
    int n = 0;
    for (int i = 0; i < S; i++) { const int index = S - i - 1; if (index % log_every_t == 0 || index == S - 1) n++; }
    return n;
}

// precompute K/V of the conditioning once per sample() call (reference recomputes S*16 times).  cat: fp32 staging for [cond | uncond],
// nb * k * context_dim floats (SamplerRun::begin reserves it at the front of the sampler scratch)
static int prepare_kv(rdm_ctx* c, float* cat, const float* cond, const float* uncond, int B, int k) {
    UNet& u = c->unet;
    const int nb = uncond ? 2 * B : B;
    const size_t cd = u.cfg.context_dim;
    RDM_TRY(ensure_bytes(c, (char**)&u.kv_cache, &u.kv_cache_bytes, (size_t)nb * k * u.kv_total * 2));
    RDM_CHECK_HIP(c, hipMemcpyAsync(cat, cond, (size_t)B * k * cd * 4, hipMemcpyDeviceToDevice, c->stream));
    if (uncond) RDM_CHECK_HIP(c, hipMemcpyAsync(cat + (size_t)B * k * cd, uncond, (size_t)B * k * cd * 4, hipMemcpyDeviceToDevice, c->stream));
    const bool skinny = xattn_skinny_ok(u, k);
    if (skinny) RDM_TRY(ensure_bytes(c, (char**)&u.xa_cache, &u.xa_cache_bytes, (size_t)nb * u.xa_total * 2));
    u.ctx_rows = nb;
    if (uncond) {      // how many trailing samples have all-zero neighbours?  (one small kernel + one 4*nb-byte read per sampling call)
        std::vector<int> flags(nb, 1);
        int* dflags = (int*)c->gn_partial;             // scratch: >= 16 KB once any forward ran; make sure it exists
        RDM_TRY(ensure_gn_partial(c, nb));
        dflags = (int*)c->gn_partial;
        RDM_CHECK_HIP(c, launch_row_nonzero(cat, nb, (long long)k * cd, dflags, c->stream));
        RDM_CHECK_HIP(c, hipMemcpyAsync(flags.data(), dflags, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
        RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
        int rows = nb;
        while (rows > 0 && flags[rows - 1] == 0) rows--;
        if (!c->deterministic) u.ctx_rows = rows;     // (which rows are "trailing" depends on the batch)
    }
    return run_with_arena(c, u.arena, u.blob, [&](Ops& o) {
        unet_compute_kv(o, u, cat, nb, k, u.kv_cache);
        if (skinny) unet_compute_xattn(o, u, u.kv_cache, nb, k, u.xa_cache);
    });
}

// ldm make_ddim_timesteps 'uniform', ascending (ddim_schedule and rdm_dpmpp_timesteps' time_uniform grid both take their list from
// here).  Returns 0, -1 for an S outside [1, T], or the first timestep that falls outside the schedule (>= T, so positive).
static int ddim_timesteps(int T, int S, std::vector<int>& ts) {
    ts.clear();
    if (S < 1 || S > T) return -1;
    const int step = T / S;
    for (int i = 0; i < T && (int)ts.size() < (T + step - 1) / step; i += step) ts.push_back(i + 1);
    for (int v : ts) if (v >= T) return v;
    return 0;
}

// DDIM schedule (ldm make_ddim_timesteps 'uniform' + make_ddim_sampling_parameters): the timesteps ts, the fp32 alphas a_t,
// alphas_prev a_prev and np.sqrt(1 - a_t) of every step (shared by the DDIM and PLMS loops; sigma is the DDIM loop's own)
static int ddim_schedule(rdm_ctx* c, const rdm_ddim_args* a, std::vector<int>& ts, std::vector<float>& at, std::vector<float>& ap,
                         std::vector<float>& s1m) {
    const int bad = a->alphas_cumprod ? ddim_timesteps(a->T, a->S, ts) : -1;
    if (bad < 0) return c->fail(-1, "bad schedule");
    if (bad > 0) return c->fail(-1, "ddim timestep %d out of range for T=%d (S must divide the schedule like the reference)", bad, a->T);
    const int total = (int)ts.size();
    at.resize(total); ap.resize(total); s1m.resize(total);
    for (int i = 0; i < total; i++) {
        at[i] = a->alphas_cumprod[ts[i]];
        ap[i] = (i == 0) ? a->alphas_cumprod[0] : a->alphas_cumprod[ts[i - 1]];
        s1m[i] = std::sqrt(1.0f - at[i]);         // np.sqrt on the fp32 tensor (ddim.py:52)
    }
    return 0;
}

// Every sample of a step shares the step's timestep, and the sampler's timesteps are known before the loop: their time-embedding rows
// (MLP + the 22 emb_layers) are computed ONCE per call as row GEMMs into a table (row i <-> ts[i]), instead of three B-row GEMMs per
// forward (72 us of a 29 ms forward).  Not in deterministic mode (the rows must come out of the same kernel configuration as
// rdm_unet_forward's): *table stays null there.
static int sampler_emb_table(rdm_ctx* c, const std::vector<int>& ts, const float** table) {
    *table = nullptr;
    if (c->deterministic) return 0;
    UNet& u = c->unet;
    const size_t total = ts.size();
    RDM_TRY(ensure_bytes(c, (char**)&u.emb_table, &u.emb_table_bytes, total * u.emb_total * 4 + total * 8 + 256));
    long long* tuniq = (long long*)((char*)u.emb_table + ((total * u.emb_total * 4 + 255) & ~(size_t)255));
    std::vector<long long> th(ts.begin(), ts.end());
    RDM_CHECK_HIP(c, hipMemcpyAsync(tuniq, th.data(), total * 8, hipMemcpyHostToDevice, c->stream));
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    RDM_TRY(run_with_arena(c, u.arena, u.blob, [&](Ops& o) { unet_time_rows(o, u, tuniq, (int)total, u.emb_table); }));
    *table = u.emb_table;
    return 0;
}

// One sampling call of the five loops.  begin() lays out the scratch in c->samp ([cond | uncond] staging, the UNet input x of nb rows,
// the [steps][nb] int64 timestep table, eps, n_extra fp32 buffers of B rows for the sampler's own state: extra[]), projects the
// conditioning's K/V, uploads the timestep table and the time-embedding table of ts, and copies x_T into x (both halves of a guided
// batch: nb = 2B, [x | x] against [cond | uncond]; later steps' kernels write both halves through x_dup).  forward(idx) is then the
// UNet at ts[idx] on x into eps.
// Device noise (philox.h): the seed and the global index of the call's first sample row
struct NoiseSeed { uint64_t seed; int64_t row0; };
// rows [row0, row0 + B) must be 32-bit row counters and a row's block counter must fit 32 bits (per_row <= 2^34)
static int check_noise_rows(rdm_ctx* c, const char* who, int64_t row0, int64_t B, int64_t per_row) {
    if (B < 1 || per_row < 1) return c->fail(-1, "%s: B and per_row must be >= 1 (B=%lld, per_row=%lld)", who, (long long)B, (long long)per_row);
    if (row0 < 0 || row0 > 0xFFFFFFFFll || B > 0xFFFFFFFFll - row0)
        return c->fail(-1, "%s: row0 + B must fit 32 bits (row0=%lld, B=%lld)", who, (long long)row0, (long long)B);
    if (per_row > (1ll << 34)) return c->fail(-1, "%s: per_row must be at most 2^34, got %lld", who, (long long)per_row);
    return 0;
}

struct SamplerRun {
    rdm_ctx* c; int B, nb, k, H, W, total; long long n1;           // n1: elements of x for B rows; total: ts.size()
    float *x, *x_dup, *eps, *extra[4]; long long* tdev; const float* emb_table;
    int log_every_t = 0, n_logged = 0; float *x_inter = nullptr, *pred_x0_inter = nullptr;     // intermediates (DDPM keeps none)
    static size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
    // a: the entry's args (batch, k, channels, height, width); uncond: null for an unguided call; log_every / x_inter_out / pred_x0_out:
    // the entry's intermediates arguments; n_extra <= 4.  The caller has checked that the UNet is loaded.
    template <class Args>       // rdm_ddim_args | rdm_dpmpp_args | rdm_unipc_args | rdm_ddpm_args: the five fields have the same names
    int begin(rdm_ctx* ctx, const Args* a, const std::vector<int>& ts, const float* x_T, const float* cond, const float* uncond,
              int log_every, float* x_inter_out, float* pred_x0_out, int n_extra) {
        c = ctx; B = a->batch; nb = uncond ? 2 * B : B; k = a->k; H = a->height; W = a->width; total = (int)ts.size();
        n1 = (long long)B * a->channels * H * W;
        log_every_t = log_every; x_inter = x_inter_out; pred_x0_inter = pred_x0_out;
        const size_t x_bytes = (size_t)n1 * 4 * (nb / B), t_bytes = (size_t)total * nb * 8, h_stride = al((size_t)n1 * 4);
        const size_t off_x = al((size_t)nb * k * c->unet.cfg.context_dim * 4), off_t = al(off_x + x_bytes), off_eps = al(off_t + t_bytes),
                     off_extra = al(off_eps + x_bytes);
        RDM_TRY(ensure_bytes(c, &c->samp, &c->samp_bytes, off_extra + n_extra * h_stride));
        RDM_TRY(prepare_kv(c, (float*)c->samp, cond, uncond, B, k));
        x = (float*)(c->samp + off_x); x_dup = uncond ? x + n1 : nullptr; eps = (float*)(c->samp + off_eps);
        for (int i = 0; i < n_extra; i++) extra[i] = (float*)(c->samp + off_extra + i * h_stride);
        tdev = (long long*)(c->samp + off_t);
        {
            std::vector<long long> th((size_t)total * nb);
            for (int i = 0; i < total; i++) for (int j = 0; j < nb; j++) th[(size_t)i * nb + j] = ts[i];
            RDM_CHECK_HIP(c, hipMemcpyAsync(tdev, th.data(), t_bytes, hipMemcpyHostToDevice, c->stream));
            RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));   // th goes out of scope
        }
        if (x_T) {              // null: a seeded entry draws the start (draw_start)
            RDM_CHECK_HIP(c, hipMemcpyAsync(x, x_T, n1 * 4, hipMemcpyDeviceToDevice, c->stream));
            if (x_dup) RDM_CHECK_HIP(c, hipMemcpyAsync(x_dup, x_T, n1 * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        return sampler_emb_table(c, ts, &emb_table);
    }
    // the start of a seeded call without x_T: row b of x = the normals of (seed, stream 0, step 0, row0 + b)
    int draw_start(const NoiseSeed& ns) {
        RngFillParams f{ns.seed, B, n1 / B, (uint32_t)ns.row0, 0u, RDM_RNG_STREAM_XT, (uint32_t*)x};
        RDM_CHECK_HIP(c, launch_rng_fill(f, true, c->stream));
        if (x_dup) RDM_CHECK_HIP(c, hipMemcpyAsync(x_dup, x, n1 * 4, hipMemcpyDeviceToDevice, c->stream));
        return 0;
    }
    StepRngParams step_rng(const NoiseSeed& ns, int step) const { return {ns.seed, n1 / B, (uint32_t)ns.row0, (uint32_t)step}; }
    int forward(int idx) {        // guided: [x | x] at the same t, so the context-independent prefix runs once (shared half = B)
        UNet& u = c->unet;
        return unet_forward_impl(c, x, (const int64_t*)(tdev + (size_t)idx * nb), nullptr, u.kv_cache, nb, k, H, W, eps, u.ctx_rows,
                                 x_dup ? B : 0, emb_table ? emb_table + (size_t)idx * u.emb_total : nullptr);
    }
    // intermediates of loop step `step` (0 .. total - 1; the rule counts the index down from total - 1): where the step kernel writes
    // pred_x0, then the copy of the new x
    bool logs(int step) const { const int index = total - 1 - step; return (index % log_every_t == 0) || (index == total - 1); }
    float* pred_x0_slot(int step) const { return (logs(step) && pred_x0_inter) ? pred_x0_inter + (size_t)n_logged * n1 : nullptr; }
    int log_x(int step) {
        if (!logs(step)) return 0;
        if (x_inter) RDM_CHECK_HIP(c, hipMemcpyAsync(x_inter + (size_t)n_logged * n1, x, n1 * 4, hipMemcpyDeviceToDevice, c->stream));
        n_logged++;
        return 0;
    }
    int finish(float* z_out) { RDM_CHECK_HIP(c, hipMemcpyAsync(z_out, x, n1 * 4, hipMemcpyDeviceToDevice, c->stream)); return 0; }
};

// The guidance arguments of the four guided entries (ddim.py:223, :231): *cfg = the batch is doubled
static int sampler_guidance(rdm_ctx* c, const char* who, float scale, const float* uncond, bool* cfg) {
    if (scale < 1.0f) return c->fail(-1, "%s: unconditional_guidance_scale must be >= 1", who);
    *cfg = scale > 1.0f;
    if (*cfg && !uncond) return c->fail(-1, "%s: unconditional_conditioning required when scale > 1", who);
    return 0;
}

// The history of the PLMS and UniPC loops: the last (up to) three values, h(0) the newest, in three buffers rotated by pointer.  The
// step kernel writes the newest value to next() -- a free buffer, or the oldest value's -- in the pass that reads h(0..2): a thread
// reads its elements of the oldest value before it overwrites them.  push() after that launch makes next() h(0).
struct HistoryRing {
    float* slot[3]; int held = 0;
    float* h(int i) const { return i < held ? slot[i] : nullptr; }
    float* next() const { return slot[held < 3 ? held : 2]; }
    void push() {
        float* newest = next();
        for (int j = held < 3 ? held : 2; j > 0; j--) slot[j] = slot[j - 1];
        slot[0] = newest;
        if (held < 3) held++;
    }
};

// The DDIM loop of rdm_ddim_sample (ns null: the step noise is read from the stack `noise`) and rdm_ddim_sample_seeded (ns: it is generated
// in the step kernel, and a null x_T is drawn).
static int ddim_sample_impl(rdm_ctx* c, const rdm_ddim_args* a, const float* x_T, const float* cond, const float* uncond,
                            const float* noise, const NoiseSeed* ns, float* z_out, float* x_inter, float* pred_x0_inter) {
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    bool cfg;
    RDM_TRY(sampler_guidance(c, "ddim", a->unconditional_guidance_scale, uncond, &cfg));
    if (ns) {
        RDM_TRY(check_noise_rows(c, "ddim (seeded)", ns->row0, a->batch, (int64_t)a->channels * a->height * a->width));
        if (((int64_t)a->channels * a->height * a->width) % 4) return c->fail(-1, "ddim (seeded): channels * height * width must be a multiple of 4");
    } else if (a->eta != 0.f && !noise) return c->fail(-1, "eta > 0 needs an explicit noise stack [S,B,C,H,W] (device RNG parity is not defined)");
    std::vector<int> ts; std::vector<float> at, ap, s1m;
    RDM_TRY(ddim_schedule(c, a, ts, at, ap, s1m));
    const int total = (int)ts.size();
    std::vector<float> sg(total);
    for (int i = 0; i < total; i++) {
        // sigma computed in float64 from the fp32 alphas like numpy does with a float64 alphas_prev array
        const double atd = (double)at[i], apd = (double)ap[i];
        sg[i] = (float)((double)a->eta * std::sqrt((1.0 - apd) / (1.0 - atd) * (1.0 - atd / apd)));
    }
    SamplerRun run;
    RDM_TRY(run.begin(c, a, ts, x_T, cond, cfg ? uncond : nullptr, a->log_every_t, x_inter, pred_x0_inter, 0));
    if (!x_T) RDM_TRY(run.draw_start(*ns));
    for (int i = 0; i < total; i++) {
        const int index = total - i - 1;         // of the ascending schedule
        RDM_TRY(run.forward(index));
        DdimStepParams p{};
        p.x = run.x; p.eps = run.eps; p.noise = (noise && a->eta != 0.f) ? noise + (size_t)i * run.n1 : nullptr;
        p.x_prev = run.x; p.x_dup = run.x_dup; p.pred_x0 = run.pred_x0_slot(i);
        p.n_per_batch = run.n1; p.a_t = at[index]; p.a_prev = ap[index]; p.sigma_t = sg[index]; p.sqrt_one_minus_at = s1m[index];
        p.scale = a->unconditional_guidance_scale; p.temperature = a->temperature; p.cfg = cfg ? 1 : 0;
        if (ns && a->eta != 0.f) {          // the noise of loop step i, in registers
            const hipError_t e = launch_ddim_step_seeded(p, run.step_rng(*ns, i), c->stream);
            if (e == hipErrorInvalidValue) return c->fail(-1, "ddim (seeded): pred_x0_inter must be 16-byte aligned");
            RDM_CHECK_HIP(c, e);
        } else RDM_CHECK_HIP(c, launch_ddim_step(p, c->stream));
        RDM_TRY(run.log_x(i));
    }
    return run.finish(z_out);
}
int rdm_ddim_sample(rdm_ctx* c, const rdm_ddim_args* a, const float* x_T, const float* cond, const float* uncond,
                    const float* noise, float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    if (!c || !a || !x_T || !cond || !z_out) return c ? c->fail(-1, "null argument") : -1;
    return ddim_sample_impl(c, a, x_T, cond, uncond, noise, nullptr, z_out, x_inter, pred_x0_inter);
}
int rdm_ddim_sample_seeded(rdm_ctx* c, const rdm_ddim_args* a, uint64_t seed, int64_t row0, const float* x_T, const float* cond,
                           const float* uncond, float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    if (!c || !a || !cond || !z_out) return c ? c->fail(-1, "null argument") : -1;
    const NoiseSeed ns{seed, row0};
    return ddim_sample_impl(c, a, x_T, cond, uncond, nullptr, &ns, z_out, x_inter, pred_x0_inter);
}

// ldm PLMSSampler.plms_sampling / p_sample_plms (eta = 0): DDIM's schedule, timesteps and intermediates, total + 1 forwards.  The
// first step is the pseudo improved Euler step: phase A stores e_t and writes x_tmp = update(x, e_t) into the UNet input, a forward at
// t_next (one of the table's rows) follows, phase B updates the kept x with (e_t + e_next) / 2.  Later steps combine e_t with up to
// three earlier e_t held in a HistoryRing.
int rdm_plms_sample(rdm_ctx* c, const rdm_ddim_args* a, const float* x_T, const float* cond, const float* uncond,
                    float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    if (!c || !a || !x_T || !cond || !z_out) return c ? c->fail(-1, "null argument") : -1;
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    if (a->eta != 0.f) return c->fail(-1, "ddim_eta must be 0 for PLMS");
    bool cfg;
    RDM_TRY(sampler_guidance(c, "plms", a->unconditional_guidance_scale, uncond, &cfg));
    std::vector<int> ts; std::vector<float> at, ap, s1m;
    RDM_TRY(ddim_schedule(c, a, ts, at, ap, s1m));
    const int total = (int)ts.size();
    SamplerRun run;         // the sampler's own scratch: the kept x, 3 history buffers
    RDM_TRY(run.begin(c, a, ts, x_T, cond, cfg ? uncond : nullptr, a->log_every_t, x_inter, pred_x0_inter, 4));
    float* xk = run.extra[0];
    HistoryRing ring{{run.extra[1], run.extra[2], run.extra[3]}};          // h(0..2) = o[-1], o[-2], o[-3]
    RDM_CHECK_HIP(c, hipMemcpyAsync(xk, x_T, run.n1 * 4, hipMemcpyDeviceToDevice, c->stream));             // the first step's x, kept beside x_tmp
    for (int i = 0; i < total; i++) {
        const int index = total - i - 1;         // of the ascending schedule
        PlmsStepParams p{};
        p.eps = run.eps; p.n = run.n1; p.a_t = at[index]; p.a_prev = ap[index]; p.sqrt_one_minus_at = s1m[index];
        p.scale = a->unconditional_guidance_scale; p.cfg = cfg ? 1 : 0;
        p.x_out = run.x; p.x_dup = run.x_dup;
        p.e_store = ring.next();
        RDM_TRY(run.forward(index));
        if (ring.held == 0) {
            p.x = xk; p.mode = PLMS_EULER_A;                   // x_tmp -> run.x (both halves); x stays in xk
            RDM_CHECK_HIP(c, launch_plms_step(p, c->stream));
            RDM_TRY(run.forward(index > 0 ? index - 1 : 0));  // t_next = time_range[min(i + 1, total - 1)]
            p.mode = PLMS_EULER_B; p.e_prev = ring.next(); p.e_store = nullptr;
        } else {
            p.x = run.x; p.mode = PLMS_STEP; p.order = ring.held;
            p.h1 = ring.h(0); p.h2 = ring.h(1); p.h3 = ring.h(2);
        }
        p.pred_x0 = run.pred_x0_slot(i);
        RDM_CHECK_HIP(c, launch_plms_step(p, c->stream));
        ring.push();
        RDM_TRY(run.log_x(i));
    }
    return run.finish(z_out);
}

// The node-list solvers (DPM-Solver++: Lu et al. 2022, ldm models/diffusion/dpm_solver/sampler.py; UniPC: Zhao et al. 2023): alpha,
// sigma and the half logSNR lambda of a timestep, in float64 from the model's fp32 alphas_cumprod
struct SolverNode { double alpha, sigma, lambda; };
static SolverNode solver_node(const float* acp, int t) {
    const double a = (double)acp[t];
    return {std::sqrt(a), std::sqrt(1.0 - a), 0.5 * std::log(a / (1.0 - a))};
}

// A node list as rdm_dpmpp_sample, rdm_unipc_sample and rdm_unipc_coefficients take it: at least 2 timesteps in [0, T - 1], strictly
// decreasing, alphas_cumprod in (0, 1) at each.  Returns what is wrong with it, *at the node at fault.
enum NodeFault { NODES_OK, NODES_TOO_FEW, NODE_OUT_OF_RANGE, NODE_NOT_DECREASING, NODE_ALPHA };
static NodeFault check_nodes(const float* acp, int T, const int* nodes, int n_nodes, int* at) {
    if (n_nodes < 2) return NODES_TOO_FEW;
    for (int j = 0; j < n_nodes; j++) {
        *at = j;
        if (nodes[j] < 0 || nodes[j] >= T) return NODE_OUT_OF_RANGE;
        if (j > 0 && nodes[j] >= nodes[j - 1]) return NODE_NOT_DECREASING;
        if (!(acp[nodes[j]] > 0.f && acp[nodes[j]] < 1.f)) return NODE_ALPHA;
    }
    return NODES_OK;
}
// ... as the error of a sampler entry (who: the sampler's name)
static int sampler_nodes(rdm_ctx* c, const char* who, const float* acp, int T, const int* nodes, int n_nodes) {
    int j = 0;
    switch (check_nodes(acp, T, nodes, n_nodes, &j)) {
    case NODES_OK: return 0;
    case NODES_TOO_FEW: return c->fail(-1, "%s needs at least 2 nodes, got %d", who, n_nodes);
    case NODE_OUT_OF_RANGE: return c->fail(-1, "%s node %d = %d outside [0, %d]", who, j, nodes[j], T - 1);
    case NODE_NOT_DECREASING: return c->fail(-1, "%s nodes must be strictly decreasing (node %d = %d after %d)", who, j, nodes[j], nodes[j - 1]);
    default: return c->fail(-1, "alphas_cumprod[%d] = %g outside (0, 1)", nodes[j], (double)acp[nodes[j]]);
    }
}

int rdm_dpmpp_timesteps(const float* alphas_cumprod, int T, int S, int skip_type, int* nodes_out) {
    if (!alphas_cumprod || !nodes_out || T < 2 || S < 1 || S > T || (skip_type != 0 && skip_type != 1)) return -1;
    int n = 0;
    if (skip_type == 0) {                 // time_uniform: DDIM's timesteps descending, then 0 (they start at 1)
        std::vector<int> ts;
        if (ddim_timesteps(T, S, ts) != 0) return -1;
        for (int i = (int)ts.size() - 1; i >= 0; i--) nodes_out[n++] = ts[i];
        nodes_out[n++] = 0;
        return n;
    }
    std::vector<double> lam(T);
    for (int t = 0; t < T; t++) {
        if (!(alphas_cumprod[t] > 0.f && alphas_cumprod[t] < 1.f)) return -1;
        lam[t] = solver_node(alphas_cumprod, t).lambda;
    }
    for (int i = 0; i <= S; i++) {        // logSNR: S + 1 targets uniform in lambda, each to the timestep of nearest lambda
        const double target = lam[T - 1] + (lam[0] - lam[T - 1]) * ((double)i / (double)S);
        int best = 0;
        for (int t = 1; t < T; t++) if (std::fabs(lam[t] - target) < std::fabs(lam[best] - target)) best = t;     // a tie keeps the smaller t
        if (n == 0 || best < nodes_out[n - 1]) nodes_out[n++] = best;
    }
    if (nodes_out[n - 1] != 0) nodes_out[n++] = 0;
    return n;
}

// The loop of rdm_dpmpp_sample's header comment: one forward and one dpmpp_step_kernel launch per step, the solver's coefficients computed
// here in float64.  The history is ONE buffer: the kernel reads m_{j-1} from it and writes m_j to it in the same pass.
int rdm_dpmpp_sample(rdm_ctx* c, const rdm_dpmpp_args* a, const float* x_T, const float* cond, const float* uncond,
                     float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    if (!c || !a || !x_T || !cond || !z_out || !a->alphas_cumprod || !a->nodes) return c ? c->fail(-1, "null argument") : -1;
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    if (a->order != 1 && a->order != 2) return c->fail(-1, "dpm-solver++ order must be 1 or 2, got %d", a->order);
    bool cfg;
    RDM_TRY(sampler_guidance(c, "dpm-solver++", a->unconditional_guidance_scale, uncond, &cfg));
    RDM_TRY(sampler_nodes(c, "dpm-solver++", a->alphas_cumprod, a->T, a->nodes, a->n_nodes));
    const int n_steps = a->n_nodes - 1;
    const std::vector<int> ts(a->nodes, a->nodes + n_steps);
    SamplerRun run;
    RDM_TRY(run.begin(c, a, ts, x_T, cond, cfg ? uncond : nullptr, a->log_every_t, x_inter, pred_x0_inter, 1));
    float* m_slot = run.extra[0];
    double h_prev = 0.0;
    for (int j = 0; j < n_steps; j++) {
        const SolverNode s = solver_node(a->alphas_cumprod, a->nodes[j]), t = solver_node(a->alphas_cumprod, a->nodes[j + 1]);
        const double h = t.lambda - s.lambda, g = -t.alpha * std::expm1(-h);       // x <- (sigma_t / sigma_s) x + g D
        const bool second = a->order == 2 && j >= 1 && !(a->lower_order_final && j == n_steps - 1);
        RDM_TRY(run.forward(j));
        DpmppStepParams p{};
        p.x = run.x; p.eps = run.eps; p.n = run.n1; p.cfg = cfg ? 1 : 0; p.scale = a->unconditional_guidance_scale;
        p.sqrt_a_s = (float)s.alpha; p.sqrt_one_minus_a_s = (float)s.sigma; p.c_x = (float)(t.sigma / s.sigma);
        if (second) {
            const double r = h_prev / h;
            p.m_prev = m_slot; p.c_0 = (float)(g * (1.0 + 1.0 / (2.0 * r))); p.c_1 = (float)(-g / (2.0 * r));
        } else {
            p.c_0 = (float)g;
        }
        p.x_out = run.x; p.x_dup = run.x_dup; p.m_store = m_slot; p.pred_x0 = run.pred_x0_slot(j);
        RDM_CHECK_HIP(c, launch_dpmpp_step(p, c->stream));
        h_prev = h;
        RDM_TRY(run.log_x(j));
    }
    return run.finish(z_out);
}

// UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models"), data prediction,
// multistep, in the notation of rdm_unipc_sample's header comment.  Everything below is float64 host code.

// rho <- R^-1 b for R [n][n], n <= 3: Gaussian elimination with partial pivoting, written out (false: singular)
static bool unipc_solve(int n, double R[3][3], double* b, double* rho) {
    for (int col = 0; col < n; col++) {
        int piv = col;
        for (int i = col + 1; i < n; i++) if (std::fabs(R[i][col]) > std::fabs(R[piv][col])) piv = i;
        if (R[piv][col] == 0.0) return false;
        if (piv != col) { for (int k = 0; k < n; k++) std::swap(R[piv][k], R[col][k]); std::swap(b[piv], b[col]); }
        for (int i = col + 1; i < n; i++) {
            const double f = R[i][col] / R[col][col];
            for (int k = col; k < n; k++) R[i][k] -= f * R[col][k];
            b[i] -= f * b[col];
        }
    }
    for (int i = n - 1; i >= 0; i--) {
        double v = b[i];
        for (int k = i + 1; k < n; k++) v -= R[i][k] * rho[k];
        rho[i] = v / R[i][i];
    }
    return true;
}

// Step s (1-based: from node s-1 to node s) at order p: phi_1 = expm1(-h), B(h), r_1 .. r_{p-1} (r_p = 1 is the corrector's own) and
// b_1 .. b_3.  lam[i] is the half logSNR of node i.
struct UnipcStep { double phi1, B, r[3], b[3]; };
static UnipcStep unipc_step_scalars(const double* lam, int s, int p, int variant) {
    UnipcStep u{};
    const double h = lam[s] - lam[s - 1], hh = -h;
    u.phi1 = std::expm1(hh);
    u.B = variant == 0 ? hh : std::expm1(hh);
    for (int i = 1; i < p; i++) u.r[i - 1] = (lam[s - 1 - i] - lam[s - 1]) / h;
    u.r[p - 1] = 1.0;
    double g = u.phi1 / hh - 1.0, fact = 1.0;              // g_i, i!
    for (int i = 1; i <= 3; i++) {
        u.b[i - 1] = g * fact / u.B;
        fact *= (double)(i + 1);
        g = g / hh - 1.0 / fact;
    }
    return u;
}

static int unipc_order(int s, int n, int order, int lower_order_final) {
    int p = order < s ? order : s;
    if (lower_order_final && n + 1 - s < p) p = n + 1 - s;
    return p;
}

// rdm_unipc_coefficients on a node list that check_nodes has passed (-1: a singular system)
static int unipc_coefficients(const float* alphas_cumprod, const int* nodes, int n_nodes, int j, int order, int variant, int corrector,
                              int lower_order_final, double* out) {
    const int n = n_nodes - 1;
    auto node = [&](int i) { return solver_node(alphas_cumprod, nodes[i]); };
    std::vector<double> lamv((size_t)n_nodes);
    for (int i = 0; i < n_nodes; i++) lamv[(size_t)i] = node(i).lambda;
    const double* lam = lamv.data();
    const SolverNode cur = node(j), nxt = node(j + 1);
    double a[5] = {0, 0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    int pc = 0;
    if (corrector && j >= 1) {                               // the correction of x_j: step j at its order, r_p = 1 for m_j itself
        pc = unipc_order(j, n, order, lower_order_final);
        UnipcStep u = unipc_step_scalars(lam, j, pc, variant);
        double rho[3] = {0.5, 0, 0};
        if (pc > 1) {
            double R[3][3], rhs[3];
            for (int i = 0; i < pc; i++) { rhs[i] = u.b[i]; for (int k = 0; k < pc; k++) R[i][k] = std::pow(u.r[k], (double)i); }
            if (!unipc_solve(pc, R, rhs, rho)) return -1;
        }
        double sum = rho[pc - 1];
        for (int i = 0; i < pc - 1; i++) sum += rho[i] / u.r[i];
        a[0] = cur.sigma / node(j - 1).sigma;
        a[1] = -cur.alpha * u.B * rho[pc - 1];
        a[2] = -cur.alpha * u.phi1 + cur.alpha * u.B * sum;
        for (int i = 0; i < pc - 1; i++) a[3 + i] = -cur.alpha * u.B * rho[i] / u.r[i];
    }
    const int pp = unipc_order(j + 1, n, order, lower_order_final);       // the prediction of u_{j+1}: step j + 1 at its order
    {
        UnipcStep u = unipc_step_scalars(lam, j + 1, pp, variant);
        double rho[2] = {0.5, 0};
        if (pp == 3) {
            double R[3][3], rhs[3];
            for (int i = 0; i < 2; i++) { rhs[i] = u.b[i]; for (int k = 0; k < 2; k++) R[i][k] = std::pow(u.r[k], (double)i); }
            if (!unipc_solve(2, R, rhs, rho)) return -1;
        }
        double sum = 0.0;
        for (int i = 0; i < pp - 1; i++) sum += rho[i] / u.r[i];
        b[0] = nxt.sigma / cur.sigma;
        b[1] = -nxt.alpha * u.phi1 + nxt.alpha * u.B * sum;
        for (int i = 0; i < pp - 1; i++) b[2 + i] = -nxt.alpha * u.B * rho[i] / u.r[i];
    }
    out[0] = cur.alpha; out[1] = cur.sigma;
    for (int i = 0; i < 5; i++) out[2 + i] = a[i];
    for (int i = 0; i < 4; i++) out[7 + i] = b[i];
    out[11] = (double)pc; out[12] = (double)pp;
    return 0;
}

int rdm_unipc_coefficients(const float* alphas_cumprod, int T, const int* nodes, int n_nodes, int j, int order, int variant, int corrector,
                           int lower_order_final, double* out) {
    int at;
    if (!alphas_cumprod || !nodes || !out || T < 2 || n_nodes < 2 || j < 0 || j >= n_nodes - 1 || order < 1 || order > 3 ||
        (variant != 0 && variant != 1) || check_nodes(alphas_cumprod, T, nodes, n_nodes, &at) != NODES_OK) return -1;
    return unipc_coefficients(alphas_cumprod, nodes, n_nodes, j, order, variant, corrector, lower_order_final, out);
}

static void unipc_fill(UnipcStepParams& p, const double* co) {
    p.alpha = (float)co[0]; p.sigma = (float)co[1];
    p.a_x = (float)co[2]; p.a_t = (float)co[3]; p.a_1 = (float)co[4]; p.a_2 = (float)co[5]; p.a_3 = (float)co[6];
    p.b_x = (float)co[7]; p.b_0 = (float)co[8]; p.b_1 = (float)co[9]; p.b_2 = (float)co[10];
    p.order_c = (int)co[11]; p.order_p = (int)co[12];
}

// The loop of rdm_unipc_sample's header comment: one forward and one unipc_step_kernel launch per step.  The sampler's own scratch is
// the kept (corrected) x and a HistoryRing of m.
int rdm_unipc_sample(rdm_ctx* c, const rdm_unipc_args* a, const float* x_T, const float* cond, const float* uncond,
                     float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    if (!c || !a || !x_T || !cond || !z_out || !a->alphas_cumprod || !a->nodes) return c ? c->fail(-1, "null argument") : -1;
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    if (a->order < 1 || a->order > 3) return c->fail(-1, "unipc order must be 1, 2 or 3, got %d", a->order);
    if (a->variant != 0 && a->variant != 1) return c->fail(-1, "unipc variant must be 0 (bh1) or 1 (bh2), got %d", a->variant);
    bool cfg;
    RDM_TRY(sampler_guidance(c, "unipc", a->unconditional_guidance_scale, uncond, &cfg));
    RDM_TRY(sampler_nodes(c, "unipc", a->alphas_cumprod, a->T, a->nodes, a->n_nodes));
    const int n_steps = a->n_nodes - 1;
    std::vector<double> co((size_t)n_steps * 13);
    for (int j = 0; j < n_steps; j++)
        if (unipc_coefficients(a->alphas_cumprod, a->nodes, a->n_nodes, j, a->order, a->variant, a->corrector, a->lower_order_final,
                               &co[(size_t)j * 13]) != 0) return c->fail(-1, "unipc coefficients of step %d are undefined on these nodes", j);
    const std::vector<int> ts(a->nodes, a->nodes + n_steps);
    SamplerRun run;
    RDM_TRY(run.begin(c, a, ts, x_T, cond, cfg ? uncond : nullptr, a->log_every_t, x_inter, pred_x0_inter, 4));
    float* xk = run.extra[0];
    HistoryRing ring{{run.extra[1], run.extra[2], run.extra[3]}};          // h(0..2) = m_{j-1}, m_{j-2}, m_{j-3}
    for (int j = 0; j < n_steps; j++) {
        RDM_TRY(run.forward(j));
        UnipcStepParams p{};
        unipc_fill(p, &co[(size_t)j * 13]);
        const int nh = p.order_c > p.order_p - 1 ? p.order_c : p.order_p - 1;
        if (nh > ring.held) return c->fail(-1, "unipc step %d needs %d earlier predictions, %d held", j, nh, ring.held);
        p.u = run.x; p.eps = run.eps; p.n = run.n1; p.cfg = cfg ? 1 : 0; p.scale = a->unconditional_guidance_scale;
        p.xc_prev = p.order_c >= 1 ? xk : nullptr;
        p.h1 = nh >= 1 ? ring.h(0) : nullptr; p.h2 = nh >= 2 ? ring.h(1) : nullptr; p.h3 = nh >= 3 ? ring.h(2) : nullptr;
        p.xc_out = a->corrector ? xk : nullptr;                // without the corrector the kept x is the UNet input itself
        p.u_next = run.x; p.x_dup = run.x_dup; p.m_store = ring.next(); p.pred_x0 = run.pred_x0_slot(j);
        RDM_CHECK_HIP(c, launch_unipc_step(p, c->stream));
        ring.push();
        RDM_TRY(run.log_x(j));
    }
    return run.finish(z_out);
}

// The ancestral loop of rdm_ddpm_sample (ns null: noise stack) and rdm_ddpm_sample_seeded (ns: generated in the step kernel; a null x_T
// is drawn).  The final step (i == 0) consumes no noise either way.
static int ddpm_sample_impl(rdm_ctx* c, const rdm_ddpm_args* a, const float* x_T, const float* cond, const float* noise, const NoiseSeed* ns,
                            float* z_out) {
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    if (a->timesteps < 1 || a->timesteps > a->T) return c->fail(-1, "bad timesteps");
    if (ns) {
        RDM_TRY(check_noise_rows(c, "ddpm (seeded)", ns->row0, a->batch, (int64_t)a->channels * a->height * a->width));
        if (((int64_t)a->channels * a->height * a->width) % 4) return c->fail(-1, "ddpm (seeded): channels * height * width must be a multiple of 4");
    }
    const int T = a->timesteps;
    std::vector<int> ts(T);
    for (int i = 0; i < T; i++) ts[i] = i;
    SamplerRun run;
    RDM_TRY(run.begin(c, a, ts, x_T, cond, nullptr, 0, nullptr, nullptr, 0));
    if (!x_T) RDM_TRY(run.draw_start(*ns));
    for (int n = 0, i = T - 1; i >= 0; i--, n++) {
        RDM_TRY(run.forward(i));
        DdpmStepParams p{};
        p.x = run.x; p.eps = run.eps; p.noise = noise ? noise + (size_t)n * run.n1 : nullptr; p.x_prev = run.x; p.n = run.n1;
        p.sqrt_recip = a->sqrt_recip_alphas_cumprod[i]; p.sqrt_recipm1 = a->sqrt_recipm1_alphas_cumprod[i];
        p.coef1 = a->posterior_mean_coef1[i]; p.coef2 = a->posterior_mean_coef2[i]; p.log_var = a->posterior_log_variance_clipped[i];
        p.clip = a->clip_denoised; p.nonzero = (i != 0); p.temperature = a->temperature;
        if (ns && p.nonzero) RDM_CHECK_HIP(c, launch_ddpm_step_seeded(p, run.step_rng(*ns, n), c->stream));      // the noise of loop step n, in registers
        else RDM_CHECK_HIP(c, launch_ddpm_step(p, c->stream));
    }
    return run.finish(z_out);
}
int rdm_ddpm_sample(rdm_ctx* c, const rdm_ddpm_args* a, const float* x_T, const float* cond, const float* noise,
                    float* z_out) {
    RDM_ENTER(c);
    if (!c || !a || !x_T || !cond || !noise || !z_out) return c ? c->fail(-1, "null argument") : -1;
    return ddpm_sample_impl(c, a, x_T, cond, noise, nullptr, z_out);
}
int rdm_ddpm_sample_seeded(rdm_ctx* c, const rdm_ddpm_args* a, uint64_t seed, int64_t row0, const float* x_T, const float* cond, float* z_out) {
    RDM_ENTER(c);
    if (!c || !a || !cond || !z_out) return c ? c->fail(-1, "null argument") : -1;
    const NoiseSeed ns{seed, row0};
    return ddpm_sample_impl(c, a, x_T, cond, nullptr, &ns, z_out);
}

// ---- device noise: the generator alone (philox.h)
int rdm_rng_words(uint64_t seed, uint32_t row, uint32_t step, uint32_t stream, uint32_t block, uint32_t* out) {
    if (!out) return -1;
    uint32_t w[4];
    philox4x32_10(seed, block, step, row, stream, w);
    for (int k = 0; k < 4; k++) out[k] = w[k];
    return 0;
}
static int op_rng_fill(rdm_ctx* c, const char* who, uint64_t seed, int64_t row0, int64_t B, int64_t per_row, uint32_t step, uint32_t stream,
                       void* out, bool normal) {
    if (!out) return c->fail(-1, "%s: null argument", who);
    if (stream >= RDM_RNG_STREAMS) return c->fail(-1, "%s: stream %u is reserved (0 = starting latent, 1 = per-step noise)", who, stream);
    RDM_TRY(check_noise_rows(c, who, row0, B, per_row));
    if ((uintptr_t)out % 4) return c->fail(-1, "%s: out must be 4-byte aligned", who);
    RngFillParams f{seed, B, per_row, (uint32_t)row0, step, stream, (uint32_t*)out};
    RDM_CHECK_HIP(c, launch_rng_fill(f, normal, c->stream));
    return 0;
}
int rdm_op_rng_words(rdm_ctx* c, uint64_t seed, int64_t row0, int64_t B, int64_t per_row, uint32_t step, uint32_t stream, uint32_t* out) {
    RDM_ENTER(c);
    if (!c) return -1;
    return op_rng_fill(c, "rdm_op_rng_words", seed, row0, B, per_row, step, stream, out, false);
}
int rdm_op_randn(rdm_ctx* c, uint64_t seed, int64_t row0, int64_t B, int64_t per_row, uint32_t step, uint32_t stream, float* out) {
    RDM_ENTER(c);
    if (!c) return -1;
    return op_rng_fill(c, "rdm_op_randn", seed, row0, B, per_row, step, stream, out, true);
}

// ---- the DPM-Solver++ and UniPC step kernels alone
int rdm_op_dpmpp_step(rdm_ctx* c, const float* x, const float* eps, const float* m_prev, long long n, int cfg, float scale, float sqrt_a_s,
                      float sqrt_one_minus_a_s, float c_x, float c_0, float c_1, float* x_out, float* x_dup, float* m_store, float* pred_x0) {
    RDM_ENTER(c);
    if (!x || !eps || !x_out || n < 1) return c->fail(-1, "rdm_op_dpmpp_step: bad argument");
    DpmppStepParams p{};
    p.x = x; p.eps = eps; p.m_prev = m_prev; p.n = n; p.cfg = cfg ? 1 : 0; p.scale = scale; p.sqrt_a_s = sqrt_a_s;
    p.sqrt_one_minus_a_s = sqrt_one_minus_a_s; p.c_x = c_x; p.c_0 = c_0; p.c_1 = c_1;
    p.x_out = x_out; p.x_dup = x_dup; p.m_store = m_store; p.pred_x0 = pred_x0;
    RDM_CHECK_HIP(c, launch_dpmpp_step(p, c->stream));
    return 0;
}
int rdm_op_unipc_step(rdm_ctx* c, const float* u, const float* eps, const float* xc_prev, const float* h1, const float* h2, const float* h3,
                      long long n, int cfg, float scale, const double* coefficients, float* xc_out, float* u_next, float* x_dup,
                      float* m_store, float* pred_x0) {
    RDM_ENTER(c);
    if (!u || !eps || !coefficients || !u_next || n < 1) return c->fail(-1, "rdm_op_unipc_step: bad argument");
    UnipcStepParams p{};
    unipc_fill(p, coefficients);
    if (p.order_c < 0 || p.order_c > 3 || p.order_p < 1 || p.order_p > 3) return c->fail(-1, "rdm_op_unipc_step: orders %d, %d outside 0..3, 1..3", p.order_c, p.order_p);
    const int nh = p.order_c > p.order_p - 1 ? p.order_c : p.order_p - 1;
    if ((p.order_c >= 1 && !xc_prev) || (nh >= 1 && !h1) || (nh >= 2 && !h2) || (nh >= 3 && !h3))
        return c->fail(-1, "rdm_op_unipc_step: orders %d, %d need xc_prev / history operands that are null", p.order_c, p.order_p);
    p.u = u; p.eps = eps; p.xc_prev = xc_prev; p.h1 = h1; p.h2 = h2; p.h3 = h3; p.n = n; p.cfg = cfg ? 1 : 0; p.scale = scale;
    p.xc_out = xc_out; p.u_next = u_next; p.x_dup = x_dup; p.m_store = m_store; p.pred_x0 = pred_x0;
    RDM_CHECK_HIP(c, launch_unipc_step(p, c->stream));
    return 0;
}

// ---- RARM (kernels in rarm.hip)
struct RarmState { int* pos; int* done; long long* tokens; float* logits; };
static RarmState rarm_state(RarmModel& m, int B2) {
    RarmState st{};
    st.pos = (int*)m.state; st.done = (int*)(m.state + 64); st.tokens = (long long*)(m.state + 256);
    // (the logits exist only after rarm_prepare(decode = true): the whole-sequence entries size the buffer without them and must not touch st.logits)
    st.logits = (float*)(m.state + 256 + (((size_t)B2 * 8 + 255) & ~(size_t)255));
    return st;
}
// decode = false: the call runs no decode step (rdm_rarm_forward_seq, rdm_rarm_nll) -- neither the K/V cache, nor the step's logits buffer,
// nor the re-associated cross-attention operands are made
static int rarm_prepare(rdm_ctx* c, int B2, int k, const float* context /*[B,k,cd] dev*/, int B, bool cfg, bool decode = true) {
    RarmModel& m = c->rarm; const rdm_rarm_cfg& g = m.cfg; const int C = m.C, L = g.sequence_length;
    if (decode) RDM_TRY(ensure_bytes(c, &m.cache, &m.cache_bytes, (size_t)g.depth * 2 * B2 * L * C * 2));
    RDM_TRY(ensure_bytes(c, &m.ctxkv, &m.ctxkv_bytes, (size_t)B2 * k * m.kv_total * 2));
    RDM_TRY(ensure_bytes(c, &m.state, &m.state_bytes, 256 + (((size_t)B2 * 8 + 255) & ~(size_t)255) + (decode ? (size_t)B2 * g.vocab_out * 4 : 0)));      // counters, tokens, the step's logits
    RDM_CHECK_HIP(c, hipMemsetAsync(m.state, 0, 256, c->stream));
    // neighbours' keys / values of every layer in one GEMM; the unconditional half of a guided batch attends to ZERO neighbours
    // (transformer.py:237-239), whose projections are zero (to_k / to_v have no bias)
    RDM_CHECK_HIP(c, hipMemsetAsync(m.ctxkv, 0, (size_t)B2 * k * m.kv_total * 2, c->stream));
    // Round 5: the per-sequence re-association pays per-sequence operands (G and U^T: 2 x 128 x C bf16 = 393 KB per sequence and layer
    // where the projections' weights are 2.4 MB per layer for ALL sequences): the one-launch form wins while launches are the cost
    // (<= 128 sequences); from RARM_XGEMM_FROM sequences on the decode step takes norm2 + to_q as a GEMM, the k-key attention and to_out +
    // residual as a GEMM (same box, profiles/r05_rarm_sweep.log: 256 sequences 399 img/s fused vs 378 as GEMMs, 512 sequences 484 vs 489).
    constexpr int RARM_XGEMM_FROM = 384;
    const bool fuse = decode && g.n_heads * k <= 128 && C <= 1024 && C % 64 == 0 && (c->deterministic || B2 < RARM_XGEMM_FROM);
    m.xa_B = 0; m.xa_k = 0;
    if (fuse) {
        RDM_TRY(ensure_bytes(c, &m.xa, &m.xa_bytes, (size_t)g.depth * 2 * B * 128 * C * 2));
        m.xa_B = B; m.xa_k = k;
    }
    return run_with_arena(c, m.arena, m.blob, [&](Ops& o) {
        bf16_t* cb = o.abf((size_t)B * k * g.context_dim);
        if (!o.plan) o.check(launch_cast_f32_bf16(context, cb, (long long)B * k * g.context_dim, c->stream), "cast ctx");
        o.linear(cb, nullptr, g.context_dim, 0, o.w<bf16_t>(m.kvw), nullptr, B * k, m.kv_total, ACT_NONE, nullptr, (bf16_t*)m.ctxkv);
        // the decode step's cross-attention re-associated per sequence (rarm.hip: rarm_xattn_decode_kernel):
        //   G_l[b][(h,j)][:] = (K_bj restricted to head h) W_q / sqrt(d),   UT_l[b][(h,j)][:] = W_o (V_bj restricted to head h)
        if (fuse) {
            constexpr int NP = 128;
            bf16_t* kexp = o.abf((size_t)B * NP * C); bf16_t* vexp = o.abf((size_t)B * NP * C); bf16_t* wqt = o.abf((size_t)C * C);
            if (!o.plan) {
                const bf16_t* kv = (const bf16_t*)m.ctxkv;
                for (int l = 0; l < g.depth; l++) {
                    const RarmBlk& bk = m.blk[l];
                    bf16_t* G = (bf16_t*)m.xa + ((size_t)l * 2) * B * NP * C; bf16_t* UT = G + (size_t)B * NP * C;
                    o.check(launch_expand_heads(kv + (size_t)l * 2 * C, m.kv_total, B, k, g.n_heads, g.d_head, NP, 1.0f / sqrtf((float)g.d_head), kexp, c->stream), "rarm expand K");
                    o.check(launch_expand_heads(kv + (size_t)l * 2 * C + C, m.kv_total, B, k, g.n_heads, g.d_head, NP, 1.0f, vexp, c->stream), "rarm expand V");
                    o.check(launch_transpose_bf16(o.w<bf16_t>(bk.wq2), wqt, C, C, c->stream), "rarm transpose Wq");
                    IgemmParams p = o.base(B * NP, C, C);
                    p.A0 = kexp; p.C0 = C; p.W = wqt; p.out_bf16 = G;
                    o.check(launch_igemm(p, false, 1, c->stream), "rarm xattn G");
                    IgemmParams q = o.base(B * NP, C, C);
                    q.A0 = vexp; q.C0 = C; q.W = o.w<bf16_t>(bk.wo2); q.out_bf16 = UT;
                    o.check(launch_igemm(q, false, 1, c->stream), "rarm xattn UT");
                }
            }
        }
    });
}
// one decode step for B2 sequences: token at position *pos -> logits of the next token
static int rarm_step(rdm_ctx* c, int B2, int k, int pos_hint = -1 /* host's copy of the position processed (profiling only: the kernels read the device counter) */) {
    RarmModel& m = c->rarm; const rdm_rarm_cfg& g = m.cfg; const int C = m.C, L = g.sequence_length;
    RarmState st = rarm_state(m, B2);
    return run_with_arena(c, m.arena, m.blob, [&](Ops& o) {
        o.single_row = true;                              // a decode step is one row per sequence throughout
        float* x = o.af32((size_t)B2 * C);
        bf16_t* ln = o.abf((size_t)B2 * C); bf16_t* qkv = o.abf((size_t)B2 * 3 * C); bf16_t* ao = o.abf((size_t)B2 * C);
        bf16_t* q2 = o.abf((size_t)B2 * C); bf16_t* ff = o.abf((size_t)B2 * 4 * C);
        if (!o.plan) o.check(launch_rarm_embed(st.tokens, o.w<float>(m.emb), o.w<float>(m.pos), st.pos, x, B2, C, g.vocab_in, c->stream), "rarm embed");
        const float scale = 1.0f / sqrtf((float)g.d_head);
        const bool ln3_fused = m.xa_B > 0 && m.xa_k == k;      // the fused cross-attention kernel also emits norm3 of its output rows
        for (int l = 0; l < g.depth; l++) {
            const RarmBlk& b = m.blk[l];
            if (!o.linear_ln(x, o.w<float>(b.ln1g), o.w<float>(b.ln1b), C, o.w<bf16_t>(b.wqkv), nullptr, B2, 3 * C, ACT_NONE, qkv)) {
                o.layernorm(x, 1, o.w<float>(b.ln1g), o.w<float>(b.ln1b), ln, 0, B2, C);
                o.linear(ln, nullptr, C, 0, o.w<bf16_t>(b.wqkv), nullptr, B2, 3 * C, ACT_NONE, nullptr, qkv);
            }
            if (!o.plan) {
                RarmAttnParams p{}; p.q = qkv; p.ldq = 3 * C; p.k_new = qkv + C; p.v_new = qkv + 2 * C;
                p.Kc = (bf16_t*)m.cache + ((size_t)l * 2) * B2 * L * C; p.Vc = (bf16_t*)m.cache + ((size_t)l * 2 + 1) * B2 * L * C;
                p.batch_stride = (long long)L * C; p.nkv = L; p.pos = st.pos; p.scale = scale; p.out = ao; p.ldo = C;
                // Head-major cache [B][head][L][64] (round 5): a (head, sequence) block reads ONE contiguous run of (pos + 1) x 128 bytes
                // instead of 128-byte pieces 2 C bytes apart.  The cache is private to this kernel (it appends the new row itself).
                p.row_stride = g.d_head; p.head_stride = (long long)L * g.d_head;
                // bytes of the K / V cache rows this step reads (positions 0 .. pos): what bounds the launch at big batches
                o.tag = "rarm.cache_attention";
                o.prof_begin(RDM_PROF_ATTENTION, pos_hint >= 0 ? (double)B2 * (pos_hint + 1) * C * 4.0 : 0.0, B2, pos_hint + 1, C);
                o.check(launch_rarm_decode_attention(p, g.n_heads, B2, c->stream), "rarm self attention");
                o.prof_end();
            }
            o.linear(ao, nullptr, C, 0, o.w<bf16_t>(b.wo1), o.w<float>(b.bo1), B2, C, ACT_NONE, nullptr, nullptr, x, x);
            if (m.xa_B > 0 && m.xa_k == k) {      // norm2 + to_q + attention over the neighbours + to_out + residual in one launch
                if (!o.plan) {
                    RarmXattnParams xp{}; xp.x = x; xp.ln_g = o.w<float>(b.ln2g); xp.ln_b = o.w<float>(b.ln2b); xp.ln_eps = 1e-5f;
                    xp.G = (const bf16_t*)m.xa + ((size_t)l * 2) * m.xa_B * 128 * C; xp.UT = xp.G + (size_t)m.xa_B * 128 * C;
                    xp.bias = o.w<float>(b.bo2); xp.B2 = B2; xp.Bc = m.xa_B; xp.C = C; xp.NP = 128; xp.heads = g.n_heads; xp.k = k;
                    if (ln3_fused) { xp.ln3_g = o.w<float>(b.ln3g); xp.ln3_b = o.w<float>(b.ln3b); xp.ln3_out = ln; }
                    o.check(launch_rarm_xattn_decode(xp, c->stream), "rarm fused cross attention");
                }
            } else {
            if (!o.linear_ln(x, o.w<float>(b.ln2g), o.w<float>(b.ln2b), C, o.w<bf16_t>(b.wq2), nullptr, B2, C, ACT_NONE, q2)) {
                o.layernorm(x, 1, o.w<float>(b.ln2g), o.w<float>(b.ln2b), ln, 0, B2, C);
                o.linear(ln, nullptr, C, 0, o.w<bf16_t>(b.wq2), nullptr, B2, C, ACT_NONE, nullptr, q2);
            }
            if (!o.plan) {
                RarmAttnParams p{}; p.q = q2; p.ldq = C; p.Kc = (bf16_t*)m.ctxkv + (size_t)l * 2 * C; p.Vc = (bf16_t*)m.ctxkv + (size_t)l * 2 * C + C;
                p.batch_stride = (long long)k * m.kv_total; p.row_stride = m.kv_total; p.nkv = k; p.scale = scale; p.out = ao; p.ldo = C;
                o.check(launch_rarm_decode_attention(p, g.n_heads, B2, c->stream), "rarm cross attention");
            }
            o.linear(ao, nullptr, C, 0, o.w<bf16_t>(b.wo2), o.w<float>(b.bo2), B2, C, ACT_NONE, nullptr, nullptr, x, x);
            }
            if (ln3_fused) {      // norm3 left the cross-attention kernel with the finished rows: a plain GEGLU GEMM on the bf16 operand
                o.linear(ln, nullptr, C, 0, o.w<bf16_t>(b.wff1), o.w<float>(b.bff1), B2, 8 * C, ACT_GEGLU, nullptr, ff);
            } else if (!o.linear_ln(x, o.w<float>(b.ln3g), o.w<float>(b.ln3b), C, o.w<bf16_t>(b.wff1), o.w<float>(b.bff1), B2, 8 * C, ACT_GEGLU, ff)) {
                o.layernorm(x, 1, o.w<float>(b.ln3g), o.w<float>(b.ln3b), ln, 0, B2, C);
                o.linear(ln, nullptr, C, 0, o.w<bf16_t>(b.wff1), o.w<float>(b.bff1), B2, 8 * C, ACT_GEGLU, nullptr, ff);
            }
            o.linear(ff, nullptr, 4 * C, 0, o.w<bf16_t>(b.wff2), o.w<float>(b.bff2), B2, C, ACT_NONE, nullptr, nullptr, x, x);
        }
        if (!o.plan) o.check(launch_cast_f32_bf16(x, ln, (long long)B2 * C, c->stream), "cast x");
        o.linear(ln, nullptr, C, 0, o.w<bf16_t>(m.wpo), o.w<float>(m.bpo), B2, g.vocab_out, ACT_NONE, nullptr, nullptr, st.logits);
    });
}
static int rarm_check(rdm_ctx* c, int b, int k, int positions) {
    RarmModel& m = c->rarm;
    if (!m.loaded) return c->fail(-1, "rarm weights not loaded");
    if (b < 1 || k < 1 || k > 1024) return c->fail(-1, "bad rarm shape b=%d k=%d", b, k);
    if (positions < 1 || positions > m.cfg.sequence_length)
        return c->fail(-1, "%d positions exceed the positional encoding (sequence_length %d)", positions, m.cfg.sequence_length);
    return 0;
}
// column i of a [b, t] int64 token matrix -> the current-token buffer (optionally duplicated for the unconditional half)
static int rarm_set_tokens(rdm_ctx* c, RarmState& st, const int64_t* tokens, int b, int t, int i, bool dup) {
    RDM_CHECK_HIP(c, hipMemcpy2DAsync(st.tokens, 8, tokens + i, (size_t)t * 8, 8, b, hipMemcpyDeviceToDevice, c->stream));
    if (dup) RDM_CHECK_HIP(c, hipMemcpy2DAsync(st.tokens + b, 8, tokens + i, (size_t)t * 8, 8, b, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}
// ---- the whole-sequence pass: RetrievalPatchTransformer.forward over all t positions of B2 sequences at once (attention.py:252-272),
// the transformer of rarm_step with t rows per sequence -- tiled GEMMs (single_row stays false: no kernel on this path is chosen by the
// row count in deterministic mode), the causal d_head-64 kernel over the sequence itself, small_attention over its k neighbour rows of
// ctxkv (rarm_prepare; the zeroed rows of a guided batch's unconditional half give zero attention output, as in the decode step).
// Sequences are independent, so they are walked in ranges of whole sequences of at most RARM_SEQ_ROWS rows: that bounds the [rows, 4C]
// hidden tensor (201 MB at C = 768) whatever b * t is.  What leaves a range:
//   logits_out  : the head GEMM's rows, [B2, t, V] fp32 (rdm_rarm_forward_seq)
//   nll_out     : -log softmax(logits)[target] per row; the head GEMM runs in pieces of RARM_NLL_ROWS rows into scratch, [b * t, V] never exists
//   fill_cache  : the K / V rows of positions 0 .. t-1 into the decode step's cache (rdm_rarm_sample_prefill); no head at all
// tokens: [tok_rows][tok_ld] int64, sequence s reads row s % tok_rows.
constexpr int RARM_SEQ_ROWS = 32768;
constexpr int RARM_NLL_ROWS = 2048;
static int rarm_seq_body(rdm_ctx* c, const int64_t* tokens, int tok_ld, int tok_rows, int B2, int t, int k, float* logits_out, const int64_t* targets,
                         float* nll_out, bool fill_cache) {
    RarmModel& m = c->rarm; const rdm_rarm_cfg& g = m.cfg; const int C = m.C, L = g.sequence_length, V = g.vocab_out;
    const int per = t >= RARM_SEQ_ROWS ? 1 : RARM_SEQ_ROWS / t;          // sequences per range
    const int nbmax = B2 < per ? B2 : per;
    return run_with_arena(c, m.arena, m.blob, [&](Ops& o) {
        const size_t Mmax = (size_t)nbmax * t;
        float* x = o.af32(Mmax * C);
        bf16_t* ln = o.abf(Mmax * C); bf16_t* qkv = o.abf(Mmax * 3 * C); bf16_t* ao = o.abf(Mmax * C);
        bf16_t* q2 = o.abf(Mmax * C); bf16_t* ff = o.abf(Mmax * 4 * C);
        float* lg = nll_out ? o.af32((size_t)(Mmax < (size_t)RARM_NLL_ROWS ? Mmax : (size_t)RARM_NLL_ROWS) * V) : nullptr;
        if (o.plan) return;
        const float scale = 1.0f / sqrtf((float)g.d_head);
        for (int s0 = 0; s0 < B2 && o.rc == 0; s0 += per) {
            const int nb = B2 - s0 < per ? B2 - s0 : per, M = nb * t;
            o.check(launch_rarm_embed_seq((const long long*)tokens, tok_ld, tok_rows, s0, o.w<float>(m.emb), o.w<float>(m.pos), x, M, t, C, g.vocab_in, c->stream),
                    "rarm embed");
            for (int l = 0; l < g.depth; l++) {
                const RarmBlk& b = m.blk[l];
                o.layernorm(x, 1, o.w<float>(b.ln1g), o.w<float>(b.ln1b), ln, 0, M, C);
                o.linear(ln, nullptr, C, 0, o.w<bf16_t>(b.wqkv), nullptr, M, 3 * C, ACT_NONE, nullptr, qkv);
                bf16_t* kc = fill_cache ? (bf16_t*)m.cache + (((size_t)l * 2) * B2 + s0) * L * C : nullptr;
                bf16_t* vc = fill_cache ? (bf16_t*)m.cache + (((size_t)l * 2 + 1) * B2 + s0) * L * C : nullptr;
                o.tag = "rarm.causal_attention";
                o.causal_d64(qkv, 3 * C, ao, C, nb, t, g.n_heads, scale, kc, vc, L);
                o.linear(ao, nullptr, C, 0, o.w<bf16_t>(b.wo1), o.w<float>(b.bo1), M, C, ACT_NONE, nullptr, nullptr, x, x);
                o.layernorm(x, 1, o.w<float>(b.ln2g), o.w<float>(b.ln2b), ln, 0, M, C);
                o.linear(ln, nullptr, C, 0, o.w<bf16_t>(b.wq2), nullptr, M, C, ACT_NONE, nullptr, q2);
                const bf16_t* kv = (const bf16_t*)m.ctxkv + (size_t)s0 * k * m.kv_total + (size_t)l * 2 * C;
                o.small_attention(q2, C, kv, m.kv_total, kv + C, m.kv_total, ao, C, nb, t, k, g.n_heads, g.d_head, 0, scale, "rarm cross attention");
                o.linear(ao, nullptr, C, 0, o.w<bf16_t>(b.wo2), o.w<float>(b.bo2), M, C, ACT_NONE, nullptr, nullptr, x, x);
                o.layernorm(x, 1, o.w<float>(b.ln3g), o.w<float>(b.ln3b), ln, 0, M, C);
                o.linear(ln, nullptr, C, 0, o.w<bf16_t>(b.wff1), o.w<float>(b.bff1), M, 8 * C, ACT_GEGLU, nullptr, ff);
                o.linear(ff, nullptr, 4 * C, 0, o.w<bf16_t>(b.wff2), o.w<float>(b.bff2), M, C, ACT_NONE, nullptr, nullptr, x, x);
            }
            if (!logits_out && !nll_out) continue;
            o.check(launch_cast_f32_bf16(x, ln, (long long)M * C, c->stream), "cast x");
            const size_t row0 = (size_t)s0 * t;
            if (logits_out) o.linear(ln, nullptr, C, 0, o.w<bf16_t>(m.wpo), o.w<float>(m.bpo), M, V, ACT_NONE, nullptr, nullptr, logits_out + row0 * V);
            if (nll_out) {
                for (int r0 = 0; r0 < M && o.rc == 0; r0 += RARM_NLL_ROWS) {
                    const int nr = M - r0 < RARM_NLL_ROWS ? M - r0 : RARM_NLL_ROWS;
                    o.linear(ln + (size_t)r0 * C, nullptr, C, 0, o.w<bf16_t>(m.wpo), o.w<float>(m.bpo), nr, V, ACT_NONE, nullptr, nullptr, lg);
                    o.check(launch_rarm_nll(lg, nr, V, (const long long*)targets + row0 + r0, nll_out + row0 + r0, c->stream), "rarm nll");
                }
            }
        }
    });
}
static int rarm_seq_check(rdm_ctx* c, int b, int k, int positions) {
    RDM_TRY(rarm_check(c, b, k, positions));
    if (k > 128) return c->fail(-1, "the whole-sequence pass attends at most 128 neighbours per sequence, got k=%d", k);
    return 0;
}
int rdm_rarm_forward(rdm_ctx* c, const int64_t* tokens, int b, int t, const float* context, int k, float* logits_out) {
    RDM_ENTER(c);
    if (!tokens || !context || !logits_out) return c->fail(-1, "null argument");
    RDM_TRY(rarm_check(c, b, k, t));
    RarmModel& m = c->rarm;
    RDM_TRY(rarm_prepare(c, b, k, context, b, false));
    RarmState st = rarm_state(m, b);
    const size_t V = m.cfg.vocab_out;
    for (int i = 0; i < t; i++) {
        RDM_TRY(rarm_set_tokens(c, st, tokens, b, t, i, false));
        RDM_CHECK_HIP(c, launch_set_int(st.pos, i, c->stream));
        RDM_TRY(rarm_step(c, b, k));
        RDM_CHECK_HIP(c, hipMemcpy2DAsync(logits_out + (size_t)i * V, (size_t)t * V * 4, st.logits, V * 4, V * 4, b, hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
}
int rdm_rarm_forward_seq(rdm_ctx* c, const int64_t* tokens, int b, int t, const float* context, int k, float* logits_out) {
    RDM_ENTER(c);
    if (!tokens || !context || !logits_out) return c->fail(-1, "null argument");
    RDM_TRY(rarm_seq_check(c, b, k, t));
    RDM_TRY(rarm_prepare(c, b, k, context, b, false, false));
    return rarm_seq_body(c, tokens, t, b, b, t, k, logits_out, nullptr, nullptr, false);
}
int rdm_rarm_nll(rdm_ctx* c, const int64_t* tokens, const int64_t* targets, int b, int t, const float* context, int k, float* nll_out) {
    RDM_ENTER(c);
    if (!tokens || !targets || !context || !nll_out) return c->fail(-1, "null argument");
    RDM_TRY(rarm_seq_check(c, b, k, t));
    RDM_TRY(rarm_prepare(c, b, k, context, b, false, false));
    return rarm_seq_body(c, tokens, t, b, b, t, k, nullptr, targets, nll_out, false);
}
static int rarm_sample_run(rdm_ctx* c, const rdm_rarm_sample_args* a, float top_p, const int64_t* cond_tokens, const float* context,
                           const float* uniforms, int64_t* tokens_out, bool prefill = false) {
    RDM_ENTER(c);
    if (!a || !cond_tokens || !context || !uniforms || !tokens_out) return c->fail(-1, "null argument");
    if (a->cond_len < 1 || a->steps < 1 || a->temperature <= 0.f) return c->fail(-1, "bad sampling arguments");
    RDM_TRY(rarm_check(c, a->batch, a->k, a->cond_len + a->steps - 1));
    RarmModel& m = c->rarm;
    const bool cfg = a->guidance_scale > 1.0f;
    const int B = a->batch, B2 = cfg ? 2 * B : B, k = a->k;
    RDM_TRY(rarm_prepare(c, B2, k, context, B, cfg));
    RarmState st = rarm_state(m, B2);
    int i0 = 0;
    if (prefill && a->cond_len > 1) {      // positions 0 .. cond_len-2 in one whole-sequence pass that fills the K/V cache; the loop below starts at the last one
        i0 = a->cond_len - 1;
        RDM_TRY(rarm_seq_body(c, cond_tokens, a->cond_len, B, B2, i0, k, nullptr, nullptr, nullptr, true));
    }
    for (int i = i0; i < a->cond_len; i++) {                   // feed the conditioning tokens (the sos token)
        RDM_TRY(rarm_set_tokens(c, st, cond_tokens, B, a->cond_len, i, cfg));
        RDM_CHECK_HIP(c, launch_set_int(st.pos, i, c->stream));
        if (i + 1 < a->cond_len) RDM_TRY(rarm_step(c, B2, k, i));
    }
    RarmSampleParams sp{}; sp.logits = st.logits; sp.vocab = m.cfg.vocab_out; sp.B = B; sp.cfg = cfg ? 1 : 0; sp.scale = a->guidance_scale;
    sp.temperature = a->temperature; sp.top_k = a->top_k > 0 ? a->top_k : m.cfg.vocab_out; sp.uniforms = uniforms; sp.pos = st.pos;
    sp.pos0 = a->cond_len - 1; sp.steps = a->steps; sp.tokens_out = (long long*)tokens_out; sp.next_tokens = st.tokens; sp.done = st.done;
    sp.top_p = top_p;
    for (int s_ = 0; s_ < a->steps; s_++) {                    // every step: the same launches (the step counter lives on the device)
        RDM_TRY(rarm_step(c, B2, k, a->cond_len - 1 + s_));
        RDM_CHECK_HIP(c, launch_rarm_sample(sp, c->stream));
    }
    return 0;
}
int rdm_rarm_sample_prefill(rdm_ctx* c, const rdm_rarm_sample_args* a, float top_p, const int64_t* cond_tokens, const float* context,
                            const float* uniforms, int64_t* tokens_out) {
    RDM_ENTER(c);
    if (!(top_p > 0.f && top_p <= 1.f)) return c->fail(-1, "rdm_rarm_sample_prefill: top_p must lie in (0, 1], got %g", (double)top_p);
    if (a && a->k > 128) return c->fail(-1, "the whole-sequence pass attends at most 128 neighbours per sequence, got k=%d", a->k);
    return rarm_sample_run(c, a, top_p, cond_tokens, context, uniforms, tokens_out, true);
}
int rdm_rarm_sample(rdm_ctx* c, const rdm_rarm_sample_args* a, const int64_t* cond_tokens, const float* context, const float* uniforms,
                    int64_t* tokens_out) {
    return rarm_sample_run(c, a, 1.0f, cond_tokens, context, uniforms, tokens_out);
}
int rdm_rarm_sample_top_p(rdm_ctx* c, const rdm_rarm_sample_args* a, float top_p, const int64_t* cond_tokens, const float* context,
                          const float* uniforms, int64_t* tokens_out) {
    RDM_ENTER(c);
    if (!(top_p > 0.f && top_p <= 1.f)) return c->fail(-1, "rdm_rarm_sample_top_p: top_p must lie in (0, 1], got %g", (double)top_p);
    return rarm_sample_run(c, a, top_p, cond_tokens, context, uniforms, tokens_out);
}

// ---- operator-level entries (parity tests, op benchmarks, the training path): argument checks, then the executors' dispatch (Ops) on
// caller-owned weights.  Their derived copies are packed per call, unless RDM_OP_FRAG_CACHE=1: the caller promises constant weights (op benchmarks).
static Ops op_exec(rdm_ctx* c) {
    static const bool cache = rdm_env_int(getenv("RDM_OP_FRAG_CACHE"), 0) != 0;
    Ops o{c, nullptr, nullptr, /*plan=*/false};
    o.const_weights = cache;
    return o;
}
static int op_linear(rdm_ctx* c, const void* a, const void* w, const float* bias, const void* res, void* out, float* out_f32,
                     int M, int N, int K, int act, float alpha, const float* rowvec, int rows_per_group) {
    Ops o = op_exec(c);
    o.linear((const bf16_t*)a, nullptr, K, 0, (const bf16_t*)w, bias, M, N, act, (const bf16_t*)res, (bf16_t*)out, out_f32, nullptr, 0,
             rowvec, N, rows_per_group, 0, alpha);
    return o.rc;
}
int rdm_op_linear(rdm_ctx* c, const void* a, const void* w, const float* bias, const void* res, void* out, float* out_f32,
                  int M, int N, int K, int act, float alpha) {
    RDM_ENTER(c);
    return op_linear(c, a, w, bias, res, out, out_f32, M, N, K, act, alpha, nullptr, 1);
}
int rdm_op_linear_rowvec(rdm_ctx* c, const void* a, const void* w, const float* bias, const float* rowvec, int rows_per_group, const void* res,
                         void* out, int M, int N, int K) {
    RDM_ENTER(c);
    if (!rowvec || rows_per_group < 1) return c->fail(-1, "rdm_op_linear_rowvec: rowvec and rows_per_group >= 1 required");
    return op_linear(c, a, w, bias, res, out, nullptr, M, N, K, ACT_NONE, 1.0f, rowvec, rows_per_group);
}
int rdm_op_linear_ln(rdm_ctx* c, const void* x, const void* w, const float* bias, const float* gamma, const float* beta, void* out,
                     int M, int N, int K, int act, float eps) {
    RDM_ENTER(c);
    if (!x || !w || !gamma || !beta || !out) return c->fail(-1, "rdm_op_linear_ln: null argument");
    IgemmParams p{}; p.M = M; p.N = N; p.K = K; p.alpha = 1.f; p.ldo = (act == ACT_GEGLU) ? N / 2 : N; p.zero_page = c->zero_page;
    p.Hin = p.Win = p.Hout = p.Wout = 1; p.stride = 1; p.rows_per_sample = 1;
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
    o.conv3((const bf16_t*)x0, (const bf16_t*)x1, C0, C1, (const bf16_t*)w, bias, B, Hin, Win, N, stride, ups, rowvec, rowvec_ld,
            (const bf16_t*)res, (bf16_t*)out);
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
    o.vq_nearest(z, codebook, norms, M, N, E, c->samp + nbytes, idx_out, nullptr);
    return o.rc;
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
    IgemmParams p{}; p.M = M; p.N = N; p.K = K; p.alpha = alpha; p.ldo = N; p.zero_page = c->zero_page;
    p.Hin = p.Win = p.Hout = p.Wout = 1; p.stride = 1; p.rows_per_sample = 1;
    p.A0 = (const bf16_t*)a; p.C0 = K; p.W = (const bf16_t*)w; p.out_bf16 = (bf16_t*)out_bf16; p.out_f32 = out_f32;
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
    o.groupnorm((const bf16_t*)x0, (const bf16_t*)x1, C0, C1, B, HW, gamma, beta, eps, silu, (bf16_t*)out);
    return o.rc;
}
int rdm_op_layernorm(rdm_ctx* c, const void* x, int in_is_f32, const float* gamma, const float* beta, int M, int C, float eps,
                     void* out) {
    RDM_ENTER(c);
    Ops o = op_exec(c);
    o.layernorm(x, in_is_f32, gamma, beta, out, 0, M, C, -1, eps);
    return o.rc;
}
int rdm_op_self_attention(rdm_ctx* c, const void* qk, const void* vt, int B, int n, int heads, void* out) {
    RDM_ENTER(c);
    Ops o = op_exec(c);
    o.flash_d32((const bf16_t*)qk, 2 * heads * 32, nullptr, (const bf16_t*)vt, (bf16_t*)out, B, n, heads);
    return o.rc;
}
int rdm_op_self_attention_qkv(rdm_ctx* c, const void* qkv, int B, int n, int heads, void* out) {
    RDM_ENTER(c);
    if (n % 64 != 0) return c->fail(-3, "rdm_op_self_attention_qkv: n = %d must be a multiple of 64 (token-major V is read by the LDS-shared kernel only)", n);
    Ops o = op_exec(c);
    o.flash_d32((const bf16_t*)qkv, 3 * heads * 32, (const bf16_t*)qkv + 2 * heads * 32, nullptr, (bf16_t*)out, B, n, heads);
    return o.rc;
}
// G / U arrive in their natural layout: their fragment-ordered images are packed per call into bwd_tmp
static int op_xattn_fused(rdm_ctx* c, const void* x, const float* ln_g, const float* ln_b, float ln_eps, const void* G, const void* U,
                          const float* bias, const void* res, void* out, int B, int n, int C, int NP, int ncols, int group,
                          const float* ln3_g, const float* ln3_b, void* ln3_out) {
    const size_t img = (size_t)B * NP * C;
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, 2 * img * 2));
    bf16_t* Gp = (bf16_t*)c->bwd_tmp; bf16_t* Up = Gp + img;
    Ops o = op_exec(c);
    o.check(launch_xattn_pack((const bf16_t*)G, (const bf16_t*)U, Gp, Up, B, NP, C, c->stream), "xattn pack");
    o.xattn_fused((const bf16_t*)x, ln_g, ln_b, ln_eps, Gp, Up, bias, (const bf16_t*)res, (bf16_t*)out, B * n, n, C, NP, ncols, group,
                  ln3_g, ln3_b, (bf16_t*)ln3_out);
    return o.rc;
}
int rdm_op_xattn_fused(rdm_ctx* c, const void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G, const void* U,
                       const float* bias, const void* res, int B, int n, int C, int NP, int ncols, int group, void* out) {
    RDM_ENTER(c);
    if ((ln_gamma != nullptr) != (ln_beta != nullptr) || (ln_gamma && res)) return c->fail(-3, "rdm_op_xattn_fused: LayerNorm needs gamma and beta, and then the residual is x itself (res must be null)");
    if (!xattn_fused_supported(Ops::xattn_params(B * n, n, C, NP, ncols, group))) return c->fail(-3, "rdm_op_xattn_fused: unsupported shape (n %% 32, C %% 64, NP %% 32, ncols <= min(NP, 128), group 1 / 2 / 4): n %d C %d NP %d ncols %d group %d", n, C, NP, ncols, group);
    return op_xattn_fused(c, x, ln_gamma, ln_beta, ln_eps, G, U, bias, res, out, B, n, C, NP, ncols, group, nullptr, nullptr, nullptr);
}
int rdm_op_xattn_fused_ln3(rdm_ctx* c, void* x, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G, const void* U,
                           const float* bias, int B, int n, int C, int NP, int ncols, int group, const float* ln3_gamma, const float* ln3_beta, void* ln3_out) {
    RDM_ENTER(c);
    if (!x || !ln_gamma || !ln_beta || !ln3_gamma || !ln3_beta || !ln3_out) return c->fail(-1, "rdm_op_xattn_fused_ln3: null argument");
    if (!xattn_fused_supported(Ops::xattn_params(B * n, n, C, NP, ncols, group))) return c->fail(-3, "rdm_op_xattn_fused_ln3: unsupported shape: n %d C %d NP %d ncols %d group %d", n, C, NP, ncols, group);
    return op_xattn_fused(c, x, ln_gamma, ln_beta, ln_eps, G, U, bias, nullptr, x, B, n, C, NP, ncols, group, ln3_gamma, ln3_beta, ln3_out);
}
int rdm_op_head_conv(rdm_ctx* c, const void* x, const float* gn_gamma, const float* gn_beta, float gn_eps, const float* w, const float* bias,
                     int B, int H, int W, int C, int Cout, float* out) {
    RDM_ENTER(c);
    if ((gn_gamma != nullptr) != (gn_beta != nullptr)) return c->fail(-3, "rdm_op_head_conv: GroupNorm needs gamma and beta");
    if (gn_gamma) RDM_TRY(ensure_gn_partial(c, B));
    Ops o = op_exec(c);
    if (!head_conv_supported(o.head_params((const bf16_t*)x, B, H, W, C, gn_gamma, gn_beta, gn_eps, w, bias, Cout, out, nullptr)))
        return c->fail(-3, "rdm_op_head_conv: unsupported shape (C %% 32, C <= 240, W %% 32, H %% 2, Cout <= 8, C %% 32 groups): C %d H %d W %d Cout %d", C, H, W, Cout);
    RDM_TRY(ensure_bytes(c, &c->bwd_tmp, &c->bwd_tmp_bytes, head_conv_wp_bytes(C)));
    o.head((const bf16_t*)x, B, H, W, C, C, gn_gamma, gn_beta, gn_eps, w, bias, Cout, out, nullptr, (bf16_t*)c->bwd_tmp);
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
    o.causal_d64((const bf16_t*)qkv, ldq, (bf16_t*)out, ldo, B, n, heads, scale, (bf16_t*)kcache, (bf16_t*)vcache, L);
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
    o.vq_attention((const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv, bias_v, (bf16_t*)out, ldo, B, n, C, scale);
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
    o.small_attention((const bf16_t*)q, ldq, (const bf16_t*)k, ldkv, (const bf16_t*)v, ldkv, (bf16_t*)out, ldo, B, nq, nkv, heads, D, causal, scale,
                      "small attention");
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
    o.single_row = true;
    if (ln_x) {
        if (!gamma || !beta || !out_bf16 || out_f32 || res_f32) return c->fail(-1, "rdm_op_linear_rows: the LayerNorm form takes gamma, beta and a bf16 output, no residual");
        if (!o.linear_ln(ln_x, gamma, beta, K, (const bf16_t*)w, bias, M, N, act, (bf16_t*)out_bf16))
            return c->fail(-5, "rdm_op_linear_rows: shape not taken by the LayerNorm-in-kernel form (M=%d N=%d K=%d act=%d, %s mode)", M, N, K, act,
                           c->deterministic ? "deterministic" : "fast");
        return o.rc;
    }
    o.linear((const bf16_t*)a, nullptr, K, 0, (const bf16_t*)w, bias, M, N, act, nullptr, (bf16_t*)out_bf16, out_f32, res_f32);
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
