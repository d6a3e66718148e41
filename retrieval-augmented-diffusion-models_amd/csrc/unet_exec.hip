// The UNet executor of librdm_hip: the conditioning's K/V and re-associated cross-attention operands, the time-embedding rows,
// unet_body, rdm_unet_forward, rdm_debug_tap, and the three functions the samplers use (declared in host.h: unet_prepare_kv,
// unet_emb_table, unet_forward_impl).  Calls only host.h: the Ops methods (dispatch.hip) and the launch_* of kernels.h.
//
// The executor mirrors the reference's module graphs
//   UNetModel.__init__/forward      rdm/modules/diffusionmodules/openaimodel.py:66-371
//   SpatialTransformer / BasicTransformerBlock / CrossAttention   rdm/modules/attention.py:20-196
//   [ldm, un-vendored] ResBlock, Down/Upsample
// but is laid out for the hardware: NHWC bf16 activations (a 1x1 conv, a Linear and a token
// sequence are the same [M,C] matrix), fused epilogues (bias, time-embedding add, residual, GEGLU,
// SiLU), no materialised skip-concat, cross-attention K/V and all 22 emb_layers projections batched
// into one GEMM each, K/V of the retrieved neighbours computed once per sample() call instead of
// once per step per layer.
#include "host.h"

// ------------------------------------------------------------------------------------ UNet forward
// kv: bf16 [B*k, kv_total] cross-attention keys/values for every SpatialTransformer (rdm_unet_forward: per call; the samplers: unet_prepare_kv)
static void unet_compute_kv(Ops& o, UNet& u, const float* context, int B, int k, bf16_t* kv_out) {
    const int cd = u.cfg.context_dim;
    bf16_t* cb = o.abf((size_t)B * k * cd);
    if (!o.plan) o.check(launch_cast_f32_bf16(context, cb, (long long)B * k * cd, o.c->stream), "cast ctx");
    o.linear({.A0 = cb, .C0 = cd, .W = o.w<bf16_t>(u.kvw), .M = B * k, .N = u.kv_total, .out_bf16 = kv_out});
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
    o.tag = "time_embed";             // (single_row: one row per sample, see LinearOp)
    o.linear({.A0 = temb, .C0 = mc, .W = o.w<bf16_t>(u.te0w), .bias = o.w<float>(u.te0b), .M = B, .N = ted, .act = ACT_SILU, .out_bf16 = e1, .single_row = true});
    bf16_t* semb = o.abf((size_t)B * ted);
    o.linear({.A0 = e1, .C0 = ted, .W = o.w<bf16_t>(u.te2w), .bias = o.w<float>(u.te2b), .M = B, .N = ted, .act = ACT_SILU, .out_bf16 = semb, .single_row = true});
    o.linear({.A0 = semb, .C0 = ted, .W = o.w<bf16_t>(u.embw), .bias = o.w<float>(u.embb), .M = B, .N = u.emb_total, .out_f32 = emb_all,
              .single_row = true});      // all 22 emb_layers in one GEMM
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
    // halves -- and so does that transformer up to its cross-attention, the first op that reads the context: its GroupNorm, proj_in,
    // norm1, the q | k | v projection and the self-attention (at 32 x 32: one of the model's three most expensive attention layers).
    // All of these run once on Bfull/2 samples.  The prefix ends at attn1.to_out, which runs on all Bfull samples (its start values
    // differ between the halves: the bias fold below) and reads its operand and its residual with a row wrap; the block's input and
    // the skip tensors already pushed are wrapped by their readers or duplicated there (leave_prefix).  Deterministic mode, and
    // rdm_debug_guidance_prefix(ctx, 0), end the prefix in front of the transformer.  B below is the batch the CURRENT layer runs on.
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
    // Leaving the prefix at transformer s0, whose input is `in`: from here on B = Bfull.
    auto leave_prefix = [&](const StW& s0, Act& in) {
        // the activation itself is duplicated only where its readers cannot wrap the batch index instead (transformer())
        const int n0 = in.H * in.W, Mfull = Bfull * n0;
        if (!o.c->deterministic && o.lin4_takes({.C0 = 4 * s0.lc, .C1 = s0.c, .M = Mfull, .N = s0.c, .res_wrap_rows = (Bfull / 2) * n0})) in.half = true;
        else expand(in);
        for (Act& a : hs) { if (o.c->deterministic) expand(a); else a.half = true; }
        B = Bfull;
    };
    const bool through_attn1 = o.c->prefix_through_attn1 && !o.c->deterministic;

    auto resblock = [&](const ResW& r, const Act& a, Act* skip) -> Act {
        const int C0 = a.C, C1 = skip ? skip->C : 0, HW = a.H * a.W, M = B * HW;
        int wrap_b = 0;                                    // > 0: the skip tensor holds Bfull/2 samples, read with a batch wrap
        if (skip && skip->half) {
            if (B == Bfull && r.skip && o.lin4_takes({.C0 = C0, .C1 = C1, .M = M, .N = r.cout, .a1_wrap_rows = (Bfull / 2) * HW})) wrap_b = Bfull / 2;
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
            o.linear({.A0 = a.p, .A1 = x1, .C0 = C0, .C1 = C1, .W = o.w<bf16_t>(r.wsk), .bias = o.w<float>(r.bsk), .M = M, .N = r.cout, .out_bf16 = sk,
                      .a1_wrap_rows = wrap_b * HW, .sample_rows = HW});
            res = sk;
        }
        bf16_t* n1 = o.abf((size_t)M * r.cin);
        o.tag = "res.gn1";
        o.groupnorm({.x0 = a.p, .x1 = x1, .C0 = C0, .C1 = C1, .HW = HW, .B = B, .L0 = a.L, .L1 = skip ? skip->L : 0,
                     .gamma = o.w<float>(r.gn1g), .beta = o.w<float>(r.gn1b), .eps = 1e-5f, .silu = 1, .out = n1, .x1_bmod = wrap_b});
        o.tap(1, n1, (size_t)M * r.cin * 2);
        bf16_t* h1 = o.abf((size_t)M * r.cout);
        o.tag = "res.conv1";
        o.conv3({.A0 = n1, .C0 = r.cin, .W = o.w<bf16_t>(r.w1), .bias = o.w<float>(r.b1), .B = B, .Hin = a.H, .Win = a.W, .N = r.cout, .out_bf16 = h1,
                 .rowvec = emb_all + r.emb_off, .rowvec_ld = emb_ld});
        o.tap(2, h1, (size_t)M * r.cout * 2);
        bf16_t* n2 = o.abf((size_t)M * r.cout);
        o.tag = "res.gn2";
        o.groupnorm({.x0 = h1, .C0 = r.cout, .HW = HW, .B = B, .L0 = r.lout, .gamma = o.w<float>(r.gn2g), .beta = o.w<float>(r.gn2b), .eps = 1e-5f, .silu = 1, .out = n2});
        o.tap(3, n2, (size_t)M * r.cout * 2);
        if (r.skip) o.tap(4, sk, (size_t)M * r.cout * 2);
        bf16_t* out = o.abf((size_t)Bfull * HW * r.cout);           // Bfull: see expand()
        o.tag = "res.conv2";
        o.conv3({.A0 = n2, .C0 = r.cout, .W = o.w<bf16_t>(r.w2), .bias = o.w<float>(r.b2), .B = B, .Hin = a.H, .Win = a.W, .N = r.cout, .res_bf16 = res, .out_bf16 = out});
        o.tap(5, out, (size_t)M * r.cout * 2);
        return Act{out, r.cout, a.H, a.W, r.lout};
    };
    auto transformer = [&](const StW& s, Act& a) -> Act {
        const int C = s.c, n = a.H * a.W;
        // pre: still inside the shared guidance prefix (the first transformer of a guided forward).  The stages up to the self-attention
        // run on the Bs = Bfull / 2 samples that exist (Ms rows); everything from attn1.to_out on runs on Bfull samples (M rows).
        const bool pre = B < Bfull;
        const int Bs = B, Ms = Bs * n, M = Bfull * n;
        // attn2 (cross over the k neighbours); samples >= Bx have all-zero neighbours: t2 = t1 + b_o exactly (see add_bias_rows_kernel)
        const int Mx = Bx * n;
        // norm2 + attn2 + residual in one kernel when the neighbours' operands are cached (xa), norm2 too when no channel is padding
        const bool xfused = xa && Mx > 0 && xattn_fused_supported({.rows = Mx, .n = n, .C = C, .NP = XA_NP, .ncols = s.heads * k, .group = k});
        const bool xln = xfused && s.lc == C && C <= 2048;
        // the neighbour bias (host.h: nn_bias, [conditional rows | as many zero rows][k]; DESIGN 3 "Neighbour bias"): the fused kernels and
        // the generic branch take it as an operand; the two-GEMM middle form has no place for it, so under a bias the conditional samples of
        // a shape the fused kernel refuses go through the generic branch, and only the never-biased samples behind them keep the two GEMMs
        const float* nbias = o.c->nn_bias_rows ? o.c->nn_bias : nullptr;
        // Round 5: in a guided batch [conditional | unconditional] (Bx = Bfull / 2) with the LayerNorm-fused cross-attention kernel,
        //   * the unconditional rows' t2 = attn1.to_out(...) + t0 + b_o2 leaves attn1.to_out's GEMM directly (b_o2 rides in the start
        //     values of those rows: Ops::linear's rowvec; one rounding less than t1 -> + b_o2), no add_bias_rows pass;
        //   * the cross-attention kernel runs IN PLACE on the conditional rows (t2 aliases t1) and emits norm3 of its finished rows, so
        //     the separate LayerNorm-3 pass only covers the unconditional rows.
        const bool xfold_shape = xln && !o.c->deterministic;
        const bool bias_fold = xfold_shape && Bx * 2 == Bfull;          // the unconditional half exists and is exactly the second half
        // attn1.to_out then reads its operand ao and its residual t0, which hold Ms rows, with a row wrap where lin4 takes the op in that
        // form (pre_wrap); elsewhere (few tiles, other widths) both are duplicated into buffers of M rows first
        const bool pre_wrap = pre && o.lin4_takes({.C0 = C, .M = M, .N = C, .rowvec = bias_fold ? o.w<float>(s.bo2) : nullptr /* set or not is all that is read */,
                                                   .rowvec_ld = C, .rows_per_sample = Mx, .a0_wrap_rows = Ms, .res_wrap_rows = Ms});
        const size_t Mh = pre_wrap ? Ms : M;         // rows allocated for t0 and ao
        // a.half: the input left the shared guidance prefix and only its first Bfull / 2 samples exist: its two readers -- the entry GroupNorm and
        // the residual of ff.net.2 x proj_out -- wrap the batch index (round 5: no 50 MB duplication pass per forward).  (pre: the GroupNorm
        // runs on those samples alone, and a.half is decided where the prefix is left, below)
        bf16_t* xn = o.abf((size_t)Ms * C);
        o.tag = "st.gn";
        o.groupnorm({.x0 = a.p, .C0 = C, .HW = n, .B = Bs, .L0 = s.lc, .gamma = o.w<float>(s.gng), .beta = o.w<float>(s.gnb), .eps = 1e-6f, .out = xn,
                     .x0_bmod = a.half ? Bfull / 2 : 0});
        o.tap(1, xn, (size_t)Ms * C * 2, pre);
        bf16_t* t0 = o.abf(Mh * C);
        o.tag = "st.proj_in";
        o.linear({.A0 = xn, .C0 = C, .W = o.w<bf16_t>(s.win), .bias = o.w<float>(s.bin), .M = Ms, .N = C, .out_bf16 = t0, .sample_rows = n, .choice_rows = M});
        o.tap(2, t0, (size_t)Ms * C * 2, pre);
        // --- attn1 (self)
        bf16_t* l1 = o.abf((size_t)Ms * C);
        // n % 64 == 0: q | k | v in ONE projection (to_v's rows follow to_q | to_k in the blob, asserted in build_unet); the flash kernel
        // reads the token-major V block through transpose reads, so no per-layer V^T GEMM (6.8 % of the forward as a batched
        // weights-as-A GEMM at 380 TFLOP/s)
        const bool vrow = (n % 64 == 0) && s.v_follows;
        const int QW = vrow ? 3 * C : 2 * C;
        bf16_t* qk = o.abf((size_t)Ms * QW);
        o.tag = "st.norm1+qkv";
        o.layernorm({.x_bf16 = t0, .gamma = o.w<float>(s.ln1g), .beta = o.w<float>(s.ln1b), .M = Ms, .C = C, .out_bf16 = l1, .Clog = s.lc});
        o.tap(3, l1, (size_t)Ms * C * 2, pre);
        o.linear({.A0 = l1, .C0 = C, .W = o.w<bf16_t>(s.wqk), .M = Ms, .N = QW, .out_bf16 = qk, .sample_rows = n, .choice_rows = M});
        o.tap(4, qk, (size_t)Ms * QW * 2, pre);
        bf16_t* ao = o.abf(Mh * C);
        o.tag = "st.self_attention";
        if (vrow) {
            o.flash_d32({.q = qk, .ldq = QW, .v = qk + 2 * C, .out = ao, .n = n}, s.heads, Bs);
        } else if (n % 32 == 0) {
            bf16_t* vt = o.abf((size_t)Ms * C);      // V^T per sample: [B][C][n] via swapped-operand GEMM
            if (!o.plan) {
                IgemmParams p = o.base(C, n, C);
                p.A0 = o.w<bf16_t>(s.wv); p.C0 = C; p.W = l1; p.sA = 0; p.sW = (long long)n * C; p.sO = (long long)C * n;
                p.out_bf16 = vt; p.ldo = n;
                o.check(launch_igemm(p, false, Bs, o.c->stream), "v^T gemm");
            }
            o.flash_d32({.q = qk, .ldq = 2 * C, .vt = vt, .out = ao, .n = n}, s.heads, Bs);
        } else {
            bf16_t* v = o.abf((size_t)Ms * C);
            o.linear({.A0 = l1, .C0 = C, .W = o.w<bf16_t>(s.wv), .M = Ms, .N = C, .out_bf16 = v, .sample_rows = n, .choice_rows = M});
            o.small_attention({.q = qk, .ldq = 2 * C, .k = qk + C, .ldk = 2 * C, .v = v, .ldv = C, .out = ao, .ldo = C, .nq = n, .nkv = n, .scale = 1.0f / sqrtf(32.f)},
                              32, s.heads, Bs, "small self attention");
        }
        o.tap(5, ao, (size_t)Ms * C * 2, pre);
        if (pre) {             // the first context-dependent op follows: leave the shared prefix (B = Bfull from here on)
            leave_prefix(s, a);
            if (!pre_wrap) { Act t0a{t0, C, a.H, a.W, s.lc}, aoa{ao, C, a.H, a.W, s.lc}; expand(t0a); expand(aoa); }
        }
        bf16_t* t1 = o.abf((size_t)M * C);
        // --- attn2 (the forms chosen at the top)
        o.tag = "st.attn1.to_out";
        LinearOp to_out{.A0 = ao, .C0 = C, .W = o.w<bf16_t>(s.wo1), .bias = o.w<float>(s.bo1), .M = M, .N = C, .res_bf16 = t0, .out_bf16 = t1, .sample_rows = n};
        if (pre_wrap) to_out.a0_wrap_rows = to_out.res_wrap_rows = Ms;
        if (bias_fold) {
            const float* zb = o.plan ? nullptr : o.c->zero_bias_pair(o.w<float>(s.bo2), C);
            if (!o.plan && !zb && o.rc == 0) o.rc = o.c->fail(-2, "out of memory for a bias table");
            to_out.rowvec = zb; to_out.rowvec_ld = C; to_out.rows_per_sample = Mx;      // rows [0, Mx) + 0, rows [Mx, M) + b_o2
        }
        o.linear(to_out);
        o.tap(6, t1, (size_t)M * C * 2);          // (with the bias fold: the unconditional rows already hold t2)
        o.tag = "st.norm2+attn2";
        bf16_t* l2 = o.abf((size_t)M * C);
        if (Mx > 0 && !xln) o.layernorm({.x_bf16 = t1, .gamma = o.w<float>(s.ln2g), .beta = o.w<float>(s.ln2b), .M = Mx, .C = C, .out_bf16 = l2, .Clog = s.lc});
        bf16_t* t2 = xfold_shape ? t1 : o.abf((size_t)M * C);
        bf16_t* l3 = o.abf((size_t)M * C);
        if (Bx < B && !bias_fold && !o.plan)
            o.check(launch_add_bias_rows(t1 + (size_t)Mx * C, o.w<float>(s.bo2), t2 + (size_t)Mx * C, (long long)(M - Mx), C, o.c->stream), "zero-context cross attention");
        // the generic branch over samples [b0, b0 + nbat): q projection -> small_attention over the k neighbours -> out projection
        auto xattn_generic = [&](int b0, int nbat, const float* kb) {
            const size_t r0 = (size_t)b0 * n * C;
            bf16_t* q2 = o.abf((size_t)M * C);
            o.linear({.A0 = l2 + r0, .C0 = C, .W = o.w<bf16_t>(s.wq2), .M = nbat * n, .N = C, .out_bf16 = q2, .sample_rows = n});
            bf16_t* ao2 = o.abf((size_t)M * C);
            const bf16_t* kv0 = kv + (size_t)b0 * k * u.kv_total + s.kv_off;
            o.small_attention({.q = q2, .ldq = C, .k = kv0, .ldk = u.kv_total, .v = kv0 + C, .ldv = u.kv_total, .out = ao2, .ldo = C,
                               .nq = n, .nkv = k, .scale = 1.0f / sqrtf(32.f), .key_bias = kb ? kb + (size_t)b0 * k : nullptr}, 32, s.heads, nbat, "cross attention");
            o.linear({.A0 = ao2, .C0 = C, .W = o.w<bf16_t>(s.wo2), .bias = o.w<float>(s.bo2), .M = nbat * n, .N = C, .res_bf16 = t1 + r0, .out_bf16 = t2 + r0, .sample_rows = n});
        };
        // samples [0, Bg) of the middle form's go through the generic branch instead: the biased ones
        const int Bg = (nbias && xa && !xfused) ? (Bx < o.c->nn_bias_rows ? Bx : o.c->nn_bias_rows) : 0;
        if (Bg > 0) xattn_generic(0, Bg, nbias);
        if (Mx == 0) {
        } else if (xa) {       // two skinny per-sample GEMMs (see unet_compute_xattn)
            bf16_t* P = o.abf((size_t)M * XA_NP);
            const bf16_t* G = xa + (size_t)B * s.xa_unit; const bf16_t* U = G + (size_t)B * XA_NP * C;
            const bf16_t* Gp = U + (size_t)B * C * XA_NP; const bf16_t* Up = Gp + (size_t)B * XA_NP * C;     // their packed images
            XattnParams xp{.G = Gp, .U = Up, .bias = o.w<float>(s.bo2), .out = t2, .rows = Mx, .n = n, .C = C, .NP = XA_NP, .ncols = s.heads * k, .group = k,
                           .key_bias = nbias};
            if (xln) {          // both GEMMs, the softmax, the residual and norm2 (and norm3) in one launch
                xp.x = t1; xp.ln_g = o.w<float>(s.ln2g); xp.ln_b = o.w<float>(s.ln2b); xp.ln_eps = 1e-5f;
                if (xfold_shape) { xp.ln3_g = o.w<float>(s.ln3g); xp.ln3_b = o.w<float>(s.ln3b); xp.ln3_out = l3; }
                o.xattn_fused(xp);
            } else if (xfused) {   // on the LayerNorm'd rows
                xp.x = l2; xp.res = t1;
                o.xattn_fused(xp);
            } else if (!o.plan && Bx > Bg) {
                const size_t r0 = (size_t)Bg * n * C, g0 = (size_t)Bg * XA_NP * C;         // (Bg = 0 without a bias)
                const int Br = Bx - Bg; const double Mr = (double)Br * n;
                IgemmParams p = o.base(n, XA_NP, C);
                p.A0 = l2 + r0; p.C0 = C; p.sA = (long long)n * C; p.W = G + g0; p.sW = (long long)XA_NP * C; p.out_bf16 = P; p.sO = (long long)n * XA_NP;
                p.act = ACT_SOFTMAXG; p.sm_group = k;
                o.prof_begin(RDM_PROF_LINEAR, 2.0 * Mr * XA_NP * (double)C);
                o.check(launch_igemm(p, false, Br, o.c->stream), "xattn scores");
                o.prof_end();
                IgemmParams q = o.base(n, C, XA_NP);
                q.A0 = P; q.C0 = XA_NP; q.sA = (long long)n * XA_NP; q.W = U + g0; q.sW = (long long)C * XA_NP; q.bias = o.w<float>(s.bo2);
                q.res_bf16 = t1 + r0; q.out_bf16 = t2 + r0; q.sO = (long long)n * C;
                o.prof_begin(RDM_PROF_LINEAR, 2.0 * Mr * C * (double)XA_NP);
                o.check(launch_igemm(q, false, Br, o.c->stream), "xattn out");
                o.prof_end();
            }
        } else {
            xattn_generic(0, Bx, nbias);
        }
        o.tap(7, t2, (size_t)M * C * 2);
        // --- GEGLU feed-forward
        o.tag = "st.norm3+geglu";
        const int FI = 4 * s.lc;                     // GEGLU hidden width: 4 x the LOGICAL channels (a multiple of 128, never padded)
        bf16_t* ff = o.abf((size_t)M * FI);
        // norm3: with xfold_shape the conditional rows' left the cross-attention kernel, only the unconditional rows' are formed here
        const int M3 = xfold_shape ? Mx : 0;
        if (M > M3) o.layernorm({.x_bf16 = t2 + (size_t)M3 * C, .gamma = o.w<float>(s.ln3g), .beta = o.w<float>(s.ln3b), .M = M - M3, .C = C,
                                 .out_bf16 = l3 + (size_t)M3 * C, .Clog = s.lc});
        o.linear({.A0 = l3, .C0 = C, .W = o.w<bf16_t>(s.wff1), .bias = o.w<float>(s.bff1), .M = M, .N = 2 * FI, .act = ACT_GEGLU, .out_bf16 = ff, .sample_rows = n});
        o.tap(8, l3, (size_t)M * C * 2);
        o.tap(9, ff, (size_t)M * FI * 2);
        bf16_t* out = o.abf((size_t)M * C);
        o.tag = "st.ff2*proj_out";
        // t3 = ff W_2^T + b_2 + t2 and out = t3 W_out^T + b_out + x are one GEMM over the K-concatenated operand [ff | t2]
        // (dual-source A) with the product weights built by the packer: t3 never exists (2 of 9 tensor passes, one launch)
        o.linear({.A0 = ff, .A1 = t2, .C0 = FI, .C1 = C, .W = o.w<bf16_t>(s.wfo), .bias = o.w<float>(s.bfo), .M = M, .N = C, .res_bf16 = a.p, .out_bf16 = out,
                  .res_wrap_rows = a.half ? (Bfull / 2) * n : 0, .sample_rows = n});
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
                    // the first context-dependent layer: the shared prefix ends inside it, at attn1.to_out (transformer()), or in front of it
                    if (B < Bfull && !through_attn1) leave_prefix(u.st[L.idx], h);
                    h = transformer(u.st[L.idx], h); break;
                case 3: {
                    const ConvW& d = u.down[L.idx];
                    bf16_t* out = o.abf((size_t)Bfull * (h.H / 2) * (h.W / 2) * d.c);
                    o.tag = "downsample";
                    o.conv3({.A0 = h.p, .C0 = d.c, .W = o.w<bf16_t>(d.w), .bias = o.w<float>(d.b), .B = B, .Hin = h.H, .Win = h.W, .N = d.c, .stride = 2, .out_bf16 = out});
                    h = Act{out, d.c, h.H / 2, h.W / 2, d.lc};
                } break;
                case 4: {
                    const ConvW& d = u.up[L.idx];
                    bf16_t* out = o.abf((size_t)Bfull * (h.H * 2) * (h.W * 2) * d.c);
                    o.tag = "upsample";
                    o.conv3({.A0 = h.p, .C0 = d.c, .W = o.w<bf16_t>(d.w), .bias = o.w<float>(d.b), .B = B, .Hin = h.H, .Win = h.W, .N = d.c, .ups = 1, .out_bf16 = out});
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
    o.head({.x = h.p, .B = B, .H = H, .W = W, .C = mc, .gamma = o.w<float>(u.outg), .beta = o.w<float>(u.outb), .eps = 1e-5f, .w = o.w<float>(u.outw), .wp = hwp,
            .bias = o.w<float>(u.outbias), .out = eps_out, .Cout = c.out_channels}, mcl, no);
}

int unet_forward_impl(rdm_ctx* c, const float* x, const int64_t* t, const float* context, const bf16_t* kv_cached,
                      int b, int k, int H, int W, float* eps_out, int ctx_rows, int shared_half, const float* emb_row) {
    UNet& u = c->unet;
    if (!u.loaded) return c->fail(-1, "unet weights not loaded");
    const int down = 1 << (u.cfg.n_channel_mult - 1);
    if (b < 1 || k < 1 || H % down || W % down) return c->fail(-1, "bad unet_forward shape b=%d k=%d H=%d W=%d", b, k, H, W);
    if (k > 256) return c->fail(-1, "k=%d neighbours exceeds the cross-attention kernel limit (256)", k);
    // (the entries have matched the bias against their conditional rows: neighbour_bias_for; this is what the kernels' indexing needs)
    if (c->nn_bias_rows && (k != c->nn_bias_k || b > 2 * c->nn_bias_rows)) return c->fail(-1, "unet forward: the neighbour bias in force (%d x %d) does not cover b=%d k=%d", c->nn_bias_rows, c->nn_bias_k, b, k);
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
    RDM_TRY(c->neighbour_bias_for("rdm_unet_forward", b, k));
    return unet_forward_impl(c, x, t, context, nullptr, b, k, H, W, eps_out);
}

int rdm_debug_tap(rdm_ctx* c, void* buf, size_t nbytes, int block, int sub) {
    if (!c) return -1;
    c->tap_buf = buf; c->tap_bytes = buf ? nbytes : 0; c->tap_block = buf ? block : -1; c->tap_sub = buf ? sub : 0;
    return 0;
}

int rdm_debug_guidance_prefix(rdm_ctx* c, int through_attn1) {
    if (!c) return -1;
    c->prefix_through_attn1 = through_attn1 != 0;
    return 0;
}

// precompute K/V of the conditioning once per sample() call (reference recomputes S*16 times).  cat: fp32 staging for [cond | uncond],
// nb * k * context_dim floats (SamplerRun::begin reserves it at the front of the sampler scratch)
int unet_prepare_kv(rdm_ctx* c, float* cat, const float* cond, const float* uncond, int B, int k) {
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

// Every sample of a step shares the step's timestep, and the sampler's timesteps are known before the loop: their time-embedding rows
// (MLP + the 22 emb_layers) are computed ONCE per call as row GEMMs into a table (row i <-> ts[i]), instead of three B-row GEMMs per
// forward (72 us of a 29 ms forward).  Not in deterministic mode (the rows must come out of the same kernel configuration as
// rdm_unet_forward's): *table stays null there.
int unet_emb_table(rdm_ctx* c, const std::vector<int>& ts, const float** table) {
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
