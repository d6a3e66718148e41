// The RARM executors of librdm_hip: the decode step (rarm_prepare, rarm_step), the whole-sequence pass (rarm_seq_body), the
// sampling loop (rarm_sample_run) and the rdm_rarm_* entries.  Calls only host.h: the Ops methods (dispatch.hip) and the launch_*
// of kernels.h; the kernels are in rarm.hip.
#include "host.h"

// ---- RARM (kernels in rarm.hip)
// rdm_debug_tap blocks of the three executors (include/rdm_hip.h): sub = 16 * layer + stage, layer 0 the executor's own stages, layer
// i + 1 transformer block i
constexpr int TAP_RARM_PREPARE = 4000, TAP_RARM_STEP = 4100, TAP_RARM_SEQ = 4200;
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
    c->tap_step = 0;
    if (fuse) {
        RDM_TRY(ensure_bytes(c, &m.xa, &m.xa_bytes, (size_t)g.depth * 2 * B * 128 * C * 2));
        m.xa_B = B; m.xa_k = k;
    }
    return run_with_arena(c, m.arena, m.blob, [&](Ops& o) {
        o.cur_block = TAP_RARM_PREPARE; o.cur_layer = 0;
        bf16_t* cb = o.abf((size_t)B * k * g.context_dim);
        if (!o.plan) o.check(launch_cast_f32_bf16(context, cb, (long long)B * k * g.context_dim, c->stream), "cast ctx");
        o.tap(1, cb, (size_t)B * k * g.context_dim * 2);
        o.linear({.A0 = cb, .C0 = g.context_dim, .W = o.w<bf16_t>(m.kvw), .M = B * k, .N = m.kv_total, .out_bf16 = (bf16_t*)m.ctxkv});
        o.tap(2, m.ctxkv, (size_t)B2 * k * m.kv_total * 2);
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
                    o.cur_layer = l + 1;
                    o.tap(1, G, (size_t)B * NP * C * 2);
                    o.tap(2, UT, (size_t)B * NP * C * 2);
                }
            }
        }
    });
}
// one decode step for B2 sequences: token at position *pos -> logits of the next token
static int rarm_step(rdm_ctx* c, int B2, int k, int pos_hint = -1 /* host's copy of the position processed (profiling only: the kernels read the device counter) */) {
    RarmModel& m = c->rarm; const rdm_rarm_cfg& g = m.cfg; const int C = m.C, L = g.sequence_length;
    RarmState st = rarm_state(m, B2);
    const size_t step = (size_t)c->tap_step++;      // this step's place in a tap buffer: stage bytes * step
    return run_with_arena(c, m.arena, m.blob, [&](Ops& o) {
        o.cur_block = TAP_RARM_STEP; o.cur_layer = 0;
        auto tap = [&](int stage, const void* p, size_t width_bytes) { o.tap(stage, p, (size_t)B2 * width_bytes, false, step * B2 * width_bytes); };
        float* x = o.af32((size_t)B2 * C);
        bf16_t* ln = o.abf((size_t)B2 * C); bf16_t* qkv = o.abf((size_t)B2 * 3 * C); bf16_t* ao = o.abf((size_t)B2 * C);
        bf16_t* q2 = o.abf((size_t)B2 * C); bf16_t* ff = o.abf((size_t)B2 * 4 * C);
        // a decode step is one row per sequence throughout: every projection of the step is B2 single_row rows
        auto lin = [&](LinearOp op) { op.M = B2; op.single_row = true; o.linear(op); };
        // a projection of LayerNorm(x; g, b): formed inside the skinny GEMM where that takes the shape, else as a pass into `ln` of its own
        // (ln_stage: the tap stage of the LayerNorm's rows, which exist only in the second form)
        auto ln_lin = [&](const float* g, const float* b, LinearOp op, int ln_stage) {
            op.ln_x = x; op.ln_g = g; op.ln_b = b; op.C0 = C; op.M = B2; op.single_row = true;
            if (o.linear_ln(op)) return;
            o.layernorm({.x_f32 = x, .gamma = g, .beta = b, .M = B2, .C = C, .out_bf16 = ln});
            tap(ln_stage, ln, (size_t)C * 2);
            op.A0 = ln;
            o.linear(op);
        };
        if (!o.plan) o.check(launch_rarm_embed(st.tokens, o.w<float>(m.emb), o.w<float>(m.pos), st.pos, x, B2, C, g.vocab_in, c->stream), "rarm embed");
        tap(1, x, (size_t)C * 4);
        const float scale = 1.0f / sqrtf((float)g.d_head);
        const bool ln3_fused = m.xa_B > 0 && m.xa_k == k;      // the fused cross-attention kernel also emits norm3 of its output rows
        for (int l = 0; l < g.depth; l++) {
            const RarmBlk& b = m.blk[l];
            o.cur_layer = l + 1;
            ln_lin(o.w<float>(b.ln1g), o.w<float>(b.ln1b), {.W = o.w<bf16_t>(b.wqkv), .N = 3 * C, .out_bf16 = qkv}, 1);
            tap(2, qkv, (size_t)3 * C * 2);
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
            tap(3, ao, (size_t)C * 2);
            lin({.A0 = ao, .C0 = C, .W = o.w<bf16_t>(b.wo1), .bias = o.w<float>(b.bo1), .N = C, .res_f32 = x, .out_f32 = x});
            tap(4, x, (size_t)C * 4);
            if (m.xa_B > 0 && m.xa_k == k) {      // norm2 + to_q + attention over the neighbours + to_out + residual in one launch
                if (!o.plan) {
                    RarmXattnParams xp{}; xp.x = x; xp.ln_g = o.w<float>(b.ln2g); xp.ln_b = o.w<float>(b.ln2b); xp.ln_eps = 1e-5f;
                    xp.G = (const bf16_t*)m.xa + ((size_t)l * 2) * m.xa_B * 128 * C; xp.UT = xp.G + (size_t)m.xa_B * 128 * C;
                    xp.bias = o.w<float>(b.bo2); xp.B2 = B2; xp.Bc = m.xa_B; xp.C = C; xp.NP = 128; xp.heads = g.n_heads; xp.k = k;
                    if (ln3_fused) { xp.ln3_g = o.w<float>(b.ln3g); xp.ln3_b = o.w<float>(b.ln3b); xp.ln3_out = ln; }
                    o.check(launch_rarm_xattn_decode(xp, c->stream), "rarm fused cross attention");
                }
            } else {
            ln_lin(o.w<float>(b.ln2g), o.w<float>(b.ln2b), {.W = o.w<bf16_t>(b.wq2), .N = C, .out_bf16 = q2}, 5);
            tap(6, q2, (size_t)C * 2);
            if (!o.plan) {
                RarmAttnParams p{}; p.q = q2; p.ldq = C; p.Kc = (bf16_t*)m.ctxkv + (size_t)l * 2 * C; p.Vc = (bf16_t*)m.ctxkv + (size_t)l * 2 * C + C;
                p.batch_stride = (long long)k * m.kv_total; p.row_stride = m.kv_total; p.nkv = k; p.scale = scale; p.out = ao; p.ldo = C;
                o.check(launch_rarm_decode_attention(p, g.n_heads, B2, c->stream), "rarm cross attention");
            }
            tap(7, ao, (size_t)C * 2);
            lin({.A0 = ao, .C0 = C, .W = o.w<bf16_t>(b.wo2), .bias = o.w<float>(b.bo2), .N = C, .res_f32 = x, .out_f32 = x});
            }
            tap(8, x, (size_t)C * 4);
            if (ln3_fused) tap(9, ln, (size_t)C * 2);
            const LinearOp geglu{.W = o.w<bf16_t>(b.wff1), .bias = o.w<float>(b.bff1), .N = 8 * C, .act = ACT_GEGLU, .out_bf16 = ff};
            if (ln3_fused) {      // norm3 left the cross-attention kernel with the finished rows: a plain GEGLU GEMM on the bf16 operand
                LinearOp op = geglu; op.A0 = ln; op.C0 = C;
                lin(op);
            } else ln_lin(o.w<float>(b.ln3g), o.w<float>(b.ln3b), geglu, 9);
            tap(10, ff, (size_t)4 * C * 2);
            lin({.A0 = ff, .C0 = 4 * C, .W = o.w<bf16_t>(b.wff2), .bias = o.w<float>(b.bff2), .N = C, .res_f32 = x, .out_f32 = x});
            tap(11, x, (size_t)C * 4);
        }
        o.cur_layer = 0;
        if (!o.plan) o.check(launch_cast_f32_bf16(x, ln, (long long)B2 * C, c->stream), "cast x");
        tap(2, ln, (size_t)C * 2);
        lin({.A0 = ln, .C0 = C, .W = o.w<bf16_t>(m.wpo), .bias = o.w<float>(m.bpo), .N = g.vocab_out, .out_f32 = st.logits});
        tap(3, st.logits, (size_t)g.vocab_out * 4);
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
// the transformer of rarm_step with t rows per sequence -- tiled GEMMs (no op here is single_row: no kernel on this path is chosen by the
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
        o.cur_block = TAP_RARM_SEQ;
        const float scale = 1.0f / sqrtf((float)g.d_head);
        for (int s0 = 0; s0 < B2 && o.rc == 0; s0 += per) {
            const int nb = B2 - s0 < per ? B2 - s0 : per, M = nb * t;
            // a range shows its rows at its own row offset of the [B2 * t, width] stage
            auto tap = [&](int stage, const void* p, size_t width_bytes) { o.tap(stage, p, (size_t)M * width_bytes, false, (size_t)s0 * t * width_bytes); };
            o.cur_layer = 0;
            o.check(launch_rarm_embed_seq((const long long*)tokens, tok_ld, tok_rows, s0, o.w<float>(m.emb), o.w<float>(m.pos), x, M, t, C, g.vocab_in, c->stream),
                    "rarm embed");
            tap(1, x, (size_t)C * 4);
            for (int l = 0; l < g.depth; l++) {
                const RarmBlk& b = m.blk[l];
                o.cur_layer = l + 1;
                o.layernorm({.x_f32 = x, .gamma = o.w<float>(b.ln1g), .beta = o.w<float>(b.ln1b), .M = M, .C = C, .out_bf16 = ln});
                tap(1, ln, (size_t)C * 2);
                o.linear({.A0 = ln, .C0 = C, .W = o.w<bf16_t>(b.wqkv), .M = M, .N = 3 * C, .out_bf16 = qkv});
                tap(2, qkv, (size_t)3 * C * 2);
                bf16_t* kc = fill_cache ? (bf16_t*)m.cache + (((size_t)l * 2) * B2 + s0) * L * C : nullptr;
                bf16_t* vc = fill_cache ? (bf16_t*)m.cache + (((size_t)l * 2 + 1) * B2 + s0) * L * C : nullptr;
                o.tag = "rarm.causal_attention";
                o.causal_d64({.qkv = qkv, .ldq = 3 * C, .out = ao, .ldo = C, .n = t, .kcache = kc, .vcache = vc, .L = L}, g.n_heads, nb, scale);
                tap(3, ao, (size_t)C * 2);
                o.linear({.A0 = ao, .C0 = C, .W = o.w<bf16_t>(b.wo1), .bias = o.w<float>(b.bo1), .M = M, .N = C, .res_f32 = x, .out_f32 = x});
                tap(4, x, (size_t)C * 4);
                o.layernorm({.x_f32 = x, .gamma = o.w<float>(b.ln2g), .beta = o.w<float>(b.ln2b), .M = M, .C = C, .out_bf16 = ln});
                tap(5, ln, (size_t)C * 2);
                o.linear({.A0 = ln, .C0 = C, .W = o.w<bf16_t>(b.wq2), .M = M, .N = C, .out_bf16 = q2});
                tap(6, q2, (size_t)C * 2);
                const bf16_t* kv = (const bf16_t*)m.ctxkv + (size_t)s0 * k * m.kv_total + (size_t)l * 2 * C;
                o.small_attention({.q = q2, .ldq = C, .k = kv, .ldk = m.kv_total, .v = kv + C, .ldv = m.kv_total, .out = ao, .ldo = C, .nq = t, .nkv = k, .scale = scale},
                                  g.d_head, g.n_heads, nb, "rarm cross attention");
                tap(7, ao, (size_t)C * 2);
                o.linear({.A0 = ao, .C0 = C, .W = o.w<bf16_t>(b.wo2), .bias = o.w<float>(b.bo2), .M = M, .N = C, .res_f32 = x, .out_f32 = x});
                tap(8, x, (size_t)C * 4);
                o.layernorm({.x_f32 = x, .gamma = o.w<float>(b.ln3g), .beta = o.w<float>(b.ln3b), .M = M, .C = C, .out_bf16 = ln});
                tap(9, ln, (size_t)C * 2);
                o.linear({.A0 = ln, .C0 = C, .W = o.w<bf16_t>(b.wff1), .bias = o.w<float>(b.bff1), .M = M, .N = 8 * C, .act = ACT_GEGLU, .out_bf16 = ff});
                tap(10, ff, (size_t)4 * C * 2);
                o.linear({.A0 = ff, .C0 = 4 * C, .W = o.w<bf16_t>(b.wff2), .bias = o.w<float>(b.bff2), .M = M, .N = C, .res_f32 = x, .out_f32 = x});
                tap(11, x, (size_t)C * 4);
            }
            if (!logits_out && !nll_out) continue;
            o.cur_layer = 0;
            o.check(launch_cast_f32_bf16(x, ln, (long long)M * C, c->stream), "cast x");
            tap(2, ln, (size_t)C * 2);
            const size_t row0 = (size_t)s0 * t;
            if (logits_out) {
                o.linear({.A0 = ln, .C0 = C, .W = o.w<bf16_t>(m.wpo), .bias = o.w<float>(m.bpo), .M = M, .N = V, .out_f32 = logits_out + row0 * V});
                tap(3, logits_out + row0 * V, (size_t)V * 4);
            }
            if (nll_out) {
                for (int r0 = 0; r0 < M && o.rc == 0; r0 += RARM_NLL_ROWS) {
                    const int nr = M - r0 < RARM_NLL_ROWS ? M - r0 : RARM_NLL_ROWS;
                    o.linear({.A0 = ln + (size_t)r0 * C, .C0 = C, .W = o.w<bf16_t>(m.wpo), .bias = o.w<float>(m.bpo), .M = nr, .N = V, .out_f32 = lg});
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
