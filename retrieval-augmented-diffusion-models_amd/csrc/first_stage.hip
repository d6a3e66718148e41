// The first-stage and CLIP executors of librdm_hip: the VQ decoder / encoder walkers (vq_body, vq_wide_body, vqenc_body), vq_range /
// vq_walk, the two CLIP towers, and every rdm_vq_* / rdm_clip_* entry (and rdm_to_uint8).  Calls only host.h: the Ops methods
// (dispatch.hip) and the launch_* of kernels.h.  The graphs are the reference's
//   CLIP                            rdm/modules/custom_clip/model.py:152-336
//   [ldm, un-vendored] Decoder / Encoder, VQModelInterface.decode
#include "host.h"

// ------------------------------------------------------------------------------------ VQ decode / encode
// ldm / taming ResnetBlock (no time embedding): GroupNorm + SiLU + 3x3 conv twice, 1x1 skip when the width changes
static bf16_t* vq_res(Ops& o, const VqRes& r, bf16_t* x, int B, int H, int W) {
    const int HW = H * W, M = B * HW;
    bf16_t* n1 = o.abf((size_t)M * r.cin);
    o.groupnorm({.x0 = x, .C0 = r.cin, .HW = HW, .B = B, .gamma = o.w<float>(r.n1g), .beta = o.w<float>(r.n1b), .eps = 1e-6f, .silu = 1, .out = n1});
    bf16_t* h1 = o.abf((size_t)M * r.cout);
    o.conv3({.A0 = n1, .C0 = r.cin, .W = o.w<bf16_t>(r.w1), .bias = o.w<float>(r.b1), .B = B, .Hin = H, .Win = W, .N = r.cout, .out_bf16 = h1});
    bf16_t* n2 = o.abf((size_t)M * r.cout);
    o.groupnorm({.x0 = h1, .C0 = r.cout, .HW = HW, .B = B, .gamma = o.w<float>(r.n2g), .beta = o.w<float>(r.n2b), .eps = 1e-6f, .silu = 1, .out = n2});
    const bf16_t* rs = x;
    if (r.skip) {
        bf16_t* s = o.abf((size_t)M * r.cout);
        o.linear({.A0 = x, .C0 = r.cin, .W = o.w<bf16_t>(r.wsk), .bias = o.w<float>(r.bsk), .M = M, .N = r.cout, .out_bf16 = s});
        rs = s;
    }
    bf16_t* out = o.abf((size_t)M * r.cout);
    o.conv3({.A0 = n2, .C0 = r.cout, .W = o.w<bf16_t>(r.w2), .bias = o.w<float>(r.b2), .B = B, .Hin = H, .Win = W, .N = r.cout, .res_bf16 = rs, .out_bf16 = out});
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
        o.groupnorm({.x0 = x, .C0 = C, .HW = n, .B = B, .gamma = o.w<float>(a.ng), .beta = o.w<float>(a.nb), .eps = 1e-6f, .out = hn});
        bf16_t* q = o.abf((size_t)M * C); bf16_t* kk = o.abf((size_t)M * C); bf16_t* v = o.abf((size_t)M * C);
        o.linear({.A0 = hn, .C0 = C, .W = o.w<bf16_t>(a.wq), .bias = o.w<float>(a.bq), .M = M, .N = C, .out_bf16 = q});
        o.linear({.A0 = hn, .C0 = C, .W = o.w<bf16_t>(a.wk), .bias = o.w<float>(a.bk), .M = M, .N = C, .out_bf16 = kk});
        o.linear({.A0 = hn, .C0 = C, .W = o.w<bf16_t>(a.wv), .M = M, .N = C, .out_bf16 = v});
        bf16_t* ao = o.abf((size_t)M * C);
        o.vq_attention({.q = q, .ldq = C, .k = kk, .ldk = C, .v = v, .ldv = C, .bias = o.w<float>(a.bv), .out = ao, .ldo = C, .n = n, .C = C, .scale = 1.0f / sqrtf((float)C)}, B);
        bf16_t* out = o.abf((size_t)M * C);
        o.linear({.A0 = ao, .C0 = C, .W = o.w<bf16_t>(a.wo), .bias = o.w<float>(a.bo), .M = M, .N = C, .res_bf16 = x, .out_bf16 = out});
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
    o.groupnorm({.x0 = x, .C0 = C, .HW = n, .B = B, .gamma = o.w<float>(a.ng), .beta = o.w<float>(a.nb), .eps = 1e-6f, .out = hn});
    if (padn) {
        bf16_t* hp = o.abf((size_t)Mp * C);
        if (!o.plan) {
            o.check(hipMemsetAsync(hp, 0, (size_t)Mp * C * 2, o.c->stream), "vq attention padding");
            o.check(hipMemcpy2DAsync(hp, prowb, hn, rowb, rowb, B, hipMemcpyDeviceToDevice, o.c->stream), "vq attention padding");
        }
        hn = hp;
    }
    bf16_t* q = o.abf((size_t)Mp * C); bf16_t* kk = o.abf((size_t)Mp * C); bf16_t* vt = o.abf((size_t)Mp * C);
    o.linear({.A0 = hn, .C0 = C, .W = o.w<bf16_t>(a.wq), .bias = o.w<float>(a.bq), .M = Mp, .N = C, .out_bf16 = q});
    o.linear({.A0 = hn, .C0 = C, .W = o.w<bf16_t>(a.wk), .bias = o.w<float>(a.bk), .M = Mp, .N = C, .out_bf16 = kk});
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
    o.linear({.A0 = ao, .C0 = C, .W = o.w<bf16_t>(a.wo), .bias = o.w<float>(a.bo), .M = M, .N = C, .res_bf16 = x, .out_bf16 = out});
    return out;
}

// debug tap (rdm_debug_tap): first-stage decoder layers are blocks 1000, 1001, ... in execution order (conv_in's output = 1000), encoder
// layers blocks 1500, 1501, ... (conv_in's output = 1500): the ranges are apart, so a decoder number never fires in an encode nor the reverse.
// tapi: the walker's running block number.  With the tap off this launches and allocates nothing.
constexpr int TAP_VQ_DECODER = 1000, TAP_VQ_ENCODER = 1500;
static void vq_tap(Ops& o, int* tapi, const bf16_t* t, int B, int H, int W, int ch) {
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
    int bin = c.ch * c.ch_mult[c.n_ch_mult - 1], tapi = TAP_VQ_DECODER;
    vq_tap(o, &tapi, h, B, H, W, bin);
    h = vq_mid(o, v.mid, h, B, H, W, &tapi);
    for (int lvl = c.n_ch_mult - 1; lvl >= 0; lvl--) {
        h = vq_blocks(o, v.levels[lvl], h, B, H, W, bin, &tapi);
        if (lvl != 0) {
            const ConvW& u = v.levels[lvl].resample;
            bf16_t* out = o.abf((size_t)B * (H * 2) * (W * 2) * u.c);
            o.conv3({.A0 = h, .C0 = u.c, .W = o.w<bf16_t>(u.w), .bias = o.w<float>(u.b), .B = B, .Hin = H, .Win = W, .N = u.c, .ups = 1, .out_bf16 = out});
            h = out; H *= 2; W *= 2;
            vq_tap(o, &tapi, h, B, H, W, u.c);
        }
    }
    bf16_t* no = o.abf((size_t)B * H * W * bin);
    bf16_t* hwp = o.abf(head_conv_wp_bytes(bin) / 2);
    o.head({.x = h, .B = B, .H = H, .W = W, .C = bin, .gamma = o.w<float>(v.noutg), .beta = o.w<float>(v.noutb), .eps = 1e-6f, .w = o.w<float>(v.coutw), .wp = hwp,
            .bias = o.w<float>(v.coutb), .out = img, .Cout = c.out_ch}, bin, no);
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
    o.linear({.A0 = zq, .C0 = c.embed_dim, .W = o.w<bf16_t>(v.pqw), .bias = o.w<float>(v.pqb), .M = M, .N = c.z_channels, .out_bf16 = h0});
    const int bin = c.ch * c.ch_mult[c.n_ch_mult - 1];
    bf16_t* h = o.abf((size_t)M * bin);
    o.conv3({.A0 = h0, .C0 = c.z_channels, .W = o.w<bf16_t>(v.cinw), .bias = o.w<float>(v.cinb), .B = B, .Hin = zr, .Win = zr, .N = bin, .out_bf16 = h});
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
    int bin = c.ch, tapi = TAP_VQ_ENCODER;
    vq_tap(o, &tapi, h, B, H, W, bin);
    for (int lvl = 0; lvl < c.n_ch_mult; lvl++) {
        h = vq_blocks(o, v.levels[lvl], h, B, H, W, bin, &tapi);
        if (lvl != c.n_ch_mult - 1) {      // F.pad(x, (0, 1, 0, 1)) + Conv2d(stride 2, padding 0): window rows 2 oy .. 2 oy + 2, zero beyond the last row / column
            const ConvW& d = v.levels[lvl].resample;
            bf16_t* out = o.abf((size_t)B * (H / 2) * (W / 2) * d.c);
            o.conv3({.A0 = h, .C0 = d.c, .W = o.w<bf16_t>(d.w), .bias = o.w<float>(d.b), .B = B, .Hin = H, .Win = W, .N = d.c, .stride = 2, .out_bf16 = out, .asym = 1});
            h = out; H /= 2; W /= 2;
            vq_tap(o, &tapi, h, B, H, W, d.c);
        }
    }
    h = vq_mid(o, v.mid, h, B, H, W, &tapi);
    bf16_t* no = o.abf((size_t)B * H * W * bin);
    if (v.wide) {
        const int M = B * H * W;
        o.groupnorm({.x0 = h, .C0 = bin, .HW = H * W, .B = B, .gamma = o.w<float>(v.noutg), .beta = o.w<float>(v.noutb), .eps = 1e-6f, .silu = 1, .out = no});
        vq_tap(o, &tapi, no, B, H, W, bin);
        bf16_t* ze = o.abf((size_t)M * c.z_channels);
        o.conv3({.A0 = no, .C0 = bin, .W = o.w<bf16_t>(v.coutw), .bias = o.w<float>(v.coutb), .B = B, .Hin = H, .Win = W, .N = c.z_channels, .out_bf16 = ze});
        vq_tap(o, &tapi, ze, B, H, W, c.z_channels);
        float* zt = o.af32((size_t)M * c.embed_dim);
        o.linear({.A0 = ze, .C0 = c.z_channels, .W = o.w<bf16_t>(v.qw), .bias = o.w<float>(v.qb), .M = M, .N = c.embed_dim, .out_f32 = zt});
        if (z && !o.plan) o.check(launch_vq_rows_to_nchw(zt, nullptr, z, B, H * W, c.embed_dim, o.c->stream), "latent to NCHW");
        return zt;
    }
    bf16_t* hwp = o.abf(head_conv_wp_bytes(bin) / 2);
    float* ze = o.af32((size_t)B * c.z_channels * H * W);
    o.head({.x = h, .B = B, .H = H, .W = W, .C = bin, .gamma = o.w<float>(v.noutg), .beta = o.w<float>(v.noutb), .eps = 1e-6f, .w = o.w<float>(v.coutw), .wp = hwp,
            .bias = o.w<float>(v.coutb), .out = ze, .Cout = c.z_channels}, bin, no);
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
// debug tap (rdm_debug_tap): the text tower is block 2000, the image tower block 3000; layer 0 = the tower's own stages (numbered in the
// bodies below), layer i + 1 = resblock i with stages 1 ln_1, 2 q|k|v, 3 attention heads, 4 x + out_proj, 5 ln_2, 6 QuickGELU hidden, 7 x + c_proj
constexpr int TAP_CLIP_TEXT = 2000, TAP_CLIP_IMAGE = 3000;
static void clip_tower(Ops& o, const std::vector<ClipBlk>& blks, float* x, int B, int L, int Wd, int heads, int causal) {
    const int M = B * L;
    bf16_t* ln = o.abf((size_t)M * Wd); bf16_t* qkv = o.abf((size_t)M * 3 * Wd); bf16_t* ao = o.abf((size_t)M * Wd);
    bf16_t* hid = o.abf((size_t)M * 4 * Wd);
    for (const ClipBlk& k : blks) {
        o.cur_layer = (int)(&k - &blks[0]) + 1;
        o.layernorm({.x_f32 = x, .gamma = o.w<float>(k.ln1g), .beta = o.w<float>(k.ln1b), .M = M, .C = Wd, .out_bf16 = ln});
        o.tap(1, ln, (size_t)M * Wd * 2);
        o.linear({.A0 = ln, .C0 = Wd, .W = o.w<bf16_t>(k.wqkv), .bias = o.w<float>(k.bqkv), .M = M, .N = 3 * Wd, .out_bf16 = qkv});
        o.tap(2, qkv, (size_t)M * 3 * Wd * 2);
        o.small_attention({.q = qkv, .ldq = 3 * Wd, .k = qkv + Wd, .ldk = 3 * Wd, .v = qkv + 2 * Wd, .ldv = 3 * Wd, .out = ao, .ldo = Wd, .nq = L, .nkv = L, .causal = causal,
                           .scale = 1.0f / sqrtf((float)(Wd / heads))}, Wd / heads, heads, B, "clip attention");
        o.tap(3, ao, (size_t)M * Wd * 2);
        o.linear({.A0 = ao, .C0 = Wd, .W = o.w<bf16_t>(k.wo), .bias = o.w<float>(k.bo), .M = M, .N = Wd, .res_f32 = x, .out_f32 = x});        // x += out_proj(attn)
        o.tap(4, x, (size_t)M * Wd * 4);
        o.layernorm({.x_f32 = x, .gamma = o.w<float>(k.ln2g), .beta = o.w<float>(k.ln2b), .M = M, .C = Wd, .out_bf16 = ln});
        o.tap(5, ln, (size_t)M * Wd * 2);
        o.linear({.A0 = ln, .C0 = Wd, .W = o.w<bf16_t>(k.wfc), .bias = o.w<float>(k.bfc), .M = M, .N = 4 * Wd, .act = ACT_QUICKGELU, .out_bf16 = hid});
        o.tap(6, hid, (size_t)M * 4 * Wd * 2);
        o.linear({.A0 = hid, .C0 = 4 * Wd, .W = o.w<bf16_t>(k.wpj), .bias = o.w<float>(k.bpj), .M = M, .N = Wd, .res_f32 = x, .out_f32 = x});  // x += mlp
        o.tap(7, x, (size_t)M * Wd * 4);
    }
    o.cur_layer = 0;
}
static void clip_text_body(Ops& o, ClipModel& m, const long long* tokens, int B, float* out) {
    const rdm_clip_cfg& c = m.cfg; const int L = c.context_length, Wd = c.transformer_width;
    o.cur_block = TAP_CLIP_TEXT; o.cur_layer = 0;
    float* x = o.af32((size_t)B * L * Wd);
    if (!o.plan) o.check(launch_clip_embed(tokens, o.w<float>(m.tok), o.w<float>(m.pos), x, B, L, Wd, o.c->stream), "clip embed");
    o.tap(1, x, (size_t)B * L * Wd * 4);
    clip_tower(o, m.text, x, B, L, Wd, c.transformer_heads, 1);
    float* eot = o.af32((size_t)B * Wd); bf16_t* ln = o.abf((size_t)B * Wd);
    if (!o.plan) o.check(launch_clip_gather_eot(tokens, x, eot, B, L, Wd, o.c->stream), "gather eot");
    o.tap(2, eot, (size_t)B * Wd * 4);
    o.layernorm({.x_f32 = eot, .gamma = o.w<float>(m.lnfg), .beta = o.w<float>(m.lnfb), .M = B, .C = Wd, .out_bf16 = ln});
    o.tap(3, ln, (size_t)B * Wd * 2);
    o.linear({.A0 = ln, .C0 = Wd, .W = o.w<bf16_t>(m.tproj), .M = B, .N = c.embed_dim, .out_f32 = out, .single_row = true});      // the pooled token: one row per sample
    o.tap(4, out, (size_t)B * c.embed_dim * 4);
}
// raw_h > 0: `img` is the un-preprocessed [B,3,raw_h,raw_w] image in [-1,1]; the bicubic resize + normalisation of
// ClipImageRetriever.preprocess (rdm/modules/retrievers.py:83-91) is fused into the patch gather
static void clip_image_body(Ops& o, ClipModel& m, const float* img, int B, float* out, int raw_h = 0, int raw_w = 0) {
    const rdm_clip_cfg& c = m.cfg; const int P = c.vision_patch_size, G = c.image_resolution / P, Wd = c.vision_width;
    const int K = 3 * P * P, L = G * G + 1;
    o.cur_block = TAP_CLIP_IMAGE; o.cur_layer = 0;
    bf16_t* patches = o.abf((size_t)B * G * G * K); float* pe = o.af32((size_t)B * G * G * Wd);
    if (!o.plan) {
        if (raw_h > 0) o.check(launch_clip_preprocess(img, B, raw_h, raw_w, c.image_resolution, P, nullptr, patches, o.c->stream), "preprocess+patchify");
        else o.check(launch_clip_patchify(img, patches, B, c.image_resolution, P, o.c->stream), "patchify");
    }
    o.tap(1, patches, (size_t)B * G * G * K * 2);
    o.linear({.A0 = patches, .C0 = K, .W = o.w<bf16_t>(m.conv1), .M = B * G * G, .N = Wd, .out_f32 = pe});
    o.tap(2, pe, (size_t)B * G * G * Wd * 4);
    float* x0 = o.af32((size_t)B * L * Wd); float* x = o.af32((size_t)B * L * Wd);
    if (!o.plan) o.check(launch_clip_vit_assemble(pe, o.w<float>(m.cls), o.w<float>(m.vpos), x0, B, G * G, Wd, o.c->stream), "vit assemble");
    o.tap(3, x0, (size_t)B * L * Wd * 4);
    o.layernorm({.x_f32 = x0, .gamma = o.w<float>(m.lnpreg), .beta = o.w<float>(m.lnpreb), .M = B * L, .C = Wd, .out_f32 = x});
    o.tap(4, x, (size_t)B * L * Wd * 4);
    clip_tower(o, m.vis, x, B, L, Wd, Wd / 64, 0);
    float* cls = o.af32((size_t)B * Wd); bf16_t* ln = o.abf((size_t)B * Wd);
    if (!o.plan) o.check(launch_gather_rows_f32(x, cls, B, L, Wd, o.c->stream), "gather cls");
    o.tap(5, cls, (size_t)B * Wd * 4);
    o.layernorm({.x_f32 = cls, .gamma = o.w<float>(m.lnpostg), .beta = o.w<float>(m.lnpostb), .M = B, .C = Wd, .out_bf16 = ln});
    o.tap(6, ln, (size_t)B * Wd * 2);
    o.linear({.A0 = ln, .C0 = Wd, .W = o.w<bf16_t>(m.vproj), .M = B, .N = c.embed_dim, .out_f32 = out, .single_row = true});      // the pooled token: one row per sample
    o.tap(7, out, (size_t)B * c.embed_dim * 4);
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
        o.vq_nearest({.z = zt, .codebook = cb, .norms = c->vq.code_norms, .M = M, .N = d.n_embed, .E = d.embed_dim, .ws = ws, .idx32 = idx32,
                      .idx64 = (long long*)indices_out + (size_t)b0 * HW});
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
    if (!c) return -1;
    if (b < 1) return c->fail(-1, "rdm_clip_encode_text: b = %d; at least one sequence", b);      // (before the pointers: an empty tensor has none)
    if (!tokens || !out) return c->fail(-1, "null argument");
    if (!c->clip.loaded) return c->fail(-1, "clip weights not loaded");
    return run_with_arena(c, c->clip.arena, c->clip.blob, [&](Ops& o) { clip_text_body(o, c->clip, (const long long*)tokens, b, out); });
}
int rdm_clip_encode_image(rdm_ctx* c, const float* image, int b, float* out) {
    RDM_ENTER(c);
    if (!c) return -1;
    if (b < 1) return c->fail(-1, "rdm_clip_encode_image: b = %d; at least one image", b);
    if (!image || !out) return c->fail(-1, "null argument");
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
