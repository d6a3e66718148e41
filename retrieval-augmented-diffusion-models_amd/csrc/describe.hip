// Model descriptions of librdm_hip: the build_* functions walk a cfg into a layer graph and a weight manifest (blob offsets), the
// cfg checks, and the one manifest routine and one load routine behind the ten rdm_*_manifest / rdm_load_* entries.
// The graphs are the reference's
//   UNetModel.__init__              rdm/modules/diffusionmodules/openaimodel.py:66-305
//   CLIP                            rdm/modules/custom_clip/model.py:152-336
//   [ldm, un-vendored] Decoder / Encoder, RetrievalPatchTransformer
#include "host.h"

struct Seg { int n, p; };
static std::string seg_spec(const char* tag, std::initializer_list<Seg> segs) {
    bool any = false; for (const Seg& g : segs) any |= g.n != g.p;
    if (!any) return "";
    std::string o = std::string("|") + tag + "=";
    bool first = true;
    for (const Seg& g : segs) { char b[48]; snprintf(b, sizeof b, "%s%d>%d", first ? "" : ",", g.n, g.p); o += b; first = false; }
    return o;
}

static void build_unet(UNet& u, const rdm_unet_cfg& c, Manifest& mf) {
    u.cfg = c;
    const int mc = c.model_channels, ted = mc * 4, mcp = pad64(mc);       // ted = 4 mc: a multiple of 64 whenever mc % 32 == 0... (128-aligned)
    // vec: fp32 vector(s) over channel segments; mat: bf16 [rows][cols]; both padded per segment
    auto vec = [&](const std::string& n, std::initializer_list<Seg> segs) {
        size_t tot = 0; for (const Seg& g : segs) tot += g.p;
        return mf.add("f32" + seg_spec("R", segs), n, tot * 4);
    };
    auto mat = [&](const char* kind, const std::string& n, std::initializer_list<Seg> rows, std::initializer_list<Seg> cols, size_t elt = 2, int taps = 1) {
        size_t r = 0, k = 0; for (const Seg& g : rows) r += g.p; for (const Seg& g : cols) k += g.p;
        return mf.add((std::string(kind) + seg_spec("R", rows) + seg_spec("C", cols)), n, r * k * taps * elt);
    };
    const Seg TED{ted, ted};
    u.te0w = mat("bf16", "time_embed.0.weight", {TED}, {{mc, mcp}}); u.te0b = vec("time_embed.0.bias", {TED});
    u.te2w = mat("bf16", "time_embed.2.weight", {TED}, {TED}); u.te2b = vec("time_embed.2.bias", {TED});
    std::string emb_w_srcs, emb_b_srcs, kv_srcs, emb_rspec, kv_rspec;
    bool emb_padded = false, kv_padded = false;
    u.emb_total = 0; u.kv_total = 0; u.xa_total = 0;
    auto in_attn = [&](int ds) { for (int i = 0; i < c.n_attention_resolutions; i++) if (c.attention_resolutions[i] == ds) return true; return false; };
    auto add_seg = [](std::string& spec, bool& padded, int n, int p) { char b[48]; snprintf(b, sizeof b, "%s%d>%d", spec.empty() ? "" : ",", n, p); spec += b; padded |= n != p; };
    auto add_res = [&](const std::string& pre, int l0, int l1, int lout) {       // input = [l0 | l1] logical channels (l1: the skip tensor, or 0)
        ResW r{}; r.l0 = l0; r.l1 = l1; r.lout = lout; r.p0 = pad64(l0); r.p1 = l1 ? pad64(l1) : 0;
        r.cin = r.p0 + r.p1; r.cout = pad64(lout); r.skip = (l0 + l1) != lout;
        const Seg S0{l0, r.p0}, S1{l1, r.p1}, SO{lout, r.cout};
        if (l1) { r.gn1g = vec(pre + ".in_layers.0.weight", {S0, S1}); r.gn1b = vec(pre + ".in_layers.0.bias", {S0, S1}); }
        else { r.gn1g = vec(pre + ".in_layers.0.weight", {S0}); r.gn1b = vec(pre + ".in_layers.0.bias", {S0}); }
        r.w1 = l1 ? mat("conv3", pre + ".in_layers.2.weight", {SO}, {S0, S1}, 2, 9) : mat("conv3", pre + ".in_layers.2.weight", {SO}, {S0}, 2, 9);
        r.b1 = vec(pre + ".in_layers.2.bias", {SO});
        r.gn2g = vec(pre + ".out_layers.0.weight", {SO}); r.gn2b = vec(pre + ".out_layers.0.bias", {SO});
        r.w2 = mat("conv3", pre + ".out_layers.3.weight", {SO}, {SO}, 2, 9); r.b2 = vec(pre + ".out_layers.3.bias", {SO});
        if (r.skip) {
            r.wsk = l1 ? mat("bf16", pre + ".skip_connection.weight", {SO}, {S0, S1}) : mat("bf16", pre + ".skip_connection.weight", {SO}, {S0});
            r.bsk = vec(pre + ".skip_connection.bias", {SO});
        }
        r.emb_off = u.emb_total; u.emb_total += r.cout;
        if (!emb_w_srcs.empty()) { emb_w_srcs += ","; emb_b_srcs += ","; }
        emb_w_srcs += pre + ".emb_layers.1.weight"; emb_b_srcs += pre + ".emb_layers.1.bias";
        add_seg(emb_rspec, emb_padded, lout, r.cout);
        u.res.push_back(r); return (int)u.res.size() - 1;
    };
    auto add_st = [&](const std::string& pre, int lch) {
        StW s{}; s.lc = lch; s.c = pad64(lch); s.heads = s.c / c.num_head_channels;
        const int ch = s.c;
        const Seg S{lch, ch}, F{4 * lch, 4 * lch};
        const std::string tb = pre + ".transformer_blocks.0";
        s.gng = vec(pre + ".norm.weight", {S}); s.gnb = vec(pre + ".norm.bias", {S});
        s.win = mat("bf16", pre + ".proj_in.weight", {S}, {S}); s.bin = vec(pre + ".proj_in.bias", {S});
        s.ln1g = vec(tb + ".norm1.weight", {S}); s.ln1b = vec(tb + ".norm1.bias", {S});
        s.wqk = mat("bf16", tb + ".attn1.to_q.weight," + tb + ".attn1.to_k.weight", {S, S}, {S});
        s.wv = mat("bf16", tb + ".attn1.to_v.weight", {S}, {S});
        s.v_follows = s.wv == s.wqk + (size_t)2 * ch * ch * 2;      // to_v directly behind to_q | to_k in the blob: q | k | v is ONE projection (else the separate V path runs)
        s.wo1 = mat("bf16", tb + ".attn1.to_out.0.weight", {S}, {S}); s.bo1 = vec(tb + ".attn1.to_out.0.bias", {S});
        s.ln2g = vec(tb + ".norm2.weight", {S}); s.ln2b = vec(tb + ".norm2.bias", {S});
        s.wq2 = mat("bf16", tb + ".attn2.to_q.weight", {S}, {S});
        s.wo2 = mat("bf16", tb + ".attn2.to_out.0.weight", {S}, {S}); s.bo2 = vec(tb + ".attn2.to_out.0.bias", {S});
        s.ln3g = vec(tb + ".norm3.weight", {S}); s.ln3b = vec(tb + ".norm3.bias", {S});
        // GEGLU hidden width 4 * lch (a multiple of 128): not padded, only its K side
        s.wff1 = mat("geglu_w", tb + ".ff.net.0.proj.weight", {{8 * lch, 8 * lch}}, {S});
        s.bff1 = mf.add("geglu_b", tb + ".ff.net.0.proj.bias", (size_t)8 * lch * 4);
        s.wff2 = mat("bf16", tb + ".ff.net.2.weight", {S}, {F}); s.bff2 = vec(tb + ".ff.net.2.bias", {S});
        s.wout = mat("bf16", pre + ".proj_out.weight", {S}, {S}); s.bout = vec(pre + ".proj_out.bias", {S});
        // ff.net.2 followed by proj_out is one linear map of [ff | t2]:  [W_out W_2 | W_out], bias W_out b_2 + b_out (packed in fp32)
        s.wfo = mat("fuse_w", tb + ".ff.net.2.weight," + pre + ".proj_out.weight", {S}, {F, S});
        s.bfo = mf.add("fuse_b" + seg_spec("R", {S}), tb + ".ff.net.2.bias," + pre + ".proj_out.weight," + pre + ".proj_out.bias", (size_t)ch * 4);
        s.kv_off = u.kv_total; u.kv_total += 2 * ch;
        s.xa_unit = u.xa_total; u.xa_total += 4LL * XA_NP * ch;      // G, U row-major + their fragment-ordered images (attention.hip: xattn_fused_kernel)
        if (!kv_srcs.empty()) kv_srcs += ",";
        kv_srcs += tb + ".attn2.to_k.weight," + tb + ".attn2.to_v.weight";
        add_seg(kv_rspec, kv_padded, lch, ch); add_seg(kv_rspec, kv_padded, lch, ch);
        u.st.push_back(s); return (int)u.st.size() - 1;
    };
    auto name_of = [](const char* grp, int i, int j) { char b[64]; snprintf(b, sizeof b, "%s.%d.%d", grp, i, j); return std::string(b); };

    // input blocks (openaimodel.py:144-215); all channel bookkeeping below is LOGICAL
    std::vector<int> chans;
    {
        UBlock b; b.where = 0; b.layers.push_back({0, 0});
        u.cinw = mf.add("f32" + seg_spec("R", {{mc, mcp}}), "input_blocks.0.0.weight", (size_t)mcp * c.in_channels * 9 * 4);     // [mc][in][3][3]: rows padded
        u.cinb = vec("input_blocks.0.0.bias", {{mc, mcp}});
        u.blocks.push_back(b); chans.push_back(mc);
    }
    int ch = mc, ds = 1, idx = 1;
    for (int level = 0; level < c.n_channel_mult; level++) {
        const int mult = c.channel_mult[level];
        for (int r = 0; r < c.num_res_blocks; r++) {
            UBlock b; b.where = 0;
            b.layers.push_back({1, add_res(name_of("input_blocks", idx, 0), ch, 0, mult * mc)});
            ch = mult * mc;
            if (in_attn(ds)) b.layers.push_back({2, add_st(name_of("input_blocks", idx, 1), ch)});
            u.blocks.push_back(b); idx++; chans.push_back(ch);
        }
        if (level != c.n_channel_mult - 1) {
            UBlock b; b.where = 0;
            ConvW d{}; d.lc = ch; d.c = pad64(ch); const std::string pre = name_of("input_blocks", idx, 0);
            d.w = mat("conv3", pre + ".op.weight", {{ch, d.c}}, {{ch, d.c}}, 2, 9); d.b = vec(pre + ".op.bias", {{ch, d.c}});
            u.down.push_back(d); b.layers.push_back({3, (int)u.down.size() - 1});
            u.blocks.push_back(b); idx++; chans.push_back(ch); ds *= 2;
        }
    }
    {   // middle (openaimodel.py:223-249)
        UBlock b; b.where = 1;
        b.layers.push_back({1, add_res("middle_block.0", ch, 0, ch)});
        b.layers.push_back({2, add_st("middle_block.1", ch)});
        b.layers.push_back({1, add_res("middle_block.2", ch, 0, ch)});
        u.blocks.push_back(b);
    }
    int oidx = 0;   // output blocks (openaimodel.py:252-305)
    for (int level = c.n_channel_mult - 1; level >= 0; level--) {
        const int mult = c.channel_mult[level];
        for (int i = 0; i <= c.num_res_blocks; i++) {
            const int ich = chans.back(); chans.pop_back();
            UBlock b; b.where = 2; int j = 0;
            b.layers.push_back({1, add_res(name_of("output_blocks", oidx, j++), ch, ich, mc * mult)});
            ch = mc * mult;
            if (in_attn(ds)) b.layers.push_back({2, add_st(name_of("output_blocks", oidx, j++), ch)});
            if (level && i == c.num_res_blocks) {
                ConvW up{}; up.lc = ch; up.c = pad64(ch); const std::string pre = name_of("output_blocks", oidx, j++);
                up.w = mat("conv3", pre + ".conv.weight", {{ch, up.c}}, {{ch, up.c}}, 2, 9); up.b = vec(pre + ".conv.bias", {{ch, up.c}});
                u.up.push_back(up); b.layers.push_back({4, (int)u.up.size() - 1}); ds /= 2;
            }
            u.blocks.push_back(b); oidx++;
        }
    }
    u.outg = vec("out.0.weight", {{mc, mcp}}); u.outb = vec("out.0.bias", {{mc, mcp}});
    // out conv weights stay [Cout][Cin][3][3] fp32 (misc.hip conv_out_kernel): the Cin axis is padded
    u.outw = mf.add(mc == mcp ? std::string("f32") : "f32_cin" + seg_spec("C", {{mc, mcp}}), "out.2.weight", (size_t)c.out_channels * mcp * 9 * 4);
    u.outbias = mf.add("f32", "out.2.bias", (size_t)c.out_channels * 4);
    u.embw = mf.add(std::string("bf16") + (emb_padded ? "|R=" + emb_rspec : ""), emb_w_srcs, (size_t)u.emb_total * ted * 2);
    u.embb = mf.add(std::string("f32") + (emb_padded ? "|R=" + emb_rspec : ""), emb_b_srcs, (size_t)u.emb_total * 4);
    u.kvw = mf.add(std::string("bf16") + (kv_padded ? "|R=" + kv_rspec : ""), kv_srcs, (size_t)u.kv_total * c.context_dim * 2);
}

static VqRes add_vq_res(Manifest& mf, const std::string& pre, int cin, int cout) {
    VqRes r{}; r.cin = cin; r.cout = cout; r.skip = cin != cout;
    r.n1g = mf.f32(pre + ".norm1.weight", cin); r.n1b = mf.f32(pre + ".norm1.bias", cin);
    r.w1 = mf.conv3(pre + ".conv1.weight", cout, cin); r.b1 = mf.f32(pre + ".conv1.bias", cout);
    r.n2g = mf.f32(pre + ".norm2.weight", cout); r.n2b = mf.f32(pre + ".norm2.bias", cout);
    r.w2 = mf.conv3(pre + ".conv2.weight", cout, cout); r.b2 = mf.f32(pre + ".conv2.bias", cout);
    if (r.skip) { r.wsk = mf.bf16(pre + ".nin_shortcut.weight", (size_t)cout * cin); r.bsk = mf.f32(pre + ".nin_shortcut.bias", cout); }
    return r;
}
static VqAttn add_vq_attn(Manifest& mf, const std::string& p, int ch) {
    VqAttn a{}; a.c = ch;
    a.ng = mf.f32(p + ".norm.weight", ch); a.nb = mf.f32(p + ".norm.bias", ch);
    a.wq = mf.bf16(p + ".q.weight", (size_t)ch * ch); a.bq = mf.f32(p + ".q.bias", ch);
    a.wk = mf.bf16(p + ".k.weight", (size_t)ch * ch); a.bk = mf.f32(p + ".k.bias", ch);
    a.wv = mf.bf16(p + ".v.weight", (size_t)ch * ch); a.bv = mf.f32(p + ".v.bias", ch);
    a.wo = mf.bf16(p + ".proj_out.weight", (size_t)ch * ch); a.bo = mf.f32(p + ".proj_out.bias", ch);
    return a;
}
// pre: "decoder.mid" / "encoder.mid"
static VqMid add_vq_mid(Manifest& mf, const std::string& pre, int ch, bool attn) {
    VqMid m{}; m.has_attn = attn;
    m.res1 = add_vq_res(mf, pre + ".block_1", ch, ch);
    if (attn) m.attn = add_vq_attn(mf, pre + ".attn_1", ch);
    m.res2 = add_vq_res(mf, pre + ".block_2", ch, ch);
    return m;
}
// pre: "decoder.up.<lvl>" / "encoder.down.<lvl>"; n_blocks ResnetBlocks ch -> bout (AttnBlocks behind them when the level's resolution
// `res` is in attn_resolutions), then the conv of `resample` ("upsample" / "downsample"; null: none).  ch leaves as the level's width.
static VqLevel add_vq_level(Manifest& mf, const rdm_vq_cfg& c, const std::string& pre, int n_blocks, int& ch, int bout, int res, const char* resample) {
    VqLevel L;
    bool at = false;
    for (int i = 0; i < c.n_attn_resolutions; i++) at = at || c.attn_resolutions[i] == res;
    for (int i = 0; i < n_blocks; i++) {
        L.blocks.push_back(add_vq_res(mf, pre + ".block." + std::to_string(i), ch, bout)); ch = bout;
        if (at) L.attn.push_back(add_vq_attn(mf, pre + ".attn." + std::to_string(i), ch));
    }
    if (resample) {
        const std::string p = pre + "." + resample + ".conv";
        L.resample.c = ch; L.resample.w = mf.conv3(p + ".weight", ch, ch); L.resample.b = mf.f32(p + ".bias", ch);
    }
    return L;
}

static void build_vq(VqModel& v, const rdm_vq_cfg& c, Manifest& mf) {
    v.cfg = c;
    v.wide = c.z_channels > 4;
    if (!c.kl) v.codebook = mf.f32("quantize.embedding.weight", (size_t)c.n_embed * c.embed_dim);
    int bin = c.ch * c.ch_mult[c.n_ch_mult - 1];
    const size_t pq = (size_t)c.z_channels * c.embed_dim;      // wide: post_quant_conv a bf16 GEMM operand, conv_in a conv3 entry; else fp32 for the stem kernels
    v.pqw = v.wide ? mf.bf16("post_quant_conv.weight", pq) : mf.f32("post_quant_conv.weight", pq); v.pqb = mf.f32("post_quant_conv.bias", c.z_channels);
    v.cinw = v.wide ? mf.conv3("decoder.conv_in.weight", bin, c.z_channels) : mf.f32("decoder.conv_in.weight", (size_t)bin * c.z_channels * 9);
    v.cinb = mf.f32("decoder.conv_in.bias", bin);
    v.mid = add_vq_mid(mf, "decoder.mid", bin, c.mid_attn);
    v.levels.assign(c.n_ch_mult, {});
    int curr_res = c.resolution >> (c.n_ch_mult - 1);
    for (int lvl = c.n_ch_mult - 1; lvl >= 0; lvl--, curr_res *= 2)
        v.levels[lvl] = add_vq_level(mf, c, "decoder.up." + std::to_string(lvl), c.num_res_blocks + 1, bin, c.ch * c.ch_mult[lvl], curr_res, lvl ? "upsample" : nullptr);
    v.noutg = mf.f32("decoder.norm_out.weight", bin); v.noutb = mf.f32("decoder.norm_out.bias", bin);
    v.coutw = mf.f32("decoder.conv_out.weight", (size_t)c.out_ch * bin * 9); v.coutb = mf.f32("decoder.conv_out.bias", c.out_ch);
}

static void build_vqenc(VqEncModel& v, const rdm_vq_cfg& c, Manifest& mf) {
    v.cfg = c;
    v.cinw = mf.f32("encoder.conv_in.weight", (size_t)c.ch * c.out_ch * 9); v.cinb = mf.f32("encoder.conv_in.bias", c.ch);
    v.levels.assign(c.n_ch_mult, {});
    int bin = c.ch, curr_res = c.resolution;
    for (int lvl = 0; lvl < c.n_ch_mult; lvl++, curr_res /= 2)
        v.levels[lvl] = add_vq_level(mf, c, "encoder.down." + std::to_string(lvl), c.num_res_blocks, bin, c.ch * c.ch_mult[lvl], curr_res,
                                     lvl != c.n_ch_mult - 1 ? "downsample" : nullptr);
    v.mid = add_vq_mid(mf, "encoder.mid", bin, c.mid_attn);
    v.noutg = mf.f32("encoder.norm_out.weight", bin); v.noutb = mf.f32("encoder.norm_out.bias", bin);
    v.wide = c.z_channels > 4;
    const size_t qc = (size_t)c.embed_dim * c.z_channels;      // wide: conv_out a conv3 entry, quant_conv a bf16 GEMM operand; else fp32 for the head / quantiser kernels
    v.coutw = v.wide ? mf.conv3("encoder.conv_out.weight", c.z_channels, bin) : mf.f32("encoder.conv_out.weight", (size_t)c.z_channels * bin * 9);
    v.coutb = mf.f32("encoder.conv_out.bias", c.z_channels);
    v.qw = v.wide ? mf.bf16("quant_conv.weight", qc) : mf.f32("quant_conv.weight", qc); v.qb = mf.f32("quant_conv.bias", c.embed_dim);
}

static void build_clip(ClipModel& m, const rdm_clip_cfg& c, Manifest& mf) {
    m.cfg = c;
    auto tower = [&](std::vector<ClipBlk>& out, const std::string& pre, int w, int layers) {
        for (int i = 0; i < layers; i++) {
            char b[96]; snprintf(b, sizeof b, "%s.resblocks.%d", pre.c_str(), i); const std::string p = b;
            ClipBlk k{};
            k.ln1g = mf.f32(p + ".ln_1.weight", w); k.ln1b = mf.f32(p + ".ln_1.bias", w);
            k.wqkv = mf.bf16(p + ".attn.in_proj_weight", (size_t)3 * w * w); k.bqkv = mf.f32(p + ".attn.in_proj_bias", 3 * w);
            k.wo = mf.bf16(p + ".attn.out_proj.weight", (size_t)w * w); k.bo = mf.f32(p + ".attn.out_proj.bias", w);
            k.ln2g = mf.f32(p + ".ln_2.weight", w); k.ln2b = mf.f32(p + ".ln_2.bias", w);
            k.wfc = mf.bf16(p + ".mlp.c_fc.weight", (size_t)4 * w * w); k.bfc = mf.f32(p + ".mlp.c_fc.bias", 4 * w);
            k.wpj = mf.bf16(p + ".mlp.c_proj.weight", (size_t)4 * w * w); k.bpj = mf.f32(p + ".mlp.c_proj.bias", w);
            out.push_back(k);
        }
    };
    const int vw = c.vision_width, g = c.image_resolution / c.vision_patch_size, tw = c.transformer_width;
    m.conv1 = mf.bf16("visual.conv1.weight", (size_t)vw * 3 * c.vision_patch_size * c.vision_patch_size);
    m.cls = mf.f32("visual.class_embedding", vw); m.vpos = mf.f32("visual.positional_embedding", (size_t)(g * g + 1) * vw);
    m.lnpreg = mf.f32("visual.ln_pre.weight", vw); m.lnpreb = mf.f32("visual.ln_pre.bias", vw);
    tower(m.vis, "visual.transformer", vw, c.vision_layers);
    m.lnpostg = mf.f32("visual.ln_post.weight", vw); m.lnpostb = mf.f32("visual.ln_post.bias", vw);
    m.vproj = mf.add("bf16_t", "visual.proj", (size_t)vw * c.embed_dim * 2);
    tower(m.text, "transformer", tw, c.transformer_layers);
    m.tok = mf.f32("token_embedding.weight", (size_t)c.vocab_size * tw);
    m.pos = mf.f32("positional_embedding", (size_t)c.context_length * tw);
    m.lnfg = mf.f32("ln_final.weight", tw); m.lnfb = mf.f32("ln_final.bias", tw);
    m.tproj = mf.add("bf16_t", "text_projection", (size_t)tw * c.embed_dim * 2);
}

static void build_rarm(RarmModel& m, const rdm_rarm_cfg& c, Manifest& mf) {
    m.cfg = c; m.C = c.n_heads * c.d_head;
    const int C = m.C;
    m.emb = mf.f32("proj_in.weight", (size_t)c.vocab_in * C);
    m.pos = mf.add("f32_t", "positional_encoding", (size_t)C * c.sequence_length * 4);
    std::string kv_srcs;
    for (int i = 0; i < c.depth; i++) {
        char b[64]; snprintf(b, sizeof b, "transformer_blocks.%d", i); const std::string p = b;
        RarmBlk k{};
        k.ln1g = mf.f32(p + ".norm1.weight", C); k.ln1b = mf.f32(p + ".norm1.bias", C);
        k.wqkv = mf.bf16(p + ".attn1.to_q.weight," + p + ".attn1.to_k.weight," + p + ".attn1.to_v.weight", (size_t)3 * C * C);
        k.wo1 = mf.bf16(p + ".attn1.to_out.0.weight", (size_t)C * C); k.bo1 = mf.f32(p + ".attn1.to_out.0.bias", C);
        k.ln2g = mf.f32(p + ".norm2.weight", C); k.ln2b = mf.f32(p + ".norm2.bias", C);
        k.wq2 = mf.bf16(p + ".attn2.to_q.weight", (size_t)C * C);
        k.wo2 = mf.bf16(p + ".attn2.to_out.0.weight", (size_t)C * C); k.bo2 = mf.f32(p + ".attn2.to_out.0.bias", C);
        k.ln3g = mf.f32(p + ".norm3.weight", C); k.ln3b = mf.f32(p + ".norm3.bias", C);
        k.wff1 = mf.add("geglu_w", p + ".ff.net.0.proj.weight", (size_t)8 * C * C * 2);
        k.bff1 = mf.add("geglu_b", p + ".ff.net.0.proj.bias", (size_t)8 * C * 4);
        k.wff2 = mf.bf16(p + ".ff.net.2.weight", (size_t)C * 4 * C); k.bff2 = mf.f32(p + ".ff.net.2.bias", C);
        if (!kv_srcs.empty()) kv_srcs += ",";
        kv_srcs += p + ".attn2.to_k.weight," + p + ".attn2.to_v.weight";
        m.blk.push_back(k);
    }
    m.kv_total = c.depth * 2 * C;
    m.kvw = mf.add("bf16", kv_srcs, (size_t)m.kv_total * c.context_dim * 2);      // the neighbours' K/V of ALL layers: one GEMM per sampling call
    m.wpo = mf.bf16("proj_out.weight", (size_t)c.vocab_out * C); m.bpo = mf.f32("proj_out.bias", c.vocab_out);
}

// One cfg check per model, called by its manifest entry (c null, load false) and by its load entry.  First what the builder walks --
// array extents, divisors: refused by both entries --, then, for `load`, what the executors and kernels take.
static int cfg_refuse(rdm_ctx* c, const char* msg) { return c ? c->fail(-1, "%s", msg) : -1; }
static int cfg_check_unet(rdm_ctx* c, const rdm_unet_cfg* g, bool /*load*/) {
    if (!g || g->n_channel_mult < 1 || g->n_channel_mult > RDM_MAX_LEVELS || g->n_attention_resolutions > RDM_MAX_LEVELS) return cfg_refuse(c, "bad unet cfg");
    if (g->model_channels % 32 || g->num_head_channels != 32 || g->context_dim % 64 || g->in_channels > 4 || g->out_channels > 4)
        return cfg_refuse(c, "unsupported unet cfg: model_channels % 32 == 0 (GroupNorm32; widths that are not multiples of 64 run zero-padded), num_head_channels == 32, context_dim % 64 == 0 required");
    return 0;
}
// first stage, decoder and encoder.  `exec`: also what the executors take (the decoder's manifest entry describes any cfg that can be walked)
static int cfg_check_first_stage(rdm_ctx* c, const rdm_vq_cfg* g, bool encoder, bool exec) {
    bool ok = g && g->n_ch_mult >= 1 && g->n_ch_mult <= RDM_MAX_LEVELS && g->n_attn_resolutions >= 0 && g->n_attn_resolutions <= RDM_MAX_LEVELS;
    if (ok && exec) {
        const bool narrow = g->embed_dim == 3 && g->z_channels == 3;      // VQ-f4; the decoder also as KL-f4
        const bool wide = g->embed_dim > 0 && g->z_channels > 0 && g->embed_dim % 64 == 0 && g->z_channels % 64 == 0 && !g->kl;      // VQGAN-f16
        ok = g->ch % 64 == 0 && g->out_ch <= 4 && (narrow || wide);
        if (encoder) ok = ok && !g->kl && g->resolution % (1 << (g->n_ch_mult - 1)) == 0;      // the VQ interface only; every Downsample halves exactly
    }
    if (ok) return 0;
    return cfg_refuse(c, encoder ? "unsupported first-stage encoder cfg: n_ch_mult in [1, RDM_MAX_LEVELS], n_attn_resolutions in [0, RDM_MAX_LEVELS], VQ interface (kl = 0), resolution a multiple of 2^(levels - 1), "
                                   "ch % 64 == 0, out_ch <= 4 and either embed_dim == z_channels == 3 (VQ-f4) or both multiples of 64 (VQGAN-f16)"
                                 : "unsupported vq cfg: n_ch_mult in [1, RDM_MAX_LEVELS], n_attn_resolutions in [0, RDM_MAX_LEVELS], ch % 64 == 0, out_ch <= 4 and either embed_dim == z_channels == 3 "
                                   "(VQ-f4 / KL-f4) or both multiples of 64 (VQGAN-f16, kl = 0)");
}
static int cfg_check_vq(rdm_ctx* c, const rdm_vq_cfg* g, bool load) { return cfg_check_first_stage(c, g, false, load); }
static int cfg_check_vqenc(rdm_ctx* c, const rdm_vq_cfg* g, bool /*load*/) { return cfg_check_first_stage(c, g, true, true); }
static int cfg_check_clip(rdm_ctx* c, const rdm_clip_cfg* g, bool load) {
    if (!g || g->vision_patch_size < 1) return cfg_refuse(c, "bad clip cfg: vision_patch_size >= 1 required");
    if (load && (g->transformer_width % 64 || g->vision_width % 64 || g->embed_dim % 8 || g->transformer_heads < 1 || g->transformer_width / g->transformer_heads != 64))
        return cfg_refuse(c, "unsupported clip cfg: widths % 64 == 0 and 64-d heads required");
    return 0;
}
static int cfg_check_rarm(rdm_ctx* c, const rdm_rarm_cfg* g, bool load) {
    if (!g || g->depth < 1 || g->n_heads < 1) return cfg_refuse(c, "bad rarm cfg: depth >= 1 and n_heads >= 1 required");
    if (load && (g->d_head != 64 || g->context_dim % 64 || g->sequence_length > 1024 || g->vocab_out % 2))
        return cfg_refuse(c, "unsupported rarm cfg: d_head == 64, context_dim % 64 == 0, sequence_length <= 1024, even vocab_out required");
    return 0;
}

// rdm_*_manifest: the description is built into a model of its own, nothing is allocated
template <typename M, typename Cfg>
static long long model_manifest(int (*check)(rdm_ctx*, const Cfg*, bool), void (*build)(M&, const Cfg&, Manifest&), const Cfg* cfg,
                                char* buf, size_t buflen, size_t* blob_bytes) {
    if (check(nullptr, cfg, false)) return -1;
    M m{}; Manifest mf; build(m, *cfg, mf);
    if (blob_bytes) *blob_bytes = (mf.total + 255) & ~(size_t)255;
    if (buf && buflen > mf.text.size()) { memcpy(buf, mf.text.c_str(), mf.text.size() + 1); }
    return (long long)mf.text.size();
}

// rdm_load_*: everything that can refuse the load comes before the first change to `live` -- a refused load leaves the model that was
// loaded before fully usable
template <typename M, typename Cfg>
static int load_model(rdm_ctx* c, M& live, int (*check)(rdm_ctx*, const Cfg*, bool), void (*build)(M&, const Cfg&, Manifest&), const Cfg* cfg,
                      const void* packed, size_t nbytes) {
    RDM_TRY(check(c, cfg, true));
    if (!packed) return c->fail(-1, "null blob");
    M next{}; Manifest mf; build(next, *cfg, mf);
    const size_t need = (mf.total + 255) & ~(size_t)255;
    if (nbytes != need) return c->fail(-1, "packed blob is %zu bytes, manifest needs %zu", nbytes, need);
    RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    c->drop_frags();                                  // derived weight layouts refer to blob addresses that may be reused
    live.release();                                   // the old weights, and the arena and everything else made for or from them
    live = next;                                      // (a description only: owns no device memory)
    RDM_CHECK_HIP(c, hipMalloc((void**)&live.blob, need));
    RDM_CHECK_HIP(c, hipMemcpy(live.blob, packed, need, hipMemcpyHostToDevice));
    live.blob_bytes = need; live.loaded = true;
    return 0;
}

long long rdm_unet_manifest(const rdm_unet_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes) { return model_manifest(cfg_check_unet, build_unet, cfg, buf, buflen, blob_bytes); }
long long rdm_vq_manifest(const rdm_vq_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes) { return model_manifest(cfg_check_vq, build_vq, cfg, buf, buflen, blob_bytes); }
long long rdm_vqenc_manifest(const rdm_vq_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes) { return model_manifest(cfg_check_vqenc, build_vqenc, cfg, buf, buflen, blob_bytes); }
long long rdm_clip_manifest(const rdm_clip_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes) { return model_manifest(cfg_check_clip, build_clip, cfg, buf, buflen, blob_bytes); }
long long rdm_rarm_manifest(const rdm_rarm_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes) { return model_manifest(cfg_check_rarm, build_rarm, cfg, buf, buflen, blob_bytes); }

int rdm_load_unet(rdm_ctx* c, const rdm_unet_cfg* cfg, const void* packed, size_t nbytes) { RDM_ENTER(c); return load_model(c, c->unet, cfg_check_unet, build_unet, cfg, packed, nbytes); }
int rdm_load_vq(rdm_ctx* c, const rdm_vq_cfg* cfg, const void* packed, size_t nbytes) { RDM_ENTER(c); return load_model(c, c->vq, cfg_check_vq, build_vq, cfg, packed, nbytes); }
int rdm_load_vqenc(rdm_ctx* c, const rdm_vq_cfg* cfg, const void* packed, size_t nbytes) { RDM_ENTER(c); return load_model(c, c->vqenc, cfg_check_vqenc, build_vqenc, cfg, packed, nbytes); }
int rdm_load_clip(rdm_ctx* c, const rdm_clip_cfg* cfg, const void* packed, size_t nbytes) { RDM_ENTER(c); return load_model(c, c->clip, cfg_check_clip, build_clip, cfg, packed, nbytes); }
int rdm_load_rarm(rdm_ctx* c, const rdm_rarm_cfg* cfg, const void* packed, size_t nbytes) { RDM_ENTER(c); return load_model(c, c->rarm, cfg_check_rarm, build_rarm, cfg, packed, nbytes); }
