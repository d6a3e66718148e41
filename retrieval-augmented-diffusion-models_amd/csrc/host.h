// What the host-side files of librdm_hip share (included only by describe.hip, dispatch.hip, context.hip, unet_exec.hip,
// first_stage.hip, samplers.hip, rarm_exec.hip and ops.hip): the entry macros, manifest / arena / model base, the description structs
// of the five models (rdm_ctx holds them by value), the context, the Ops dispatch struct and run_with_arena.  No function crosses a
// file boundary but the Ops methods, the rdm_* entries and the three UNet functions declared at the end, which samplers.hip calls.
// The C ABI itself is declared in include/rdm_hip.h; every rdm_* definition takes its C linkage from there.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rdm_hip.h"
#include "kernels.h"
#include "knn.h"

#define RDM_CHECK_HIP(ctx, expr)                                                            \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) return (ctx)->fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define RDM_TRY(expr)            \
    do {                         \
        int _r = (expr);         \
        if (_r != 0) return _r;  \
    } while (0)

// Every C-ABI entry binds the calling thread to the context's device for the duration of the call and restores the
// caller's current device on exit (a context for device 1 used from a thread whose current device is 0 must neither
// launch on device 0 nor leave the caller's device changed).
struct DevGuard {
    int prev = -1; bool changed = false;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DevGuard() { if (changed && prev >= 0) (void)hipSetDevice(prev); }
    DevGuard(const DevGuard&) = delete; DevGuard& operator=(const DevGuard&) = delete;
};
#define RDM_ENTER(c) if (!(c)) return -1; DevGuard _dev_guard((c)->device)

// ------------------------------------------------------------------------------------ manifest
struct Manifest {
    std::string text;
    size_t total = 0;
    size_t add(const std::string& kind, const std::string& srcs, size_t nbytes) {      // kind may carry a padding recipe ("|R=..|C=..", build_unet)
        total = (total + 255) & ~(size_t)255;
        const size_t off = total;
        text += std::to_string(off) + " " + std::to_string(nbytes) + " " + kind + " "; text += srcs; text += "\n";
        total += nbytes;
        return off;
    }
    // the unpadded kinds every builder uses, by element count
    size_t f32(const std::string& n, size_t numel) { return add("f32", n, numel * 4); }
    size_t bf16(const std::string& n, size_t numel) { return add("bf16", n, numel * 2); }
    size_t conv3(const std::string& n, size_t cout, size_t cin) { return add("conv3", n, cout * cin * 9 * 2); }      // bf16 [cout][3][3][cin]
};

// ------------------------------------------------------------------------------------ arena
struct Arena {
    char* base = nullptr; size_t cap = 0, off = 0, peak = 0; bool planning = false;
    void reset() { off = 0; }
    void* alloc(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        void* p = base ? base + off : (void*)(uintptr_t)(off + 256);
        off += bytes;
        if (off > peak) peak = off;
        return p;
    }
};

// ------------------------------------------------------------------------------------ what every model owns
template <typename T> static void free_dev(T*& p, size_t& bytes) { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
// A model is a description (cfg, layer graph, blob offsets: filled by its build_* function, which allocates nothing) plus the
// device memory behind it.  A description without memory may be copied (load_model builds one aside and assigns it).
struct ModelBase {
    char* blob = nullptr; size_t blob_bytes = 0; Arena arena; bool loaded = false;
    void release() { free_dev(blob, blob_bytes); free_dev(arena.base, arena.cap); loaded = false; }      // (the caller has synchronised)
};

// ------------------------------------------------------------------------------------ UNet description
// Channel padding.  Every GEMM / conv K loop advances in 64-channel slices and the skip-concat split points sit on slice boundaries,
// so an activation with C channels is held with P(C) = C rounded up to 64 of them, the tail zero: models/rdm/ffhq has
// model_channels 224 (224 / 448 / 672 / 896: multiples of 32 only).  Weights are padded to match by the packer -- the manifest kind
// carries the recipe, "|R=" row segments and "|C=" channel segments as logical>padded pairs, absent when nothing is padded (the
// ImageNet models: byte-identical manifests) -- with zero rows / columns / biases / norm affines in the tail, so a padded channel
// stays exactly zero through every layer.  Only the normalisations must know the LOGICAL counts (group membership and divisor of
// GroupNorm, mean / variance of LayerNorm); attention simply gains all-zero heads.  cin / cout / c below are PHYSICAL counts.
inline int pad64(int c) { return (c + 63) & ~63; }
struct ResW { int cin, cout; size_t gn1g, gn1b, w1, b1, gn2g, gn2b, w2, b2, wsk, bsk; int emb_off; bool skip; int l0, l1, lout, p0, p1; };
constexpr int XA_NP = 128;        // padded (heads x neighbours) width of the skinny cross-attention operands

struct StW {
    int c, heads; size_t gng, gnb, win, bin, ln1g, ln1b, wqk, wv, wo1, bo1, ln2g, ln2b, wq2, wo2, bo2, ln3g, ln3b, wff1,
        bff1, wff2, bff2, wout, bout, wfo, bfo; int kv_off; long long xa_unit;   // xa_unit: per-sample element offset of this layer's (G, U) pair
    int lc;                           // logical channels (c is padded)
    bool v_follows;
};
struct ConvW { int c; size_t w, b; int lc; };
struct ULayer { int kind; int idx; };            // 0 conv_in, 1 res, 2 st, 3 down, 4 up
struct UBlock { int where; std::vector<ULayer> layers; };   // where: 0 input, 1 middle, 2 output

struct UNet : ModelBase {
    rdm_unet_cfg cfg{};
    std::vector<UBlock> blocks; std::vector<ResW> res; std::vector<StW> st; std::vector<ConvW> down, up;
    size_t te0w, te0b, te2w, te2b, embw, embb, kvw, cinw, cinb, outg, outb, outw, outbias;
    int emb_total = 0, kv_total = 0; long long xa_total = 0;         // xa_total: per-sample elements of all (G, U) pairs
    bf16_t* xa_cache = nullptr; size_t xa_cache_bytes = 0;
    // cached cross-attention K/V for the current conditioning
    bf16_t* kv_cache = nullptr; size_t kv_cache_bytes = 0;
    float* emb_table = nullptr; size_t emb_table_bytes = 0;      // rdm_ddim_sample: one row of emb_total floats per sampler timestep
    int ctx_rows = 0;            // samples [ctx_rows, B') of the cached conditioning have ALL-ZERO neighbours (the unconditional half of
                                 // a guided batch): their cross-attention is the output bias, no GEMM runs for them
    void release() { free_dev(xa_cache, xa_cache_bytes); free_dev(kv_cache, kv_cache_bytes); free_dev(emb_table, emb_table_bytes); ModelBase::release(); }
};

// ------------------------------------------------------------------------------------ first-stage description (decoder and encoder)
// ldm / taming Decoder and Encoder are built from the same pieces: ResnetBlocks (+ one AttnBlock per block at attn_resolutions) per
// level, a resampling conv between levels, and a res - attn - res middle.
struct VqRes { int cin, cout; size_t n1g, n1b, w1, b1, n2g, n2b, w2, b2, wsk, bsk; bool skip; };
struct VqAttn { int c; size_t ng, nb, wq, bq, wk, bk, wv, bv, wo, bo; };
struct VqLevel {
    std::vector<VqRes> blocks;
    std::vector<VqAttn> attn;          // one per block, or none
    ConvW resample{};                  // the level's Upsample / stride-2 Downsample conv (the last level walked has none)
};
struct VqMid { VqRes res1, res2; VqAttn attn; bool has_attn; };

struct VqModel : ModelBase {
    rdm_vq_cfg cfg{};
    bool wide = false;                             // z_channels > 4 (taming VQGAN-f16: 256): latent handled as bf16 NHWC tokens, GEMM-class
                                                   // post_quant_conv / conv_in; else the 3-channel VQ-f4 path (tiny fp32 stem kernels)
    size_t codebook, pqw, pqb, cinw, cinb, noutg, noutb, coutw, coutb;
    VqMid mid;
    std::vector<VqLevel> levels;                   // indexed by level (walked high to low; level 0 has no upsample)
    float* code_norms = nullptr;                   // |e_j|^2 of the codebook (vqcode.hip), made on first use by rdm_vq_encode_indices
    void release() { if (code_norms) (void)hipFree(code_norms); code_norms = nullptr; ModelBase::release(); }
};

// First-stage ENCODER (VQ-f4: training input; VQGAN-f16: image -> codes).
// ldm Encoder (ldm/modules/diffusionmodules/model.py; un-vendored: restated from the published code, parity unpinned) as reached from
// MinimalRETRODiffusion.get_input -> encode_first_stage -> VQModelInterface.encode = quant_conv(encoder(x)) under torch.no_grad()
// (rdm/models/diffusion/ddpm.py:390-391): conv_in, per level num_res_blocks ResnetBlocks (+ AttnBlocks at attn_resolutions) and a
// stride-2 Downsample conv with (0, 1, 0, 1) zero padding, mid res-attn-res, GroupNorm + swish + conv_out, quant_conv (1x1).
// The taming VQGAN-f16 encoder (wide latent; un-vendored, parity unpinned) is the same graph: only the tail's weights are stored otherwise
// (conv_out as conv3 bf16, quant_conv as a bf16 GEMM operand: vqenc_body).
struct VqEncModel : ModelBase {
    rdm_vq_cfg cfg{};
    bool wide = false;                             // z_channels > 4 (taming VQGAN-f16): conv_out is an ordinary 3x3 conv, quant_conv a GEMM with an fp32 token-major output
    size_t cinw, cinb, noutg, noutb, coutw, coutb, qw, qb;
    std::vector<VqLevel> levels;                   // indexed by level (walked low to high; the last level has no downsample)
    VqMid mid;
};

// ------------------------------------------------------------------------------------ CLIP description
struct ClipBlk { size_t ln1g, ln1b, wqkv, bqkv, wo, bo, ln2g, ln2b, wfc, bfc, wpj, bpj; };
struct ClipModel : ModelBase {
    rdm_clip_cfg cfg{};
    std::vector<ClipBlk> text, vis;
    size_t tok, pos, lnfg, lnfb, tproj;                               // text
    size_t conv1, cls, vpos, lnpreg, lnpreb, lnpostg, lnpostb, vproj;  // vision
};

// ------------------------------------------------------------------------------------ RARM transformer description
struct RarmBlk { size_t ln1g, ln1b, wqkv, wo1, bo1, ln2g, ln2b, wq2, wo2, bo2, ln3g, ln3b, wff1, bff1, wff2, bff2; };
struct RarmModel : ModelBase {
    rdm_rarm_cfg cfg{}; int C = 0, kv_total = 0;
    std::vector<RarmBlk> blk;
    size_t emb, pos, kvw, wpo, bpo;
    // sampling state: per-layer self-attention K/V cache [depth][2][B'][L][C], projected neighbours [B'*k][depth*2*C],
    // device step counter / completion counter / current tokens, logits of the current step
    char* cache = nullptr; size_t cache_bytes = 0;
    char* ctxkv = nullptr; size_t ctxkv_bytes = 0;
    char* state = nullptr; size_t state_bytes = 0;
    // decode-step cross-attention operands per layer (rarm_prepare): [depth][2][Bc][128][C] bf16 (G, UT), valid for xa_B conditional sequences and xa_k neighbours
    char* xa = nullptr; size_t xa_bytes = 0; int xa_B = 0, xa_k = 0;
    void release() { free_dev(cache, cache_bytes); free_dev(ctxkv, ctxkv_bytes); free_dev(state, state_bytes); free_dev(xa, xa_bytes); xa_B = xa_k = 0; ModelBase::release(); }
};

// ------------------------------------------------------------------------------------ context
struct rdm_ctx {
    int device = 0; hipStream_t stream = nullptr; char err[512] = {0};
    void* zero_page = nullptr; float* eye3 = nullptr;
    UNet unet; VqModel vq; VqEncModel vqenc; ClipModel clip; RarmModel rarm; KnnDb db;
    float* gn_partial = nullptr; size_t gn_partial_bytes = 0;
    char* splitk_ws = nullptr; size_t splitk_ws_bytes = 0;   // fp32 partial planes of the K-split halo convs
    char* samp = nullptr; size_t samp_bytes = 0;     // sampler scratch
    // derived weight layouts, built on first use per weight and dropped when a model is reloaded: fragment-ordered copies of the 3x3 conv
    // weights (conv_halo4.hip) and of the Linear / 1x1 weights (lin4.hip; optionally scaled by a LayerNorm's gamma, with the (s, b') table
    // of the folded LayerNorm beside it).  Keyed on everything the copy depends on -- the entry is the copy of exactly that
    // (weight, shape, kind, gamma): two weights can never alias one entry.
    struct FragKey {
        const void* W; int N, K, kind; const void* aux;       // kind: 0 conv3x3, 1 linear, 2 linear GEGLU-ordered, 3 / 4 = 1 / 2 with LayerNorm folded in (aux = gamma)
        bool operator==(const FragKey& o) const { return W == o.W && N == o.N && K == o.K && kind == o.kind && aux == o.aux; }
    };
    struct FragKeyHash {
        size_t operator()(const FragKey& k) const {
            size_t h = std::hash<const void*>()(k.W);
            for (size_t v : {(size_t)k.N, (size_t)k.K, (size_t)k.kind, (size_t)(uintptr_t)k.aux}) h = (h ^ v) * 0x9E3779B97F4A7C15ull + (h >> 29);
            return h;
        }
    };
    struct FragVal { bf16_t* frag; float* sb; };
    std::unordered_map<FragKey, FragVal, FragKeyHash> wfrag;
    char* bwd_tmp = nullptr; size_t bwd_tmp_bytes = 0;          // scratch of the backward ops (backward.hip)
    char* wfrag_tmp = nullptr; size_t wfrag_tmp_bytes = 0;      // derived copies of caller-owned weights, re-packed per call (Ops::derived)
    void drop_frags() { for (auto& kv : wfrag) { (void)hipFree(kv.second.frag); if (kv.second.sb) (void)hipFree(kv.second.sb); } wfrag.clear(); }
    // derived copy of kind `kind` of the weight W [N][K] (conv kinds: K = input channels): 0 = fragment-ordered 3x3 conv weights
    // (conv_halo4.hip), 1 / 2 = fragment-ordered Linear / 1x1 weights (lin4.hip; 2: GEGLU-ordered), 5 = [4][N][2][2][Cin] phase weights of
    // a fused-upsample conv (igemm.hip CONV == 3)
    static size_t derived_bytes(int kind, int N, int K) { return (size_t)N * K * 2 * (kind == 0 ? 9 : kind == 5 ? 16 : 1); }
    hipError_t pack_derived(int kind, const bf16_t* W, bf16_t* d, int N, int K) {
        return kind == 0 ? launch_conv_w_fragpack(W, d, N, K, stream)
             : kind == 5 ? launch_conv_phase_weights(W, d, N, K, stream)
                         : launch_lin_w_fragpack(W, d, N, K, K, kind == 2, stream);
    }
    // (the copies are packed on `stream`; rdm_set_stream synchronises the old stream before it installs another one, so a copy is
    //  complete before any other stream can launch a kernel that reads it)
    const bf16_t* cached_derived(const bf16_t* W, int N, int K, int kind) {
        const FragKey key{W, N, K, kind, nullptr};
        auto it = wfrag.find(key);
        if (it != wfrag.end()) return it->second.frag;
        bf16_t* d = nullptr;
        if (hipMalloc((void**)&d, derived_bytes(kind, N, K)) != hipSuccess) return nullptr;
        if (pack_derived(kind, W, d, N, K) != hipSuccess) { (void)hipFree(d); return nullptr; }
        wfrag[key] = FragVal{d, nullptr};
        return d;
    }
    // [2][C] fp32 = {0, b}: the rowvec of attn1.to_out over a guided batch's [conditional | unconditional] halves (unet_body: the
    // unconditional rows' cross-attention is exactly attn2.to_out's bias b, which then rides in attn1.to_out's start values)
    const float* zero_bias_pair(const float* b, int C) {
        const FragKey key{b, C, 2, 6, nullptr};
        auto it = wfrag.find(key);
        if (it != wfrag.end()) return it->second.sb;
        float* t = nullptr;
        if (hipMalloc((void**)&t, (size_t)2 * C * sizeof(float)) != hipSuccess) return nullptr;
        if (hipMemsetAsync(t, 0, (size_t)C * sizeof(float), stream) != hipSuccess ||
            hipMemcpyAsync(t + C, b, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) { (void)hipFree(t); return nullptr; }
        wfrag[key] = FragVal{nullptr, t};
        return t;
    }
    // batch-invariant execution (rdm_set_deterministic / env RDM_DETERMINISTIC): every kernel-selection decision (skinny vs tiled GEMM,
    // halo vs generic conv, conv split-K, the zero-context shortcut) is a function of the PER-SAMPLE layer shape only, so a row's
    // result is bitwise independent of the batch it sits in and of the number of ranks the batch is sharded over
    bool deterministic = rdm_env_int(getenv("RDM_DETERMINISTIC"), 0) != 0;
    // debug tap (rdm_debug_tap): the output activation of top-level UNet block `tap_block` (NHWC bf16) is copied into tap_buf by the next forward
    void* tap_buf = nullptr; size_t tap_bytes = 0; int tap_block = -1, tap_sub = 0;      // tap_sub: 0 = the block's output, else 16 * layer-in-block + stage (unet_body)
    int tap_step = 0;      // decode steps (rarm_step) run so far by the current RARM entry: step s shows its stage at byte offset s * (stage bytes)
    // rdm_debug_guidance_prefix: 1 = the shared guidance prefix of a guided forward runs through the first transformer's self-attention,
    // 0 = it ends in front of that transformer (unet_body)
    int prefix_through_attn1 = 1;
    // neighbour bias (rdm_set_neighbour_bias): device fp32 [2 * nn_bias_rows][nn_bias_k], the caller's validated rows followed by as many
    // all-zero rows -- the unconditional half of a guided batch, which is never biased -- so that a kernel over [cond | uncond] samples
    // indexes it by the sample; null: none set.  neighbour_bias_for: the pointer a UNet call over `rows` conditional samples runs under
    // (null without a bias), or -1 with a message when the bias that is set has another shape.
    float* nn_bias = nullptr; size_t nn_bias_bytes = 0; int nn_bias_rows = 0, nn_bias_k = 0;
    int neighbour_bias_for(const char* who, int rows, int k) {
        if (!nn_bias_rows || (rows == nn_bias_rows && k == nn_bias_k)) return 0;
        return fail(-1, "%s: a neighbour bias of %d rows x %d neighbours is set, the call has %d conditional samples x %d neighbours (set a matching bias, or clear it with a null pointer)",
                    who, nn_bias_rows, nn_bias_k, rows, k);
    }
    // RCCL communicator (rdm_comm_*): library handle from dlopen, function table, communicator
    void* rccl_lib = nullptr; void* comm = nullptr; int comm_world = 0;
    // optional per-launch HIP-event profiler for the GEMM-class kernels (bench.py roofline)
    unsigned prof = 0;           // bit k set: record HIP events around launches of kind k (RDM_PROF_* in rdm_hip.h)
    struct ProfRec { hipEvent_t a, b; int kind; double flops; const char* tag; int d0, d1, d2; };      // tag: the op's role in the graph (string literal), d*: its shape
    std::vector<ProfRec> prof_recs; std::vector<hipEvent_t> prof_pool;
    hipEvent_t prof_event() {
        if (!prof_pool.empty()) { hipEvent_t e = prof_pool.back(); prof_pool.pop_back(); return e; }
        hipEvent_t e; hipEventCreate(&e); return e;
    }
    int fail(int code, const char* fmt, ...) {
        va_list ap; va_start(ap, fmt); vsnprintf(err, sizeof err, fmt, ap); va_end(ap); return code;
    }
};

inline int ensure_bytes(rdm_ctx* c, char** p, size_t* have, size_t need) {
    if (*have >= need) return 0;
    if (*p) { RDM_CHECK_HIP(c, hipStreamSynchronize(c->stream)); RDM_CHECK_HIP(c, hipFree(*p)); *p = nullptr; *have = 0; }
    RDM_CHECK_HIP(c, hipMalloc((void**)p, need));
    *have = need; return 0;
}

inline int ensure_gn_partial(rdm_ctx* c, int B) {
    const size_t need = (size_t)B * 32 * 64 * 2 * sizeof(float);
    return ensure_bytes(c, (char**)&c->gn_partial, &c->gn_partial_bytes, need);
}

// The kernel dispatch of the model executors and of the operator-level entries (rdm_op_*): which kernel runs an op, with which
// parameters.  Weight and bias operands are device pointers (executors: o.w<T>(offset) into the model blob).  Every op is one struct,
// filled at the call site by field name; a field a call does not name keeps the default written here (pointers null, counts 0).
// The fields that IgemmParams also has carry its names and meanings.

// out[M, N] = act(alpha A W^T + bias) (+ rowvec) (+ res), A = [A0 | A1] with K = C0 + C1 columns.  (GEGLU: out has N / 2 columns)
struct LinearOp {
    const bf16_t* A0 = nullptr; const bf16_t* A1 = nullptr; int C0 = 0, C1 = 0;
    const float* ln_x = nullptr; const float* ln_g = nullptr; const float* ln_b = nullptr;      // Ops::linear_ln only: A = LayerNorm(ln_x [M][C0] fp32; ln_g, ln_b), A0 unused
    const bf16_t* W = nullptr; const float* bias = nullptr;
    int M = 0, N = 0;
    int act = ACT_NONE;
    const bf16_t* res_bf16 = nullptr; const float* res_f32 = nullptr;
    bf16_t* out_bf16 = nullptr; float* out_f32 = nullptr;
    const float* rowvec = nullptr; int rowvec_ld = 0, rows_per_sample = 1;      // a per-column add shared by each group of rows_per_sample rows (row stride rowvec_ld)
    int a0_wrap_rows = 0, a1_wrap_rows = 0, res_wrap_rows = 0;                  // lin4 only (callers ask lin4_takes first): A0 / A1 / res_bf16 hold that many rows, row m reads m % rows
    float alpha = 1.f;                                                          // (the skinny and mid-size kernels take alpha == 1 only)
    // what the kernel choice reads besides the shape (dispatch.hip: linear_kernel, and the lin4 rule of the deterministic mode):
    bool single_row = false;     // the operand has ONE row per sample (time embedding, RARM decode step, pooled CLIP token)
    int sample_rows = 0;         // rows per sample of the operand where the caller knows them (the UNet's blocks), 0 = unknown
    int choice_rows = 0;         // > M: the op is a shared stage of a guided batch, run once on M of choice_rows logical rows (unet_body's prefix inside the
                                 // first transformer): its kernel is chosen as for choice_rows rows, so a row's value does not depend on where the prefix ends
};
// 3x3 conv over [B, Hin, Win, C0 (+ C1)] NHWC -> [B, Hout, Wout, N]: stride 1 / 2, or ups = 1: on the nearest-2x upsampled input
struct Conv3Op {
    const bf16_t* A0 = nullptr; const bf16_t* A1 = nullptr; int C0 = 0, C1 = 0;
    const bf16_t* W = nullptr; const float* bias = nullptr;
    int B = 0, Hin = 0, Win = 0, N = 0, stride = 1, ups = 0;
    const bf16_t* res_bf16 = nullptr; bf16_t* out_bf16 = nullptr;
    const float* rowvec = nullptr; int rowvec_ld = 0;       // a per-column add per SAMPLE (the time embedding), row stride rowvec_ld
    int asym = 0;                                           // IgemmParams::asym
};
// LayerNorm over rows of C (statistics over the first Clog, the rest zero padding): exactly one x_* and one out_* is given
struct LayerNormOp {
    const float* x_f32 = nullptr; const bf16_t* x_bf16 = nullptr;
    const float* gamma = nullptr; const float* beta = nullptr;
    int M = 0, C = 0;
    float* out_f32 = nullptr; bf16_t* out_bf16 = nullptr;
    int Clog = -1;                                          // -1: = C
    float eps = 1e-5f;
};
// nearest codebook row of every token (vqcode.hip): z f32 [M, E], codebook f32 [N, E], norms = |e_j|^2 (launch_vq_code_norms), ws of
// vq_nearest_ws_bytes(M, N); first minimum on ties, indices as int32 and / or int64
struct VqNearestOp {
    const float* z = nullptr; const float* codebook = nullptr; const float* norms = nullptr;
    long long M = 0; int N = 0, E = 0;
    char* ws = nullptr; int* idx32 = nullptr; long long* idx64 = nullptr;
};

struct Ops {
    rdm_ctx* c; Arena* ar; const char* blob; bool plan; int rc = 0;
    template <typename T> const T* w(size_t off) const { return (const T*)(blob + off); }
    bf16_t* abf(size_t n) { return (bf16_t*)ar->alloc(n * 2); }
    float* af32(size_t n) { return (float*)ar->alloc(n * 4); }
    void check(hipError_t e, const char* what) {
        if (e != hipSuccess && rc == 0) rc = c->fail(-3, "%s: %s", what, hipGetErrorString(e));
    }
    IgemmParams base(int M, int N, int K) const { return igemm_plain(M, N, K, c->zero_page); }
    // Derived weight copies (rdm_ctx::derived_bytes): with constant weights (the executors' blobs; the op entries when their caller promises
    // constant weights) built once per weight and cached in the context, otherwise packed per call into wfrag_tmp.
    // null: the copy could not be made, and the op runs a kernel that reads W itself.
    bool const_weights = true;
    const bf16_t* derived(const bf16_t* W, int N, int K, int kind);
    // the dispatch proper (dispatch.hip, documented there).  Nothing that chooses a kernel is state of Ops: it travels in the op.
    bool lin4_takes(const LinearOp& op);          // reads M, N, C0, C1, a0_wrap_rows, a1_wrap_rows, res_wrap_rows, rowvec (set or not), rowvec_ld, rows_per_sample
    void linear(const LinearOp& op);              // (ignores ln_*)
    bool linear_ln(const LinearOp& op);
    void conv3(const Conv3Op& op);
    int cur_block = -1, cur_layer = 0;           // position in the UNet's block table (debug tap)
    // twice: ptr holds the first half of the logical tensor, whose second half equals it; offset: where in the buffer the copy lands (clipped)
    void tap(int stage, const void* ptr, size_t nbytes, bool twice = false, size_t offset = 0);
    bool prof_open = false;
    const char* tag = "";        // role of the ops that follow in the graph ("st.proj_in", "res.conv1", ...): rdm_prof_dump groups by it
    void prof_begin(int kind, double work, int d0 = 0, int d1 = 0, int d2 = 0);
    void prof_end();
    // The ops below take their kernel's own parameter struct (kernels.h) with the caller's fields named; the dispatch fills in what it
    // owns: groups, nchunk, partial (GroupNorm, head), k = q + C and the strides that follow from it (flash), scale_log2e.
    void groupnorm(GnParams p);
    HeadParams head_params(HeadParams hp) const;
    void head(HeadParams hp, int Clog = 0, bf16_t* tmp = nullptr);      // Clog: logical channels of x (0: = C); tmp [B, H, W, C]: needed only where the fused kernel does not apply
    void vq_nearest(const VqNearestOp& op);
    void layernorm(const LayerNormOp& op);
    void flash_d32(FlashParams f, int heads, int B);
    void causal_d64(CausalD64Params f, int heads, int B, float scale);
    void vq_attention(const VqAttnParams& f, int B);
    void small_attention(const SmallAttnParams& p, int D, int heads, int B, const char* what);
    void xattn_fused(const XattnParams& q);
};

// plan (count bytes) -> ensure arena -> run
template <typename F>
static int run_with_arena(rdm_ctx* c, Arena& ar, const char* blob, F&& body) {
    Ops plan{c, &ar, blob, true};
    char* keep = ar.base; ar.base = nullptr; ar.reset(); ar.peak = 0;
    body(plan);
    const size_t need = ar.peak + 4096;
    ar.base = keep;
    RDM_TRY(ensure_bytes(c, &ar.base, &ar.cap, need));
    ar.reset();
    Ops run{c, &ar, blob, false};
    body(run);
    return run.rc;
}

// ------------------------------------------------------------------------------------ UNet executor, as the samplers use it
// (unet_exec.hip; once per sampling call: the conditioning's K/V into UNet::kv_cache / xa_cache / ctx_rows, the time-embedding rows
// of ts into UNet::emb_table; then one forward per step against them)
int unet_prepare_kv(rdm_ctx* c, float* cat, const float* cond, const float* uncond, int B, int k);
int unet_emb_table(rdm_ctx* c, const std::vector<int>& ts, const float** table);
int unet_forward_impl(rdm_ctx* c, const float* x, const int64_t* t, const float* context, const bf16_t* kv_cached,
                      int b, int k, int H, int W, float* eps_out, int ctx_rows = -1, int shared_half = 0, const float* emb_row = nullptr);
