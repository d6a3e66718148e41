/* librdm_hip.so — C ABI of the MI355X-native retrieval-augmented diffusion sampling path.
 *
 * The reference (CompVis/retrieval-augmented-diffusion-models) is pure Python and has no FFI
 * boundary; each entry point below names the reference call it replaces (file:line relative to
 * the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - return 0 on success, negative on error; rdm_last_error(ctx) gives the message.
 *   - no exceptions cross the ABI; no torch types; plain pointers and sizes.
 *   - pointers marked [dev] are device pointers on the context's HIP device (e.g.
 *     torch.Tensor.data_ptr()); [host] are host pointers.  The caller owns every buffer; the
 *     library keeps no reference to caller memory after a call returns, except rdm_db_load with
 *     copy = 0, which is documented there.
 *   - work is enqueued on the context's stream (rdm_set_stream; default = the null stream, which is
 *     also torch's default current stream) and calls return after enqueue unless noted.
 *   - a context is bound to one device and is not thread-safe.
 *   - layouts at the boundary are the reference's: NCHW fp32 images/latents, [B,k,512] fp32
 *     conditioning, int64 timesteps/tokens.  Internal layout (NHWC bf16) is private.
 */
#ifndef RDM_HIP_H
#define RDM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rdm_ctx rdm_ctx;

#define RDM_MAX_LEVELS 8

/* UNetModel constructor arguments that shape the sampling graph
 * (rdm/modules/diffusionmodules/openaimodel.py:66-129; models/rdm/imagenet/config.yaml:36-59). */
typedef struct {
    int in_channels, out_channels, model_channels, num_res_blocks;
    int n_attention_resolutions, attention_resolutions[RDM_MAX_LEVELS];
    int n_channel_mult, channel_mult[RDM_MAX_LEVELS];
    int num_head_channels, context_dim;
} rdm_unet_cfg;

/* First-stage decoder: ldm VQModelInterface ddconfig (models/rdm/imagenet/config.yaml:60-80) and taming VQModel ddconfig of the
 * RARM models (models/rarm/imagenet/dogs/config.yaml:28-51: embed_dim = z_channels = 256, ch_mult 1,1,2,2,4, attn_resolutions [16]). */
typedef struct {
    int embed_dim, n_embed, z_channels, ch, n_ch_mult, ch_mult[RDM_MAX_LEVELS];
    int num_res_blocks, out_ch, resolution, mid_attn, kl; /* kl=1: AutoencoderKL decode (no quantiser) */
    int n_attn_resolutions, attn_resolutions[RDM_MAX_LEVELS];   /* AttnBlock after every ResnetBlock of the levels at these resolutions */
} rdm_vq_cfg;

/* RetrievalPatchTransformer constructor arguments of the RARM models (rdm/modules/attention.py:206-249;
 * models/rarm/imagenet/dogs/config.yaml:14-27: continuous = false, causal, cross_attend, positional_encodings). */
typedef struct {
    int vocab_in, vocab_out;      /* in_channels (token embedding rows, incl. mask / sos tokens), out_channels (logits) */
    int n_heads, d_head, depth, context_dim, sequence_length;
} rdm_rarm_cfg;

/* LatentImageRETRO.sample arguments (rdm/models/autoregression/transformer.py:224-294). */
typedef struct {
    int batch, k;                 /* sequences, neighbours per sequence in r [batch,k,context_dim] */
    int cond_len, steps;          /* conditioning tokens c [batch,cond_len] (the sos token), tokens to sample */
    float temperature; int top_k; /* top_k <= 0: no filter */
    float guidance_scale;         /* > 1: batch doubled with zero neighbours, logits_u + s (logits_c - logits_u) (:237-253) */
} rdm_rarm_sample_args;

/* CLIP constructor arguments (rdm/modules/custom_clip/model.py:238-252). */
typedef struct {
    int embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size;
    int context_length, vocab_size, transformer_width, transformer_heads, transformer_layers;
} rdm_clip_cfg;

/* DDIMSampler.sample arguments the native loop implements (rdm/models/diffusion/ddim.py:58-140). */
typedef struct {
    int S;                 /* number of DDIM steps */
    int batch;             /* B */
    int k;                 /* neighbours in the conditioning [B,k,context_dim] */
    int channels, height, width;      /* latent shape (3,64,64) */
    float eta, temperature;
    float unconditional_guidance_scale;   /* >= 1; > 1 enables CFG batch doubling (ddim.py:229-238) */
    int log_every_t;       /* intermediates rule, ddim.py:207 */
    /* schedule: the model's fp32 alphas_cumprod buffer [T] (ddim.py:30) */
    int T; const float* alphas_cumprod; /* [host] */
} rdm_ddim_args;

/* DPM-Solver++(2M) arguments (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models";
 * ldm models/diffusion/dpm_solver/sampler.py): the multistep data-prediction solver on an explicit list of integer timesteps. */
typedef struct {
    int batch, k, channels, height, width;
    float unconditional_guidance_scale;   /* >= 1; > 1 enables CFG batch doubling */
    int order;             /* 1 (= DDIM with eta 0) | 2 (2M) */
    int lower_order_final; /* the last step is first order (recommended below 15 steps) */
    int log_every_t;       /* intermediates rule of the DDIM loop over n_nodes - 1 steps */
    int T; const float* alphas_cumprod; /* [host] the model's fp32 buffer [T] */
    int n_nodes; const int* nodes;      /* [host] strictly decreasing timesteps in [0, T-1]; the UNet runs at nodes[0 .. n_nodes-2] */
} rdm_dpmpp_args;

/* UniPC arguments (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models"): the
 * multistep data-prediction predictor-corrector on an explicit list of integer timesteps. */
typedef struct {
    int batch, k, channels, height, width;
    float unconditional_guidance_scale;   /* >= 1; > 1 enables CFG batch doubling */
    int order;             /* 1 | 2 | 3: the predictor's order; the corrector adds one */
    int variant;           /* 0 = bh1 (B(h) = -h) | 1 = bh2 (B(h) = expm1(-h)) */
    int corrector;         /* 0: predictor only (order 2, bh2 is then DPM-Solver++(2M); order 1 is DDIM with eta 0) */
    int lower_order_final; /* step s of n runs at order min(order, s, n + 1 - s) instead of min(order, s) */
    int log_every_t;       /* intermediates rule of the DDIM loop over n_nodes - 1 steps */
    int T; const float* alphas_cumprod; /* [host] the model's fp32 buffer [T] */
    int n_nodes; const int* nodes;      /* [host] strictly decreasing timesteps in [0, T-1]; the UNet runs at nodes[0 .. n_nodes-2] */
} rdm_unipc_args;

/* ldm LatentDiffusion.p_sample_loop arguments (reached from rdm/models/diffusion/ddpm.py:1008). */
typedef struct {
    int timesteps;         /* loop runs reversed(range(timesteps)) */
    int batch, k, channels, height, width;
    int clip_denoised; float temperature;
    int T;                 /* schedule length; arrays below are fp32 [T], [host] */
    const float* sqrt_recip_alphas_cumprod; const float* sqrt_recipm1_alphas_cumprod;
    const float* posterior_mean_coef1; const float* posterior_mean_coef2;
    const float* posterior_log_variance_clipped;
} rdm_ddpm_args;

/* ---- context -------------------------------------------------------------------------------- */
int rdm_ctx_create(int device_id, rdm_ctx** out);
void rdm_ctx_destroy(rdm_ctx* ctx);
const char* rdm_last_error(rdm_ctx* ctx);
/* Frees the grow-only work buffers of the context (backward scratch incl. up to 256 MB of fp32 weight-gradient planes per conv,
 * split-K planes, per-call weight re-packs, sampler scratch); they are re-created on demand.  Weights, caches and arenas stay. */
int rdm_release_scratch(rdm_ctx* ctx);
int rdm_set_stream(rdm_ctx* ctx, void* hip_stream);
const char* rdm_version(void);
/* Batch-invariant ("deterministic") execution: every kernel-selection decision of the library (skinny vs tiled GEMM, halo vs generic
 * 3x3 conv, conv split-K, the zero-context shortcut) becomes a function of the per-sample layer shape only, so a sample's result is
 * bitwise independent of the batch it is computed in and of the number of ranks the batch is sharded over (the reference gives no such
 * guarantee either way: cuDNN picks algorithms per shape).  Default off (env RDM_DETERMINISTIC=1 turns it on for new contexts); the
 * speed cost is stated in DESIGN.md. */
int rdm_set_deterministic(rdm_ctx* ctx, int on);
int rdm_get_deterministic(rdm_ctx* ctx);

/* ---- weights --------------------------------------------------------------------------------
 * The library defines the packed-blob layout; rdm_*_manifest writes it as text, one line per entry:
 *     <offset> <nbytes> <kind> <src>[,<src>...]
 * where <src> are the reference's own state_dict keys and <kind> is one of
 *   f32 | bf16 | bf16_t | conv3 | geglu_w | geglu_b   (see DESIGN.md section 2), or a DERIVED entry
 *   fuse_w  <ff.net.2.weight>,<proj_out.weight>                  -> bf16 [C][5C] = [W_out W_2 | W_out]   (multiplied out in fp64)
 *   fuse_b  <ff.net.2.bias>,<proj_out.weight>,<proj_out.bias>    -> f32  [C]     = W_out b_2 + b_out
 * (the SpatialTransformer's ff.net.2 and proj_out run as one GEMM, attention.py:88-96 + 190-195).
 * The caller fills a host blob accordingly and hands it to rdm_load_*, which copies it to HBM.
 * Returns the number of bytes needed for the text (excluding NUL) if buf is too small. */
long long rdm_unet_manifest(const rdm_unet_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes);
long long rdm_vq_manifest(const rdm_vq_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes);
long long rdm_clip_manifest(const rdm_clip_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes);
/* replaces torch.load + load_state_dict for model.diffusion_model / first_stage_model / CLIP
 * (scripts/rdm_sample.py:163-170, rdm/modules/retrievers.py:76). packed [host]. */
int rdm_load_unet(rdm_ctx* ctx, const rdm_unet_cfg* cfg, const void* packed, size_t nbytes);
int rdm_load_vq(rdm_ctx* ctx, const rdm_vq_cfg* cfg, const void* packed, size_t nbytes);
int rdm_load_clip(rdm_ctx* ctx, const rdm_clip_cfg* cfg, const void* packed, size_t nbytes);
/* RARM transformer (state_dict keys of rdm.modules.attention.RetrievalPatchTransformer, prefix `transformer.` stripped);
 * extra manifest kind  f32_t  = 2-D tensor stored transposed (positional_encoding [C,L] -> [L][C]). */
long long rdm_rarm_manifest(const rdm_rarm_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes);
int rdm_load_rarm(rdm_ctx* ctx, const rdm_rarm_cfg* cfg, const void* packed, size_t nbytes);

/* ---- UNet: UNetModel.forward(x, timesteps, context) (openaimodel.py:335-371) via
 *      MinimalRETRODiffusion.apply_model (rdm/models/diffusion/ddpm.py:445-458).
 * x [dev] f32 [b,Cin,H,W]; t [dev] int64 [b]; ctx [dev] f32 [b,k,context_dim]; eps_out [dev] f32 [b,Cout,H,W]. */
int rdm_unet_forward(rdm_ctx* ctx, const float* x, const int64_t* t, const float* context, int b, int k, int H, int W,
                     float* eps_out);

/* ---- neighbour bias: one additive term per (sample, neighbour) on the UNet's cross-attention scores (the `mask` argument of ldm's
 * CrossAttention.forward, rdm/modules/attention.py:42-58, as an additive term).
 *   bias[b][j], fp32, is added to EVERY head's score of neighbour j of sample b, after the 1/sqrt(d) scale and before the softmax over the
 *   k neighbours.  0 is the unbiased model; log w makes the neighbour count w times; -inf removes it: its probability is exactly 0 and
 *   its (finite) embedding has no influence on the result at all.  Refused with -1 and a message (the context stays usable, the bias
 *   that was in force stays in force): +inf, NaN, and a row without a finite entry.  The neighbour embeddings themselves must be
 *   finite; masked places conventionally hold zeros.
 *   The bias belongs to the conditional rows: the unconditional half of a guided batch is never biased (it is skipped through the
 *   to_out.bias shortcut when its neighbours are all zero, and attends its caller-given neighbours unbiased otherwise).
 * bias_host: HOST fp32 [rows][k]; the library validates it and keeps a device copy, in force until cleared (bias_host NULL; rows and k are
 * then ignored) or replaced.  Honoured by rdm_unet_forward (rows == b) and by rdm_unet_forward_guided and every sampler entry (DDIM, PLMS,
 * DPM-Solver++, UniPC, DDPM, seeded or not, the SDE solver, rdm_ddim_decode / _encode / _inpaint; rows == batch), in deterministic
 * mode too.  A bias whose (rows, k) does not match such a call makes the call fail with -1 and a message: it is never silently
 * ignored.  The RARM, CLIP, first-stage and training entries do not read it.
 * rdm_get_neighbour_bias: 1 = a bias is set (*rows, *k filled), 0 = none (*rows = *k = 0); either pointer may be NULL. */
int rdm_set_neighbour_bias(rdm_ctx* ctx, const float* bias_host, int rows, int k);
int rdm_get_neighbour_bias(rdm_ctx* ctx, int* rows, int* k);

/* ---- device noise ------------------------------------------------------------------------------
 * The library's own definition of "sample i of seed s": Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key
 * increments 0x9E3779B9 / 0xBB67AE85, ten rounds) with
 *     key        = (seed low 32 bits, seed high 32 bits)
 *     counter[0] = block   = (element index WITHIN the sample row) >> 2
 *     counter[1] = step    = draw index: the loop step counted from 0 in loop order (the i-th step taken)
 *     counter[2] = row     = GLOBAL sample index, row0 + b
 *     counter[3] = stream  = 0: the forward process's noise | 1: per-step update noise | >= 2: reserved, refused by the entries
 * Stream 0 is the noise of the forward process q(x_t | x_0): step 0 the starting latent x_T (and rdm_op_q_sample_seeded's noise), step i + 1
 * the noise the inpainting loop gives the known region at loop step i (a seeded rdm_ddim_inpaint).
 * Element e of a row takes output word e & 3 of block e >> 2: rows never share a block, and a value depends on (seed, stream, step, row, e)
 * only -- not on the batch size, on how row0 splits a batch, on the grid or on the vector width.  Normals are Box-Muller on the word pairs
 * (w0, w1) and (w2, w3): u = ((w >> 9) + 0.5) 2^-23 (exact in fp32, strictly inside (0, 1), so |z| <= 5.77), r = sqrtf(-2 logf(u1)),
 * sincospif(2 u2, &s, &c); element 2h = r c, element 2h + 1 = r s of pair h.  row0 + B must fit 32 bits and per_row must be at most 2^34.
 *
 * rdm_rng_words: host code only (ctx-free): the four words of one block, out[4] [host].  Returns 0, -1 for a null out.
 * rdm_op_rng_words / rdm_op_randn: the word / the normal each element of B rows of per_row elements would consume at (step, stream), rows
 * row0 .. row0 + B - 1; out [dev] [B, per_row] (uint32 / f32).  Any per_row >= 1 (a row's last block may be partial); an out that is not
 * 16-byte aligned, or a per_row that is no multiple of 4, takes scalar stores.
 *
 * rdm_noise: where a sampler loop or a step op takes its noise from -- the one `noise` argument of every entry that consumes some.  A NULL
 * pointer, or seeded == 0 with a NULL stack, is no noise source, and each entry says what it then does.  seeded != 0: loop step i applies
 * the normals of (seed, stream 1, step i, row0 + b), generated in registers in the pass that applies them -- bit for bit the stack form fed
 * with rdm_op_randn(seed, row0, B, per_row, step = i, stream = 1).  A seeded call has no scalar form: C*H*W (the ops: per_row, which must
 * divide n) must be a multiple of 4, every operand 16-byte aligned, and rows [row0, row0 + B) must pass the row check above (-1 with a
 * message otherwise).  A seeded loop that takes x_T may be given a NULL one: the start is then the normals of (seed, stream 0, step 0).
 * seeded != 0 together with a stack is refused (-1, "give a seed or a stack, not both"); the context stays usable. */
typedef struct rdm_noise {
    const float* stack;    /* [dev] caller's noise tensor, or NULL */
    int          seeded;   /* != 0: the library's generator under (seed, row0); stack must be NULL */
    uint64_t     seed;
    int64_t      row0;
    int64_t      per_row;  /* read by the rdm_op_* entries only (the loops derive it from args) */
    uint32_t     step;     /* read by the rdm_op_* entries only (the loops count it) */
} rdm_noise;
int rdm_rng_words(uint64_t seed, uint32_t row, uint32_t step, uint32_t stream, uint32_t block, uint32_t* out);
int rdm_op_rng_words(rdm_ctx* ctx, uint64_t seed, int64_t row0, int64_t B, int64_t per_row, uint32_t step, uint32_t stream, uint32_t* out);
int rdm_op_randn(rdm_ctx* ctx, uint64_t seed, int64_t row0, int64_t B, int64_t per_row, uint32_t step, uint32_t stream, float* out);

/* ---- samplers -------------------------------------------------------------------------------
 * DDIMSampler.sample / ddim_sampling / p_sample_ddim (rdm/models/diffusion/ddim.py:58-268).
 * x_T [dev] f32 [B,C,H,W]; cond, uncond [dev] f32 [B,k,ctx_dim] (uncond may be NULL when scale == 1);
 * noise (rdm_noise above): the stack is [dev] f32 [S,B,C,H,W], consumed in loop order; a source is required when eta > 0, and with eta == 0
 * no step noise is drawn from either kind.  x_T may be NULL only when seeded;
 * z_out [dev] f32 [B,C,H,W]; x_inter / pred_x0_inter [dev] f32 [n_inter,B,C,H,W] or NULL, filled for the
 * steps ddim.py:207 logs (n_inter = rdm_ddim_num_intermediates). */
int rdm_ddim_num_intermediates(int S, int log_every_t);
int rdm_ddim_sample(rdm_ctx* ctx, const rdm_ddim_args* args, const float* x_T, const float* cond, const float* uncond,
                    const rdm_noise* noise, float* z_out, float* x_inter, float* pred_x0_inter);
/* ldm PLMSSampler.sample / plms_sampling / p_sample_plms (ldm/models/diffusion/plms.py): pseudo linear multistep sampling on DDIM's
 * schedule with eta = 0 (args->eta != 0 is an error, as make_schedule's ValueError; temperature has no effect there).  The first step is
 * the pseudo improved Euler step (two forwards), later steps combine the guided eps with up to three earlier ones: S' + 1 forwards for
 * S' sampler timesteps.  Arguments as rdm_ddim_sample without the noise stack; the intermediates follow the DDIM rule
 * (n_inter = rdm_ddim_num_intermediates), pred_x0_inter holding the pred_x0 of the combined eps. */
int rdm_plms_sample(rdm_ctx* ctx, const rdm_ddim_args* args, const float* x_T, const float* cond, const float* uncond,
                    float* z_out, float* x_inter, float* pred_x0_inter);
/* DPM-Solver++(2M) (Lu et al. 2022; ldm models/diffusion/dpm_solver/sampler.py, multistep "dpmsolver++") on integer timesteps.  With
 * a = alphas_cumprod[t] in float64, alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(a / (1 - a)) / 2, step j goes from
 * s = nodes[j] to t = nodes[j+1]: m_j = (x - sigma_s eps) / alpha_s with the guided eps, h_j = lambda_t - lambda_s,
 * D = (1 + 1/(2r)) m_j - (1/(2r)) m_{j-1} with r = h_{j-1} / h_j when order == 2, j >= 1 and not (lower_order_final and the last step),
 * else D = m_j; x <- (sigma_t / sigma_s) x - alpha_t expm1(-h_j) D.  n_nodes - 1 UNet forwards; the result lives at the noise level of
 * nodes[n_nodes-1].  Order 1 is DDIM with eta = 0.  pred_x0_inter holds m_j; the intermediates follow the DDIM rule over
 * n_nodes - 1 steps (n_inter = rdm_ddim_num_intermediates(n_nodes - 1, log_every_t)).  Other arguments as rdm_plms_sample. */
int rdm_dpmpp_sample(rdm_ctx* ctx, const rdm_dpmpp_args* args, const float* x_T, const float* cond, const float* uncond,
                     float* z_out, float* x_inter, float* pred_x0_inter);
/* Node lists for rdm_dpmpp_sample, host code only (ctx-free).  skip_type 0 (time_uniform): DDIM's S-step timesteps descending, then 0
 * (S / T as rdm_ddim_sample).  skip_type 1 (logSNR): S + 1 targets uniform in lambda from lambda(T-1) to lambda(0), each rounded to the
 * timestep of nearest lambda (ties to the smaller t), duplicates dropped, 0 appended when missing -- fewer than S steps when targets
 * collide.  nodes_out holds S + 1 entries (time_uniform with an S that does not divide T: ceil(T / (T / S)) + 1); returns the number of
 * nodes written, or a negative value for bad arguments. */
int rdm_dpmpp_timesteps(const float* alphas_cumprod, int T, int S, int skip_type, int* nodes_out);
/* UniPC (Zhao et al. 2023), multistep data prediction on integer timesteps; node quantities alpha_i, sigma_i, lambda_i as in
 * rdm_dpmpp_sample, n = n_nodes - 1 steps and n forwards at nodes[0 .. n-1].  u_j is the UNet input at node j (u_0 = x_0 = x_T),
 * m_j = (u_j - sigma_j eps_j) / alpha_j with the guided eps at (u_j, nodes[j]).  Step s (1-based, ending at node s) has order
 * p = min(order, s), with lower_order_final also at most n + 1 - s.  h = lambda_s - lambda_{s-1}, hh = -h, phi_1 = expm1(hh), B = hh (bh1) or
 * expm1(hh) (bh2); r_i = (lambda_{s-1-i} - lambda_{s-1}) / h for i < p, r_p = 1; g_1 = phi_1 / hh - 1, g_{i+1} = g_i / hh - 1 / (i+1)!,
 * b_i = g_i i! / B; R_{i,k} = r_k^{i-1}.  Predictor weights (p - 1 values): none, [1/2], or the solution of R[1..2,1..2] rho = b[1..2];
 * corrector weights (p values): [1/2] for p = 1, else the solution of R rho = b.  With D_i = (m_{s-1-i} - m_{s-1}) / r_i and
 * base = (sigma_s / sigma_{s-1}) x_{s-1} - alpha_s phi_1 m_{s-1}:  u_s = base - alpha_s B sum_{i<p} rho^p_i D_i, and, m_s being the forward at u_s,
 * x_s = base - alpha_s B (sum_{i<p} rho^c_i D_i + rho^c_p (m_s - m_{s-1})).  Corrector off: x_s = u_s.  The last node is not corrected; the
 * result is u_n.  One forward and one fused kernel pass per step: the pass after forward j corrects x_j and predicts u_{j+1}.
 * x_inter holds u_{j+1}, pred_x0_inter m_j, by the DDIM rule over n steps (n_inter = rdm_ddim_num_intermediates(n, log_every_t)).
 * Node lists come from rdm_dpmpp_timesteps.  Other arguments as rdm_plms_sample. */
int rdm_unipc_sample(rdm_ctx* ctx, const rdm_unipc_args* args, const float* x_T, const float* cond, const float* uncond,
                     float* z_out, float* x_inter, float* pred_x0_inter);
/* The scalars of the pass after forward j (0 <= j <= n_nodes - 2) of rdm_unipc_sample, host code only (ctx-free), float64 from the fp32
 * alphas_cumprod.  out[13] = alpha_j, sigma_j, a_x, a_t, a_1, a_2, a_3, b_x, b_0, b_1, b_2, order_c, order_p with
 * x_j = a_x x_{j-1} + a_t m_j + a_1 m_{j-1} + a_2 m_{j-2} + a_3 m_{j-3} (order_c = the order of step j, 0 when x_j = u_j: j = 0 or no corrector;
 * coefficients beyond the order are 0) and u_{j+1} = b_x x_j + b_0 m_j + b_1 m_{j-1} + b_2 m_{j-2} (order_p = the order of step j + 1).
 * Returns 0, or a negative value for bad arguments (nodes as rdm_unipc_sample requires them). */
int rdm_unipc_coefficients(const float* alphas_cumprod, int T, const int* nodes, int n_nodes, int j, int order, int variant, int corrector,
                           int lower_order_final, double* out);
/* ldm LatentDiffusion.p_sample_loop / p_sample (no CFG on this path).
 * noise (rdm_noise, required): the stack is [dev] f32 [timesteps,B,C,H,W], consumed in loop order; the final step consumes none from
 * either kind.  x_T may be NULL only when seeded. */
int rdm_ddpm_sample(rdm_ctx* ctx, const rdm_ddpm_args* args, const float* x_T, const float* cond, const rdm_noise* noise,
                    float* z_out);

/* SDE-DPM-Solver++(2M): the "sde-dpmsolver++" multistep update of Lu et al.'s reference implementation, a stochastic sampler at
 * DPM-Solver++'s step counts, on rdm_dpmpp_sample's arguments, node quantities and order rule.  Step j from s = nodes[j] to t = nodes[j+1],
 * h = lambda_t - lambda_s, m_j = (x - sigma_s eps) / alpha_s with the guided eps:
 *     g   = alpha_t (1 - exp(-2h))                                           (= -alpha_t expm1(-2h))
 *     x  <- (sigma_t / sigma_s) exp(-h) x + g m_j  [+ (g / (2r)) (m_j - m_{j-1}), r = h_{j-1} / h, on a second-order step]
 *           + sigma_t sqrt(1 - exp(-2h)) z_j,   z_j ~ N(0, I)
 * The host flattens this in float64 to x <- c_x x + c_0 m_j + c_1 m_{j-1} + c_n z_j; the kernel sums left to right in fp32.  The noise is
 * not scaled by an eta.  noise (rdm_noise, required): z_j = stack[j], [dev] f32 [n_nodes - 1, B, C, H, W], or drawn at step j when seeded;
 * x_T may be NULL only when seeded.  pred_x0_inter holds m_j; intermediates and other arguments as rdm_dpmpp_sample. */
int rdm_dpmpp_sde_sample(rdm_ctx* ctx, const rdm_dpmpp_args* args, const float* x_T, const float* cond, const float* uncond,
                         const rdm_noise* noise, float* z_out, float* x_inter, float* pred_x0_inter);

/* ---- image-to-image on the DDIM schedule (ldm DDIMSampler.stochastic_encode / encode / decode; the reference's vendored ddim.py stops
 * before them) ------------------------------------------------------------------------------------
 * The schedule of args->S has `total` ascending timesteps ts[0 .. total-1] (total may exceed S, as in rdm_ddim_sample), levels
 * a_t[i] = alphas_cumprod[ts[i]] and a_prev[i] = alphas_cumprod[0] for i = 0, else alphas_cumprod[ts[i-1]].  "Level index i" is a_t[i].
 *
 * rdm_ddim_decode: x_latent [dev] f32 [B,C,H,W] is taken to be at level index t_start - 1; the DDIM step runs at indices
 * t_start - 1 ... 0 -- t_start forwards -- with the step arithmetic, CFG batch doubling, eta, temperature and intermediates rule of
 * rdm_ddim_sample over t_start steps (n_inter = rdm_ddim_num_intermediates(t_start, log_every_t)).  1 <= t_start <= total;
 * t_start == total is rdm_ddim_sample, bit for bit.  noise as rdm_ddim_sample's, the stack [dev] f32 [t_start,B,C,H,W]; seeded, step i of
 * THIS call (counted from 0) draws at step i.  x_latent is required either way.
 *
 * rdm_ddim_encode: deterministic DDIM inversion, t_enc steps up the schedule (1 <= t_enc <= total).  Step i = 0 .. t_enc - 1 moves the
 * iterate from level a_prev[i] to level a_t[i]:
 *     e = e_c (scale == 1) | e_u + scale (e_c - e_u);  pred_x0 = (x - sqrt(1 - a_prev[i]) e) / sqrt(a_prev[i]);
 *     x <- sqrt(a_t[i]) pred_x0 + sqrt(1 - a_t[i]) e
 * with the UNet evaluated on the current iterate at the TARGET timestep ts[i] (not ldm's loop index, not the current level's timestep:
 * DESIGN.md section 3 has the measurement).  The result is at level index t_enc - 1: what rdm_ddim_decode(t_start = t_enc) expects.
 * args->eta must be 0; args->unconditional_guidance_scale is the inversion's own scale (1 unless the caller knows better: guided
 * inversion diverges).  x_inter [dev] f32 [n_inter,B,C,H,W] or NULL: the iterate after the steps with i % log_every_t == 0 or
 * i == t_enc - 1 (n_inter = rdm_ddim_num_intermediates(t_enc, log_every_t)).
 *
 * All three return -1 with a message, and leave the context usable, for a t_start / t_enc outside [1, total], a null pointer, a missing
 * uncond at scale > 1, and eta != 0 on encode. */
int rdm_ddim_decode(rdm_ctx* ctx, const rdm_ddim_args* args, int t_start, const float* x_latent, const float* cond, const float* uncond,
                    const rdm_noise* noise, float* z_out, float* x_inter, float* pred_x0_inter);
int rdm_ddim_encode(rdm_ctx* ctx, const rdm_ddim_args* args, int t_enc, const float* x0, const float* cond, const float* uncond,
                    float* z_out, float* x_inter);
/* The inversion step kernel alone on caller-owned [dev] f32 buffers of n elements (eps: 2n under cfg, [cond | uncond]): pred_x0 =
 * (x - sqrt_one_minus_a_cur e) / sqrt_a_cur, x_out = sqrt_a_next pred_x0 + sqrt_one_minus_a_next e.  x_out may be x; x_dup and pred_x0
 * may be NULL.  float4 accesses when n % 4 == 0 and every operand is 16-byte aligned, else scalar ones. */
int rdm_op_ddim_inverse_step(rdm_ctx* ctx, const float* x, const float* eps, long long n, int cfg, float scale, float sqrt_a_cur,
                             float sqrt_one_minus_a_cur, float sqrt_a_next, float sqrt_one_minus_a_next, float* x_out,
                             float* x_dup_or_null, float* pred_x0_or_null);
/* ldm stochastic_encode without a noise tensor: out = sqrt_a x0 + sqrt_1ma z over B rows of per_row elements, z the normals of
 * (seed, stream 0, step 0, row0 + b) drawn in registers -- the normals a seeded sampling call starts from, so rows [row0, row0 + B) may
 * be split over calls.  per_row % 4 == 0 and 16-byte aligned x0 / out are required (-1 otherwise).  out may be x0. */
int rdm_op_q_sample_seeded(rdm_ctx* ctx, const float* x0, int64_t B, int64_t per_row, float sqrt_a, float sqrt_1ma, uint64_t seed,
                           int64_t row0, float* out);

/* ---- inpainting on the DDIM schedule (ldm DDIMSampler.ddim_sampling with mask / x0) ------------------
 * The blend: out = (sqrt_a x0 + sqrt_1ma z) m + (1 - m) x over [B,C,H,W] in fp32, every operation rounded on its own (no FMA), in
 * the order written: where m = 1 the result is fp32(sqrt_a x0 + sqrt_1ma z) and where m = 0 it is x, bit for bit.  x0 [dev] f32
 * [B,C,H,W] is the known latent; mask [dev] f32 [B,mask_channels,H,W] holds m in [0, 1], 1 = KEEP THE KNOWN LATENT (ldm's convention),
 * with mask_channels = 1 (one plane for every channel) or C.
 *
 * rdm_op_masked_blend: the kernel alone on caller-owned buffers; z (rdm_noise): the stack is [dev] f32 [B,C,H,W]; no noise source reads z
 * as zeros (the last blend of a keep-the-known-region call, at sqrt_a = 1, sqrt_1ma = 0).  out may be x; x_dup (or NULL) receives the same
 * values.  float4 accesses when B*C*H*W % 4 == 0, H*W % 4 == 0 and every operand is 16-byte aligned, else scalar ones.
 * Seeded, z is drawn on STREAM 0 at z->step (per_row is C*H*W, the field is not read) -- bit-identical to the stack form fed with
 * rdm_op_randn(seed, row0, B, C*H*W, step, stream = 0).  The loops use step = i + 1 for loop step i (step 0 is the starting latent).
 * C*H*W % 4 == 0 and 16-byte aligned x, x0, out, x_dup are then required (-1 otherwise); the mask may have any alignment, and when
 * H*W % 4 != 0 -- a block then straddles channel planes -- it is indexed per element.
 *
 * rdm_ddim_inpaint: rdm_ddim_decode's loop (same arguments, scalars, intermediates) with the blend before every forward: loop step
 * i = 0 .. t_start - 1 works at level index = t_start - 1 - i and first replaces the iterate by the blend at that level,
 * sqrt_a = sqrt(a_t[index]), sqrt_1ma = sqrt(1 - a_t[index]) in float64 from the fp32 alpha, rounded, z = q_noise[i]; then the UNet
 * forward, then rdm_ddim_decode's step.  The result of the last step is not blended, as in ldm's loop.  q_noise [dev] f32
 * [t_start,B,C,H,W], consumed in loop order: required unless noise is seeded, and then it must be NULL; noise as rdm_ddim_decode's.  A
 * seeded call takes neither stack: the update noise of loop step i is (seed, stream 1, step i), the known region's (seed, stream 0,
 * step i + 1), both for rows row0 + b, and the loop is bit-identical to the stack loop fed with rdm_op_randn's outputs.  It needs
 * channels * height * width % 4 == 0 and a 16-byte aligned x0.
 *
 * Both return -1 with a message, and leave the context usable, for a null x, x0, mask (or q_noise in the stack loop), a q_noise beside a
 * seed, a mask_channels that is neither 1 nor C, a t_start outside [1, total], and what rdm_ddim_decode refuses. */
int rdm_op_masked_blend(rdm_ctx* ctx, const float* x, const float* x0, const float* mask, const rdm_noise* z, int64_t B, int C, int H,
                        int W, int mask_channels, float sqrt_a, float sqrt_1ma, float* out, float* x_dup_or_null);
int rdm_ddim_inpaint(rdm_ctx* ctx, const rdm_ddim_args* args, int t_start, const float* x_latent, const float* x0, const float* mask,
                     int mask_channels, const float* cond, const float* uncond, const rdm_noise* noise, const float* q_noise, float* z_out,
                     float* x_inter, float* pred_x0_inter);
/* One guided UNet forward exactly as the sampling loops run it (rdm_unet_forward on [x | x], [cond | uncond] computes the same function
 * through other kernel configurations: every sample's own prefix, no zero-context shortcut, the time embedding per row): x [dev] f32
 * [B,Cin,H,W] at the one timestep t; cond, uncond [dev] f32 [B,k,ctx_dim]; eps_out [dev] f32 [2B,Cout,H,W], rows cond | uncond.  What a
 * caller's own loop uses when its iterates must be the native loop's -- the per-step path of DDIMSampler.encode: a step up the schedule
 * carries a difference in eps on undamped. */
int rdm_unet_forward_guided(rdm_ctx* ctx, const float* x, int64_t t, const float* cond, const float* uncond, int B, int k, int H, int W,
                            float* eps_out);

/* ---- first stage: LatentDiffusion.decode_first_stage -> VQModelInterface.decode
 *      (called at rdm/models/diffusion/ddpm.py:840, 981). z [dev] f32 [b,3,h,w] -> img [dev] f32 [b,3,H,W];
 * indices_out [dev] int32 [b*h*w] or NULL. */
int rdm_vq_decode(rdm_ctx* ctx, const float* z, int b, int force_not_quantize, float* img_out, int32_t* indices_out);
/* first_stage_model.quantize(z) (taming VectorQuantizer2.forward: nearest codebook entry, first minimum on ties, straight-through form
 * z + (e - z)) WITHOUT post_quant_conv -- what DDIMSampler.p_sample_ddim applies to pred_x0 under quantize_x0 = True
 * (rdm/models/diffusion/ddim.py:260-261).  z [dev] f32 [b,3,h,w] -> zq_out [dev] f32 [b,3,h,w]; indices_out [dev] int32 [b*h*w] or NULL. */
int rdm_vq_quantize(rdm_ctx* ctx, const float* z, int b, float* zq_out, int32_t* indices_out);
/* taming Net2NetTransformer.decode_to_img (reached from rdm/models/autoregression/transformer.py:296-312): code indices
 * [dev] int64 [b, h*w] -> quantize.get_codebook_entry -> post_quant_conv -> Decoder -> img_out [dev] f32 [b,3,R,R].
 * For first stages with a wide latent (VQGAN-f16, z_channels % 64 == 0). */
int rdm_vq_decode_indices(rdm_ctx* ctx, const int64_t* indices, int b, float* img_out);
/* The first stage at any size (ldm's "convolutional sampling": decode_first_stage / VQModelInterface.decode on a conv-only autoencoder,
 * rdm/models/diffusion/ddpm.py:840 behind sample_log(custom_shape=) at ddpm.py:988-1011).  rdm_vq_decode and rdm_vq_quantize above are
 * these two at the cfg's own latent size h = w = resolution / f, f = 2^(levels - 1).
 *   rdm_vq_decode_hw:   z [dev] f32 [b,z_channels,h,w] -> img_out [dev] f32 [b,out_ch,f*h,f*w]; indices_out [dev] int32 [b,h*w] or NULL
 *   rdm_vq_quantize_hw: z [dev] f32 [b,3,h,w] -> zq_out [dev] f32 [b,3,h,w]; indices_out as above
 * Any h, w >= 1.  What runs where: 3x3 convs of levels whose width is at most 64 with 256 % width == 0, or a multiple of 64 with
 * height % 4 == 0, on the halo kernels, every other width on the generic implicit GEMM; an AttnBlock over at most 4096 pixels materialises
 * its n x n scores (n = h*w, padded to a multiple of 64; a batch is walked in ranges of at most 8 GiB of them), beyond that it streams them
 * (rdm_op_vq_attention; widths that are multiples of 128 up to 512 -- any other width keeps materialising, up to 46336 pixels).  A latent
 * whose largest activation passes 2^30 elements per sample is refused (-1); work buffers that cannot be allocated: -2.  Not for wide
 * latents (VQGAN-f16: its 256-token sequence fixes its size) -- rdm_vq_decode_indices / rdm_vq_encode_indices stay square. */
int rdm_vq_decode_hw(rdm_ctx* ctx, const float* z, int b, int h, int w, int force_not_quantize, float* img_out, int32_t* indices_out);
int rdm_vq_quantize_hw(rdm_ctx* ctx, const float* z, int b, int h, int w, float* zq_out, int32_t* indices_out);
/* ---- first stage, encoder side (training input): LatentDiffusion.encode_first_stage -> VQModelInterface.encode = quant_conv(encoder(x))
 *      under torch.no_grad(), reached from MinimalRETRODiffusion.shared_step -> get_input (rdm/models/diffusion/ddpm.py:390-391).
 * Same rdm_vq_cfg as the decoder (the encoder mirrors it: ddconfig is shared); state_dict keys `encoder.*`, `quant_conv.*`.
 * img [dev] f32 [b,out_ch,R,R] -> z_out [dev] f32 [b,embed_dim,R/f,R/f] (no quantisation: VQModelInterface quantises in decode). */
long long rdm_vqenc_manifest(const rdm_vq_cfg* cfg, char* buf, size_t buflen, size_t* blob_bytes);
int rdm_load_vqenc(rdm_ctx* ctx, const rdm_vq_cfg* cfg, const void* packed, size_t nbytes);
int rdm_vq_encode(rdm_ctx* ctx, const float* img, int b, float* z_out);
/* Wide latents (taming VQGAN-f16: embed_dim % 64 == 0 && z_channels % 64 == 0, the condition under which rdm_load_vq takes a wide
 * decoder) are accepted by the three entries above as well; rdm_vq_encode then returns z_out [b,embed_dim,h,w] = quant_conv(encoder(x)).
 *
 * rdm_vq_encode_indices: taming VQModel.encode as reached from Net2NetTransformer.encode_to_z (un-vendored, parity unpinned):
 *   quant_z, _, info = first_stage_model.encode(x); indices = info[2].view(b, -1)
 * i.e. the nearest codebook row (first minimum on ties) of every latent token; the image-completion path of LatentImageRETRO.log_images
 * (rdm/models/autoregression/transformer.py:448, :457-462).  Needs rdm_load_vqenc AND rdm_load_vq (the codebook is the decoder blob's
 * quantize.embedding.weight) with the same wide cfg.  Batches beyond the first stage's activation range are walked in ranges. */
int rdm_vq_encode_indices(rdm_ctx* ctx, const float* img /*[dev] f32 [b,out_ch,R,R]*/, int b, int64_t* indices_out /*[dev] [b, h*w]*/,
                          float* quant_out_or_null /*[dev] f32 [b,embed_dim,h,w] = codebook rows*/);
/* VQModelInterface.encode at any image size: img [dev] f32 [b,out_ch,H,W], H and W positive multiples of f -> z_out [dev] f32
 * [b,embed_dim,H/f,W/f].  rdm_vq_encode is this at H = W = resolution.  VQ-f4 (3-channel latent) only. */
int rdm_vq_encode_hw(rdm_ctx* ctx, const float* img, int b, int H, int W, float* z_out);
/* scripts/rdm_sample.py:203-214 custom_to_np/custom_to_pil: f32 NCHW [-1,1] -> uint8 NHWC (truncating). */
int rdm_to_uint8(rdm_ctx* ctx, const float* img, int b, int c, int h, int w, uint8_t* out);

/* ---- RARM: RetrievalPatchTransformer.forward(x, context) (rdm/modules/attention.py:199-272) and LatentImageRETRO.sample
 *      (rdm/models/autoregression/transformer.py:224-294).  Both run token by token against a per-layer K/V cache (the
 *      reference re-runs the whole prefix for every new token, :241-248).
 * forward: tokens [dev] int64 [b,t]; context [dev] f32 [b,k,context_dim]; logits_out [dev] f32 [b,t,vocab_out].
 * sample : cond_tokens [dev] int64 [b,cond_len]; context as above; uniforms [dev] f32 [steps,b] in [0,1) — the multinomial draw
 *          of step s for sequence i is the inverse CDF (vocabulary order) at uniforms[s,i]; tokens_out [dev] int64 [b,steps]. */
int rdm_rarm_forward(rdm_ctx* ctx, const int64_t* tokens, int b, int t, const float* context, int k, float* logits_out);
int rdm_rarm_sample(rdm_ctx* ctx, const rdm_rarm_sample_args* args, const int64_t* cond_tokens, const float* context,
                    const float* uniforms, int64_t* tokens_out);
/* rdm_rarm_sample with the nucleus (top-p) filter that `sample`, `sampling_util` and `log_images` name as `top_p` and the reference
 * refuses (rdm/models/autoregression/transformer.py:279-280 `assert top_p==1., 'not yet implemented'`, :427, :454-472).  top_p in
 * (0, 1], anything else (NaN included) is an argument error; 1 is rdm_rarm_sample itself.  Below 1, per sequence and step, AFTER the
 * top-k rule (survivors K, ties with the k-th kept): p_i = softmax over K; the nucleus is { i in K : g_i >= theta } for the LARGEST
 * logit value theta present in K whose mass M(theta) = sum of p_i over g_i >= theta reaches top_p -- the smallest descending prefix
 * that reaches top_p, the crossing token kept, every token tied with the last kept one kept too.  The draw is unchanged. */
int rdm_rarm_sample_top_p(rdm_ctx* ctx, const rdm_rarm_sample_args* args, float top_p, const int64_t* cond_tokens, const float* context,
                          const float* uniforms, int64_t* tokens_out);
/* ---- RARM over whole sequences: one transformer pass over all t positions (causal self-attention at d_head 64 on the MFMA units,
 *      csrc/attention.hip: causal_d64_kernel) instead of t decode steps.  Sequences are walked in ranges of at most 32 768 rows
 *      (RARM_SEQ_ROWS, csrc/rarm_exec.hip), so the scratch does not grow with b * t.  At most 128 neighbours per sequence (k <= 128).
 * rdm_rarm_forward_seq: RetrievalPatchTransformer.forward(x, context) (rdm/modules/attention.py:252-272): the contract of
 *      rdm_rarm_forward -- tokens [dev] int64 [b,t], context [dev] f32 [b,k,context_dim], logits_out [dev] f32 [b,t,vocab_out]. */
int rdm_rarm_forward_seq(rdm_ctx* ctx, const int64_t* tokens, int b, int t, const float* context, int k, float* logits_out);
/* LatentImageRETRO.forward + compute_loss without the mean (rdm/models/autoregression/transformer.py:62-70, 213-222):
 *      nll_out[i,j] = -log softmax(logits[i,j,:])[targets[i,j]], F.cross_entropy(reduction='none').  tokens, targets [dev] int64 [b,t],
 *      targets in [0, vocab_out) (outside: NaN); nll_out [dev] f32 [b,t].  The head GEMM runs in row pieces into bounded scratch:
 *      [b*t, vocab_out] logits are never formed. */
int rdm_rarm_nll(rdm_ctx* ctx, const int64_t* tokens, const int64_t* targets, int b, int t, const float* context, int k, float* nll_out);
/* rdm_rarm_sample_top_p (top_p = 1: rdm_rarm_sample) whose conditioning prefix -- `c_indices` and the kept codes of an image completion,
 *      transformer.py:232-248 -- is fed in ONE whole-sequence pass over positions 0 .. cond_len-2 that fills the decode step's K/V cache;
 *      the token-by-token loop then starts at position cond_len-1.  cond_len == 1: nothing to prefill, the very launches of rdm_rarm_sample. */
int rdm_rarm_sample_prefill(rdm_ctx* ctx, const rdm_rarm_sample_args* args, float top_p, const int64_t* cond_tokens, const float* context,
                            const float* uniforms, int64_t* tokens_out);

/* ---- CLIP: CLIP.encode_text / encode_image (rdm/modules/custom_clip/model.py:304-320), used by
 *      ClipImageRetriever / CLIPTextEmbedder (rdm/modules/retrievers.py:67-117).
 * tokens [dev] int64 [b,context_length]; image [dev] f32 [b,3,R,R] already CLIP-normalised; out [dev] f32 [b,embed]. */
int rdm_clip_encode_text(rdm_ctx* ctx, const int64_t* tokens, int b, float* out);
int rdm_clip_encode_image(rdm_ctx* ctx, const float* image, int b, float* out);
/* ClipImageRetriever.preprocess (rdm/modules/retrievers.py:83-91): kornia bicubic resize (align_corners=True, no antialias)
 * of image [dev] f32 [b,3,h,w] in [-1,1] to the tower resolution R, then (x+1)/2 and the CLIP mean/std -> out [dev] f32 [b,3,R,R]. */
int rdm_clip_preprocess(rdm_ctx* ctx, const float* image, int b, int h, int w, float* out);
/* ClipImageRetriever.forward (retrievers.py:93-95) = encode_image(preprocess(x)) with the preprocessing fused into the
 * patch-embedding gather (the resized image is never materialised): image [dev] f32 [b,3,h,w] in [-1,1] -> out [dev] f32 [b,embed]. */
int rdm_clip_encode_image_raw(rdm_ctx* ctx, const float* image, int b, int h, int w, float* out);

/* ---- retrieval: DatasetBuilder.train_searcher + searcher.search_batched
 *      (rdm/data/retrieval_dataset/dsetbuilder.py:534-619, 490; call sites ddpm.py:298,734,906).
 * rdm_db_load: emb [host or dev] fp16 or fp32 [n,dim] raw embeddings; the searcher's dataset is
 *   fp16(x/||x||) held in HBM (dsetbuilder.py:574).  dtype: 0 = fp16, 1 = fp32. is_device: 1 if emb is [dev].
 * rdm_knn: q [dev] f32 [b,dim] raw queries (normalised internally, dsetbuilder.py:487);
 *   idx_out [dev] uint32 [b,k] by descending score, ties -> lower index; score_out [dev] f32 [b,k] (or NULL). */
int rdm_db_load(rdm_ctx* ctx, const void* emb, long long n, int dim, int dtype, int is_device);
long long rdm_db_size(rdm_ctx* ctx);
int rdm_knn(rdm_ctx* ctx, const float* q, int b, int k, uint32_t* idx_out, float* score_out);
/* The same search with the scores as the fp64 values the ranking was made on (score_out [dev] f64 [b,k]).  For a database whose ROWS are
 * sharded over GPUs ("when memory matters"): every rank searches its rows, the per-rank lists are exchanged (one
 * all-gather of [b,k] (index, score) pairs) and merged under the same total order (score desc, global index asc) -- on the fp32
 * scores two rows whose fp64 scores differ could tie and swap. */
int rdm_knn_f64(rdm_ctx* ctx, const float* q, int b, int k, uint32_t* idx_out, double* score_out);
/* 1 if the last rdm_knn could not certify its MFMA-scored candidate set for some query (a cluster of near-duplicates within the
 * score error bound around the k-th neighbour) and answered it by the exact fp64 pass instead; 0 otherwise.  Diagnostic only:
 * the result is exact either way. */
int rdm_knn_last_fallback(rdm_ctx* ctx);
/* data_pool['embedding'][nns] gather (dsetbuilder.py:493): idx [dev] uint32 [n_idx] -> out [dev] f32 [n_idx,dim]
 * of the RAW (un-normalised) embeddings (rdm_db_load keeps a raw copy in HBM next to the normalised one). */
int rdm_db_gather(rdm_ctx* ctx, const uint32_t* idx, long long n_idx, float* out);
/* Read-outs of the search for the tests (tests/test_knn_cpu.py, tests/test_gpu_knn_stages.py).
 * rdm_knn_select: what rdm_knn does for a database of n rows x dim, b queries and k neighbours; host only, no device.  path: which scan
 *   scores the database -- GENERIC (any dim, both fp16 words of the query), D512 (dim 512, hi word only) or BULK (b >= 128 and at
 *   least 16 tiles of 256 rows: 128-query walkers, hi word only).  ksel: entries per lane list; rescored: merged candidates re-scored
 *   exactly (>= k); lists_per_block: lists per query a scan block (BULK: a walker) writes; queries_per_launch: 64, BULK 512;
 *   eps: the bound on |approximate - exact| score the certificate runs with, a function of path and dim (csrc/knn.hip).
 *   Returns -1 for arguments rdm_db_load / rdm_knn refuse.  The search takes path and eps from this very function.
 * rdm_op_knn_stages: rdm_knn for ONE query group (b <= 64, or a BULK launch of 128 <= b <= 512) through the same launches, copying
 *   out every stage.  The caller sets the capacities and the [dev] pointers (any may be NULL); rows = query rows prepared (64, BULK
 *   128 per group), nlists = lists per query.  qn f32 / qh, ql fp16 [rows, dim] (rows b.. are padding); cand_s f32 / cand_i uint32
 *   [rows, nlists, ksel], each list by (score desc, index asc), empty slots (-inf, 0xffffffff); per query [b] the merge's verdict
 *   BEFORE the exact fallback: flag (1 = not certified), tau / tau_idx (k-th exact score and its row among the re-scored
 *   candidates), theta (largest approximate score of anything dropped); certified iff theta + eps < tau.
 * rdm_db_rows: the normalised database rows [row0, row0 + rows) as fp16 [rows, dim] into out [dev]. */
enum { RDM_KNN_SCAN_GENERIC = 1, RDM_KNN_SCAN_D512 = 2, RDM_KNN_SCAN_BULK = 3 };
typedef struct rdm_knn_form { int path, ksel, rescored, lists_per_block, queries_per_launch; float eps; } rdm_knn_form;
typedef struct rdm_knn_stages {
    int rows_cap, nlists_cap;                       /* in: query rows / lists per query the arrays below hold */
    float* qn; void* qh; void* ql;
    float* cand_s; uint32_t* cand_i;
    int* flag; double* tau; uint32_t* tau_idx; float* theta;
    int rows, nlists; rdm_knn_form form;            /* out */
} rdm_knn_stages;
int rdm_knn_select(long long n, int dim, int b, int k, rdm_knn_form* form_out);
int rdm_op_knn_stages(rdm_ctx* ctx, const float* q, int b, int k, uint32_t* idx_out, float* score_out, rdm_knn_stages* stages);
int rdm_db_rows(rdm_ctx* ctx, long long row0, long long rows, void* out_f16);
/* ---- filtered retrieval: the exact top-k over the rows a per-query bitmap allows (conditioning on a class, a style subset, a held-out
 *      split, a deny list) in ONE pass over the resident database, whatever the number of different masks in the batch.
 * A mask is rdm_knn_mask_words(n) 64-bit words (n rounded up to the scans' 256-row tile, / 64; host only): bit r % 64 of word r / 64 set
 *   = row r may be returned.  Bits at or beyond n are ignored (all-ones words are fine).
 * rdm_knn_filtered: rdm_knn with allow [dev] uint64 [n_masks, words] and mask_of_query [host] int32 [b] (NULL: every query uses mask
 *   0).  Same order and scores as rdm_knn, over the allowed rows only: disallowed rows enter no candidate list and are skipped by the
 *   exact fallback, so the exactness certificate holds unchanged for the subset.  A query whose mask allows fewer than k rows gets
 *   those rows followed by (0xffffffff, -inf) entries, and the call succeeds.  Refused: allow == NULL, n_masks < 1, a mask_of_query
 *   entry outside [0, n_masks) (the message names the query), zero-norm queries as in rdm_knn.  rdm_knn_last_fallback reports on it.
 *   The filter is an argument of the call: nothing of it stays on the context.
 * rdm_knn_filtered_f64: the same with the fp64 scores (rdm_knn_f64; shard merges).
 * rdm_op_knn_stages_filtered: rdm_op_knn_stages through the launches of rdm_knn_filtered.
 * rdm_op_row_mask: one mask from rows [dev] int64 [n_rows] (duplicates allowed; invert = 1: the complement within [0, n)) into
 *   bits_out [dev] uint64 [words]; an index outside [0, n) is an error (found by the kernel, reported after it).
 * rdm_op_row_mask_count: counts_out [host] [n_masks] = allowed rows below n of each mask of allow [dev] [n_masks, words]. */
int rdm_knn_mask_words(long long n);
int rdm_knn_filtered(rdm_ctx* ctx, const float* q, int b, int k, const uint64_t* allow, int n_masks, const int32_t* mask_of_query,
                     uint32_t* idx_out, float* score_out);
int rdm_knn_filtered_f64(rdm_ctx* ctx, const float* q, int b, int k, const uint64_t* allow, int n_masks, const int32_t* mask_of_query,
                         uint32_t* idx_out, double* score_out);
int rdm_op_knn_stages_filtered(rdm_ctx* ctx, const float* q, int b, int k, const uint64_t* allow, int n_masks, const int32_t* mask_of_query,
                               uint32_t* idx_out, float* score_out, rdm_knn_stages* stages);
int rdm_op_row_mask(rdm_ctx* ctx, const int64_t* rows, long long n_rows, long long n, int invert, uint64_t* bits_out);
int rdm_op_row_mask_count(rdm_ctx* ctx, const uint64_t* allow, int n_masks, long long n, long long* counts_out);

/* ---- multi-GPU: one process and one context per device; the path has ONE exchange, an all-gather -- of the
 * decoded images (replicated database) or of the per-shard (index, score) top-k pairs (row-sharded database).  Thin wrappers
 * around RCCL (loaded with dlopen at rdm_comm_init: single-GPU users never touch it) for callers that bind the C ABI directly;
 * the Python mirror reaches the same RCCL through torch.distributed (rdm_amd/parallel.py).  The reference has no multi-GPU
 * sampling (scripts/rdm_sample.py is single-process); the reference-side analogue is DDP's process group in main.py:783-785.
 *   rdm_comm_unique_id: rank 0 fills a 128-byte id and hands it to the other ranks by any out-of-band means.
 *   rdm_comm_init:      every rank, same id; binds the communicator to the context's device and stream.
 *   rdm_comm_all_gather: recv[dev] (world * nbytes) <- send[dev] (nbytes) of every rank, in rank order; enqueued on the stream. */
int rdm_comm_unique_id(rdm_ctx* ctx, void* id128 /*[host] 128 bytes*/);
int rdm_comm_init(rdm_ctx* ctx, const void* id128 /*[host]*/, int rank, int world);
int rdm_comm_all_gather(rdm_ctx* ctx, const void* send /*[dev]*/, void* recv /*[dev]*/, size_t nbytes);
/* gradient all-reduce of data-parallel training (the reference: DDP inside pytorch_lightning's Trainer, main.py:783-785): buf [dev] f32
 * [count] <- sum over ranks (average != 0: divided by the world size), in place, enqueued on the stream. */
int rdm_comm_all_reduce_f32(rdm_ctx* ctx, float* buf /*[dev]*/, size_t count, int average);
int rdm_comm_destroy(rdm_ctx* ctx);

/* ---- measurement: optional HIP-event brackets around launches on the context stream, by kernel class.
 * enable: bit mask of (1 << RDM_PROF_*) kinds to record (0 = off).  collect: sums elapsed ms and ALGORITHMIC work of the
 * launches of one kind recorded since the last reset -- FLOPs (2*M*N*K; 4*n^2*d per attention head) for the MFMA-bound
 * kinds, bytes (minimal tensor / database passes) for the HBM-bound kinds.  Used by bench.py for the roofline objects. */
enum { RDM_PROF_CONV3X3 = 0, RDM_PROF_LINEAR = 1, RDM_PROF_KNN = 2, RDM_PROF_ATTENTION = 3, RDM_PROF_GROUPNORM = 4,
       RDM_PROF_LAYERNORM = 5,
       RDM_PROF_UPSCONV = 6 /* Upsample's nearest-2x + conv3x3 run by output phase (2 x 2 taps at source resolution): EXECUTED FLOPs, 4/9 of the nine-tap count */ };
int rdm_prof_enable(rdm_ctx* ctx, int kind_mask);
int rdm_prof_collect(rdm_ctx* ctx, int kind, long long* launches, double* ms, double* flops);
int rdm_prof_reset(rdm_ctx* ctx);
/* one CSV row per recorded launch since the last reset: kind, the op's role in the executor's graph ("st.proj_in", "res.conv1", ...; the
 * reference modules behind the roles: rdm/modules/attention.py:122-196, ldm ResBlock), its shape (M, N, K | rows, channels | B, n, C),
 * elapsed ms and algorithmic work -- the per-op table behind DESIGN.md's level-by-level costs (tools/op_trace.py). */
int rdm_prof_dump(rdm_ctx* ctx, const char* path);
/* Box calibration for bench.py's `calibration` object (no reference counterpart: the reference has no benchmark harness; the
 * boxes of the MI355X pool differ by +-4..5 % in sustained clock under the package power cap and the headline moves with them).  Two FIXED
 * instruction streams that do not change when a product kernel does: (1) back-to-back v_mfma_f32_32x32x16_bf16 on random bf16 operands, one wave
 * per SIMD on every CU, for ~mfma_ms of wall time -> sustained dense-bf16 TFLOP/s under this box's power cap; (2) stream_reps 16-byte-per-lane
 * copies of stream_bytes -> HBM read + write GB/s.  buf [dev]: scratch of at least max(1 MiB, 2 * stream_bytes) bytes; either result
 * pointer may be null (probe skipped).  Synchronous on the context's stream. */
int rdm_calib_probe(rdm_ctx* ctx, void* buf /*[dev]*/, size_t buf_bytes, double mfma_ms, size_t stream_bytes, int stream_reps,
                    double* mfma_tflops /*[host]*/, double* stream_gbps /*[host]*/);
/* test hook: the next UNet forwards copy ONE intermediate activation (bf16, row-major [rows, width] as the executor holds it: NHWC) into
 * buf [dev] (at most nbytes).  block: index into the top-level block table (state-dict order: input_blocks.0 .., middle_block,
 * output_blocks.0 ..; openaimodel.py:355-368's loop).  sub = 0: the block's output; sub = 16 * (layer inside the block) + stage:
 *   ResBlock stages 1 in_layers norm+SiLU, 2 in_layers conv + emb, 3 out_layers norm+SiLU, 4 skip_connection, 5 output;
 *   SpatialTransformer stages 1 norm, 2 proj_in, 3 norm1, 4 q|k|v, 5 attn1 heads, 6 x + attn1, 7 x + attn2, 8 norm3, 9 GEGLU, 10 output
 *   (rdm/modules/attention.py:92-96, 170-196).  buf null: off.  tests/test_gpu_emul.py compares the library with the CPU restatement of its
 * arithmetic stage by stage, TEACHER-FORCED, through this.
 * The CLIP towers (rdm_clip_encode_text: block 2000; rdm_clip_encode_image[_raw]: block 3000) show their tensors the same way, each copied
 * as it is stored (fp32 or bf16, row-major); sub = 16 * layer + stage with layer 0 the tower's own stages and layer i + 1 resblock i
 * (B sequences of L = context_length tokens / G^2 + 1 patch tokens, width W, patch size P, embedding E):
 *   text, layer 0:   1 token + positional embedding f32 [B L, W], 2 the EOT rows (first maximum of the ids) f32 [B, W], 3 ln_final of
 *                    them bf16 [B, W], 4 the projected embedding f32 [B, E];
 *   image, layer 0:  1 patch matrix bf16 [B G^2, 3 P^2] (columns in (c, py, px) order), 2 patch embeddings f32 [B G^2, W], 3 cls | patches +
 *                    positional f32 [B (G^2 + 1), W], 4 ln_pre f32, 5 the cls rows after the last resblock f32 [B, W], 6 ln_post bf16
 *                    [B, W], 7 the projected embedding f32 [B, E];
 *   resblock:        1 ln_1 bf16 [rows, W], 2 q|k|v bf16 [rows, 3 W], 3 attention heads bf16 [rows, W], 4 x + out_proj f32 [rows, W],
 *                    5 ln_2 bf16, 6 QuickGELU hidden bf16 [rows, 4 W], 7 x + c_proj f32 (the block's output).
 * tests/test_gpu_clip.py holds every one of them to an fp64 restatement on the library's own inputs.
 * The first stage shows its layer outputs as bf16 NHWC tokens [B, H W, C], copied as stored and clipped to nbytes, sub = 0, numbered in
 * execution order.  Decoder (rdm_vq_decode*): block 1000 = conv_in's output, then mid.block_1, mid.attn_1, mid.block_2, then per level
 * (coarse to fine) each ResnetBlock, each AttnBlock where the level has one, and the Upsample conv's output.  Encoder (rdm_vq_encode*):
 * block 1500 = conv_in's output, then per level (fine to coarse) each ResnetBlock, each AttnBlock where the level has one, and the
 * Downsample conv's output, then mid.block_1, mid.attn_1, mid.block_2; a wide latent (VQGAN-f16) adds norm_out + swish and conv_out.
 * A decoder number never fires during an encode, nor an encoder number during a decode.  tests/test_gpu_emul.py and
 * tests/test_gpu_vq_encoder.py compare each layer teacher-forced with oracle/vq_emul.py.
 * The RARM transformer shows its executors the same way (each tensor copied as it is stored, row-major; sub = 16 * layer + stage, layer 0
 * the executor's own stages, layer i + 1 transformer block i; B sequences with k neighbours, B2 = 2 B rows in a guided sampling call,
 * else B; C = n_heads * d_head, V = vocab_out):
 *   block 4000, the per-call preparation (every rdm_rarm_* entry):
 *     layer 0:       1 the neighbours cast to bf16 [B k, context_dim], 2 the neighbours' keys | values of all layers, bf16
 *                    [B2 k, depth * 2 C] (layer l's keys at column 2 l C, its values at 2 l C + C; the unconditional rows zero);
 *     layer l + 1:   1 G_l = expand_heads(K_l) / sqrt(d_head) . W_q, 2 UT_l = W_o . expand_heads(V_l), each bf16 [B, 128, C] -- only in a
 *                    call whose decode steps take the one-launch cross-attention (n_heads * k <= 128, and B2 < 384 or deterministic mode);
 *   block 4100, the decode step (rdm_rarm_forward, the rdm_rarm_sample* loops), rows = B2:
 *     layer 0:       1 token + positional embedding f32 [rows, C], 2 the final x cast to bf16 [rows, C], 3 the logits f32 [rows, V];
 *     block:         1 norm1 bf16 [rows, C], 2 q|k|v bf16 [rows, 3 C], 3 self-attention heads bf16 [rows, C], 4 x + attn1.to_out f32,
 *                    5 norm2 bf16, 6 attn2.to_q bf16, 7 cross-attention heads bf16, 8 x + attn2 f32, 9 norm3 bf16, 10 GEGLU hidden bf16
 *                    [rows, 4 C], 11 x + ff.net.2 f32 (the block's output).
 *     A stage the chosen form does not hold in memory does not fire: 1, 5 and 9 exist only where the LayerNorm runs as a pass of its own
 *     (not formed inside the skinny GEMM: more than 192 rows outside deterministic mode, or a shape the in-kernel form declines); in the
 *     one-launch cross-attention 5, 6 and 7 do not exist and 9 is the norm3 the kernel emits.  One entry runs many steps: step s, counted
 *     over the decode steps of that entry, lands at byte offset s * (stage bytes), clipped to nbytes, so that one rdm_rarm_forward over t
 *     positions (or one sampling call) shows a stage at every position: [steps, rows, width].
 *   block 4200, the whole-sequence pass (rdm_rarm_forward_seq, rdm_rarm_nll, the prefix of rdm_rarm_sample_prefill), rows = B2 t, sequence
 *     major: the decode step's layer and stage numbers, all eleven block stages always; layer 0 stages 2 and 3 where the call has a head
 *     (3: rdm_rarm_forward_seq only).  Each range of sequences the pass walks lands at its own row offset, clipped.
 * A 4100 number never fires in the whole-sequence pass, nor a 4200 number in a decode step.  tests/test_gpu_rarm_stages.py holds every
 * stage to a float64 restatement of that stage on the library's own tapped inputs (tests/_rarm_stage_ref.py). */
int rdm_debug_tap(rdm_ctx* ctx, void* buf /*[dev]*/, size_t nbytes, int block, int sub);
/* test hook: where the SHARED GUIDANCE PREFIX of a guided sampler forward ends.  With classifier-free guidance the UNet batch is
 * [x | x] with contexts [cond | uncond] (ddim.py:229-234), and everything in front of the first cross-attention computes the same values
 * for both halves, so it runs once on the first half.  through_attn1 = 1 (the default): the prefix covers the layers in front of the
 * first SpatialTransformer AND that transformer's norm, proj_in, norm1, q|k|v projection and self-attention; it ends at attn1.to_out,
 * which reads its operand and residual with a row wrap (or from duplicated copies where the wrapped GEMM form does not take the shape).
 * 0: the prefix ends in front of that transformer.  Both give bit-identical results (every row's arithmetic is the same; the shared
 * stages choose their kernels as for the whole batch): tests/test_gpu_guided_prefix.py compares them inside one process.  rdm_debug_tap
 * shows a stage that ran on the first half as the logical tensor, the second half a copy of the first.  Deterministic mode always ends
 * the prefix in front of the transformer.  Not an environment switch, and not meant for production use. */
int rdm_debug_guidance_prefix(rdm_ctx* ctx, int through_attn1);

/* ---- operator-level entry points (used by the parity tests; thin wrappers over the kernels) ---- */
int rdm_op_linear(rdm_ctx* ctx, const void* a_bf16, const void* w_bf16, const float* bias, const void* residual_bf16,
                  void* out_bf16, float* out_f32, int M, int N, int K, int act, float alpha);
/* out[m] = a[m] W^T + bias + rowvec[m / rows_per_group] (+ residual[m]): nn.Linear with a per-row-group additive vector (rowvec f32
 * [ceil(M / rows_per_group), N]).  The executor uses it for attn1.to_out over a guided batch [conditional | unconditional]
 * (rdm/modules/attention.py:237-238 with ddim.py:229-234's batch): the unconditional rows' cross-attention is exactly attn2.to_out's
 * bias, which rides in the projection's start values for those rows (two groups; any group count on the generic GEMM). */
int rdm_op_linear_rowvec(rdm_ctx* ctx, const void* a_bf16, const void* w_bf16, const float* bias, const float* rowvec, int rows_per_group,
                         const void* residual_bf16, void* out_bf16, int M, int N, int K);
/* out = act(LayerNorm(x; gamma, beta, eps) W^T + bias) in ONE kernel: nn.LayerNorm followed by nn.Linear as in BasicTransformerBlock
 * (rdm/modules/attention.py:147-168: `self.attn1(self.norm1(x))`, `self.ff(self.norm3(x))`), the LayerNorm folded into the GEMM
 * (lin4.hip).  x bf16 [M, K] RAW rows, w bf16 [N, K] (GEGLU: rows in the packed [32 x | 32 gates] order), out bf16 [M, N] (GEGLU: [M, N/2]).
 * Returns -5 when the shape is not one the folded kernel takes (the executors then run LayerNorm + Linear). */
int rdm_op_linear_ln(rdm_ctx* ctx, const void* x_bf16, const void* w_bf16, const float* bias, const float* gamma, const float* beta,
                     void* out_bf16, int M, int N, int K, int act, float eps);
int rdm_op_conv3x3(rdm_ctx* ctx, const void* x0_bf16, const void* x1_bf16, int C0, int C1, const void* w_bf16,
                   const float* bias, const float* rowvec, int rowvec_ld, const void* residual_bf16, void* out_bf16,
                   int B, int Hin, int Win, int N, int stride, int ups);
/* The first-stage encoder's Downsample conv alone ([ldm] Downsample(with_conv): F.pad(x, (0, 1, 0, 1)) then Conv2d(kernel 3, stride 2,
 * padding 0)), exactly the call the encoder makes: the 3x3 window of output (oy, ox) starts AT input (2 oy, 2 ox), zero beyond the last
 * row and column.  x bf16 NHWC [B, Hin, Win, C], w bf16 [N][3][3][C], bias f32 [N] or null, out bf16 [B, Hin / 2, Win / 2, N].  C % 64 == 0
 * and N even; odd Hin or Win are an argument error and no launch (the context stays usable). */
int rdm_op_conv3x3_down(rdm_ctx* ctx, const void* x_bf16, int C, const void* w_bf16, const float* bias, void* out_bf16, int B, int Hin, int Win,
                        int N);
/* the nearest-code kernel of rdm_vq_encode_indices alone, on caller-given operands: idx_out[m] = argmin_j |e_j|^2 - 2 z_m . e_j, evaluated
 * in fp32 on fp32-input MFMAs, first minimum on ties (taming VectorQuantizer2: torch.argmin); bitwise independent of M.  Any M, N >= 1;
 * E % 64 == 0 and E <= 512, otherwise an argument error and no launch.  Every index lies in [0, N), also for non-finite z. */
int rdm_op_vq_nearest_code(rdm_ctx* ctx, const float* z /*[dev] [M,E]*/, const float* codebook /*[dev] [N,E]*/, long long M, int N, int E,
                           int32_t* idx_out /*[dev] [M]*/);
/* ---- quality metrics on feature sets (csrc/metrics.hip): x f32 [dev] [n, d] row-major, d % 32 == 0 and 32 <= d <= 4096 (anything else: an
 * argument error naming the op and the value, no launch, the context stays usable).
 * Frechet distance (Heusel et al. 2017, FID = |mu_a - mu_b|^2 + Tr(S_a + S_b - 2 (S_a S_b)^1/2)): its sufficient statistics.
 * sum [dev] f64 [d] += SUM_i x_i and outer [dev] f64 [d, d] += SUM_i x_i x_i^T, products and sums in fp64 (v_mfma_f64_16x16x4_f64).  In / out:
 * the caller zeroes both once and folds any number of batches in.  No atomics; a call's reduction order depends on (n, d) alone, so it
 * is reproducible, and differently chunked calls differ by fp64 rounding only. */
int rdm_op_moments_f64(rdm_ctx* ctx, const float* x, int n, int d, double* sum, double* outer);
/* Improved precision and recall (Kynkaanniemi et al. 2019, eq. 3): radius2_out [dev] f32 [n], entry i = the squared Euclidean distance from
 * row i to its k-th nearest OTHER row, NN_k(x_i, X \ {x_i})^2.  Self is left out by index, so a duplicate row is a neighbour at distance 0.
 * 1 <= k <= 8 and k < n.  d2(a, b) = max(0, |a|^2 + |b|^2 - 2 a.b) in fp32 on fp32-input MFMAs, norms and dot product by one chain over k
 * (equal rows: exactly 0); |d2 - exact| <= 5e-7 (|a|^2 + |b|^2) for d <= 1024.  A pair's value does not depend on n or on where the pair
 * lands; the n x n distances are streamed, never stored. */
int rdm_op_knn_radius(rdm_ctx* ctx, const float* x, int n, int d, int k, float* radius2_out);
/* The same paper's f(probe_i, Ref): hit_out [dev] uint8 [m], 1 iff some j has d2(probe_i, ref_j) <= ref_radius2[j] (ref_radius2 [dev] f32 [n],
 * from rdm_op_knn_radius on ref); precision = mean f(generated, Real), recall = mean f(real, Generated).  d2 as above.  m, n >= 1. */
int rdm_op_manifold_hits(rdm_ctx* ctx, const float* probe /*[m,d]*/, int m, const float* ref /*[n,d]*/, const float* ref_radius2, int n, int d,
                         unsigned char* hit_out);
/* Density (Naeem et al. 2020, eq. 7): density = 1 / (k M) SUM_j SUM_i 1[Y_j in B(X_i, NND_k(X_i))] over generated rows Y_j and real rows X_i.
 * count_out [dev] int32 [m], entry i = #{ j : d2(probe_i, ref_j) <= ref_radius2[j] }: the balls of the reference set that probe i lies in
 * (probe = generated, ref = real, ref_radius2 from rdm_op_knn_radius on ref); density = SUM count / (k m).  rdm_op_manifold_hits that counts
 * where it ORs: count > 0 equals that entry's hit, bit for bit.  d2 as for rdm_op_knn_radius: |d2 - exact| <= 5e-7 (|a|^2 + |b|^2) for
 * d <= 1024.  m, n >= 1. */
int rdm_op_manifold_counts(rdm_ctx* ctx, const float* probe /*[m,d]*/, int m, const float* ref /*[n,d]*/, const float* ref_radius2 /*[n]*/,
                           int n, int d, int32_t* count_out /*[m]*/);
/* Coverage (the same paper, eq. 9): coverage = 1 / N SUM_i 1[exists j: Y_j in B(X_i, NND_k(X_i))] = mean over real rows i of
 * [min_j d2(X_i, Y_j) <= radius2_i].  d2_out [dev] f32 [m], entry i = min_j d2(probe_i, ref_j), nothing left out (probe = real, ref =
 * generated).  d2 as for rdm_op_knn_radius: |d2 - exact| <= 5e-7 (|a|^2 + |b|^2) for d <= 1024, the same value the other entries see for
 * the pair; a probe equal to a reference row gives exactly 0.  m, n >= 1. */
int rdm_op_nearest_d2(rdm_ctx* ctx, const float* probe /*[m,d]*/, int m, const float* ref /*[n,d]*/, int n, int d, float* d2_out /*[m]*/);
/* KID (Binkowski et al. 2018): the unbiased MMD^2 = SUM_{i != j} k(x_i, x_j) / (m (m - 1)) + SUM_{i != j} k(y_i, y_j) / (n (n - 1))
 * - 2 SUM_{i, j} k(x_i, y_j) / (m n) under k(x, y) = (gamma x.y + coef0)^3 (the paper: gamma = 1 / d, coef0 = 1), averaged over subsets.
 * This entry gives the row sums of one such kernel matrix per group: rowsum_out [dev] f64 [groups, m], entry (g, i) = SUM_j (gamma
 * probe_gi . ref_gj + coef0)^3 over the n reference rows of the SAME group, without the pair j == i (row index within the group) when
 * exclude_same_index is non-zero: the diagonal of XX or YY.  Error statement: the dot product in fp32 on the chain of rdm_op_knn_radius,
 * dot product within 2.5e-7 (|a|^2 + |b|^2), all later arithmetic fp64 (gamma and coef0 widened as given).  No atomics: a row's sum does
 * not depend on m, on the group count or on where the row lands.  m, n >= 1; 1 <= groups <= 65535 and groups * max(m, n) must fit an int. */
int rdm_op_poly3_rowsums(rdm_ctx* ctx, const float* probe /*[groups,m,d]*/, int m, const float* ref /*[groups,n,d]*/, int n, int d, int groups,
                         int exclude_same_index, float gamma, float coef0, double* rowsum_out /*[groups,m]*/);
/* the RARM sampler kernel alone (taming top_k_logits + softmax + multinomial as an inverse CDF in vocabulary order, after the
 * classifier-free combine lu + scale (lc - lu) and the temperature; transformer.py:237-263): logits [dev] f32 [(cfg ? 2 : 1) * b, vocab]
 * (conditional rows first), uniforms [dev] f32 [b], tokens_out [dev] int64 [b].  top_k <= 0: no filter. */
int rdm_op_rarm_sampler(rdm_ctx* ctx, const float* logits, int b, int vocab, int cfg, float guidance_scale, float temperature,
                        int top_k, const float* uniforms, int64_t* tokens_out);
/* the same kernel with the nucleus filter of rdm_rarm_sample_top_p (the `top_p` of transformer.py:279-280, unbuilt there): top_p in
 * (0, 1], 1 = no nucleus filter.  kept_out: optional [dev] int32 [b], receives the number of tokens each row kept (after top-k and top-p). */
int rdm_op_rarm_sampler_top_p(rdm_ctx* ctx, const float* logits, int b, int vocab, int cfg, float guidance_scale, float temperature,
                              int top_k, float top_p, const float* uniforms, int64_t* tokens_out, int32_t* kept_out);
/* ---- backward building blocks of the training step (reference rdm/models/diffusion/ddpm.py:390-443 shared_step -> ldm
 * p_losses -> autograd through UNetModel): gradients of the ResBlock's ops.  bf16 activations / activation gradients, fp32 weight
 * gradients.  conv3x3: stride 1, pad 1, weights [N][3][3][C].  Tested against torch autograd (tests/test_gpu_backward.py). */
int rdm_op_conv3x3_dgrad(rdm_ctx* ctx, const void* dy_bf16 /*[B,H,W,N]*/, const void* w_bf16, void* dx_bf16 /*[B,H,W,C]*/, int B, int H, int W,
                         int C, int N);
int rdm_op_conv3x3_wgrad(rdm_ctx* ctx, const void* x_bf16 /*[B,H,W,C]*/, const void* dy_bf16 /*[B,H,W,N]*/, float* dw /*[N,3,3,C]*/, int B, int H,
                         int W, int C, int N);
int rdm_op_groupnorm_bwd(rdm_ctx* ctx, const void* x_bf16, const void* dy_bf16, const float* gamma, const float* beta, int B, int HW, int C,
                         float eps, int silu, void* dx_bf16, float* dgamma, float* dbeta);
int rdm_op_layernorm_bwd(rdm_ctx* ctx, const void* x_bf16, const void* dy_bf16, const float* gamma, int M, int C, float eps, void* dx_bf16,
                         float* dgamma, float* dbeta);
/* The same two with the gradient of a residual path joined in the kernel: dx = (norm gradient) + residual (bf16, dx's shape; one rounding).
 * Where autograd adds the branch's gradient to the skip connection's (x + f(norm(x)) in ResBlock / BasicTransformerBlock). */
int rdm_op_groupnorm_bwd_add(rdm_ctx* ctx, const void* x_bf16, const void* dy_bf16, const float* gamma, const float* beta, int B, int HW, int C,
                             float eps, int silu, const void* residual_bf16, void* dx_bf16, float* dgamma, float* dbeta);
int rdm_op_layernorm_bwd_add(rdm_ctx* ctx, const void* x_bf16, const void* dy_bf16, const float* gamma, int M, int C, float eps,
                             const void* residual_bf16, void* dx_bf16, float* dgamma, float* dbeta);
/* nn.Linear weight gradient dW [N, K] fp32 = dy^T a for dy [M, N], a [M, K] bf16 (autograd of F.linear in the training step): K-split
 * over the M rows, deterministic fixed-order sum of the fp32 partial planes. */
int rdm_op_linear_wgrad(rdm_ctx* ctx, const void* dy_bf16, const void* a_bf16, float* dw, long long M, int N, int K);
/* Which kernel the two weight-gradient ops run for a shape, host only (no device call); the ops dispatch on this same function.
 *   conv != 0: rdm_op_conv3x3_wgrad at (B, H, W, C, N) (M, K ignored); conv == 0: rdm_op_linear_wgrad at (M, N, K) (B, H, W, C ignored).
 *   path: CONV9_LW4 / 5 / 6 = the nine-tap kernel at image width 16 / 32 / 64; TN9 / TN1 = the per-tap transpose-free kernel with 9 taps / 1 tap;
 *   the fallbacks copy both operands transposed and run the implicit GEMM.  Z = fp32 planes summed in plane order (1: straight into dw);
 *   per_plane = what one plane reduces over: chunks of max(32, W) pixels (CONV9), rows (TN), padded K' positions (fallbacks);
 *   remap: CONV9 = the number of leading planes dealt whole to the XCDs (Z & ~7; the rest in launch order), TN = 1 when tiles * Z is a
 *   multiple of 8 and the blocks of a (tile, plane) share an XCD, fallbacks 0.  Returns -1 for a shape the op refuses (the two share one check: B, H, W, N >= 1, C even >= 2 and B H W
 *   within int for the conv; 1 <= M within int, N and K even >= 2 for the linear op). */
enum { RDM_WGRAD_CONV9_LW4 = 1, RDM_WGRAD_CONV9_LW5 = 2, RDM_WGRAD_CONV9_LW6 = 3, RDM_WGRAD_TN9 = 4, RDM_WGRAD_TN1 = 5, RDM_WGRAD_CONV_FALLBACK = 6,
       RDM_WGRAD_LINEAR_FALLBACK = 7 };
typedef struct rdm_wgrad_form { int path, Z, per_plane, remap; } rdm_wgrad_form;
int rdm_wgrad_select(int conv, int B, int H, int W, int C, int N, long long M, int K, rdm_wgrad_form* form_out);
int rdm_op_colsum(rdm_ctx* ctx, const void* x_bf16 /*[M,N]*/, float* out /*[N]*/, long long M, int N);
int rdm_op_transpose(rdm_ctx* ctx, const void* x_bf16 /*[rows,cols]*/, void* y_bf16 /*[cols,rows]*/, int rows, int cols);
int rdm_op_add(rdm_ctx* ctx, const void* a_bf16, const void* b_bf16, void* out_bf16, long long n);
/* One DDIM update, the kernel of rdm_ddim_sample alone on caller-owned [dev] f32 buffers of n elements (eps: 2n under cfg, [cond | uncond]),
 * with the kernel's own scalars -- the caller owns the schedule: e = cfg ? eps[n + i] + scale (eps[i] - eps[n + i]) : eps[i];
 * pred_x0 = (x - sqrt_one_minus_at e) / sqrtf(a_t); x_prev = sqrtf(a_prev) pred_x0 + sqrtf(1 - a_prev - sigma_t^2) e
 * + sigma_t noise temperature (no noise source: the last term is absent, whatever sigma_t); x_dup <- x_prev.  x_prev may be x.
 * noise (rdm_noise): the stack holds n elements; seeded, the noise of element i is the normal of (seed, stream 1, noise->step,
 * row0 + i / per_row, i % per_row) with noise->per_row, and rows [row0, row0 + n / per_row) must pass the device-noise row check. */
int rdm_op_ddim_step(rdm_ctx* ctx, const float* x, const float* eps, const rdm_noise* noise, long long n, int cfg, float scale, float a_t,
                     float a_prev, float sigma_t, float sqrt_one_minus_at, float temperature, float* x_prev, float* x_dup_or_null,
                     float* pred_x0_or_null);
/* One PLMS update, the kernel of rdm_plms_sample alone (fp32, n elements, eta = 0): e_t = the guided eps as above.
 *   mode 0 (step):    e' = e_t | (3 e_t - h1) / 2 | (23 e_t - 16 h1 + 5 h2) / 12 | (55 e_t - 59 h1 + 37 h2 - 9 h3) / 24 at order 0 | 1 | 2 | 3;
 *                     e_store <- e_t (after the history reads: e_store may be h3)
 *   mode 1 (Euler A): e' = e_t; e_store <- e_t        mode 2 (Euler B): e' = (e_prev + e_t) / 2; e_store is not written
 * pred_x0 = (x - sqrt_one_minus_at e') / sqrtf(a_t); x_out = sqrtf(a_prev) pred_x0 + sqrtf(1 - a_prev) e'; x_dup <- x_out.  x_out may be x.
 * Returns -1 with a message, and launches nothing, for a mode outside 0..2, an order outside 0..3, a null e_prev in mode 2, a null history
 * operand the order reads in mode 0, and a null e_store in modes 0 and 1. */
int rdm_op_plms_step(rdm_ctx* ctx, const float* x, const float* eps, const float* e_prev_or_null, const float* h1_or_null,
                     const float* h2_or_null, const float* h3_or_null, long long n, int cfg, float scale, float a_t, float a_prev,
                     float sqrt_one_minus_at, int mode, int order, float* e_store_or_null, float* x_out, float* x_dup_or_null,
                     float* pred_x0_or_null);
/* One ancestral DDPM update, the kernel of rdm_ddpm_sample alone (fp32, n elements): x0 = sqrt_recip x - sqrt_recipm1 eps, clamped to
 * [-1, 1] when clip; x_prev = coef1 x0 + coef2 x + (nonzero ? expf(0.5 log_var) noise temperature : 0).  x_prev may be x.  nonzero == 0
 * ignores a noise stack; nonzero != 0 without a noise source is refused (-1).  noise as rdm_op_ddim_step's. */
int rdm_op_ddpm_step(rdm_ctx* ctx, const float* x, const float* eps, const rdm_noise* noise, long long n, float sqrt_recip,
                     float sqrt_recipm1, float coef1, float coef2, float log_var, int clip, int nonzero, float temperature, float* x_prev);
/* One DPM-Solver++ update, the kernel of rdm_dpmpp_sample alone (fp32, n elements): e = cfg ? eps[n + i] + scale (eps[i] - eps[n + i])
 * : eps[i]; m0 = (x - sqrt_one_minus_a_s e) / sqrt_a_s; x_out = c_x x + c_0 m0 + c_1 m_prev (no m_prev: the last term is absent);
 * x_dup <- x_out, m_store <- m0, pred_x0 <- m0.  m_store may be m_prev itself. */
int rdm_op_dpmpp_step(rdm_ctx* ctx, const float* x, const float* eps, const float* m_prev_or_null, long long n, int cfg, float scale,
                      float sqrt_a_s, float sqrt_one_minus_a_s, float c_x, float c_0, float c_1, float* x_out, float* x_dup_or_null,
                      float* m_store_or_null, float* pred_x0_or_null);
/* One SDE-DPM-Solver++ update, the kernel of rdm_dpmpp_sde_sample alone (fp32, n elements): e and m0 as rdm_op_dpmpp_step;
 * x_out = ((c_x x + c_0 m0) + c_1 m_prev) + c_n z (no m_prev: the c_1 term is absent), with the formula's flattened coefficients
 * c_x = (sigma_t / sigma_s) exp(-h), c_0 + c_1 = alpha_t (1 - exp(-2h)), c_n = sigma_t sqrt(1 - exp(-2h)) -- the caller owns the schedule;
 * x_dup <- x_out, m_store <- m0, pred_x0 <- m0.  m_store may be m_prev itself.  z: noise (rdm_noise, required), as rdm_op_ddim_step's. */
int rdm_op_dpmpp_sde_step(rdm_ctx* ctx, const float* x, const float* eps, const float* m_prev_or_null, const rdm_noise* noise, long long n,
                          int cfg, float scale, float sqrt_a_s, float sqrt_one_minus_a_s, float c_x, float c_0, float c_1, float c_n,
                          float* x_out, float* x_dup_or_null, float* m_store_or_null, float* pred_x0_or_null);
/* One UniPC pass, the kernel of rdm_unipc_sample alone (fp32, n elements; coefficients [host]: the 13 doubles of rdm_unipc_coefficients,
 * rounded to fp32 here): e = cfg ? eps[n + i] + scale (eps[i] - eps[n + i]) : eps[i]; m = (u - sigma e) / alpha;
 * xc = order_c ? a_x xc_prev + a_t m + a_1 h1 (+ a_2 h2) (+ a_3 h3) : u; u_next = b_x xc + b_0 m (+ b_1 h1) (+ b_2 h2), terms up to the
 * orders; xc_out <- xc, x_dup <- u_next, m_store <- m, pred_x0 <- m.  Operands the orders do not reach may be null.  u_next may be u,
 * xc_out may be xc_prev, m_store may be any history slot. */
int rdm_op_unipc_step(rdm_ctx* ctx, const float* u, const float* eps, const float* xc_prev_or_null, const float* h1_or_null,
                      const float* h2_or_null, const float* h3_or_null, long long n, int cfg, float scale, const double* coefficients,
                      float* xc_out_or_null, float* u_next, float* x_dup_or_null, float* m_store_or_null, float* pred_x0_or_null);
/* Elementwise pieces of the UNet's training graph: SiLU of the time-embedding MLP (`nn.SiLU()` in
 * openaimodel.py time_embed / emb_layers) -- dy null: out bf16 = silu(x), else out fp32 = dy * silu'(x) -- and the 2 x 2 sum pooling
 * that is the gradient of Upsample's nearest-neighbour F.interpolate: x bf16 [B, 2H, 2W, C] -> out bf16 [B, H, W, C]. */
int rdm_op_silu(rdm_ctx* ctx, const float* x, const float* dy_or_null, void* out_bf16_or_f32, long long n);
int rdm_op_sumpool2(rdm_ctx* ctx, const void* x_bf16, void* out_bf16, int B, int H, int W, int C);
/* The elementwise steps of MinimalRETRODiffusion.shared_step -> forward -> ldm p_losses around the UNet (rdm/models/diffusion/ddpm.py:390-443):
 *   rdm_op_q_sample   LatentDiffusion.q_sample: x_t = sqrt_ac[b] x0 + sqrt_1mac[b] noise; x0 / noise / out f32 NCHW [B,C,H,W] (out may be
 *                     NULL), out_nhwc bf16 [B,H,W,cpad] (may be NULL; channels >= C zero): the operand of the native training forward;
 *   rdm_op_mse_loss   p_losses (l2, eps parameterisation): se[b] = mean_{chw} (eps - target)^2 and, when deps is given,
 *                     deps = coef[b] (eps - target); eps / deps bf16 NHWC [B,H,W,ldc] (first C channels), target f32 NCHW;
 *   rdm_op_where_rows out[b,:] = mask[b] ? a[b,:] : x[b,:] (the Bernoulli(p_uncond) conditioning switch, :393-396); mask uint8 [rows];
 *   rdm_op_timestep_embedding  ldm timestep_embedding: t int64 [B] -> bf16 [B, ld] = [cos | sin | zero tail];
 *   rdm_op_colsum_samples      x bf16 [B,HW,N] -> bf16 [B,N], sum over a sample's pixels (gradient of the time-embedding row a ResBlock adds);
 *   rdm_op_expand2    x bf16 [B,H,W,C] -> [B,2H,2W,C]: mode 0 zero insertion (stride-2 conv gradient as a stride-1 one), mode 1 nearest copy. */
int rdm_op_q_sample(rdm_ctx* ctx, const float* x0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac, float* out_or_null,
                    void* out_nhwc_bf16_or_null, int B, int C, int H, int W, int cpad);
int rdm_op_mse_loss(rdm_ctx* ctx, const void* eps_nhwc_bf16, const float* target, const float* coef_or_null, float* se, void* deps_nhwc_bf16_or_null,
                    int B, int C, int H, int W, int ldc);
int rdm_op_where_rows(rdm_ctx* ctx, const unsigned char* mask, const float* a, const float* x, float* out, long long rows, long long n);
int rdm_op_timestep_embedding(rdm_ctx* ctx, const int64_t* t, void* out_bf16, int B, int dim, int ld);
int rdm_op_colsum_samples(rdm_ctx* ctx, const void* x_bf16, void* out_bf16, int B, int HW, int N);
int rdm_op_expand2(rdm_ctx* ctx, const void* x_bf16, void* out_bf16, int B, int H, int W, int C, int mode);
/* LitEma.forward (ldm/modules/ema.py: `shadow.sub_(one_minus_decay * (shadow - param))`; the caller computes
 * decay = min(decay, (1 + num_updates) / (10 + num_updates)) like the reference) on fp32 tensors in place. */
int rdm_op_ema(rdm_ctx* ctx, float* shadow, const float* param, long long n, float one_minus_decay);
/* One AdamW step (torch.optim.AdamW: decoupled weight decay, bias-corrected moments; the reference's configure_optimizers,
 * rdm/models/diffusion/ddpm.py, hands the UNet parameters to it) on fp32 master parameters / moments in place; p_bf16 (optional) receives
 * the bf16 working copy the kernels read.  step counts from 1.  The hyper-parameters are doubles: 1 - beta and the bias corrections 1 - beta^step
 * are differences of nearly equal numbers (1 - 0.999f is 1.3e-5 short of 1e-3), so they are taken in double here and rounded once for the kernel. */
int rdm_op_adamw(rdm_ctx* ctx, float* p, const float* grad, float* exp_avg, float* exp_avg_sq, void* p_bf16_or_null, long long n, double lr,
                 double beta1, double beta2, double eps, double weight_decay, int step);
/* The same two over LISTS of tensors (host arrays of n device pointers and element counts; p_bf16 may be null, or hold null entries): the
 * UNet has 688 parameter tensors, most of them tiny -- 48 tensors per launch instead of one launch each.  Same arithmetic per element. */
int rdm_op_adamw_multi(rdm_ctx* ctx, int n, float* const* p, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                       void* const* p_bf16_or_null, const long long* numel, double lr, double beta1, double beta2, double eps, double weight_decay, int step);
int rdm_op_ema_multi(rdm_ctx* ctx, int n, float* const* shadow, const float* const* param, const long long* numel, float one_minus_decay);
/* Attention backward, unfused first version (autograd through ldm CrossAttention.forward, attention.py:52-72:
 * sim = einsum(q, k) * scale; attn = sim.softmax(-1); out = einsum(attn, v)).  The scores are materialised per (sample, head):
 *   rdm_op_heads   x [B, n, ldx] (head h = columns [h D, (h+1) D)) <-> per-head matrices zero-padded to 64 columns:
 *                  mode 0 -> [B H][n][64], mode 1 -> transposed [B H][64][n], mode 2: [B H][n][64] -> [B, n, H D];
 *   rdm_op_bmm     out[z] = alpha * A[z] W[z]^T for batch contiguous bf16 matrices A [M, K], W [N, K] (K % 64 == 0), bf16 and / or fp32 out;
 *   rdm_op_transpose_batched, rdm_op_softmax (fp32 scores -> bf16 probabilities, row-wise), rdm_op_softmax_bwd
 *   (dS = P * (dP - rowsum(P * dP))).  rdm_amd/training.py attention_forward / attention_backward assemble them. */
/* Fused attention backward for d_head = 32 (no n x m score matrix): q, o, dout [B, n, heads * 32], k, v [B, m, heads * 32] bf16 (o = the forward
 * output) -> dq [B, n, C], dk, dv [B, m, C] bf16.  n, m multiples of 32 (pad the keys and mask them with rdm_op_softmax otherwise). */
int rdm_op_attention_bwd(rdm_ctx* ctx, const void* q, const void* k, const void* v, const void* o, const void* dout, int B, int n, int m, int heads,
                         void* dq, void* dk, void* dv);
int rdm_op_bmm(rdm_ctx* ctx, const void* a_bf16, const void* w_bf16, void* out_bf16_or_null, float* out_f32_or_null, int batch, int M, int N, int K,
               float alpha);
int rdm_op_heads(rdm_ctx* ctx, const void* x_bf16, void* out_bf16, int B, int n, int H, int D, int ldx, int mode);
int rdm_op_transpose_batched(rdm_ctx* ctx, const void* x_bf16, void* y_bf16, int batch, int rows, int cols);
int rdm_op_softmax(rdm_ctx* ctx, const float* scores, void* p_bf16, long long rows, int n, int n_valid /* columns >= n_valid are padding: probability 0 (0 = all valid) */);
int rdm_op_softmax_bwd(rdm_ctx* ctx, const void* p_bf16, const float* dp, void* ds_bf16, long long rows, int n);
/* GEGLU (ldm attention.py GEGLU.forward: `x, gate = proj(x).chunk(2, dim=-1); return x * F.gelu(gate)`) on an UNPERMUTED
 * pre-activation pre [M, 2F] = [x | gate], bf16.  dh null: forward, out [M, F].  dh [M, F] given: backward, out [M, 2F] = [dx | dgate]
 * (what autograd computes for that line in the training step). */
int rdm_op_geglu(rdm_ctx* ctx, const void* pre_bf16, const void* dh_bf16_or_null, void* out_bf16, long long M, int F);
int rdm_op_groupnorm(rdm_ctx* ctx, const void* x0_bf16, const void* x1_bf16, int C0, int C1, int B, int HW,
                     const float* gamma, const float* beta, float eps, int silu, void* out_bf16);
int rdm_op_layernorm(rdm_ctx* ctx, const void* x, int in_is_f32, const float* gamma, const float* beta, int M, int C,
                     float eps, void* out_bf16);
/* The two forms only the CLIP towers run (custom_clip/model.py:166-187, 216-224): LayerNorm of fp32 rows [M, C] to fp32 (visual.ln_pre),
 * and out_f32 [M, N] = act(a w^T + bias) + res_f32 through the tiled GEMM at any M (the towers' `x = x + attn(...)`, `x = x + mlp(...)` on
 * the fp32 residual stream): a bf16 [M, K], w bf16 [N, K], bias / res_f32 fp32 or null; out_f32 may be the very buffer res_f32 points
 * to (each element is read once, by the lane that then writes it).  N even, K % 64 == 0; act: none, QuickGELU or SiLU. */
int rdm_op_layernorm_f32(rdm_ctx* ctx, const float* x, const float* gamma, const float* beta, int M, int C, float eps, float* out_f32);
int rdm_op_linear_res_f32(rdm_ctx* ctx, const void* a_bf16, const void* w_bf16, const float* bias, const float* res_f32, float* out_f32,
                          int M, int N, int K, int act);
int rdm_op_self_attention(rdm_ctx* ctx, const void* qk_bf16, const void* vt_bf16, int B, int n, int heads,
                          void* out_bf16);
/* the same attention from ONE fused projection qkv [B, n, 3C] = [q | k | v] (the UNet sampling path's form: V stays token-major and is
 * transposed inside the kernel's LDS reads); n % 64 == 0 */
int rdm_op_self_attention_qkv(rdm_ctx* ctx, const void* qkv_bf16, int B, int n, int heads, void* out_bf16);
/* CrossAttention over k retrieved neighbours (rdm/modules/attention.py:52-72) in the re-associated per-sample form the UNet path uses:
 *   out[b] = softmax_groups(x[b] G[b]^T) U[b]^T + bias + res[b]
 * x / res / out bf16 [B, n, C], G bf16 [B, NP, C] (row h*k + j = key j restricted to head h, times W_q / sqrt(d)), U bf16 [B, C, NP]
 * (column h*k + j = W_o applied to value j restricted to head h); softmax over groups of `group` (= k: 1, 2, 4) adjacent columns of
 * the first ncols = heads * k columns.  n % 32 == 0, C % 64 == 0, NP % 32 == 0, ncols <= min(NP, 128).  bias / res may be null.
 * With ln_gamma / ln_beta given (res null) the LayerNorm in front and the residual are folded in as well:
 *   out[b] = softmax_groups(LayerNorm(x[b]) G[b]^T) U[b]^T + bias + x[b]      (norm2 + attn2 + residual of BasicTransformerBlock,
 * attention.py:238). */
int rdm_op_xattn_fused(rdm_ctx* ctx, const void* x_bf16, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G_bf16,
                       const void* U_bf16, const float* bias, const void* res_bf16, int B, int n, int C, int NP, int ncols, int group,
                       void* out_bf16);
/* The LayerNorm-folded form IN PLACE with norm3 emitted as well (what the executor runs on a guided batch's conditional rows):
 *   x[b] <- softmax_groups(LayerNorm(x[b]; ln) G[b]^T) U[b]^T + bias + x[b];   ln3_out[b] = LayerNorm(x[b] (the bf16 rows just stored); ln3)
 * i.e. `x = attn2(norm2(x), context) + x` followed by `norm3(x)` of BasicTransformerBlock (attention.py:238-239) in one launch. */
int rdm_op_xattn_fused_ln3(rdm_ctx* ctx, void* x_bf16_inout, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G_bf16,
                           const void* U_bf16, const float* bias, int B, int n, int C, int NP, int ncols, int group,
                           const float* ln3_gamma, const float* ln3_beta, void* ln3_out_bf16);
/* Both of the above under a neighbour bias (see rdm_set_neighbour_bias for the semantics): key_bias [dev] fp32 [B, group], entry
 * [b][j] added to the score columns h * group + j of sample b before the group softmax; -inf entries allowed, every row needs one finite
 * entry (the caller's duty here: the device values are not read back).  ln3_out given: the in-place LN + norm3 form (x is written,
 * out must be x or null, res null, ln_gamma / ln_beta / ln3_gamma / ln3_beta required); else rdm_op_xattn_fused's plain or LN form.
 * With group 1 a finite bias cannot change the result: it is bitwise the unbiased one. */
int rdm_op_xattn_fused_biased(rdm_ctx* ctx, void* x_bf16, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G_bf16,
                              const void* U_bf16, const float* bias, const void* res_bf16, int B, int n, int C, int NP, int ncols, int group,
                              void* out_bf16, const float* ln3_gamma, const float* ln3_beta, void* ln3_out_bf16, const float* key_bias);
/* Causal self-attention at d_head 64 over all n positions (CrossAttention.forward with RetrievalPatchTransformer's causal mask,
 * rdm/modules/attention.py:42-74, 199-272): qkv bf16 [B*n rows at stride ldq] = q | k | v thirds of heads*64 columns each, head h in columns
 * h*64..h*64+63 of its third; out bf16 [B*n, heads*64] at stride ldo; 1 <= n <= 1024.  kcache / vcache (both or neither) [B][heads][L][64]
 * bf16: rows 0..n-1 receive the K / V columns of qkv bit for bit (the decode step's cache layout), rows >= n are not touched. */
int rdm_op_causal_attention_d64(rdm_ctx* ctx, const void* qkv_bf16, int ldq, int B, int n, int heads, float scale, void* out_bf16, int ldo,
                                void* kcache_bf16_or_null, void* vcache_bf16_or_null, int L);
/* ---- the RARM decode step's kernels, one at a time (rarm_step of rdm_rarm_forward / rdm_rarm_sample: one row per sequence)
 * Which kernel a one-row-per-sequence linear op runs, host only (no device call): kernel = one of RDM_LINEAR_ROWS_*; for the skinny kernel
 * (sgemm.hip) also its instantiation: 16*ma rows x 16*nb weight rows per block, u k-steps of 32 per batch of loads, nw waves splitting K,
 * ln = the LayerNorm formed in the kernel, geglu.  The library's own dispatch asks this same function. */
enum { RDM_LINEAR_ROWS_REFUSED = 0, RDM_LINEAR_ROWS_SGEMM = 1, RDM_LINEAR_ROWS_MGEMM = 2, RDM_LINEAR_ROWS_TILED = 3 };
typedef struct rdm_linear_rows_form { int kernel, ma, nb, u, nw, ln, geglu; } rdm_linear_rows_form;
/* The kernel rdm_op_linear_rows launches for (M, N, K, act) with a LayerNorm operand (ln != 0) or a bf16 one, in fast (deterministic = 0) or
 * deterministic mode.  RDM_LINEAR_ROWS_REFUSED: the LayerNorm form declines the shape (the executor then runs LayerNorm and the plain op). */
int rdm_linear_rows_select(int M, int N, int K, int act, int ln, int deterministic, rdm_linear_rows_form* form_out);
/* A linear op of the decode step, as the executor calls it (one row per sequence, in the context's current mode):
 *   out[M, N (N/2: GEGLU)] = act(A W^T + bias) (+ res_f32),  A = a_bf16 [M, K], or LayerNorm(ln_x_f32 [M, K]; gamma, beta, eps 1e-5) formed in
 * the kernel (exactly one of a_bf16 / ln_x_f32; the LayerNorm form: K = 768, bf16 output only, no residual).  w bf16 [N, K] (GEGLU: rows in
 * the packed order of the model blob), bias f32 [N] or NULL, res_f32 [M, N] or NULL, out_bf16 and / or out_f32; out_f32 == res_f32 is allowed
 * (the residual stream updated in place).  Where the LayerNorm form declines the shape the call fails with -5: it does not fall back. */
int rdm_op_linear_rows(rdm_ctx* ctx, const void* a_bf16_or_null, const float* ln_x_f32_or_null, const float* ln_gamma, const float* ln_beta,
                       const void* w_bf16, const float* bias_or_null, const float* res_f32_or_null, void* out_bf16_or_null, float* out_f32_or_null,
                       int M, int N, int K, int act);
/* The decode step's attention over a K/V cache at d_head 64 (rarm.hip): q bf16 [batch rows at stride ldq], head h in columns h*64..h*64+63;
 * cache element (b, j, h, d) at b*batch_stride + j*row_stride + h*head_stride + d (head_stride 0 = 64: the heads side by side in a row).
 * Self mode (k_new / v_new given, same stride ldq): the new rows are stored at cache row pos and rows 0..pos are attended (0 <= pos < nkv =
 * the cache's capacity <= 1024).  Cross mode (k_new = v_new = NULL): rows 0..nkv-1 are attended; pos = -1, or >= 0 to hold the call to the
 * block-per-(head, sequence) kernel (otherwise 1..8 keys at batch >= 128 take the few-key kernel).  out bf16 [batch rows at stride ldo].
 * Strides are multiples of 8 elements, pointers 16-byte aligned. */
int rdm_op_rarm_decode_attention(rdm_ctx* ctx, const void* q_bf16, int ldq, const void* k_new_bf16_or_null, const void* v_new_bf16_or_null,
                                 void* kcache_bf16, void* vcache_bf16, long long batch_stride, int row_stride, long long head_stride, int nkv, int pos,
                                 float scale, void* out_bf16, int ldo, int heads, int batch);
/* The decode step's cross-attention over k neighbours in one launch, on operands re-associated per sequence:
 *   x[b] += softmax_per_head(LayerNorm(x[b]; ln) G[b]^T) UT[b] + bias  (b < Bc);   x[b] += bias  (Bc <= b < B2: zero neighbours)
 * x f32 [B2, C] in place; G, UT bf16 [Bc][NP][C], row h*k + j for head h, neighbour j; the softmax runs over each head's k columns.
 * ln3_gamma / ln3_beta / ln3_out (all or none): ln3_out bf16 [B2, C] = LayerNorm of the finished rows.  C % 8 == 0, C <= 1024,
 * heads * k <= min(128, NP). */
int rdm_op_rarm_xattn_decode(rdm_ctx* ctx, float* x_f32_inout, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* G_bf16,
                             const void* UT_bf16, const float* bias, int B2, int Bc, int C, int NP, int heads, int k, const float* ln3_gamma_or_null,
                             const float* ln3_beta_or_null, void* ln3_out_bf16_or_null);
/* Token embedding + positional encoding into the fp32 residual stream: x[r] = emb[token(r)] + pos_t[position(r)], emb f32 [vocab, C], pos_t
 * f32 [L, C]; a token id outside [0, vocab) reads row 0.  pos >= 0: the decode step (t = 1): token(r) = tokens[r], position pos < L.
 * pos = -1: the whole-sequence pass: row r is position r % t (t <= L) of sequence r / t, token(r) = tokens[((seq0 + r / t) % tok_rows) *
 * tok_ld + r % t], tokens int64 [tok_rows, tok_ld >= t]. */
int rdm_op_rarm_embed(rdm_ctx* ctx, const int64_t* tokens, int tok_ld, int tok_rows, int seq0, const float* emb_f32, const float* pos_t_f32,
                      float* x_f32, long long rows, int t, int C, int vocab, int L, int pos);
/* The first stage's AttnBlock without its n x n scores (ldm/modules/diffusionmodules/model.py AttnBlock.forward: q k^T * C^-1/2 -> softmax ->
 * . v over the h*w pixels, one head of C channels; what rdm_vq_decode_hw / rdm_vq_encode_hw run beyond 4096 pixels):
 *   out[b] = softmax(q[b] k[b]^T * scale) v[b] + bias_v
 * q, k, v bf16 token-major [B*n rows at strides ldq / ldk / ldv, multiples of 8, 16-byte aligned] (column blocks of one fused q | k | v
 * projection may be passed), bias_v f32 [C] or NULL, out bf16 [B*n, C] at stride ldo (a multiple of 4).  Any n >= 1; C a multiple of 128,
 * at most 512.  The arithmetic of rdm_op_bmm(alpha) -> rdm_op_softmax -> rdm_op_bmm: fp32 scores, the normalised probability rounded to
 * bf16, fp32 accumulation, one rounding of the result; two sweeps over the keys per 64 query rows, nothing of size n x n in memory, and a
 * sample's result does not depend on B. */
int rdm_op_vq_attention(rdm_ctx* ctx, const void* q_bf16, int ldq, const void* k_bf16, int ldk, const void* v_bf16, int ldv,
                        const float* bias_v_or_null, int B, int n, int C, float scale, void* out_bf16, int ldo);
/* nll_out[r] = logsumexp(logits[r,:]) - logits[r, targets[r]] in fp32 (F.cross_entropy(reduction='none'), transformer.py:62-70):
 * logits f32 [rows, vocab] (vocab even), targets int64 [rows]; a target outside [0, vocab) gives NaN. */
int rdm_op_rarm_nll(rdm_ctx* ctx, const float* logits, long long rows, int vocab, const int64_t* targets, float* nll_out);
/* ---- RARM training (the backward of LatentImageRETRO.training_step, rdm/models/autoregression/transformer.py:46-57)
 * Gradient of rdm_op_causal_attention_d64: the same qkv (stride ldq, a multiple of 8), out = the forward's bf16 output (stride ldo, a
 * multiple of 4), dout bf16 [B*n, heads*64] (stride lddo, a multiple of 8) -> dqkv bf16 = dq | dk | dv in the layout of qkv (stride ldd, a
 * multiple of 4; columns beyond 3*heads*64 are not touched).  1 <= n <= 1024; no n x n matrix in memory; fp32 accumulation; every element
 * written once, so two calls agree bitwise.  Scratch: the context's backward scratch (rdm_release_scratch returns it). */
int rdm_op_causal_attention_d64_bwd(rdm_ctx* ctx, const void* qkv_bf16, int ldq, const void* out_bf16, int ldo, const void* dout_bf16, int lddo,
                                    int B, int n, int heads, float scale, void* dqkv_bf16, int ldd);
/* dlogits[r,:] = gscale * (softmax(logits[r,:]) - onehot(targets[r])) (gscale = 1/rows: the gradient of the mean cross-entropy): fp32
 * arithmetic, one rounding to bf16 [rows, vocab].  nll_out f32 [rows] or null: bitwise what rdm_op_rarm_nll gives.  vocab even; a target
 * outside [0, vocab) gives NaN in its row. */
int rdm_op_rarm_nll_bwd(rdm_ctx* ctx, const float* logits, long long rows, int vocab, const int64_t* targets, float gscale, void* dlogits_bf16,
                        float* nll_out_or_null);
/* Gradient of an embedding lookup: dw f32 [V, C], dw[v,:] = sum of dy[m,:] (bf16 [M, C]) over tokens[m] == v in ascending m; rows of unused
 * ids are written as zero (no pre-clear), ids outside [0, V) are ignored.  No atomics: two calls agree bitwise.  C <= 12288. */
int rdm_op_embedding_grad(rdm_ctx* ctx, const int64_t* tokens, const void* dy_bf16, int M, int C, int V, float* dw_f32);
/* The UNet's `out` head (openaimodel.py:307-311: GroupNorm32 + SiLU + 3x3 conv to out_channels) and the VQ decoder's norm_out + swish +
 * conv_out as one statistics pass + one kernel: x bf16 NHWC [B, H, W, C] raw, 32 groups; gn_gamma / gn_beta null: no norm, x is convolved
 * as is.  w fp32 [Cout, C, 3, 3], bias fp32 [Cout] or null, out fp32 NCHW [B, Cout, H, W].  C % 32 == 0, C <= 240, W % 32 == 0, H even,
 * Cout <= 8. */
int rdm_op_head_conv(rdm_ctx* ctx, const void* x_bf16, const float* gn_gamma, const float* gn_beta, float gn_eps, const float* w,
                     const float* bias, int B, int H, int W, int C, int Cout, float* out_f32);
int rdm_op_small_attention(rdm_ctx* ctx, const void* q_bf16, int ldq, const void* k_bf16, const void* v_bf16, int ldkv,
                           int B, int nq, int nkv, int heads, int D, int causal, float scale, void* out_bf16, int ldo);
/* The same with key_bias [dev] fp32 [B, nkv] added to every head's scaled score of key j of sample b (the UNet's cross-attention at
 * k = 3, 8, 16 and at odd token counts under a neighbour bias).  -inf keys are skipped: they contribute exactly nothing, whatever their
 * k / v rows hold; every row needs one finite entry.  Not with causal (-1). */
int rdm_op_small_attention_biased(rdm_ctx* ctx, const void* q_bf16, int ldq, const void* k_bf16, const void* v_bf16, int ldkv,
                                  int B, int nq, int nkv, int heads, int D, int causal, float scale, void* out_bf16, int ldo,
                                  const float* key_bias);
/* Gradient of rdm_op_small_attention for the UNet's cross-attention (ldm CrossAttention, rdm/modules/attention.py:52-72, with the few
 * retrieved-neighbour embeddings as keys): d_head = 32, 1..32 keys, not causal.  q [B, nq, ldq], k / v [B, nkv, ldkv], dout [B, nq, ldo]
 * (head h = columns [32 h, 32 h + 32)) -> dq [B, nq, 32 heads], dk / dv [B, nkv, 32 heads], all bf16; sums in a fixed order. */
int rdm_op_small_attention_bwd(rdm_ctx* ctx, const void* q_bf16, int ldq, const void* k_bf16, const void* v_bf16, int ldkv, const void* dout_bf16, int ldo,
                               int B, int nq, int nkv, int heads, float scale, void* dq_bf16, void* dk_bf16, void* dv_bf16);
/* The stem conv in front of the UNet, the VQ decoder and the encoder (conv_in_kernel): 3x3, pad 1, x fp32 NCHW [B, Cin, H, W], w fp32
 * [Cout, Cin, 3, 3], bias fp32 [Cout] -> out bf16 NHWC [B, H, W, Cout]; one fp32 FMA chain per element, one rounding.  1 <= Cin <= 4,
 * Cout % 8 == 0, any H x W. */
int rdm_op_conv_in(rdm_ctx* ctx, const float* x_f32, const float* w_f32, const float* bias_f32, int B, int Cin, int H, int W, int Cout,
                   void* out_bf16);
/* The VALU head conv (conv_out_kernel), the one the models fall back to where rdm_op_head_conv's fused kernel refuses a shape (W % 32,
 * odd H): 3x3, pad 1, x bf16 NHWC [B, H, W, Cin], w fp32 [Cout, Cin, 3, 3], bias fp32 [Cout] -> out fp32 NCHW [B, Cout, H, W].
 * Cin % 64 == 0, 1 <= Cout <= 4, Cout * Cin <= 1820, any H x W. */
int rdm_op_conv_out(rdm_ctx* ctx, const void* x_bf16, const float* w_f32, const float* bias_f32, int B, int H, int W, int Cin, int Cout,
                    float* out_f32);

#ifdef __cplusplus
}
#endif
#endif
