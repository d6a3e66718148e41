// The sampling loops of librdm_hip (DDIM, PLMS, DPM-Solver++(2M) and its SDE form -- one loop, dpmpp_sample_impl --, UniPC, DDPM): their
// schedules, SamplerRun (one sampling call's scratch, tables and UNet forward), NoiseSource (where a loop's step noise comes from: a stack,
// a seed, or nowhere: the entries' one rdm_noise argument), the rdm_*_sample entries, the device-noise entries, DDIM image-to-image (rdm_ddim_decode: the
// DDIM loop begun part-way down the schedule; rdm_ddim_encode: the loop that runs UP it; rdm_ddim_inpaint: decode with the known latent
// blended in before every forward) and the step-kernel op entries.
// Calls into unet_exec.hip through the three functions host.h declares (unet_prepare_kv, unet_emb_table, unet_forward_impl) and
// into the launch_* of kernels.h.  The loops are the reference's
//   DDIMSampler                     rdm/models/diffusion/ddim.py:27-268
//   [ldm, un-vendored] p_sample_loop
#include "host.h"
#include "philox.h"

// ---- samplers
int rdm_ddim_num_intermediates(int S, int log_every_t) {
    int n = 0;
    for (int i = 0; i < S; i++) { const int index = S - i - 1; if (index % log_every_t == 0 || index == S - 1) n++; }
    return n;
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
// Where a loop's step noise comes from: a caller's stack, the generator under (seed, row0), or nowhere (a deterministic loop) -- never two
// of them: noise_source builds it from an entry's rdm_noise argument (who: the entry's name) and refuses one that names both.
struct NoiseSource {
    const float* stack = nullptr; bool seeded = false; NoiseSeed seed{};
    bool none() const { return !seeded && !stack; }
};
static int noise_source(rdm_ctx* c, const char* who, const rdm_noise* n, NoiseSource* ns) {
    *ns = NoiseSource{};
    if (n && n->seeded && n->stack) return c->fail(-1, "%s: give a seed or a stack, not both", who);
    if (n && n->seeded) { ns->seeded = true; ns->seed = {n->seed, n->row0}; }
    else if (n) ns->stack = n->stack;
    return 0;
}
// What a seeded loop asks of the call's shape (who: the sampler's name): check_noise_rows, and whole Philox blocks per row
template <class Args>
static int check_seeded(rdm_ctx* c, const char* who, const NoiseSource& ns, const Args* a) {
    if (!ns.seeded) return 0;
    const std::string w = std::string(who) + " (seeded)";
    const int64_t per_row = (int64_t)a->channels * a->height * a->width;
    RDM_TRY(check_noise_rows(c, w.c_str(), ns.seed.row0, a->batch, per_row));
    if (per_row % 4) return c->fail(-1, "%s: channels * height * width must be a multiple of 4", w.c_str());
    return 0;
}
// ... and of a seeded step launch: after check_seeded the one operand that can still be misaligned is the caller's pred_x0_inter
static int seeded_launched(rdm_ctx* c, const char* who, hipError_t e) {
    if (e == hipErrorInvalidValue) return c->fail(-1, "%s (seeded): pred_x0_inter must be 16-byte aligned", who);
    RDM_CHECK_HIP(c, e);
    return 0;
}

struct SamplerRun {
    rdm_ctx* c; int B, nb, k, H, W, total; long long n1;           // n1: elements of x for B rows; total: ts.size()
    float *x, *x_dup, *eps, *extra[4]; long long* tdev; const float* emb_table;
    int log_every_t = 0, n_logged = 0; float *x_inter = nullptr, *pred_x0_inter = nullptr;     // intermediates (DDPM keeps none)
    bool ascending = false;       // the encode loop: the intermediates rule reads the loop step itself as the schedule index
    static size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
    // a: the entry's args (batch, k, channels, height, width); uncond: null for an unguided call; log_every / x_inter_out / pred_x0_out:
    // the entry's intermediates arguments; n_extra <= 4.  The caller has checked that the UNet is loaded.
    template <class Args>       // rdm_ddim_args | rdm_dpmpp_args | rdm_unipc_args | rdm_ddpm_args: the five fields have the same names
    int begin(rdm_ctx* ctx, const Args* a, const std::vector<int>& ts, const float* x_T, const float* cond, const float* uncond,
              int log_every, float* x_inter_out, float* pred_x0_out, int n_extra) {
        c = ctx; B = a->batch; nb = uncond ? 2 * B : B; k = a->k; H = a->height; W = a->width; total = (int)ts.size();
        RDM_TRY(c->neighbour_bias_for("sampler", B, k));       // a neighbour bias in force belongs to exactly these B conditional samples
        n1 = (long long)B * a->channels * H * W;
        log_every_t = log_every; x_inter = x_inter_out; pred_x0_inter = pred_x0_out;
        const size_t x_bytes = (size_t)n1 * 4 * (nb / B), t_bytes = (size_t)total * nb * 8, h_stride = al((size_t)n1 * 4);
        const size_t off_x = al((size_t)nb * k * c->unet.cfg.context_dim * 4), off_t = al(off_x + x_bytes), off_eps = al(off_t + t_bytes),
                     off_extra = al(off_eps + x_bytes);
        RDM_TRY(ensure_bytes(c, &c->samp, &c->samp_bytes, off_extra + n_extra * h_stride));
        RDM_TRY(unet_prepare_kv(c, (float*)c->samp, cond, uncond, B, k));
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
        return unet_emb_table(c, ts, &emb_table);
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
    bool logs(int step) const { const int index = ascending ? step : total - 1 - step; return (index % log_every_t == 0) || (index == total - 1); }
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

// The DDIM loop of rdm_ddim_sample (the step noise is read from ns.stack, or, seeded, generated in the step kernel, and a null x_T is
// drawn) and of rdm_ddim_decode: n_run steps down from level index n_run - 1 (n_run < 0: the whole schedule).  The run is the loop over
// the schedule cut to its first n_run entries.
// Inpainting (rdm_ddim_inpaint): before the forward of loop step i the iterate is blended with the known latent x0 noised
// to that step's level, x <- (sqrt(a) x0 + sqrt(1 - a) z_i) m + (1 - m) x with a = a_t[index] (masked_blend_kernel; the scalars are float64
// square roots of the fp32 alpha, rounded, as rdm_ddim_encode's).  z_i is row i of q_noise, or -- a seeded loop, q_noise null -- drawn in
// the blend kernel from (seed, stream 0, step i + 1).  The result of the last step is not blended, as in ldm's loop.
struct InpaintSource { const float* x0; const float* mask; int mask_channels; const float* q_noise; };
static int ddim_sample_impl(rdm_ctx* c, const rdm_ddim_args* a, int n_run, const float* x_T, const float* cond, const float* uncond,
                            const NoiseSource& ns, float* z_out, float* x_inter, float* pred_x0_inter, const InpaintSource* ip = nullptr) {
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    bool cfg;
    RDM_TRY(sampler_guidance(c, "ddim", a->unconditional_guidance_scale, uncond, &cfg));
    RDM_TRY(check_seeded(c, "ddim", ns, a));
    if (ip && ip->mask_channels != 1 && ip->mask_channels != a->channels)
        return c->fail(-1, "ddim inpaint: mask_channels must be 1 or channels = %d, got %d", a->channels, ip->mask_channels);
    if (!ns.seeded && a->eta != 0.f && !ns.stack) return c->fail(-1, "eta > 0 needs an explicit noise stack [S,B,C,H,W] (device RNG parity is not defined)");
    std::vector<int> ts; std::vector<float> at, ap, s1m;
    RDM_TRY(ddim_schedule(c, a, ts, at, ap, s1m));
    if (n_run >= 0) {
        if (n_run < 1 || n_run > (int)ts.size()) return c->fail(-1, "ddim decode: t_start must lie in [1, %d], got %d", (int)ts.size(), n_run);
        ts.resize((size_t)n_run);
    }
    const int total = (int)ts.size();
    std::vector<float> sg(total);
    for (int i = 0; i < total; i++) {
        // sigma computed in float64 from the fp32 alphas like numpy does with a float64 alphas_prev array
        const double atd = (double)at[i], apd = (double)ap[i];
        sg[i] = (float)((double)a->eta * std::sqrt((1.0 - apd) / (1.0 - atd) * (1.0 - atd / apd)));
    }
    SamplerRun run;
    RDM_TRY(run.begin(c, a, ts, x_T, cond, cfg ? uncond : nullptr, a->log_every_t, x_inter, pred_x0_inter, 0));
    if (!x_T) RDM_TRY(run.draw_start(ns.seed));
    for (int i = 0; i < total; i++) {
        const int index = total - i - 1;         // of the ascending schedule
        if (ip) {
            const double ad = (double)at[index];
            MaskedBlendParams m{};
            m.x = run.x; m.x0 = ip->x0; m.mask = ip->mask; m.out = run.x; m.x_dup = run.x_dup;
            m.n = run.n1; m.chw = run.n1 / run.B; m.hw = (long long)run.H * run.W; m.mask_channels = ip->mask_channels;
            m.sqrt_a = (float)std::sqrt(ad); m.sqrt_1ma = (float)std::sqrt(1.0 - ad);
            const StepRngParams g = run.step_rng(ns.seed, i + 1);         // seeded: the known region's noise of loop step i, in registers
            if (!ns.seeded) m.z = ip->q_noise + (size_t)i * run.n1;
            const hipError_t e = launch_masked_blend(m, ns.seeded ? &g : nullptr, c->stream);
            if (ns.seeded && e == hipErrorInvalidValue) return c->fail(-1, "ddim inpaint (seeded): x0 must be 16-byte aligned");
            RDM_CHECK_HIP(c, e);
        }
        RDM_TRY(run.forward(index));
        DdimStepParams p{};
        p.x = run.x; p.eps = run.eps; p.noise = (ns.stack && a->eta != 0.f) ? ns.stack + (size_t)i * run.n1 : nullptr;
        p.x_prev = run.x; p.x_dup = run.x_dup; p.pred_x0 = run.pred_x0_slot(i);
        p.n_per_batch = run.n1; p.a_t = at[index]; p.a_prev = ap[index]; p.sigma_t = sg[index]; p.sqrt_one_minus_at = s1m[index];
        p.scale = a->unconditional_guidance_scale; p.temperature = a->temperature; p.cfg = cfg ? 1 : 0;
        const StepRngParams g = run.step_rng(ns.seed, i), *rng = (ns.seeded && a->eta != 0.f) ? &g : nullptr;   // the noise of loop step i, in registers
        if (rng) RDM_TRY(seeded_launched(c, "ddim", launch_ddim_step(p, rng, c->stream)));
        else RDM_CHECK_HIP(c, launch_ddim_step(p, nullptr, c->stream));
        RDM_TRY(run.log_x(i));
    }
    return run.finish(z_out);
}
int rdm_ddim_sample(rdm_ctx* c, const rdm_ddim_args* a, const float* x_T, const float* cond, const float* uncond,
                    const rdm_noise* noise, float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    NoiseSource ns;
    RDM_TRY(noise_source(c, "rdm_ddim_sample", noise, &ns));
    if (!a || (!x_T && !ns.seeded) || !cond || !z_out) return c->fail(-1, "null argument");
    return ddim_sample_impl(c, a, -1, x_T, cond, uncond, ns, z_out, x_inter, pred_x0_inter);
}

// ldm DDIMSampler.decode: the DDIM loop from a latent at level index t_start - 1
int rdm_ddim_decode(rdm_ctx* c, const rdm_ddim_args* a, int t_start, const float* x_latent, const float* cond, const float* uncond,
                    const rdm_noise* noise, float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    NoiseSource ns;
    RDM_TRY(noise_source(c, "rdm_ddim_decode", noise, &ns));
    if (!a || !x_latent || !cond || !z_out) return c->fail(-1, "null argument");
    if (t_start < 1) return c->fail(-1, "ddim decode: t_start must be at least 1, got %d", t_start);
    return ddim_sample_impl(c, a, t_start, x_latent, cond, uncond, ns, z_out, x_inter, pred_x0_inter);
}

// DDIM inpainting: rdm_ddim_decode's loop with the blend above before every forward
int rdm_ddim_inpaint(rdm_ctx* c, const rdm_ddim_args* a, int t_start, const float* x_latent, const float* x0, const float* mask, int mask_channels,
                     const float* cond, const float* uncond, const rdm_noise* noise, const float* q_noise, float* z_out, float* x_inter,
                     float* pred_x0_inter) {
    RDM_ENTER(c);
    NoiseSource ns;
    RDM_TRY(noise_source(c, "rdm_ddim_inpaint", noise, &ns));
    if (ns.seeded && q_noise) return c->fail(-1, "rdm_ddim_inpaint: give a seed or a q_noise stack, not both");
    if (!a || !x_latent || !x0 || !mask || (!q_noise && !ns.seeded) || !cond || !z_out) return c->fail(-1, "null argument");
    if (t_start < 1) return c->fail(-1, "ddim inpaint: t_start must be at least 1, got %d", t_start);
    const InpaintSource ip{x0, mask, mask_channels, q_noise};
    return ddim_sample_impl(c, a, t_start, x_latent, cond, uncond, ns, z_out, x_inter, pred_x0_inter, &ip);
}

// Deterministic DDIM inversion (rdm_ddim_encode's header comment): t_enc steps UP the schedule, step i from level a_prev[i] to a_t[i] with
// the UNet on the current iterate at the TARGET timestep ts[i].  The scalars are float64 square roots of the fp32 alphas, rounded.
int rdm_ddim_encode(rdm_ctx* c, const rdm_ddim_args* a, int t_enc, const float* x0, const float* cond, const float* uncond, float* z_out,
                    float* x_inter) {
    RDM_ENTER(c);
    if (!c || !a || !x0 || !cond || !z_out) return c ? c->fail(-1, "null argument") : -1;
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    if (a->eta != 0.f) return c->fail(-1, "ddim encode: eta must be 0 (the inversion is deterministic)");
    bool cfg;
    RDM_TRY(sampler_guidance(c, "ddim encode", a->unconditional_guidance_scale, uncond, &cfg));
    std::vector<int> ts; std::vector<float> at, ap, s1m;
    RDM_TRY(ddim_schedule(c, a, ts, at, ap, s1m));
    if (t_enc < 1 || t_enc > (int)ts.size()) return c->fail(-1, "ddim encode: t_enc must lie in [1, %d], got %d", (int)ts.size(), t_enc);
    ts.resize((size_t)t_enc);
    SamplerRun run;
    run.ascending = true;
    RDM_TRY(run.begin(c, a, ts, x0, cond, cfg ? uncond : nullptr, a->log_every_t, x_inter, nullptr, 0));
    for (int i = 0; i < t_enc; i++) {
        RDM_TRY(run.forward(i));
        const double ac = (double)ap[i], an = (double)at[i];
        DdimInverseStepParams p{};
        p.x = run.x; p.eps = run.eps; p.x_out = run.x; p.x_dup = run.x_dup; p.n = run.n1;
        p.sa_c = (float)std::sqrt(ac); p.s1m_c = (float)std::sqrt(1.0 - ac); p.sa_n = (float)std::sqrt(an); p.s1m_n = (float)std::sqrt(1.0 - an);
        p.scale = a->unconditional_guidance_scale; p.cfg = cfg ? 1 : 0;
        RDM_CHECK_HIP(c, launch_ddim_inverse_step(p, c->stream));
        RDM_TRY(run.log_x(i));
    }
    return run.finish(z_out);
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

// The float64 coefficients of one DPM-Solver++ step from node s to node t (h = lambda_t - lambda_s, h_prev the step before's):
// x <- c_x x + g D (+ c_n z), D = m0 or, at second order, (1 + 1/(2r)) m0 - (1/(2r)) m_prev with r = h_prev / h.
struct DpmppCoefficients { double c_x, c_0, c_1, c_n; };
static DpmppCoefficients dpmpp_coefficients(const SolverNode& s, const SolverNode& t, double h, double h_prev, bool second, bool sde) {
    DpmppCoefficients k{};
    double g;
    if (sde) {
        const double q = -std::expm1(-2.0 * h);       // q = 1 - exp(-2h)
        g = t.alpha * q; k.c_x = t.sigma / s.sigma * std::exp(-h); k.c_n = t.sigma * std::sqrt(q);
    } else {
        g = -t.alpha * std::expm1(-h); k.c_x = t.sigma / s.sigma;
    }
    if (second) {
        const double r = h_prev / h;
        k.c_0 = g * (1.0 + 1.0 / (2.0 * r)); k.c_1 = -g / (2.0 * r);
    } else {
        k.c_0 = g;
    }
    return k;
}

// The loop of rdm_dpmpp_sample (sde false: the ODE step, no noise) and of rdm_dpmpp_sde_sample (z_j is row j of ns.stack, or
// drawn in the step kernel at step counter j, and a null x_T is drawn): one forward and one step-kernel launch per step.  The history is
// ONE buffer: the kernel reads m_{j-1} from it and writes m_j to it in the same pass.  who: the solver's name in the messages.
static int dpmpp_sample_impl(rdm_ctx* c, const rdm_dpmpp_args* a, bool sde, const char* who, const NoiseSource& ns, const float* x_T,
                             const float* cond, const float* uncond, float* z_out, float* x_inter, float* pred_x0_inter) {
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    if (a->order != 1 && a->order != 2) return c->fail(-1, "%s order must be 1 or 2, got %d", who, a->order);
    bool cfg;
    RDM_TRY(sampler_guidance(c, who, a->unconditional_guidance_scale, uncond, &cfg));
    RDM_TRY(sampler_nodes(c, who, a->alphas_cumprod, a->T, a->nodes, a->n_nodes));
    RDM_TRY(check_seeded(c, who, ns, a));
    const int n_steps = a->n_nodes - 1;
    const std::vector<int> ts(a->nodes, a->nodes + n_steps);
    SamplerRun run;
    RDM_TRY(run.begin(c, a, ts, x_T, cond, cfg ? uncond : nullptr, a->log_every_t, x_inter, pred_x0_inter, 1));
    if (!x_T) RDM_TRY(run.draw_start(ns.seed));
    float* m_slot = run.extra[0];
    double h_prev = 0.0;
    for (int j = 0; j < n_steps; j++) {
        const SolverNode s = solver_node(a->alphas_cumprod, a->nodes[j]), t = solver_node(a->alphas_cumprod, a->nodes[j + 1]);
        const double h = t.lambda - s.lambda;
        const bool second = a->order == 2 && j >= 1 && !(a->lower_order_final && j == n_steps - 1);
        const DpmppCoefficients k = dpmpp_coefficients(s, t, h, h_prev, second, sde);
        RDM_TRY(run.forward(j));
        DpmppStepParams p{};
        p.x = run.x; p.eps = run.eps; p.n = run.n1; p.cfg = cfg ? 1 : 0; p.scale = a->unconditional_guidance_scale;
        p.sqrt_a_s = (float)s.alpha; p.sqrt_one_minus_a_s = (float)s.sigma;
        p.c_x = (float)k.c_x; p.c_0 = (float)k.c_0; p.c_1 = (float)k.c_1; p.c_n = (float)k.c_n;
        p.m_prev = second ? m_slot : nullptr; p.noise = ns.stack ? ns.stack + (size_t)j * run.n1 : nullptr;
        p.x_out = run.x; p.x_dup = run.x_dup; p.m_store = m_slot; p.pred_x0 = run.pred_x0_slot(j);
        const StepRngParams g = run.step_rng(ns.seed, j);         // seeded: the noise of loop step j, in registers
        if (ns.seeded) RDM_TRY(seeded_launched(c, who, launch_dpmpp_step(p, &g, c->stream)));
        else RDM_CHECK_HIP(c, launch_dpmpp_step(p, nullptr, c->stream));
        h_prev = h;
        RDM_TRY(run.log_x(j));
    }
    return run.finish(z_out);
}
int rdm_dpmpp_sample(rdm_ctx* c, const rdm_dpmpp_args* a, const float* x_T, const float* cond, const float* uncond,
                     float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    if (!c || !a || !x_T || !cond || !z_out || !a->alphas_cumprod || !a->nodes) return c ? c->fail(-1, "null argument") : -1;
    return dpmpp_sample_impl(c, a, false, "dpm-solver++", NoiseSource{}, x_T, cond, uncond, z_out, x_inter, pred_x0_inter);
}
int rdm_dpmpp_sde_sample(rdm_ctx* c, const rdm_dpmpp_args* a, const float* x_T, const float* cond, const float* uncond, const rdm_noise* noise,
                         float* z_out, float* x_inter, float* pred_x0_inter) {
    RDM_ENTER(c);
    NoiseSource ns;
    RDM_TRY(noise_source(c, "rdm_dpmpp_sde_sample", noise, &ns));
    if (!a || (!x_T && !ns.seeded) || !cond || ns.none() || !z_out || !a->alphas_cumprod || !a->nodes) return c->fail(-1, "null argument");
    return dpmpp_sample_impl(c, a, true, "sde-dpm-solver++", ns, x_T, cond, uncond, z_out, x_inter, pred_x0_inter);
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

// The ancestral loop of rdm_ddpm_sample (the noise stack ns.stack, or, seeded, generated in the step kernel; a null x_T is drawn).  The
// final step (i == 0) consumes no noise either way.
static int ddpm_sample_impl(rdm_ctx* c, const rdm_ddpm_args* a, const float* x_T, const float* cond, const NoiseSource& ns, float* z_out) {
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    if (a->timesteps < 1 || a->timesteps > a->T) return c->fail(-1, "bad timesteps");
    RDM_TRY(check_seeded(c, "ddpm", ns, a));
    const int T = a->timesteps;
    std::vector<int> ts(T);
    for (int i = 0; i < T; i++) ts[i] = i;
    SamplerRun run;
    RDM_TRY(run.begin(c, a, ts, x_T, cond, nullptr, 0, nullptr, nullptr, 0));
    if (!x_T) RDM_TRY(run.draw_start(ns.seed));
    for (int n = 0, i = T - 1; i >= 0; i--, n++) {
        RDM_TRY(run.forward(i));
        DdpmStepParams p{};
        p.x = run.x; p.eps = run.eps; p.noise = ns.stack ? ns.stack + (size_t)n * run.n1 : nullptr; p.x_prev = run.x; p.n = run.n1;
        p.sqrt_recip = a->sqrt_recip_alphas_cumprod[i]; p.sqrt_recipm1 = a->sqrt_recipm1_alphas_cumprod[i];
        p.coef1 = a->posterior_mean_coef1[i]; p.coef2 = a->posterior_mean_coef2[i]; p.log_var = a->posterior_log_variance_clipped[i];
        p.clip = a->clip_denoised; p.nonzero = (i != 0); p.temperature = a->temperature;
        const StepRngParams g = run.step_rng(ns.seed, n);         // seeded: the noise of loop step n, in registers
        RDM_CHECK_HIP(c, launch_ddpm_step(p, ns.seeded && p.nonzero ? &g : nullptr, c->stream));
    }
    return run.finish(z_out);
}
int rdm_ddpm_sample(rdm_ctx* c, const rdm_ddpm_args* a, const float* x_T, const float* cond, const rdm_noise* noise,
                    float* z_out) {
    RDM_ENTER(c);
    NoiseSource ns;
    RDM_TRY(noise_source(c, "rdm_ddpm_sample", noise, &ns));
    if (!a || (!x_T && !ns.seeded) || !cond || ns.none() || !z_out) return c->fail(-1, "null argument");
    return ddpm_sample_impl(c, a, x_T, cond, ns, z_out);
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

// ---- one guided forward the way the sampling loops run it: a one-step SamplerRun without an update (K/V projected once, the trailing
// zero-context rows and the B-row prefix of the doubled batch shared, the timestep's embedding row from the table).  eps_out: [2B] rows,
// cond | uncond.
int rdm_unet_forward_guided(rdm_ctx* c, const float* x, int64_t t, const float* cond, const float* uncond, int B, int k, int H, int W,
                            float* eps_out) {
    RDM_ENTER(c);
    if (!x || !cond || !uncond || !eps_out) return c->fail(-1, "null argument");
    if (!c->unet.loaded) return c->fail(-1, "unet weights not loaded");
    if (B < 1 || k < 1 || H < 1 || W < 1 || t < 0 || t > 0x7fffffffll)
        return c->fail(-1, "rdm_unet_forward_guided: bad shape B=%d k=%d H=%d W=%d or timestep %lld", B, k, H, W, (long long)t);
    rdm_ddim_args a{};
    a.batch = B; a.k = k; a.channels = c->unet.cfg.in_channels; a.height = H; a.width = W;
    SamplerRun run;
    RDM_TRY(run.begin(c, &a, std::vector<int>{(int)t}, x, cond, uncond, 1, nullptr, nullptr, 0));
    RDM_TRY(run.forward(0));
    RDM_CHECK_HIP(c, hipMemcpyAsync(eps_out, run.eps, (size_t)run.n1 * 2 * 4, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// ---- the inversion step and the seeded forward process alone
int rdm_op_ddim_inverse_step(rdm_ctx* c, const float* x, const float* eps, long long n, int cfg, float scale, float sqrt_a_cur,
                             float sqrt_one_minus_a_cur, float sqrt_a_next, float sqrt_one_minus_a_next, float* x_out, float* x_dup, float* pred_x0) {
    RDM_ENTER(c);
    if (!x || !eps || !x_out || n < 1) return c->fail(-1, "rdm_op_ddim_inverse_step: bad argument");
    DdimInverseStepParams p{};
    p.x = x; p.eps = eps; p.x_out = x_out; p.x_dup = x_dup; p.pred_x0 = pred_x0; p.n = n; p.cfg = cfg ? 1 : 0; p.scale = scale;
    p.sa_c = sqrt_a_cur; p.s1m_c = sqrt_one_minus_a_cur; p.sa_n = sqrt_a_next; p.s1m_n = sqrt_one_minus_a_next;
    RDM_CHECK_HIP(c, launch_ddim_inverse_step(p, c->stream));
    return 0;
}
int rdm_op_q_sample_seeded(rdm_ctx* c, const float* x0, int64_t B, int64_t per_row, float sqrt_a, float sqrt_1ma, uint64_t seed, int64_t row0,
                           float* out) {
    RDM_ENTER(c);
    if (!c) return -1;
    if (!x0 || !out) return c->fail(-1, "rdm_op_q_sample_seeded: null argument");
    RDM_TRY(check_noise_rows(c, "rdm_op_q_sample_seeded", row0, B, per_row));
    const QSampleSeededParams p{x0, out, seed, B, per_row, (uint32_t)row0, sqrt_a, sqrt_1ma};
    const hipError_t e = launch_q_sample_seeded(p, c->stream);
    if (e == hipErrorInvalidValue) return c->fail(-1, "rdm_op_q_sample_seeded: per_row must be a multiple of 4 and x0, out 16-byte aligned");
    RDM_CHECK_HIP(c, e);
    return 0;
}

// ---- the inpainting blend alone
static int masked_blend_fill(rdm_ctx* c, const char* who, MaskedBlendParams& p, const float* x, const float* x0, const float* mask, int64_t B,
                             int C, int H, int W, int mask_channels, float sqrt_a, float sqrt_1ma, float* out, float* x_dup) {
    if (!x || !x0 || !mask || !out) return c->fail(-1, "%s: null argument", who);
    if (B < 1 || C < 1 || H < 1 || W < 1 || B > (1ll << 40) / ((long long)C * H * W))
        return c->fail(-1, "%s: bad shape B=%lld C=%d H=%d W=%d", who, (long long)B, C, H, W);
    if (mask_channels != 1 && mask_channels != C) return c->fail(-1, "%s: mask_channels must be 1 or C = %d, got %d", who, C, mask_channels);
    p.x = x; p.x0 = x0; p.mask = mask; p.out = out; p.x_dup = x_dup;
    p.hw = (long long)H * W; p.chw = p.hw * C; p.n = p.chw * B; p.mask_channels = mask_channels; p.sqrt_a = sqrt_a; p.sqrt_1ma = sqrt_1ma;
    return 0;
}
int rdm_op_masked_blend(rdm_ctx* c, const float* x, const float* x0, const float* mask, const rdm_noise* z, int64_t B, int C, int H, int W,
                        int mask_channels, float sqrt_a, float sqrt_1ma, float* out, float* x_dup) {
    RDM_ENTER(c);
    NoiseSource ns;
    RDM_TRY(noise_source(c, "rdm_op_masked_blend", z, &ns));
    MaskedBlendParams p{};
    RDM_TRY(masked_blend_fill(c, "rdm_op_masked_blend", p, x, x0, mask, B, C, H, W, mask_channels, sqrt_a, sqrt_1ma, out, x_dup));
    p.z = ns.stack;
    StepRngParams g{};
    if (ns.seeded) {
        RDM_TRY(check_noise_rows(c, "rdm_op_masked_blend (seeded)", z->row0, B, p.chw));
        g = {z->seed, p.chw, (uint32_t)z->row0, z->step};
    }
    const hipError_t e = launch_masked_blend(p, ns.seeded ? &g : nullptr, c->stream);
    if (ns.seeded && e == hipErrorInvalidValue)
        return c->fail(-1, "rdm_op_masked_blend (seeded): C * H * W must be a multiple of 4, and x, x0, out, x_dup 16-byte aligned");
    RDM_CHECK_HIP(c, e);
    return 0;
}

// ---- the DDIM, PLMS and DDPM step kernels alone: the kernels' own scalars, as the loops above fill them
// The noise of a step op entry `who`: ns from its rdm_noise argument and, seeded, the row check of n / per_row rows and the kernel's counters in *g
static int op_step_noise(rdm_ctx* c, const char* who, const rdm_noise* noise, long long n, NoiseSource* ns, StepRngParams* g) {
    RDM_TRY(noise_source(c, who, noise, ns));
    if (!ns->seeded) return 0;
    const std::string w = std::string(who) + " (seeded)";
    RDM_TRY(check_noise_rows(c, w.c_str(), noise->row0, noise->per_row >= 1 ? n / noise->per_row : 0, noise->per_row));
    *g = {noise->seed, noise->per_row, (uint32_t)noise->row0, noise->step};
    return 0;
}
// ... and its launch: what a seeded step kernel, which has no scalar form, asks of the call's shape
static int op_step_launched(rdm_ctx* c, const char* who, const NoiseSource& ns, hipError_t e) {
    if (ns.seeded && e == hipErrorInvalidValue)
        return c->fail(-1, "%s (seeded): per_row must be a multiple of 4 that divides n, and every operand 16-byte aligned", who);
    RDM_CHECK_HIP(c, e);
    return 0;
}
static void ddim_step_fill(DdimStepParams& p, const float* x, const float* eps, long long n, int cfg, float scale, float a_t, float a_prev,
                           float sigma_t, float sqrt_one_minus_at, float temperature, float* x_prev, float* x_dup, float* pred_x0) {
    p.x = x; p.eps = eps; p.x_prev = x_prev; p.x_dup = x_dup; p.pred_x0 = pred_x0; p.n_per_batch = n; p.cfg = cfg ? 1 : 0; p.scale = scale;
    p.a_t = a_t; p.a_prev = a_prev; p.sigma_t = sigma_t; p.sqrt_one_minus_at = sqrt_one_minus_at; p.temperature = temperature;
}
int rdm_op_ddim_step(rdm_ctx* c, const float* x, const float* eps, const rdm_noise* noise, long long n, int cfg, float scale, float a_t,
                     float a_prev, float sigma_t, float sqrt_one_minus_at, float temperature, float* x_prev, float* x_dup, float* pred_x0) {
    RDM_ENTER(c);
    if (!x || !eps || !x_prev || n < 1) return c->fail(-1, "rdm_op_ddim_step: bad argument");
    NoiseSource ns; StepRngParams g{};
    RDM_TRY(op_step_noise(c, "rdm_op_ddim_step", noise, n, &ns, &g));
    DdimStepParams p{};
    ddim_step_fill(p, x, eps, n, cfg, scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, temperature, x_prev, x_dup, pred_x0);
    p.noise = ns.stack;
    return op_step_launched(c, "rdm_op_ddim_step", ns, launch_ddim_step(p, ns.seeded ? &g : nullptr, c->stream));
}

int rdm_op_plms_step(rdm_ctx* c, const float* x, const float* eps, const float* e_prev, const float* h1, const float* h2, const float* h3,
                     long long n, int cfg, float scale, float a_t, float a_prev, float sqrt_one_minus_at, int mode, int order, float* e_store,
                     float* x_out, float* x_dup, float* pred_x0) {
    RDM_ENTER(c);
    if (!x || !eps || !x_out || n < 1) return c->fail(-1, "rdm_op_plms_step: bad argument");
    if (mode != PLMS_STEP && mode != PLMS_EULER_A && mode != PLMS_EULER_B) return c->fail(-1, "rdm_op_plms_step: mode %d is none of 0 (step), 1 (Euler A), 2 (Euler B)", mode);
    if (order < 0 || order > 3) return c->fail(-1, "rdm_op_plms_step: order %d outside 0..3", order);
    if (mode == PLMS_EULER_B && !e_prev) return c->fail(-1, "rdm_op_plms_step: Euler B reads e_prev, which is null");
    if (mode == PLMS_STEP && ((order >= 1 && !h1) || (order >= 2 && !h2) || (order >= 3 && !h3)))
        return c->fail(-1, "rdm_op_plms_step: order %d needs history operands that are null", order);
    if (mode != PLMS_EULER_B && !e_store) return c->fail(-1, "rdm_op_plms_step: mode %d writes e_store, which is null", mode);
    PlmsStepParams p{};
    p.x = x; p.eps = eps; p.e_prev = e_prev; p.h1 = h1; p.h2 = h2; p.h3 = h3; p.n = n; p.cfg = cfg ? 1 : 0; p.scale = scale;
    p.a_t = a_t; p.a_prev = a_prev; p.sqrt_one_minus_at = sqrt_one_minus_at; p.mode = mode; p.order = order;
    p.e_store = e_store; p.x_out = x_out; p.x_dup = x_dup; p.pred_x0 = pred_x0;
    RDM_CHECK_HIP(c, launch_plms_step(p, c->stream));
    return 0;
}

static void ddpm_step_fill(DdpmStepParams& p, const float* x, const float* eps, long long n, float sqrt_recip, float sqrt_recipm1, float coef1,
                           float coef2, float log_var, int clip, int nonzero, float temperature, float* x_prev) {
    p.x = x; p.eps = eps; p.x_prev = x_prev; p.n = n; p.sqrt_recip = sqrt_recip; p.sqrt_recipm1 = sqrt_recipm1; p.coef1 = coef1; p.coef2 = coef2;
    p.log_var = log_var; p.clip = clip ? 1 : 0; p.nonzero = nonzero ? 1 : 0; p.temperature = temperature;
}
int rdm_op_ddpm_step(rdm_ctx* c, const float* x, const float* eps, const rdm_noise* noise, long long n, float sqrt_recip, float sqrt_recipm1,
                     float coef1, float coef2, float log_var, int clip, int nonzero, float temperature, float* x_prev) {
    RDM_ENTER(c);
    if (!x || !eps || !x_prev || n < 1) return c->fail(-1, "rdm_op_ddpm_step: bad argument");
    NoiseSource ns; StepRngParams g{};
    RDM_TRY(op_step_noise(c, "rdm_op_ddpm_step", noise, n, &ns, &g));
    if (nonzero && ns.none()) return c->fail(-1, "rdm_op_ddpm_step: nonzero needs a noise operand (a stack or a seed)");
    DdpmStepParams p{};
    ddpm_step_fill(p, x, eps, n, sqrt_recip, sqrt_recipm1, coef1, coef2, log_var, clip, nonzero, temperature, x_prev);
    p.noise = ns.stack;
    return op_step_launched(c, "rdm_op_ddpm_step", ns, launch_ddpm_step(p, ns.seeded ? &g : nullptr, c->stream));
}

// ---- the DPM-Solver++ and UniPC step kernels alone
static void dpmpp_step_fill(DpmppStepParams& p, const float* x, const float* eps, const float* m_prev, const float* noise, long long n, int cfg,
                            float scale, float sqrt_a_s, float sqrt_one_minus_a_s, float c_x, float c_0, float c_1, float c_n, float* x_out,
                            float* x_dup, float* m_store, float* pred_x0) {
    p.x = x; p.eps = eps; p.m_prev = m_prev; p.noise = noise; p.n = n; p.cfg = cfg ? 1 : 0; p.scale = scale; p.sqrt_a_s = sqrt_a_s;
    p.sqrt_one_minus_a_s = sqrt_one_minus_a_s; p.c_x = c_x; p.c_0 = c_0; p.c_1 = c_1; p.c_n = c_n;
    p.x_out = x_out; p.x_dup = x_dup; p.m_store = m_store; p.pred_x0 = pred_x0;
}
int rdm_op_dpmpp_step(rdm_ctx* c, const float* x, const float* eps, const float* m_prev, long long n, int cfg, float scale, float sqrt_a_s,
                      float sqrt_one_minus_a_s, float c_x, float c_0, float c_1, float* x_out, float* x_dup, float* m_store, float* pred_x0) {
    RDM_ENTER(c);
    if (!x || !eps || !x_out || n < 1) return c->fail(-1, "rdm_op_dpmpp_step: bad argument");
    DpmppStepParams p{};
    dpmpp_step_fill(p, x, eps, m_prev, nullptr, n, cfg, scale, sqrt_a_s, sqrt_one_minus_a_s, c_x, c_0, c_1, 0.f, x_out, x_dup, m_store, pred_x0);
    RDM_CHECK_HIP(c, launch_dpmpp_step(p, nullptr, c->stream));
    return 0;
}
int rdm_op_dpmpp_sde_step(rdm_ctx* c, const float* x, const float* eps, const float* m_prev, const rdm_noise* noise, long long n, int cfg,
                          float scale, float sqrt_a_s, float sqrt_one_minus_a_s, float c_x, float c_0, float c_1, float c_n, float* x_out, float* x_dup,
                          float* m_store, float* pred_x0) {
    RDM_ENTER(c);
    if (!x || !eps || !x_out || n < 1) return c->fail(-1, "rdm_op_dpmpp_sde_step: bad argument");
    NoiseSource ns; StepRngParams g{};
    RDM_TRY(op_step_noise(c, "rdm_op_dpmpp_sde_step", noise, n, &ns, &g));
    if (ns.none()) return c->fail(-1, "rdm_op_dpmpp_sde_step: bad argument");
    DpmppStepParams p{};
    dpmpp_step_fill(p, x, eps, m_prev, ns.stack, n, cfg, scale, sqrt_a_s, sqrt_one_minus_a_s, c_x, c_0, c_1, c_n, x_out, x_dup, m_store, pred_x0);
    return op_step_launched(c, "rdm_op_dpmpp_sde_step", ns, launch_dpmpp_step(p, ns.seeded ? &g : nullptr, c->stream));
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
