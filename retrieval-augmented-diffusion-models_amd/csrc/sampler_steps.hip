// The sampling update kernels (DDIM, PLMS, DPM-Solver++ and its SDE form, UniPC, DDIM inversion, DDPM), their seeded forms, the
// device-noise kernels and, at the end, the inpainting blend with its seeded form (gfx950).
#include "kernels.h"
#include "philox.h"

// ------------------------------------------------------------------ DDIM / DDPM updates (fp32)
// rdm/models/diffusion/ddim.py:229-238 (CFG combine) + :253-267 (update), fused into one pass.
// eps holds [B] rows (scale == 1) or [2B] rows (cond | uncond). Scalars are the fp32 values the
// reference materialises with torch.full_like; sqrt taken in fp32 on device like a_t.sqrt().
__global__ void ddim_step_kernel(DdimStepParams p) {
    const float sa = sqrtf(p.a_t), sap = sqrtf(p.a_prev);
    const float dirc = sqrtf(1.0f - p.a_prev - p.sigma_t * p.sigma_t);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n_per_batch;
         i += (long long)gridDim.x * blockDim.x) {
        float e = p.eps[i];
        if (p.cfg) { const float eu = p.eps[p.n_per_batch + i]; e = eu + p.scale * (e - eu); }
        const float x = p.x[i];
        const float x0 = (x - p.sqrt_one_minus_at * e) / sa;
        const float dir = dirc * e;
        const float nz = p.noise ? p.sigma_t * p.noise[i] * p.temperature : 0.f;
        const float xp = sap * x0 + dir + nz;
        p.x_prev[i] = xp;
        if (p.x_dup) p.x_dup[i] = xp;
        if (p.pred_x0) p.pred_x0[i] = x0;
    }
}

// ------------------------------------------------------------------ what the PLMS, DPM-Solver++ and UniPC step kernels share
template <int V> __device__ __forceinline__ void step_ld(const float* p, long long i, float (&v)[V]) {
    if constexpr (V == 4) { const float4 t = *(const float4*)(p + i); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = p[i];
}
template <int V> __device__ __forceinline__ void step_st(float* p, long long i, const float (&v)[V]) {
    if constexpr (V == 4) *(float4*)(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    else p[i] = v[0];
}
// The guided eps of the PLMS, DPM-Solver++ and UniPC passes: e of the cond rows, or u + scale (e - u) with u the uncond rows n further on
// (cfg).  The contraction pragma holds for the function body it is written in, so this helper carries its own.
template <int V> __device__ __forceinline__ void step_guided_eps(const float* eps, long long n, long long i, int cfg, float scale, float (&e)[V]) {
#pragma clang fp contract(off)
    step_ld<V>(eps, i, e);
    if (cfg) {
        float u[V]; step_ld<V>(eps + n, i, u);
#pragma unroll
        for (int k = 0; k < V; k++) e[k] = u[k] + scale * (e[k] - u[k]);
    }
}
// One launch of a step kernel over n elements: the float4 instantiation k4 when n % 4 == 0 and every operand is 16-byte aligned (null
// is), else the scalar k1; 256 threads on at most 2048 blocks.
template <class P>
static hipError_t launch_step(long long n, std::initializer_list<const void*> ptrs, const P& p, void (*k4)(P), void (*k1)(P), hipStream_t st) {
    if (n <= 0) return hipSuccess;
    bool vec = n % 4 == 0;
    for (const void* q : ptrs) vec = vec && ((uintptr_t)q % 16 == 0);
    const long long nv = vec ? n / 4 : n;
    const int grid = (int)std::min<long long>((nv + 255) / 256, 2048);
    (vec ? k4 : k1)<<<grid, 256, 0, st>>>(p);
    return hipGetLastError();
}

// ------------------------------------------------------------------ PLMS update (fp32, eta = 0)
// ldm PLMSSampler.p_sample_plms: CFG combine, the linear-multistep combination of e_t with up to three earlier e_t, and the DDIM
// update (get_x_prev_and_pred_x0 with sigma_t = 0), one pass per step.  Same association, true divisions and no FMA contraction as the
// torch expressions, so a torch restatement agrees to rounding.  V = 4: float4 accesses (the launcher checks n % 4 and alignment).
template <int V>
__global__ __launch_bounds__(256) void plms_step_kernel(PlmsStepParams p) {
#pragma clang fp contract(off)
    const float sa = sqrtf(p.a_t), sap = sqrtf(p.a_prev), s1p = sqrtf(1.0f - p.a_prev);
    const long long nv = p.n / V;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * V;
        float e[V], x[V], o[V];
        step_guided_eps<V>(p.eps, p.n, i, p.cfg, p.scale, e);
        step_ld<V>(p.x, i, x);
        if (p.mode == PLMS_EULER_B) {
            float q[V]; step_ld<V>(p.e_prev, i, q);
#pragma unroll
            for (int k = 0; k < V; k++) o[k] = (q[k] + e[k]) / 2.0f;
        } else {
#pragma unroll
            for (int k = 0; k < V; k++) o[k] = e[k];
            if (p.mode == PLMS_STEP && p.order >= 1) {
                float a[V]; step_ld<V>(p.h1, i, a);
                if (p.order == 1) {
#pragma unroll
                    for (int k = 0; k < V; k++) o[k] = (3.0f * e[k] - a[k]) / 2.0f;
                } else {
                    float b[V]; step_ld<V>(p.h2, i, b);
                    if (p.order == 2) {
#pragma unroll
                        for (int k = 0; k < V; k++) o[k] = (23.0f * e[k] - 16.0f * a[k] + 5.0f * b[k]) / 12.0f;
                    } else {
                        float c[V]; step_ld<V>(p.h3, i, c);
#pragma unroll
                        for (int k = 0; k < V; k++) o[k] = (55.0f * e[k] - 59.0f * a[k] + 37.0f * b[k] - 9.0f * c[k]) / 24.0f;
                    }
                }
            }
            step_st<V>(p.e_store, i, e);          // after the history reads: e_store may be h3's slot
        }
        float xo[V], x0[V];
#pragma unroll
        for (int k = 0; k < V; k++) { x0[k] = (x[k] - p.sqrt_one_minus_at * o[k]) / sa; xo[k] = sap * x0[k] + s1p * o[k]; }
        step_st<V>(p.x_out, i, xo);
        if (p.x_dup) step_st<V>(p.x_dup, i, xo);
        if (p.pred_x0) step_st<V>(p.pred_x0, i, x0);
    }
}
hipError_t launch_plms_step(const PlmsStepParams& p, hipStream_t st) {
    return launch_step(p.n, {p.x, p.eps, p.eps + (p.cfg ? p.n : 0), p.e_prev, p.h1, p.h2, p.h3, p.e_store, p.x_out, p.x_dup, p.pred_x0}, p,
                       plms_step_kernel<4>, plms_step_kernel<1>, st);
}

// ------------------------------------------------------------------ DPM-Solver++ update, ODE and SDE (fp32)
// Lu et al. 2022 (DPM-Solver++, multistep data prediction; ldm models/diffusion/dpm_solver/dpm_solver.py multistep_dpm_solver_update
// with algorithm_type "dpmsolver++" / "sde-dpmsolver++"): CFG combine, m0 = (x - sigma_s e) / alpha_s, and
// x_out = ((c_x x + c_0 m0) + c_1 m_prev) + c_n z, one pass per step with the coefficients the host computes in float64
// (dpmpp_sample_impl); the ODE step (NOISE false) has no fourth term.  True divisions, no FMA contraction, the sum taken left to right.
// m_store may be m_prev's own slot: a thread reads its elements of m_prev before it writes m_store and no other thread touches them, so
// the loop keeps ONE history slot.  dpmpp_update is the element arithmetic of the three kernels: dpmpp_step_kernel has no z,
// dpmpp_sde_step_kernel reads it from memory, dpmpp_sde_step_seeded_kernel (with the device-noise kernels) draws it in registers, and
// the two SDE forms then round alike.  V = 4: float4 accesses (the launcher checks n % 4 and alignment).
template <int V, bool NOISE>
__device__ __forceinline__ void dpmpp_update(const DpmppStepParams& p, long long i, const float (&z)[V]) {
#pragma clang fp contract(off)
    float e[V], x[V], m0[V], xo[V];
    step_guided_eps<V>(p.eps, p.n, i, p.cfg, p.scale, e);
    step_ld<V>(p.x, i, x);
#pragma unroll
    for (int k = 0; k < V; k++) { m0[k] = (x[k] - p.sqrt_one_minus_a_s * e[k]) / p.sqrt_a_s; xo[k] = p.c_x * x[k] + p.c_0 * m0[k]; }
    if (p.m_prev) {
        float q[V]; step_ld<V>(p.m_prev, i, q);
#pragma unroll
        for (int k = 0; k < V; k++) xo[k] = xo[k] + p.c_1 * q[k];
    }
    if constexpr (NOISE) {
#pragma unroll
        for (int k = 0; k < V; k++) xo[k] = xo[k] + p.c_n * z[k];
    }
    if (p.m_store) step_st<V>(p.m_store, i, m0);          // after the m_prev read: m_store may be that slot
    step_st<V>(p.x_out, i, xo);
    if (p.x_dup) step_st<V>(p.x_dup, i, xo);
    if (p.pred_x0) step_st<V>(p.pred_x0, i, m0);
}
template <int V>
__global__ __launch_bounds__(256) void dpmpp_step_kernel(DpmppStepParams p) {
    const long long nv = p.n / V;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const float none[V] = {};
        dpmpp_update<V, false>(p, v * V, none);
    }
}
template <int V>
__global__ __launch_bounds__(256) void dpmpp_sde_step_kernel(DpmppStepParams p) {
    const long long nv = p.n / V;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * V;
        float z[V]; step_ld<V>(p.noise, i, z);
        dpmpp_update<V, true>(p, i, z);
    }
}

// ------------------------------------------------------------------ UniPC predict-and-correct (fp32)
// Zhao et al. 2023 (UniPC, data prediction, multistep): after the forward at node j one pass forms m = (u - sigma_j e) / alpha_j from
// the guided eps, corrects the kept iterate, xc = a_x xc_prev + a_t m + a_1 h1 + a_2 h2 + a_3 h3 (order_c history terms; order_c == 0:
// xc = u), and predicts the next UNet input, u_next = b_x xc + b_0 m + b_1 h1 + b_2 h2 (order_p - 1 history terms), with the nine
// coefficients the host computes in float64 (rdm_unipc_coefficients).  True divisions, no FMA contraction, both sums taken left to
// right.  A thread reads its elements of u, xc_prev and the history before it writes any output and no other thread touches them, so
// u_next may be u, xc_out may be xc_prev, and m_store may be the oldest history slot (the ring rotates by pointer, as PLMS's does).
// V = 4: float4 accesses (the launcher checks n % 4 and alignment).
template <int V>
__global__ __launch_bounds__(256) void unipc_step_kernel(UnipcStepParams p) {
#pragma clang fp contract(off)
    const long long nv = p.n / V;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * V;
        float e[V], u[V], m[V], xc[V], un[V], h1[V], h2[V], h3[V];
        step_guided_eps<V>(p.eps, p.n, i, p.cfg, p.scale, e);
        step_ld<V>(p.u, i, u);
        const int nh = p.order_c > p.order_p - 1 ? p.order_c : p.order_p - 1;        // history slots this pass reads
        if (nh >= 1) step_ld<V>(p.h1, i, h1);
        if (nh >= 2) step_ld<V>(p.h2, i, h2);
        if (nh >= 3) step_ld<V>(p.h3, i, h3);
#pragma unroll
        for (int k = 0; k < V; k++) m[k] = (u[k] - p.sigma * e[k]) / p.alpha;
        if (p.order_c >= 1) {
            float xp[V]; step_ld<V>(p.xc_prev, i, xp);
#pragma unroll
            for (int k = 0; k < V; k++) {
                xc[k] = p.a_x * xp[k] + p.a_t * m[k];
                xc[k] = xc[k] + p.a_1 * h1[k];
                if (p.order_c >= 2) xc[k] = xc[k] + p.a_2 * h2[k];
                if (p.order_c >= 3) xc[k] = xc[k] + p.a_3 * h3[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; k++) xc[k] = u[k];
        }
#pragma unroll
        for (int k = 0; k < V; k++) {
            un[k] = p.b_x * xc[k] + p.b_0 * m[k];
            if (p.order_p >= 2) un[k] = un[k] + p.b_1 * h1[k];
            if (p.order_p >= 3) un[k] = un[k] + p.b_2 * h2[k];
        }
        if (p.m_store) step_st<V>(p.m_store, i, m);           // after the history reads: m_store may be h3's slot
        if (p.xc_out) step_st<V>(p.xc_out, i, xc);            // after the xc_prev read: xc_out may be that slot
        step_st<V>(p.u_next, i, un);
        if (p.x_dup) step_st<V>(p.x_dup, i, un);
        if (p.pred_x0) step_st<V>(p.pred_x0, i, m);
    }
}
hipError_t launch_unipc_step(const UnipcStepParams& p, hipStream_t st) {
    return launch_step(p.n, {p.u, p.eps, p.eps + (p.cfg ? p.n : 0), p.xc_prev, p.h1, p.h2, p.h3, p.xc_out, p.u_next, p.x_dup, p.m_store, p.pred_x0}, p, unipc_step_kernel<4>, unipc_step_kernel<1>, st);
}

// ------------------------------------------------------------------ DDIM inversion step (fp32, eta = 0)
// One step UP the schedule (rdm_ddim_encode; Song et al. 2021's ODE run in reverse, the form of ldm DDIMSampler.encode): CFG combine,
// pred_x0 = (x - s1m_c e) / sa_c at the CURRENT level, x_out = sa_n pred_x0 + s1m_n e at the NEXT one, the four scalars computed by the
// host in float64.  True division, no FMA contraction, as the other step kernels.  x_out may be x.  V = 4: float4 accesses (the launcher
// checks n % 4 and alignment).
template <int V>
__global__ __launch_bounds__(256) void ddim_inverse_step_kernel(DdimInverseStepParams p) {
#pragma clang fp contract(off)
    const long long nv = p.n / V;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * V;
        float e[V], x[V], x0[V], xo[V];
        step_guided_eps<V>(p.eps, p.n, i, p.cfg, p.scale, e);
        step_ld<V>(p.x, i, x);
#pragma unroll
        for (int k = 0; k < V; k++) { x0[k] = (x[k] - p.s1m_c * e[k]) / p.sa_c; xo[k] = p.sa_n * x0[k] + p.s1m_n * e[k]; }
        step_st<V>(p.x_out, i, xo);
        if (p.x_dup) step_st<V>(p.x_dup, i, xo);
        if (p.pred_x0) step_st<V>(p.pred_x0, i, x0);
    }
}
hipError_t launch_ddim_inverse_step(const DdimInverseStepParams& p, hipStream_t st) {
    return launch_step(p.n, {p.x, p.eps, p.eps + (p.cfg ? p.n : 0), p.x_out, p.x_dup, p.pred_x0}, p, ddim_inverse_step_kernel<4>,
                       ddim_inverse_step_kernel<1>, st);
}

// ldm LatentDiffusion.p_sample: x0 = c_recip*x - c_recipm1*eps; clamp; mean; + sigma*z
__global__ void ddpm_step_kernel(DdpmStepParams p) {
    const float sd = p.nonzero ? expf(0.5f * p.log_var) : 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (long long)gridDim.x * blockDim.x) {
        const float x = p.x[i];
        float x0 = p.sqrt_recip * x - p.sqrt_recipm1 * p.eps[i];
        if (p.clip) x0 = fminf(1.f, fmaxf(-1.f, x0));
        const float mean = p.coef1 * x0 + p.coef2 * x;
        p.x_prev[i] = mean + (p.nonzero ? sd * p.noise[i] * p.temperature : 0.f);
    }
}

// ------------------------------------------------------------------ device noise (philox.h)
// One element of the DDIM / DDPM update on a noise value z held in a register: the expressions of ddim_step_kernel / ddpm_step_kernel, term
// for term.  Those two kernels keep their own text (routed through these functions hipcc vectorises their kernel-argument loads and
// un-fuses two of ddpm_step_kernel's FMAs: other bits), and add the noise term after a branch, so never fused into the sum; here it is
// always present, and joins the sum in a block without FMA contraction.  Both forms then round alike.
struct DdimStepScalars { float sa, sap, dirc; };
__device__ __forceinline__ DdimStepScalars ddim_step_scalars(const DdimStepParams& p) {
    return {sqrtf(p.a_t), sqrtf(p.a_prev), sqrtf(1.0f - p.a_prev - p.sigma_t * p.sigma_t)};
}
__device__ __forceinline__ float ddim_update(const DdimStepParams& p, const DdimStepScalars& s, float e, float eu, float x, float z, float& x0) {
    if (p.cfg) e = eu + p.scale * (e - eu);
    x0 = (x - p.sqrt_one_minus_at * e) / s.sa;
    const float dir = s.dirc * e;
    const float nz = p.sigma_t * z * p.temperature;
    const float det = s.sap * x0 + dir;
    {
#pragma clang fp contract(off)
        return det + nz;
    }
}
__device__ __forceinline__ float ddpm_update(const DdpmStepParams& p, float sd, float x, float eps, float z) {
    float x0 = p.sqrt_recip * x - p.sqrt_recipm1 * eps;
    if (p.clip) x0 = fminf(1.f, fmaxf(-1.f, x0));
    const float mean = p.coef1 * x0 + p.coef2 * x;
    const float nz = p.nonzero ? sd * z * p.temperature : 0.f;
    {
#pragma clang fp contract(off)
        return mean + nz;
    }
}
// The DDIM / DDPM / SDE-DPM-Solver++ updates with the step's noise generated in registers, in the pass that applies it: a thread takes ONE
// Philox block -- four consecutive elements of one sample row (per_row % 4 == 0: rows never share a block) -- derives (row, block) from
// its flat vector index, and applies the update to the four normals.  The loops are bit-identical to stack loops fed with rdm_op_randn's
// output (tests/test_gpu_device_noise.py, tests/test_gpu_dpmpp_sde.py hold them to that).  float4 accesses throughout (the launcher
// checks alignment).  The three kernels write the (row, block) derivation out: behind a shared device function hipcc schedules all
// three differently, and most of the DDIM / DDPM arithmetic has no contraction pragma to pin its rounding (profiles/sampler_steps_split_isa.log).
__global__ __launch_bounds__(256) void ddim_step_seeded_kernel(DdimStepParams p, StepRngParams g) {
    const DdimStepScalars s = ddim_step_scalars(p);
    const long long nv = p.n_per_batch >> 2, bpr = g.per_row >> 2;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * 4, r = v / bpr;
        float z[4], e[4], u[4] = {}, x[4], xp[4], x0[4];
        philox_normal4(g.seed, (uint32_t)(v - r * bpr), g.step, g.row0 + (uint32_t)r, RDM_RNG_STREAM_STEP, z);
        step_ld<4>(p.eps, i, e);
        if (p.cfg) step_ld<4>(p.eps + p.n_per_batch, i, u);
        step_ld<4>(p.x, i, x);
#pragma unroll
        for (int k = 0; k < 4; k++) xp[k] = ddim_update(p, s, e[k], u[k], x[k], z[k], x0[k]);
        step_st<4>(p.x_prev, i, xp);
        if (p.x_dup) step_st<4>(p.x_dup, i, xp);
        if (p.pred_x0) step_st<4>(p.pred_x0, i, x0);
    }
}
__global__ __launch_bounds__(256) void ddpm_step_seeded_kernel(DdpmStepParams p, StepRngParams g) {
    const float sd = p.nonzero ? expf(0.5f * p.log_var) : 0.f;
    const long long nv = p.n >> 2, bpr = g.per_row >> 2;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * 4, r = v / bpr;
        float z[4], e[4], x[4], xp[4];
        philox_normal4(g.seed, (uint32_t)(v - r * bpr), g.step, g.row0 + (uint32_t)r, RDM_RNG_STREAM_STEP, z);
        step_ld<4>(p.eps, i, e);
        step_ld<4>(p.x, i, x);
#pragma unroll
        for (int k = 0; k < 4; k++) xp[k] = ddpm_update(p, sd, x[k], e[k], z[k]);
        step_st<4>(p.x_prev, i, xp);
    }
}
// The SDE-DPM-Solver++ update on noise drawn in registers: ddim_step_seeded_kernel's (row, block) derivation, dpmpp_update's arithmetic
__global__ __launch_bounds__(256) void dpmpp_sde_step_seeded_kernel(DpmppStepParams p, StepRngParams g) {
    const long long nv = p.n >> 2, bpr = g.per_row >> 2;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long r = v / bpr;
        float z[4];
        philox_normal4(g.seed, (uint32_t)(v - r * bpr), g.step, g.row0 + (uint32_t)r, RDM_RNG_STREAM_STEP, z);
        dpmpp_update<4, true>(p, v * 4, z);
    }
}
// The seeded step kernels have no scalar form: n and per_row multiples of 4 (per_row dividing n), every operand 16-byte aligned.
static bool seeded_step_ok(long long n, long long per_row, std::initializer_list<const void*> ptrs) {
    bool ok = n > 0 && per_row > 0 && per_row % 4 == 0 && n % per_row == 0;
    for (const void* q : ptrs) ok = ok && ((uintptr_t)q % 16 == 0);
    return ok;
}
// One launch of a seeded step kernel over n elements, launch_step's counterpart: hipErrorInvalidValue unless seeded_step_ok
template <class P>
static hipError_t launch_step_seeded(long long n, std::initializer_list<const void*> ptrs, const P& p, const StepRngParams& g,
                                     void (*k)(P, StepRngParams), hipStream_t st) {
    if (!seeded_step_ok(n, g.per_row, ptrs)) return hipErrorInvalidValue;
    const int grid = (int)std::min<long long>((n / 4 + 255) / 256, 2048);
    k<<<grid, 256, 0, st>>>(p, g);
    return hipGetLastError();
}
// The launchers of the three updates: rng null -> the kernel that reads p.noise (the ODE step when that is null too), else the seeded one
hipError_t launch_ddim_step(const DdimStepParams& p, const StepRngParams* rng, hipStream_t st) {
    if (rng) return launch_step_seeded(p.n_per_batch, {p.x, p.eps, p.eps + (p.cfg ? p.n_per_batch : 0), p.x_prev, p.x_dup, p.pred_x0}, p, *rng, ddim_step_seeded_kernel, st);
    int grid = (int)((p.n_per_batch + 255) / 256); if (grid > 2048) grid = 2048;
    ddim_step_kernel<<<grid, 256, 0, st>>>(p);
    return hipGetLastError();
}
hipError_t launch_ddpm_step(const DdpmStepParams& p, const StepRngParams* rng, hipStream_t st) {
    if (rng) return launch_step_seeded(p.n, {p.x, p.eps, p.x_prev}, p, *rng, ddpm_step_seeded_kernel, st);
    int grid = (int)((p.n + 255) / 256); if (grid > 2048) grid = 2048;
    ddpm_step_kernel<<<grid, 256, 0, st>>>(p);
    return hipGetLastError();
}
hipError_t launch_dpmpp_step(const DpmppStepParams& p, const StepRngParams* rng, hipStream_t st) {
    if (rng) return launch_step_seeded(p.n, {p.x, p.eps, p.eps + (p.cfg ? p.n : 0), p.m_prev, p.x_out, p.x_dup, p.m_store, p.pred_x0}, p, *rng, dpmpp_sde_step_seeded_kernel, st);
    const bool sde = p.noise != nullptr;
    return launch_step(p.n, {p.x, p.eps, p.eps + (p.cfg ? p.n : 0), p.m_prev, p.noise, p.x_out, p.x_dup, p.m_store, p.pred_x0}, p,
                       sde ? dpmpp_sde_step_kernel<4> : dpmpp_step_kernel<4>, sde ? dpmpp_sde_step_kernel<1> : dpmpp_step_kernel<1>, st);
}

// The forward process on a noise value that never reaches memory: out = sqrt_a x0 + sqrt_1ma z with z the starting-latent normals
// (stream 0, step 0) of the element's (row, block), derived from the flat vector index as in ddim_step_seeded_kernel.  Both products
// are rounded before the sum (no FMA contraction), so the result is the one of the same expression on rdm_op_randn's output.
__global__ __launch_bounds__(256) void q_sample_seeded_kernel(QSampleSeededParams p) {
#pragma clang fp contract(off)
    const long long bpr = p.per_row >> 2, nv = p.rows * bpr;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * 4, r = v / bpr;
        float z[4], x[4], o[4];
        philox_normal4(p.seed, (uint32_t)(v - r * bpr), 0u, p.row0 + (uint32_t)r, RDM_RNG_STREAM_XT, z);
        step_ld<4>(p.x0, i, x);
#pragma unroll
        for (int k = 0; k < 4; k++) { const float a = p.sqrt_a * x[k], b = p.sqrt_1ma * z[k]; o[k] = a + b; }
        step_st<4>(p.out, i, o);
    }
}
hipError_t launch_q_sample_seeded(const QSampleSeededParams& p, hipStream_t st) {
    if (p.rows <= 0 || p.per_row <= 0 || p.rows > (1ll << 62) / p.per_row || !seeded_step_ok(p.rows * p.per_row, p.per_row, {p.x0, p.out})) return hipErrorInvalidValue;
    const int grid = (int)std::min<long long>((p.rows * (p.per_row / 4) + 255) / 256, 2048);
    q_sample_seeded_kernel<<<grid, 256, 0, st>>>(p);
    return hipGetLastError();
}

// What each element of B rows of per_row elements would consume: the Philox word (NORMAL = false) or the normal made of it, one block
// of four elements per thread.  V = 4: one 16-byte store (per_row % 4 == 0 and out aligned); V = 1: scalar stores, a row's last block cut
// at the row's end (any per_row >= 1, any 4-byte aligned out).
template <bool NORMAL, int V>
__global__ __launch_bounds__(256) void rng_fill_kernel(RngFillParams p) {
    const long long bpr = (p.per_row + 3) >> 2, nblk = p.rows * bpr;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nblk; v += (long long)gridDim.x * 256) {
        const long long r = v / bpr, b = v - r * bpr;
        uint32_t w[4];
        philox4x32_10(p.seed, (uint32_t)b, p.step, p.row0 + (uint32_t)r, p.stream, w);
        if constexpr (NORMAL) {
            float z[4];
            box_muller(w[0], w[1], z[0], z[1]);
            box_muller(w[2], w[3], z[2], z[3]);
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = __float_as_uint(z[k]);
        }
        uint32_t* dst = p.out + r * p.per_row + b * 4;
        if constexpr (V == 4) *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
        else {
            const long long left = p.per_row - b * 4;
#pragma unroll
            for (int k = 0; k < 4; k++) if (k < left) dst[k] = w[k];
        }
    }
}
hipError_t launch_rng_fill(const RngFillParams& p, bool normal, hipStream_t st) {
    if (p.rows <= 0 || p.per_row <= 0) return hipErrorInvalidValue;
    const bool vec = p.per_row % 4 == 0 && (uintptr_t)p.out % 16 == 0;
    const long long nblk = p.rows * ((p.per_row + 3) >> 2);
    const int grid = (int)std::min<long long>((nblk + 255) / 256, 2048);
    (normal ? (vec ? rng_fill_kernel<true, 4> : rng_fill_kernel<true, 1>) : (vec ? rng_fill_kernel<false, 4> : rng_fill_kernel<false, 1>))<<<grid, 256, 0, st>>>(p);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the inpainting blend (fp32)
// ldm DDIMSampler.ddim_sampling with a mask: before a step's forward, img = q_sample(x0, t) * mask + (1 - mask) * img.  The expression of the
// per-step path (models/diffusion/ddim.py _masked_blend over _q_sample), term for term: both products of the forward process rounded,
// their sum rounded, the product with m, 1 - m, its product with x, the last sum -- true operations, no FMA contraction.  With m = 1 the
// result is fp32(sqrt_a x0 + sqrt_1ma z) and with m = 0 it is x, bit for bit.  A pass of its own beside the step kernels, which it leaves
// as they are: B*C*H*W floats once per step, next to a UNet forward.
__device__ __forceinline__ float masked_blend_value(float sa, float s1m, float x0, float z, float m, float x) {
#pragma clang fp contract(off)
    const float a = sa * x0, b = s1m * z;
    const float q = a + b;
    const float known = q * m, om = 1.0f - m;
    const float kept = om * x;
    return known + kept;
}
// element i = b chw + rem of [B, C, H, W] -> its element of the mask [B, mask_channels, H, W]
__device__ __forceinline__ long long masked_blend_mask_index(const MaskedBlendParams& p, long long i, long long b, long long rem) {
    return p.mask_channels != 1 ? i : b * p.hw + rem % p.hw;
}
__device__ __forceinline__ long long masked_blend_mask_index(const MaskedBlendParams& p, long long i) {
    if (p.mask_channels != 1) return i;
    const long long b = i / p.chw;
    return masked_blend_mask_index(p, i, b, i - b * p.chw);
}
// V = 4: float4 accesses; hw % 4 == 0, so the four elements lie in one channel plane and share one aligned mask quad (the launcher checks).
template <int V>
__global__ __launch_bounds__(256) void masked_blend_kernel(MaskedBlendParams p) {
    const long long nv = p.n / V;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * V;
        float x[V], x0[V], m[V], z[V] = {}, o[V];
        step_ld<V>(p.x, i, x);
        step_ld<V>(p.x0, i, x0);
        step_ld<V>(p.mask, masked_blend_mask_index(p, i), m);
        if (p.z) step_ld<V>(p.z, i, z);
#pragma unroll
        for (int k = 0; k < V; k++) o[k] = masked_blend_value(p.sqrt_a, p.sqrt_1ma, x0[k], z[k], m[k], x[k]);
        step_st<V>(p.out, i, o);
        if (p.x_dup) step_st<V>(p.x_dup, i, o);
    }
}
// The same arithmetic on noise drawn in registers: one Philox block per thread, four consecutive elements of one sample row, (row, block)
// derived from the flat vector index as in ddim_step_seeded_kernel -- stream 0 (RDM_RNG_STREAM_XT) at step g.step >= 1, the forward
// process's noise of the known region (philox.h).  chw % 4 == 0: rows never share a block.  When hw % 4 != 0 a block straddles channel
// planes and the mask is indexed per element (p.mask_vec == 0).  Bit-identical to masked_blend_kernel fed with rdm_op_randn's output.
__global__ __launch_bounds__(256) void masked_blend_seeded_kernel(MaskedBlendParams p, StepRngParams g) {
    const long long nv = p.n >> 2, bpr = g.per_row >> 2;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
        const long long i = v * 4, r = v / bpr, rem = (v - r * bpr) * 4;         // element i is element rem of row r
        float z[4], x[4], x0[4], m[4], o[4];
        philox_normal4(g.seed, (uint32_t)(v - r * bpr), g.step, g.row0 + (uint32_t)r, RDM_RNG_STREAM_XT, z);
        step_ld<4>(p.x, i, x);
        step_ld<4>(p.x0, i, x0);
        if (p.mask_vec) step_ld<4>(p.mask, masked_blend_mask_index(p, i, r, rem), m);
        else {
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = p.mask[masked_blend_mask_index(p, i + k, r, rem + k)];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = masked_blend_value(p.sqrt_a, p.sqrt_1ma, x0[k], z[k], m[k], x[k]);
        step_st<4>(p.out, i, o);
        if (p.x_dup) step_st<4>(p.x_dup, i, o);
    }
}
hipError_t launch_masked_blend(const MaskedBlendParams& p, const StepRngParams* rng, hipStream_t st) {
    if (rng) {
        if (rng->per_row != p.chw || !seeded_step_ok(p.n, rng->per_row, {p.x, p.x0, p.out, p.x_dup})) return hipErrorInvalidValue;
        MaskedBlendParams q = p;
        q.z = nullptr; q.mask_vec = (p.hw % 4 == 0 && (uintptr_t)p.mask % 16 == 0) ? 1 : 0;
        const int grid = (int)std::min<long long>((p.n / 4 + 255) / 256, 2048);
        masked_blend_seeded_kernel<<<grid, 256, 0, st>>>(q, *rng);
        return hipGetLastError();
    }
    if (p.n <= 0) return hipSuccess;
    bool vec = p.n % 4 == 0 && p.hw % 4 == 0;               // launch_step's rule, and whole mask quads
    for (const void* q : {(const void*)p.x, (const void*)p.x0, (const void*)p.mask, (const void*)p.z, (const void*)p.out, (const void*)p.x_dup})
        vec = vec && ((uintptr_t)q % 16 == 0);
    const long long nv = vec ? p.n / 4 : p.n;
    const int grid = (int)std::min<long long>((nv + 255) / 256, 2048);
    (vec ? masked_blend_kernel<4> : masked_blend_kernel<1>)<<<grid, 256, 0, st>>>(p);
    return hipGetLastError();
}
