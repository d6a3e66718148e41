// The library's counter-based noise generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel Random Numbers: As Easy as 1, 2, 3",
// SC'11) and the Box-Muller transform of its words.  ONE definition for host and device; the counter / key layout is part of the ABI
// (include/rdm_hip.h, DESIGN.md section 3 "Device noise").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RDM_RNG_STREAM_XT 0u      // the forward process's noise: step 0 the starting latent x_T, step i + 1 the known region of inpainting loop step i
#define RDM_RNG_STREAM_STEP 1u    // per-step update noise
#define RDM_RNG_STREAMS 2u        // streams >= this are reserved: the entries refuse them

// key = (seed lo, seed hi); counter = (block, step, row, stream) -> four 32-bit words.  Ten rounds: the counter's halves are multiplied
// by 0xD2511F53 / 0xCD9E8D57, the high products crossed with the key, the key raised by the Weyl increments 0x9E3779B9 / 0xBB67AE85.
__host__ __device__ inline void philox4x32_10(uint64_t seed, uint32_t block, uint32_t step, uint32_t row, uint32_t stream, uint32_t (&w)[4]) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t c0 = block, c1 = step, c2 = row, c3 = stream;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// Box-Muller on one word pair: u = ((w >> 9) + 0.5) 2^-23 is exact in fp32 and strictly inside (0, 1) (23 random bits, centred), so
// r = sqrt(-2 ln u1) <= 5.77 and is never infinite; the angle is 2 pi u2 through sincospif on the EXACT argument 2 u2 (no rounded 2 pi).
// z0 = r cos, z1 = r sin.  No fast-math forms: logf, sqrtf and sincospif are the library functions with their documented ulp bounds
// (tests/test_gpu_device_noise.py counts them into the bound it holds rdm_op_randn to).
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
    const float u1 = ((float)(wa >> 9) + 0.5f) * 1.1920928955078125e-07f;        // 2^-23
    const float u2 = ((float)(wb >> 9) + 0.5f) * 1.1920928955078125e-07f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    z0 = r * c; z1 = r * s;
}
// The four normals of one Philox block: elements 4 block .. 4 block + 3 of a row (element 2h from cos, 2h + 1 from sin of pair h).
__device__ __forceinline__ void philox_normal4(uint64_t seed, uint32_t block, uint32_t step, uint32_t row, uint32_t stream, float (&z)[4]) {
    uint32_t w[4];
    philox4x32_10(seed, block, step, row, stream, w);
    box_muller(w[0], w[1], z[0], z[1]);
    box_muller(w[2], w[3], z[2], z[3]);
}
