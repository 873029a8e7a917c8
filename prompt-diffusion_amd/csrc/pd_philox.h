// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the engine's seeded standard normals.
// A counter-based generator: one block maps (counter[4], key[2]) to four uint32 values with no state, so the draw of a latent
// element is a function of its address alone (include/pdengine.h, "Seeded noise": key = seed, counter = (e / 4, sample, draw,
// stream), lane = e % 4) -- whatever the grid, the batch split or the kernel that evaluates it.
#pragma once
#include <stdint.h>

#include "../../include/pdengine.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PD_HD __host__ __device__ __forceinline__
#else
#define PD_HD inline
#endif

PD_HD void pd_philox4x32_10_block(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4]) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// engine state the kernels read (pd_set_rng): {seed_lo, seed_hi, sample_base_lo, sample_base_hi} in a small device buffer
struct PdRng { const uint32_t* state; };

#if defined(__HIPCC__) || defined(__CUDACC__)
// u(r) = r 2^-32 + 2^-33 in (0, 1]: the scaling is exact, the one rounding is (float)r
__device__ __forceinline__ float pd_philox_u01(uint32_t r) { return (float)r * 2.3283064365386963e-10f + 1.1641532182693481e-10f; }

// lane 0 / 1: sqrt(-2 log u(r0)) (cos, sin)(2 pi u(r1)); lane 2 / 3 the same from r2, r3.  Accurate logf / sincospif / sqrtf.
__device__ __forceinline__ float pd_philox_normal_lane(const uint32_t r[4], int lane) {
    const bool hi = (lane & 2) != 0;
    const float u0 = pd_philox_u01(hi ? r[2] : r[0]), u1 = pd_philox_u01(hi ? r[3] : r[1]);
    const float rad = sqrtf(-2.0f * logf(u0));
    float sn, cs;
    sincospif(2.0f * u1, &sn, &cs);
    return rad * ((lane & 1) ? sn : cs);
}

// all four lanes of one block at once, for a kernel whose thread owns elements 4q .. 4q + 3 of a sample: the two radii and the two
// sincospif are each evaluated once, on the operands pd_philox_normal_lane gives them, so z[l] has that function's bits
__device__ __forceinline__ void pd_philox_normal4(const uint32_t r[4], float z[4]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u0 = pd_philox_u01(r[2 * h]), u1 = pd_philox_u01(r[2 * h + 1]);
        const float rad = sqrtf(-2.0f * logf(u0));
        float sn, cs;
        sincospif(2.0f * u1, &sn, &cs);
        z[2 * h] = rad * cs;
        z[2 * h + 1] = rad * sn;
    }
}

// the draw at (stream, draw, sample b of this call, element e of the sample in the caller's NCHW order)
__device__ __forceinline__ float pd_rng_normal(const PdRng& g, uint32_t stream, uint32_t draw, uint32_t b, long long e) {
    uint32_t r[4];
    pd_philox4x32_10_block((uint32_t)(e >> 2), g.state[2] + b, draw, stream, g.state[0], g.state[1], r);
    return pd_philox_normal_lane(r, (int)(e & 3));
}
#endif
