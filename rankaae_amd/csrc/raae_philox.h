// Philox4x32-10 (Salmon et al. 2011) and the Gaussians of the step's numbering: shared by the tape fill and the step
// head (raae_optim.hip) and the augmentation kernels (raae_augment.hip).
#pragma once
#include "raae_common.h"

namespace raae {

__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
__device__ __forceinline__ void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c[0], c[1], c[2], c[3], k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// four N(0, 1) values: Philox block `qg` (= position in the numbering of the step's Gaussian elements / 4) of step `ctr`
__device__ __forceinline__ void normal4(long qg, unsigned long long ctr, unsigned long long seed, float (&o)[4]) {
    uint32_t c[4] = {(uint32_t)qg, (uint32_t)(qg >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32)};
    philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float r0 = sqrtf(-2.f * logf(u01(c[0]))), r1 = sqrtf(-2.f * logf(u01(c[2])));
    const float a0 = 6.283185307179586f * u01(c[1]), a1 = 6.283185307179586f * u01(c[3]);
    o[0] = r0 * cosf(a0); o[1] = r0 * sinf(a0); o[2] = r1 * cosf(a1); o[3] = r1 * sinf(a1);
}

}  // namespace raae
