// The counter-based generator of the sampled token steps (greedy.hip, truncate.hip): a draw depends on nothing but its own
// coordinates (seed, global row, position, token), so both kernels -- and the host (tests/test_gpu_round4.py) -- recompute any draw.
#pragma once
#include "common.h"

namespace wm {

// uniform in (0, 1) from (seed, row, position, token): three rounds of the murmur3 finaliser over the mixed-in coordinates
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float gumbel_noise(uint32_t key, int n) {
    const uint32_t h = fmix32(fmix32(key ^ ((uint32_t)n * 0x27d4eb2fu)) + 0x9e3779b9u * (uint32_t)n);
    // (0, 1), 24 bits.  Above 2^23 the + 0.5f rounds to even: 16777215 + 0.5 would become 2^24, u = 1 and g = +inf (a token drawn
    // whatever its logit, once in 2^24 tokens); the bound keeps u <= 1 - 2^-24 and g <= 16.64
    const float u = fminf((float)(h >> 8) + 0.5f, 16777215.0f) * (1.0f / 16777216.0f);
    return -__logf(-__logf(u));
}

}  // namespace wm
