// Philox4x32-10 (Salmon et al., SC'11), shared by the kernels that draw per-pixel noise: the additive gaussian noise of
// augment.hip and the rectangle fill of strongview.hip.  Both key it with a 64-bit seed and count by (pixel index,
// image id), so a value depends on (seed, id, pixel) alone -- not on the batch position or the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cnuda {

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// the block of (seed, image id, pixel): counter = (pixel lo, pixel hi, id lo, id hi), key = (seed lo, seed hi)
__device__ __forceinline__ void philox_pixel_block(unsigned long long seed, long long id, long long pixel, uint32_t c[4]) {
    c[0] = (uint32_t)pixel, c[1] = (uint32_t)((unsigned long long)pixel >> 32);
    c[2] = (uint32_t)id, c[3] = (uint32_t)((unsigned long long)id >> 32);
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// a 23-bit uniform in (0, 1) from one word: never 0 or 1
__device__ __forceinline__ float philox_uniform(uint32_t word) {
    return ((float)(word >> 9) + 0.5f) * (1.0f / 8388608.0f);
}

}  // namespace cnuda
