// philox.h -- the counter-based generator behind the device draws (random_draws.hip) and the dropout masks (dropout.hip):
// the round function and the word -> U[0, 1) map, stated once.  The stream itself (key, counter layout, which word an
// element owns) is defined at srgan_random_fill in include/srgan_hip.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace srgan {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;     // the two round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;     // the key schedule's Weyl increments
constexpr float TWO_POW_MINUS_24 = 5.9604644775390625e-08f;

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds on the counter c
// under the key (k0, k1), which is bumped between rounds.
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c[0]), lo0 = PHILOX_M0 * c[0];
    const uint32_t hi1 = __umulhi(PHILOX_M1, c[2]), lo1 = PHILOX_M1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
}

// The top 24 bits of a word as a multiple of 2^-24 in [0, 1): exact in fp32.
__device__ __forceinline__ float unit24(uint32_t w) { return (float)(w >> 8) * TWO_POW_MINUS_24; }

// The four output words of Philox block `block` of draw `draw` in iteration `iteration` under the key (seed_lo, seed_hi):
// counter (block & 0xffffffff, block >> 32, draw, iteration); word j belongs to element 4 * block + j.
__device__ __forceinline__ void draw_block_words(uint64_t block, uint32_t draw, uint32_t iteration, uint32_t seed_lo,
                                                 uint32_t seed_hi, uint32_t w[4]) {
  w[0] = (uint32_t)block;
  w[1] = (uint32_t)(block >> 32);
  w[2] = draw;
  w[3] = iteration;
  philox4x32_10(w, seed_lo, seed_hi);
}

}  // namespace srgan
