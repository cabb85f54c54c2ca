// random_draws.hip -- the three random tensors of a training iteration (z for the discriminator step, alpha for the
// interpolates, z for the generator step: reference srgan.py:286-289, 364, 301) drawn on the device by a counter-based
// generator.  Element e of a draw is a pure function of (seed, iteration, draw id, e): nothing is carried from launch to
// launch but the 16-byte state {seed_lo, seed_hi, iteration, 0}, so a captured fill replays as the next iteration's draw
// once srgan_random_advance has run, a data-parallel rank fills exactly its rows of the global tensor, and the result does
// not depend on the grid or on the stream schedule.  The stream is defined in include/srgan_hip.h (srgan_random_fill).
#include <math.h>
#include "common.h"
#include "philox.h"      // the round function and unit24, shared with dropout.hip

namespace srgan {
namespace {

// Box-Muller on one word pair: u1 = 1 - unit24(even) in (0, 1], u2 = unit24(odd); the even element gets r cos(2 pi u2),
// the odd one r sin(2 pi u2).  Precise device functions only (no fast intrinsics), and every product is rounded on its
// own: a product contracted into the offset's addition would make the value with an offset differ from
// fl(value without + (+/-)offset).
__device__ __forceinline__ void normal_pair(uint32_t w_even, uint32_t w_odd, float& even, float& odd) {
  const float u1 = 1.0f - unit24(w_even);
  const float r = sqrtf(__fmul_rn(-2.0f, logf(u1)));
  float s, c;
  sincospif(2.0f * unit24(w_odd), &s, &c);
  even = __fmul_rn(r, c);
  odd = __fmul_rn(r, s);
}

// One thread per Philox block (4 consecutive elements) in a grid-stride loop over the blocks that intersect
// [first, first + n); a thread stores only the elements of its block that lie inside that window.
__global__ void __launch_bounds__(256) random_fill_kernel(float* __restrict__ out, int64_t n, int64_t first, int kind,
                                                          float offset, uint32_t draw, const uint32_t* __restrict__ state) {
  const uint32_t seed_lo = state[0], seed_hi = state[1], iteration = state[2];
  const uint64_t first_block = (uint64_t)first >> 2;
  const uint64_t blocks = (((uint64_t)first + (uint64_t)n - 1) >> 2) - first_block + 1;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t block = first_block + b;
    uint32_t w[4];
    draw_block_words(block, draw, iteration, seed_lo, seed_hi, w);
    float v[4];
    if (kind == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = unit24(w[j]);
    } else {
      normal_pair(w[0], w[1], v[0], v[1]);
      normal_pair(w[2], w[3], v[2], v[3]);
      if (offset != 0.0f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __fadd_rn(v[j], (w[j] & 1u) ? offset : -offset);
      }
    }
    const int64_t at = (int64_t)(block << 2) - first;      // where element 0 of the block sits in out: -3 .. n - 1
    if (at >= 0 && at + 4 <= n && (((uintptr_t)(out + at)) & 15) == 0) {
      *reinterpret_cast<float4*>(out + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (at + j >= 0 && at + j < n) out[at + j] = v[j];
    }
  }
}

__global__ void random_advance_kernel(uint32_t* state) { state[2] += 1u; }

}  // namespace
}  // namespace srgan

using namespace srgan;

extern "C" {

int srgan_random_fill(float* out, int64_t n, int64_t first, int32_t kind, float offset, int32_t draw, const uint32_t* state,
                      void* stream) {
  SRGAN_REQUIRE(out && state, SRGAN_EINVAL, "srgan_random_fill pointers");
  SRGAN_REQUIRE(n >= 0 && n <= ((int64_t)1 << 31) - 1, SRGAN_EINVAL, "srgan_random_fill: n within max_tensor_elements");
  SRGAN_REQUIRE(first >= 0 && first <= INT64_MAX - n, SRGAN_EINVAL, "srgan_random_fill: first");
  SRGAN_REQUIRE((kind == 0 || kind == 1) && draw >= 0 && isfinite(offset), SRGAN_EINVAL, "srgan_random_fill: kind, draw, offset");
  if (n == 0) return SRGAN_OK;
  const int64_t blocks = ((first + n - 1) >> 2) - (first >> 2) + 1;
  hipLaunchKernelGGL(random_fill_kernel, dim3(stream_grid(blocks, 256)), dim3(256), 0, (hipStream_t)stream, out, n, first,
                     (int)kind, offset, (uint32_t)draw, state);
  return launch_status();
}

int srgan_random_advance(uint32_t* state, void* stream) {
  SRGAN_REQUIRE(state, SRGAN_EINVAL, "srgan_random_advance: state");
  hipLaunchKernelGGL(random_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
  return launch_status();
}

}  // extern "C"
