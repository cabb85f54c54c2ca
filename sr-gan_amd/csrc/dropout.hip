// dropout.hip -- inverted dropout whose mask is never stored (reference crowd/models.py:350-353: F.dropout on a dense layer's
// new features): element e is kept when element e of a uniform device draw (random_draws.hip's stream, kind 0) is >= p, so
// the forward pass, the backward pass and the gradient penalty's recorded double backward regenerate the same mask from
// (seed, iteration, draw, e) -- the operation is linear with a fixed mask and one kernel serves all three.  The contract is
// at srgan_dropout in include/srgan_hip.h.
#include <math.h>
#include "common.h"
#include "philox.h"

namespace srgan {
namespace {

// One thread per Philox block (4 consecutive elements of the draw) in a grid-stride loop over the blocks that intersect
// [first, first + total), total = rows * row_elems < 2^31.  Element g = 4 * block - first + j of the operation sits in row
// g / row_elems at column g % row_elems; the rows of x and y are x_stride / y_stride floats apart (a channel slice of a
// wider NCHW tensor).  A block that lies inside one row and whose two addresses are 16-byte aligned moves as one float4 each
// way; ragged ends, blocks that straddle two rows and misaligned rows go element by element.  No __restrict__: x == y is
// allowed (every thread reads its own elements before it writes them).
__global__ void __launch_bounds__(256) dropout_kernel(const float* x, float* y, uint32_t total, uint32_t row_elems,
                                                      int64_t x_stride, int64_t y_stride, int64_t first, float p, float scale,
                                                      uint32_t draw, const uint32_t* __restrict__ state) {
  const uint32_t seed_lo = state[0], seed_hi = state[1], iteration = state[2];
  const uint64_t first_block = (uint64_t)first >> 2;
  const uint64_t blocks = (((uint64_t)first + (uint64_t)total - 1) >> 2) - first_block + 1;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < blocks; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t block = first_block + b;
    uint32_t w[4];
    draw_block_words(block, draw, iteration, seed_lo, seed_hi, w);
    const int64_t at = (int64_t)(block << 2) - first;      // element 0 of the block as an element of the operation: -3 .. total - 1
    if (at >= 0 && at + 4 <= (int64_t)total) {
      const uint32_t row = (uint32_t)at / row_elems, column = (uint32_t)at - row * row_elems;
      const float* source = x + (int64_t)row * x_stride + column;
      float* target = y + (int64_t)row * y_stride + column;
      if (column + 4 <= row_elems && ((((uintptr_t)source) | ((uintptr_t)target)) & 15) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(source);
        float4 out;
        out.x = unit24(w[0]) >= p ? __fmul_rn(v.x, scale) : 0.0f;
        out.y = unit24(w[1]) >= p ? __fmul_rn(v.y, scale) : 0.0f;
        out.z = unit24(w[2]) >= p ? __fmul_rn(v.z, scale) : 0.0f;
        out.w = unit24(w[3]) >= p ? __fmul_rn(v.w, scale) : 0.0f;
        *reinterpret_cast<float4*>(target) = out;
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t g = at + j;
      if (g < 0 || g >= (int64_t)total) continue;
      const uint32_t row = (uint32_t)g / row_elems, column = (uint32_t)g - row * row_elems;
      const float v = x[(int64_t)row * x_stride + column];
      y[(int64_t)row * y_stride + column] = unit24(w[j]) >= p ? __fmul_rn(v, scale) : 0.0f;
    }
  }
}

}  // namespace
}  // namespace srgan

using namespace srgan;

extern "C" {

int srgan_dropout(const float* x, float* y, int64_t rows, int64_t row_elems, int64_t x_row_stride, int64_t y_row_stride,
                  int64_t first, float p, int32_t draw, const uint32_t* state, void* stream) {
  SRGAN_REQUIRE(x && y && state, SRGAN_EINVAL, "srgan_dropout pointers");
  SRGAN_REQUIRE(rows >= 0 && row_elems >= 0 && first >= 0, SRGAN_EINVAL, "srgan_dropout: rows, row_elems, first");
  SRGAN_REQUIRE(x_row_stride >= row_elems && y_row_stride >= row_elems, SRGAN_EINVAL, "srgan_dropout: row strides");
  SRGAN_REQUIRE(draw >= 0, SRGAN_EINVAL, "srgan_dropout: draw");
  SRGAN_REQUIRE(isfinite(p) && p >= 0.0f && p <= 1.0f, SRGAN_EINVAL, "srgan_dropout: p within [0, 1]");
  const int64_t limit = ((int64_t)1 << 31) - 1;
  SRGAN_REQUIRE(rows == 0 || row_elems <= limit / rows, SRGAN_ERANGE, "srgan_dropout: rows * row_elems within max_tensor_elements");
  const int64_t total = rows * row_elems;
  SRGAN_REQUIRE(first <= INT64_MAX - total, SRGAN_EINVAL, "srgan_dropout: first + rows * row_elems");
  if (total == 0) return SRGAN_OK;
  const float scale = 1.0f / (1.0f - p);                   // p == 1: inf, never used (every uniform is < 1)
  const int64_t blocks = ((first + total - 1) >> 2) - (first >> 2) + 1;
  hipLaunchKernelGGL(dropout_kernel, dim3(stream_grid(blocks, 256)), dim3(256), 0, (hipStream_t)stream, x, y, (uint32_t)total,
                     (uint32_t)row_elems, x_row_stride, y_row_stride, first, p, scale, (uint32_t)draw, state);
  return launch_status();
}

}  // extern "C"
