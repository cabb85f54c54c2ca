// evaluation_sums.h -- the fixed-order fp64 workgroup sums of the evaluation kernels (crowd_evaluation.hip,
// regression_evaluation.hip): no atomics, so the same inputs give the same bits.  A translation unit that includes this
// switches FMA contraction off itself (`#pragma clang fp contract(off)`) where its squares must be rounded products.
#pragma once
#include "common.h"

namespace srgan {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) v += __shfl_xor(v, offset, 64);
  return v;
}

// The workgroup's total of N running sums, valid in thread 0: the wave64 butterfly, then the four waves in wave order
// through LDS.  256 threads, every one of them calls.
template <int N>
__device__ __forceinline__ void block_sums_f64(double (&v)[N], double (*scratch)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    v[k] = wave_sum_f64(v[k]);
    if (lane == 0) scratch[k][wave] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((scratch[k][0] + scratch[k][1]) + scratch[k][2]) + scratch[k][3];
  }
}

}  // namespace srgan
