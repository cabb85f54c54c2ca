// bn_train.h -- what the two training-mode batch-norm translation units share (batch_norm_train.hip: fp32 NCHW;
// blocked16_batch_norm.hip: the blocked layout of blocked16.h): the pre-activation, Chan's merge of (count, mean, M2)
// triples with its fixed reduction tree, and the choice of images per workgroup.
#pragma once
#include "common.h"

namespace srgan {

// The pre-activation, shared by the forward and both backward kernels: the leaky mask is bit-consistent.
__device__ __forceinline__ float bn_train_pre(float x, float mean, float a, float beta) { return fmaf(x - mean, a, beta); }
__device__ __forceinline__ float bn_train_scale(float inv_std, float gamma) { return __fmul_rn(inv_std, gamma); }

struct Moments { float n, mean, m2; };      // count (a float: exact up to 2^24, the entry point's limit), mean, sum of squared deviations about it

// Chan et al.: the moments of the union of two disjoint sets.
__device__ __forceinline__ Moments merge_moments(const Moments& a, const Moments& b) {
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  const float n = a.n + b.n, delta = b.mean - a.mean, w = b.n / n;
  return Moments{n, fmaf(delta, w, a.mean), a.m2 + b.m2 + delta * delta * a.n * w};
}

// The 64 lanes' moments in a fixed shuffle-down tree: lane 0.
__device__ __forceinline__ Moments wave_moments(Moments v) {
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    const Moments other{__shfl_down(v.n, offset, 64), __shfl_down(v.mean, offset, 64), __shfl_down(v.m2, offset, 64)};
    v = merge_moments(v, other);
  }
  return v;
}

// The four waves' moments (lane 0 of each wave wrote its own), merged in a fixed order.
__device__ __forceinline__ Moments merge_four_moments(const Moments& w0, const Moments& w1, const Moments& w2, const Moments& w3) {
  return merge_moments(merge_moments(w0, w1), merge_moments(w2, w3));
}

// The three above as the Ops of ordered_lane_finish (split_finish.h): the workgroups of a row meet in the tree of a workgroup.
struct LaneMoments {
  using Value = Moments;
  static __device__ __forceinline__ Moments combine(const Moments& a, const Moments& b) { return merge_moments(a, b); }
  static __device__ __forceinline__ Moments wave(const Moments& v) { return wave_moments(v); }
  static __device__ __forceinline__ Moments four(const Moments& w0, const Moments& w1, const Moments& w2, const Moments& w3) {
    return merge_four_moments(w0, w1, w2, w3);
  }
};

// The 256 threads' moments in a fixed tree (shuffle-down inside each wave, then the four waves in order): thread 0.
__device__ __forceinline__ Moments block_moments_256(Moments v, Moments* scratch4) {
  v = wave_moments(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) scratch4[wave] = v;
  __syncthreads();
  Moments total{0.f, 0.f, 0.f};
  if (threadIdx.x == 0) total = merge_four_moments(scratch4[0], scratch4[1], scratch4[2], scratch4[3]);
  return total;
}

// Images per workgroup: ~2048 workgroups of at least 4096 elements where the shape allows it (as srgan_bn_act_bwd).
// `rows` = what the grid's x runs over (channels; channel groups of a blocked tensor), `plane` = fp32 elements -- or as
// many 4-byte units -- per row and image.
inline int images_per_workgroup(int N, int rows, int64_t plane) {
  int per = 1;
  while (per < N && ((int64_t)rows * ((N + per - 1) / per) > 2048 || (int64_t)per * plane < 4096) &&
         (int64_t)rows * ((N + 2 * per - 1) / (2 * per)) >= 1024)
    per *= 2;
  return per;
}

}  // namespace srgan
