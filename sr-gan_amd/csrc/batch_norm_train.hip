// batch_norm_train.hip -- training-mode batch normalisation (batch statistics) for fp32 NCHW tensors: the DCGAN
// generators' norm layers, which the reference never freezes (srgan.py:171; age/models.py:16-21 with batch_norm on).
//
// (The same four passes on blocked bf16 / fp16 / fp32 tensors: blocked16_batch_norm.hip; what the two share: bn_train.h.)
//
// Four HBM-bound kernels, all on one decomposition: a workgroup owns channel c of a group of images [n0, n1), lanes
// along the plane (float4 when HW % 4 == 0 and the tensors are 16-byte aligned, scalars otherwise):
//   stats       one read of x  -> mean, inv_std (+ the running buffers and num_batches_tracked)
//   forward     one read, one write: y = leaky((x - mean) * inv_std * gamma + beta, slope)
//   bwd reduce  reads g, x     -> sum g', sum g' * xhat per channel (= g_beta, g_gamma; accumulated when asked)
//   bwd apply   reads g, x, writes gx = gamma * inv_std * (g' - sum g' / M - xhat * sum g' xhat / M)
// g' = g * (pre-activation > 0 ? 1 : slope) is recomputed from x through bn_train_pre(), the forward's own function.
//
// The variance comes from deviations about a mean, never from E[x^2] - E[x]^2: a thread holds a tile's 16 (4) values
// in registers, takes their mean, sums the squared deviations, and merges (count, mean, M2) triples with Chan's
// formula -- thread, wave (a fixed shuffle tree), workgroup, and then the channel's workgroups through the stream's
// workspace in part order (split_finish.h: no fp32 atomics on data, the same bits on every run).
// Roofline: HBM; algorithmic bytes = 4 * elements per tensor read or written.
#include <initializer_list>
#include "bn_train.h"
#include "common.h"
#include "launchers.h"
#include "split_finish.h"

namespace srgan {

__device__ unsigned int g_bn_train_tickets[SPLIT_TICKET_SETS * ROW_FINISH_ROWS];

// Offset of element `idx` (in units of W floats) of the workgroup's chunk: channel c of images n0, n0 + 1, ...
template <int W>
__device__ __forceinline__ int64_t chunk_offset(int idx, int per_plane, int n0, int C, int c, int64_t HW) {
  const int nl = idx / per_plane, i = idx - nl * per_plane;
  return ((int64_t)(n0 + nl) * C + c) * HW + (int64_t)i * W;
}

template <int W>
__global__ __launch_bounds__(256) void bn_train_stats_kernel(const float* __restrict__ x, float* __restrict__ mean_out,
                                                             float* __restrict__ inv_std_out, float* running_mean,
                                                             float* running_var, long long* batches_tracked, float momentum,
                                                             float eps, int N, int C, int64_t HW, int images_per_block,
                                                             float* partial, unsigned int* tickets) {
  __shared__ Moments scratch[4][1];
  const int tid = (int)threadIdx.x, c = (int)blockIdx.x, part = (int)blockIdx.y, parts = (int)gridDim.y;
  const int n0 = part * images_per_block, n1 = min(N, n0 + images_per_block);
  const int per_plane = (int)(HW / W), total = (n1 - n0) * per_plane;
  Moments mine{0.f, 0.f, 0.f};
  for (int base = 0; base < total; base += 1024) {      // a tile: four loads per thread in flight, kept in registers
    float v[4][W];
    bool ok[4];
    float sum = 0.f;
    int count = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = base + j * 256 + tid;
      ok[j] = idx < total;
      if (ok[j]) {
        const float* p = x + chunk_offset<W>(idx, per_plane, n0, C, c, HW);
        if constexpr (W == 4) {
          const float4 q = *reinterpret_cast<const float4*>(p);
          v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
        } else {
          v[j][0] = *p;
        }
      } else {
#pragma unroll
        for (int e = 0; e < W; ++e) v[j][e] = 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok[j]) {
#pragma unroll
        for (int e = 0; e < W; ++e) sum += v[j][e];
        count += W;
      }
    if (count == 0) continue;
    Moments tile{(float)count, sum / (float)count, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok[j]) {
#pragma unroll
        for (int e = 0; e < W; ++e) { const float d = v[j][e] - tile.mean; tile.m2 = fmaf(d, d, tile.m2); }
      }
    mine = merge_moments(mine, tile);
  }
  Moments all = block_moments_256(mine, scratch[0]);       // thread 0: this workgroup's images
  // the channel's workgroups meet in the workspace in part order (split_finish.h)
  if (!ordered_lane_finish<LaneMoments, 1>(all, partial + (int64_t)c * parts * 3, part, parts, tickets + c, scratch)) return;
  if (tid != 0) return;
  const float variance = all.m2 / all.n;                   // biased: the one the batch is normalised with
  mean_out[c] = all.mean;
  inv_std_out[c] = 1.f / sqrtf(variance + eps);
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * all.mean;
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (all.m2 / (all.n - 1.f));   // unbiased
  if (batches_tracked && c == 0) *batches_tracked += 1;
}

// Visit the workgroup's chunk: f(offset) for every run of W floats.
template <int W, typename F>
__device__ __forceinline__ void for_chunk(int N, int C, int64_t HW, int images_per_block, F f) {
  const int c = (int)blockIdx.x;
  const int n0 = (int)blockIdx.y * images_per_block, n1 = min(N, n0 + images_per_block);
  const int per_plane = (int)(HW / W), total = (n1 - n0) * per_plane;
#pragma unroll 4
  for (int idx = (int)threadIdx.x; idx < total; idx += 256) f(chunk_offset<W>(idx, per_plane, n0, C, c, HW));
}

template <int W>
__device__ __forceinline__ void load_run(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void store_run(float* p, const float (&v)[W]) {
  if constexpr (W == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

template <int W>
__global__ __launch_bounds__(256) void bn_train_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ inv_std, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float slope, float* __restrict__ y,
                                                           int N, int C, int64_t HW, int images_per_block) {
  const int c = (int)blockIdx.x;
  const float mu = mean[c], a = bn_train_scale(inv_std[c], gamma[c]), b = beta[c];
  for_chunk<W>(N, C, HW, images_per_block, [&](int64_t at) {
    float v[W];
    load_run<W>(x + at, v);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float pre = bn_train_pre(v[e], mu, a, b);
      v[e] = pre > 0.f ? pre : pre * slope;
    }
    store_run<W>(y + at, v);
  });
}

template <int W>
__global__ __launch_bounds__(256) void bn_train_bwd_reduce_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ inv_std,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float slope,
                                                                  float* __restrict__ sums, float* g_gamma, float* g_beta, int N,
                                                                  int C, int64_t HW, int images_per_block, float* partial,
                                                                  unsigned int* tickets) {
  __shared__ float scratch[4];
  const int c = (int)blockIdx.x;
  const float mu = mean[c], is = inv_std[c], a = bn_train_scale(is, gamma[c]), b = beta[c];
  float plain = 0.f, weighted = 0.f;
  for_chunk<W>(N, C, HW, images_per_block, [&](int64_t at) {
    float gv[W], xv[W];
    load_run<W>(g + at, gv);
    load_run<W>(x + at, xv);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float gp = bn_train_pre(xv[e], mu, a, b) > 0.f ? gv[e] : gv[e] * slope;
      plain += gp;
      weighted = fmaf(gp, (xv[e] - mu) * is, weighted);
    }
  });
  float v[2];
  v[0] = block_sum_256(plain, scratch);
  __syncthreads();
  v[1] = block_sum_256(weighted, scratch);
  __syncthreads();
  if (ordered_row_finish<2>(v, partial ? partial + (int64_t)c * gridDim.y * 2 : nullptr, (int)blockIdx.y, (int)gridDim.y, tickets + c, scratch)) {
    sums[c] = v[0];
    sums[C + c] = v[1];
    if (g_beta) g_beta[c] += v[0];
    if (g_gamma) g_gamma[c] += v[1];
  }
}

template <int W>
__global__ __launch_bounds__(256) void bn_train_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ inv_std,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float slope,
                                                                 const float* __restrict__ sums, float* __restrict__ gx, int N,
                                                                 int C, int64_t HW, int images_per_block, float inv_count) {
  const int c = (int)blockIdx.x;
  const float mu = mean[c], is = inv_std[c], a = bn_train_scale(is, gamma[c]), b = beta[c];
  const float mean_g = sums[c] * inv_count, mean_gx = sums[C + c] * inv_count;
  for_chunk<W>(N, C, HW, images_per_block, [&](int64_t at) {
    float gv[W], xv[W];
    load_run<W>(g + at, gv);
    load_run<W>(x + at, xv);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float gp = bn_train_pre(xv[e], mu, a, b) > 0.f ? gv[e] : gv[e] * slope;
      gv[e] = a * (gp - mean_g - (xv[e] - mu) * is * mean_gx);
    }
    store_run<W>(gx + at, gv);
  });
}

static bool vectorisable(int64_t HW, std::initializer_list<const void*> tensors) {
  uintptr_t bits = 0;
  for (const void* t : tensors) bits |= (uintptr_t)t;
  return (HW & 3) == 0 && (bits & 15) == 0;
}

static int shape_status(int32_t N, int32_t C, int64_t HW, const char* what) {
  SRGAN_REQUIRE(N > 0 && C > 0 && HW > 0, SRGAN_EINVAL, what);
  SRGAN_REQUIRE((int64_t)N * HW < ((int64_t)1 << 31) - 2048, SRGAN_ERANGE, what);      // a channel is indexed with 32 bits
  return SRGAN_OK;
}

// Records of the live profile (srgan_profile_begin / _report): kinds 20 stats, 21 forward, 22 backward reduce, 23 backward
// apply, each with its algorithmic bytes and 0 FLOP.  bench.py's legend does not name them and its workloads never launch
// them; a profiled workload with the switch on would count their time in the bracketed kernel time.
static int finish_bracket(int slot, hipStream_t stream, int32_t N, int32_t C, int64_t HW, LaunchKind kind, int per, int parts, double tensors) {
  return profile_bracket_end_bytes(slot, stream, C, (int64_t)N * HW, 0, kind, 256, per, parts, 4.0 * tensors * (double)N * C * (double)HW, 0);
}

int bn_train_stats_run(const float* x, float* mean, float* inv_std, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, float momentum, float eps, int32_t N, int32_t C, int64_t HW,
                       hipStream_t stream) {
  RowFinishGrid grid{images_per_workgroup(N, C, HW)};
  if (const int status = row_finish_grid(C, N, 3, g_bn_train_tickets, stream, "srgan_batch_norm_train_stats grid", &grid)) return status;
  const int slot = profile_bracket_begin(stream);
  if (vectorisable(HW, {x}))
    hipLaunchKernelGGL(bn_train_stats_kernel<4>, dim3(C, grid.parts), dim3(256), 0, stream, x, mean, inv_std, running_mean, running_var,
                       reinterpret_cast<long long*>(num_batches_tracked), momentum, eps, N, C, HW, grid.per, grid.partial, grid.tickets);
  else
    hipLaunchKernelGGL(bn_train_stats_kernel<1>, dim3(C, grid.parts), dim3(256), 0, stream, x, mean, inv_std, running_mean, running_var,
                       reinterpret_cast<long long*>(num_batches_tracked), momentum, eps, N, C, HW, grid.per, grid.partial, grid.tickets);
  const int status = launch_status();
  finish_bracket(slot, stream, N, C, HW, KIND_BN_STATS, grid.per, grid.parts, 1.0);
  return status;
}

int bn_train_fwd_run(const float* x, const float* mean, const float* inv_std, const float* gamma, const float* beta, float slope,
                     float* y, int32_t N, int32_t C, int64_t HW, hipStream_t stream) {
  const int per = images_per_workgroup(N, C, HW), parts = (N + per - 1) / per;
  SRGAN_REQUIRE(parts <= 65535, SRGAN_ERANGE, "srgan_batch_norm_train_fwd grid");
  const int slot = profile_bracket_begin(stream);
  if (vectorisable(HW, {x, y}))
    hipLaunchKernelGGL(bn_train_fwd_kernel<4>, dim3(C, parts), dim3(256), 0, stream, x, mean, inv_std, gamma, beta, slope, y, N, C,
                       HW, per);
  else
    hipLaunchKernelGGL(bn_train_fwd_kernel<1>, dim3(C, parts), dim3(256), 0, stream, x, mean, inv_std, gamma, beta, slope, y, N, C,
                       HW, per);
  const int status = launch_status();
  finish_bracket(slot, stream, N, C, HW, KIND_BN_FWD, per, parts, 2.0);
  return status;
}

int bn_train_bwd_reduce_run(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                            const float* beta, float slope, float* sums, float* g_gamma, float* g_beta, int32_t N, int32_t C,
                            int64_t HW, hipStream_t stream) {
  RowFinishGrid grid{images_per_workgroup(N, C, HW)};
  if (const int status = row_finish_grid(C, N, 2, g_bn_train_tickets, stream, "srgan_batch_norm_train_bwd_reduce grid", &grid)) return status;
  const int slot = profile_bracket_begin(stream);
  if (vectorisable(HW, {g, x}))
    hipLaunchKernelGGL(bn_train_bwd_reduce_kernel<4>, dim3(C, grid.parts), dim3(256), 0, stream, g, x, mean, inv_std, gamma, beta, slope,
                       sums, g_gamma, g_beta, N, C, HW, grid.per, grid.partial, grid.tickets);
  else
    hipLaunchKernelGGL(bn_train_bwd_reduce_kernel<1>, dim3(C, grid.parts), dim3(256), 0, stream, g, x, mean, inv_std, gamma, beta, slope,
                       sums, g_gamma, g_beta, N, C, HW, grid.per, grid.partial, grid.tickets);
  const int status = launch_status();
  finish_bracket(slot, stream, N, C, HW, KIND_BN_BWD_REDUCE, grid.per, grid.parts, 2.0);
  return status;
}

int bn_train_bwd_apply_run(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                           const float* beta, float slope, const float* sums, float* gx, int32_t N, int32_t C, int64_t HW,
                           hipStream_t stream) {
  const int per = images_per_workgroup(N, C, HW), parts = (N + per - 1) / per;
  SRGAN_REQUIRE(parts <= 65535, SRGAN_ERANGE, "srgan_batch_norm_train_bwd_apply grid");
  const float inv_count = (float)(1.0 / ((double)N * (double)HW));
  const int slot = profile_bracket_begin(stream);
  if (vectorisable(HW, {g, x, gx}))
    hipLaunchKernelGGL(bn_train_bwd_apply_kernel<4>, dim3(C, parts), dim3(256), 0, stream, g, x, mean, inv_std, gamma, beta, slope,
                       sums, gx, N, C, HW, per, inv_count);
  else
    hipLaunchKernelGGL(bn_train_bwd_apply_kernel<1>, dim3(C, parts), dim3(256), 0, stream, g, x, mean, inv_std, gamma, beta, slope,
                       sums, gx, N, C, HW, per, inv_count);
  const int status = launch_status();
  finish_bracket(slot, stream, N, C, HW, KIND_BN_BWD_APPLY, per, parts, 3.0);
  return status;
}

}  // namespace srgan

using namespace srgan;

extern "C" {

int srgan_batch_norm_train_stats(const float* x, float* mean, float* inv_std, float* running_mean, float* running_var,
                                 int64_t* num_batches_tracked, float momentum, float eps, int32_t N, int32_t C, int64_t HW,
                                 void* stream) {
  if (const int status = shape_status(N, C, HW, "srgan_batch_norm_train_stats shape")) return status;
  SRGAN_REQUIRE(x && mean && inv_std && (int64_t)N * HW >= 2 && eps >= 0.f, SRGAN_EINVAL,
                "srgan_batch_norm_train_stats arguments (at least two values per channel)");
  SRGAN_REQUIRE((int64_t)N * HW <= ((int64_t)1 << 24), SRGAN_ERANGE,
                "srgan_batch_norm_train_stats: at most 2^24 values per channel (the counts are carried as fp32)");
  return bn_train_stats_run(x, mean, inv_std, running_mean, running_var, num_batches_tracked, momentum, eps, N, C, HW,
                            (hipStream_t)stream);
}

int srgan_batch_norm_train_fwd(const float* x, const float* mean, const float* inv_std, const float* gamma, const float* beta,
                               float slope, float* y, int32_t N, int32_t C, int64_t HW, void* stream) {
  if (const int status = shape_status(N, C, HW, "srgan_batch_norm_train_fwd shape")) return status;
  SRGAN_REQUIRE(x && mean && inv_std && gamma && beta && y, SRGAN_EINVAL, "srgan_batch_norm_train_fwd arguments");
  return bn_train_fwd_run(x, mean, inv_std, gamma, beta, slope, y, N, C, HW, (hipStream_t)stream);
}

int srgan_batch_norm_train_bwd_reduce(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                                      const float* beta, float slope, float* sums, float* g_gamma, float* g_beta, int32_t N,
                                      int32_t C, int64_t HW, void* stream) {
  if (const int status = shape_status(N, C, HW, "srgan_batch_norm_train_bwd_reduce shape")) return status;
  SRGAN_REQUIRE(g && x && mean && inv_std && gamma && beta && sums, SRGAN_EINVAL, "srgan_batch_norm_train_bwd_reduce arguments");
  return bn_train_bwd_reduce_run(g, x, mean, inv_std, gamma, beta, slope, sums, g_gamma, g_beta, N, C, HW, (hipStream_t)stream);
}

int srgan_batch_norm_train_bwd_apply(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                                     const float* beta, float slope, const float* sums, float* gx, int32_t N, int32_t C, int64_t HW,
                                     void* stream) {
  if (const int status = shape_status(N, C, HW, "srgan_batch_norm_train_bwd_apply shape")) return status;
  SRGAN_REQUIRE(g && x && mean && inv_std && gamma && beta && sums && gx, SRGAN_EINVAL,
                "srgan_batch_norm_train_bwd_apply arguments");
  return bn_train_bwd_apply_run(g, x, mean, inv_std, gamma, beta, slope, sums, gx, N, C, HW, (hipStream_t)stream);
}

}  // extern "C"
