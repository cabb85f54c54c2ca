// blocked16_batch_norm.hip -- training-mode batch normalisation (batch statistics) on tensors in the BLOCKED layout of
// blocked16.h ([N][ceil(C / g)][H][W][g], g = 8 for bf16 / fp16, 4 for fp32: one 16-byte slot per pixel and channel group),
// so that a DCGAN generator with norm layers stays on the blocked kernels end to end (batch_norm_train.hip is the fp32 NCHW
// twin; bn_train.h holds what the two share).
//
// Five HBM-bound kernels on one decomposition: a workgroup owns channel GROUP g of a run of images [n0, n1), lanes along
// the pixels of the (image, group) planes, every access one whole slot (16 bytes); all arithmetic fp32 between h_unpack and
// h_pack (one rounding to nearest even at the store):
//   stats       one read of x  -> mean, inv_std (+ the running buffers and num_batches_tracked)
//   forward     one read, one write: y = leaky((x - mean) * inv_std * gamma + beta, slope); eval mode passes running statistics
//   bwd reduce  reads s, x     -> sum s, sum s * xhat per channel (= g_beta, g_gamma; accumulated when asked)
//   bwd apply   reads s, x (and the mask reference of x), writes gx = gamma * inv_std * (s - sum s / M - xhat * sum s xhat / M)
//   frozen bwd  the norm with GIVEN statistics (the frozen layers of D / DNN): a per-channel affine map, so ONE pass reads s
//               (and x for the gamma sums, the mask reference for gx) -> gx = s * gamma * inv_std, g_gamma, g_beta
// `s` follows the blocked path's pre-masked convention (blocked16.py): it arrives multiplied by the derivative of this layer's
// activation, so the backward kernels know no slope of their own; `ref` / `slope` of the apply kernel are the mask of the
// tensor x itself (epi 2 of the contraction kernels).
//
// A thread keeps g running (mean, M2) pairs and ONE count -- the g channels of a slot always come together -- and merges a
// tile of four slots at a time by Chan's formula; thread, wave, workgroup as in batch_norm_train.hip, and the workgroups of a
// group meet in the stream's workspace in part order (split_finish.h's ticket protocol: no fp32 atomics on data).
// Channels beyond C in the last group are written as zeros and never index a per-channel array.
// Roofline: HBM; algorithmic bytes = element size * elements per tensor read or written.
#include "blocked16.h"
#include "bn_train.h"
#include "common.h"
#include "launchers.h"
#include "split_finish.h"

namespace srgan {

__device__ unsigned int g_h_bn_tickets[SPLIT_TICKET_SETS * ROW_FINISH_ROWS];

// Slot index of element `idx` of the workgroup's chunk: group g of images n0, n0 + 1, ...
__device__ __forceinline__ int64_t h_bn_slot(int idx, int HW, int n0, int CG, int g) {
  const int nl = idx / HW, i = idx - nl * HW;
  return ((int64_t)(n0 + nl) * CG + g) * HW + i;
}

template <int PREC>
__global__ __launch_bounds__(256) void h_bn_stats_kernel(const Slot* __restrict__ x, float* __restrict__ mean_out,
                                                         float* __restrict__ inv_std_out, float* running_mean, float* running_var,
                                                         long long* batches_tracked, float momentum, float eps, int N, int C,
                                                         int HW, int images_per_block, float* partial, unsigned int* tickets) {
  constexpr int G = HGroup<PREC>::N;
  __shared__ Moments scratch[4][G];
  const int tid = (int)threadIdx.x, g = (int)blockIdx.x, CG = (int)gridDim.x, part = (int)blockIdx.y, parts = (int)gridDim.y;
  const int n0 = part * images_per_block, n1 = min(N, n0 + images_per_block);
  const int total = (n1 - n0) * HW;
  float count = 0.f, mean[G], m2[G];
#pragma unroll
  for (int j = 0; j < G; ++j) mean[j] = m2[j] = 0.f;
  for (int base = 0; base < total; base += 1024) {      // a tile: four slot loads per thread in flight, kept in registers
    float v[4][G];
    bool ok[4];
    int slots = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = base + q * 256 + tid;
      ok[q] = idx < total;
      if (ok[q]) {
        h_unpack<PREC>(x[h_bn_slot(idx, HW, n0, CG, g)], v[q]);
        ++slots;
      } else {
#pragma unroll
        for (int j = 0; j < G; ++j) v[q][j] = 0.f;
      }
    }
    if (slots == 0) continue;
    // Chan's merge of the tile into the running moments; the count and hence the weight are the same for all G channels
    // (tile_mean needs no exact division: M2 about a point within an ulp of the mean differs from the true one by
    // n * ulp^2, and 1 / 1, 1 / 2, 1 / 4 are exact anyway)
    const float tile_n = (float)slots, per_n = 1.f / tile_n, merged_n = count + tile_n, w = tile_n / merged_n, cross = count * w;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float tile_mean = ((v[0][j] + v[1][j]) + (v[2][j] + v[3][j])) * per_n;
      float tile_m2 = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (ok[q]) { const float d = v[q][j] - tile_mean; tile_m2 = fmaf(d, d, tile_m2); }
      const float delta = tile_mean - mean[j];
      mean[j] = fmaf(delta, w, mean[j]);
      m2[j] += tile_m2 + delta * delta * cross;
    }
    count = merged_n;
  }
  // Workgroup: every channel's wave tree first (shuffles only), ONE barrier, then thread j merges the four waves of channel j
  // (the fixed tree of block_moments_256, all g channels side by side instead of g barriers in a row).
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const Moments w = wave_moments(Moments{count, mean[j], m2[j]});
    if (lane == 0) scratch[wave][j] = w;
  }
  __syncthreads();
  Moments mine{0.f, 0.f, 0.f};                             // thread j < G: channel j of this workgroup's images
  if (tid < G) mine = merge_four_moments(scratch[0][tid], scratch[1][tid], scratch[2][tid], scratch[3][tid]);
  // the group's workgroups meet in the workspace in part order, in the same tree (split_finish.h)
  if (!ordered_lane_finish<LaneMoments, G>(mine, partial + (int64_t)g * parts * (3 * G), part, parts, tickets + g, scratch)) return;
  const int c = g * G + tid;
  if (tid == 0 && g == 0 && batches_tracked) *batches_tracked += 1;
  if (tid >= G || c >= C) return;
  const float variance = mine.m2 / mine.n;                 // biased: the one the batch is normalised with
  mean_out[c] = mine.mean;
  inv_std_out[c] = 1.f / sqrtf(variance + eps);
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mine.mean;
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (mine.m2 / (mine.n - 1.f));   // unbiased
}

// Visit the workgroup's chunk: f(slot index) for every slot of group blockIdx.x in this workgroup's images.
template <typename F>
__device__ __forceinline__ void h_bn_for_chunk(int N, int HW, int images_per_block, F f) {
  const int g = (int)blockIdx.x, CG = (int)gridDim.x;
  const int n0 = (int)blockIdx.y * images_per_block, n1 = min(N, n0 + images_per_block);
  const int total = (n1 - n0) * HW;
#pragma unroll 4
  for (int idx = (int)threadIdx.x; idx < total; idx += 256) f(h_bn_slot(idx, HW, n0, CG, g));
}

template <int PREC>
__global__ __launch_bounds__(256) void h_bn_fwd_kernel(const Slot* __restrict__ x, const float* __restrict__ mean,
                                                       const float* __restrict__ inv_std, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float slope, Slot* __restrict__ y, int N,
                                                       int C, int HW, int images_per_block) {
  constexpr int G = HGroup<PREC>::N;
  const int first = (int)blockIdx.x * G, live = min(G, C - first);
  float mu[G], a[G], b[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const bool real = j < live;
    mu[j] = real ? mean[first + j] : 0.f;
    a[j] = real ? bn_train_scale(inv_std[first + j], gamma[first + j]) : 0.f;
    b[j] = real ? beta[first + j] : 0.f;
  }
  h_bn_for_chunk(N, HW, images_per_block, [&](int64_t at) {
    float v[G];
    h_unpack<PREC>(x[at], v);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float pre = bn_train_pre(v[j], mu[j], a[j], b[j]);
      v[j] = j < live ? (pre > 0.f ? pre : pre * slope) : 0.f;
    }
    y[at] = h_pack<PREC>(v);
  });
}

template <int PREC>
__global__ __launch_bounds__(256) void h_bn_bwd_reduce_kernel(const Slot* __restrict__ s, const Slot* __restrict__ x,
                                                              const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                              float* __restrict__ sums, float* g_gamma, float* g_beta, int N, int C,
                                                              int HW, int images_per_block, float* partial, unsigned int* tickets) {
  constexpr int G = HGroup<PREC>::N;
  __shared__ float waves[4][2 * G];
  __shared__ float scratch[4];
  const int g = (int)blockIdx.x, first = g * G, live = min(G, C - first);
  float mu[G], is[G], plain[G], weighted[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    mu[j] = j < live ? mean[first + j] : 0.f;
    is[j] = j < live ? inv_std[first + j] : 0.f;
    plain[j] = weighted[j] = 0.f;
  }
  h_bn_for_chunk(N, HW, images_per_block, [&](int64_t at) {
    float sv[G], xv[G];
    h_unpack<PREC>(s[at], sv);
    h_unpack<PREC>(x[at], xv);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      plain[j] += sv[j];
      weighted[j] = fmaf(sv[j], (xv[j] - mu[j]) * is[j], weighted[j]);
    }
  });
  // the 2 g sums of the workgroup with ONE barrier: every wave's butterfly first, then the four waves in a fixed order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const float a = wave_sum(plain[j]), b = wave_sum(weighted[j]);
    if (lane == 0) { waves[wave][j] = a; waves[wave][G + j] = b; }
  }
  __syncthreads();
  float v[2 * G];
#pragma unroll
  for (int i = 0; i < 2 * G; ++i) v[i] = (waves[0][i] + waves[1][i]) + (waves[2][i] + waves[3][i]);
  const int parts = (int)gridDim.y;
  if (ordered_row_finish<2 * G>(v, partial ? partial + (int64_t)g * parts * (2 * G) : nullptr, (int)blockIdx.y, parts,
                                tickets ? tickets + g : nullptr, scratch)) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (j >= live) break;
      const int c = first + j;
      sums[c] = v[j];
      sums[C + c] = v[G + j];
      if (g_beta) g_beta[c] += v[j];
      if (g_gamma) g_gamma[c] += v[G + j];
    }
  }
}

template <int PREC>
__global__ __launch_bounds__(256) void h_bn_bwd_apply_kernel(const Slot* __restrict__ s, const Slot* __restrict__ x,
                                                             const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                             const float* __restrict__ gamma, const float* __restrict__ sums,
                                                             const Slot* __restrict__ ref, float slope, Slot* __restrict__ gx, int N,
                                                             int C, int HW, int images_per_block, float inv_count) {
  constexpr int G = HGroup<PREC>::N;
  const int first = (int)blockIdx.x * G, live = min(G, C - first);
  float mu[G], is[G], a[G], mean_s[G], mean_sx[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const bool real = j < live;
    mu[j] = real ? mean[first + j] : 0.f;
    is[j] = real ? inv_std[first + j] : 0.f;
    a[j] = real ? bn_train_scale(is[j], gamma[first + j]) : 0.f;
    mean_s[j] = real ? sums[first + j] * inv_count : 0.f;
    mean_sx[j] = real ? sums[C + first + j] * inv_count : 0.f;
  }
  h_bn_for_chunk(N, HW, images_per_block, [&](int64_t at) {
    float sv[G], xv[G];
    h_unpack<PREC>(s[at], sv);
    h_unpack<PREC>(x[at], xv);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float value = a[j] * (sv[j] - mean_s[j] - (xv[j] - mu[j]) * is[j] * mean_sx[j]);
      sv[j] = j < live ? value : 0.f;
    }
    if (ref) {
      const Slot r = ref[at];
#pragma unroll
      for (int j = 0; j < G; ++j) sv[j] *= h_slot_positive<PREC>(r, j) ? 1.f : slope;
    }
    gx[at] = h_pack<PREC>(sv);
  });
}

// The backward of the norm with GIVEN statistics, y = (x - mean) * inv_std * gamma + beta: every derivative of a per-channel
// affine map is "scale per channel, then mask", so one pass serves the plain backward (gx and both parameter sums), the
// recorded backward (gx alone) and the double backward (s = the cotangent, x = the first sweep's gradient, mean = nullptr).
// GX: write gx = s * gamma * inv_std (times the mask of `ref`).  SUMS: 0 none, 1 sum s, 2 sum s and sum s * (x - mean); the
// sums leave as g_beta[c] += sum s, g_gamma[c] += inv_std[c] * sum s (x - mean), where the pointers are given.
// REF: `ref` is given.  A thread takes a TILE of four slots at a time: all their loads are issued before the first is used
// (the lambda loop of h_bn_for_chunk compiles to one load in flight per thread, which leaves a workgroup of a few slots per
// thread waiting for HBM latency four times in a row); a slot beyond the chunk re-reads the chunk's last slot and counts as zero.
template <int PREC, bool GX, int SUMS, bool REF>
__global__ __launch_bounds__(256) void h_frozen_norm_bwd_kernel(const Slot* __restrict__ s, const Slot* __restrict__ x,
                                                                const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                                const float* __restrict__ gamma, const Slot* __restrict__ ref,
                                                                float slope, Slot* __restrict__ gx, float* g_gamma, float* g_beta,
                                                                int N, int C, int HW, int images_per_block, float* partial,
                                                                unsigned int* tickets) {
  constexpr int G = HGroup<PREC>::N;
  constexpr int V = SUMS == 2 ? 2 * G : G;
  const int g = (int)blockIdx.x, CG = (int)gridDim.x, first = g * G, live = min(G, C - first);
  float mu[G], a[G], plain[G], weighted[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const bool real = j < live;
    mu[j] = (real && mean) ? mean[first + j] : 0.f;
    a[j] = real ? bn_train_scale(inv_std[first + j], gamma[first + j]) : 0.f;
    plain[j] = weighted[j] = 0.f;
  }
  const int n0 = (int)blockIdx.y * images_per_block, n1 = min(N, n0 + images_per_block);
  const int total = (n1 - n0) * HW;                          // >= 1: every workgroup of the grid owns an image
  for (int base = 0; base < total; base += 1024) {
    int64_t at[4];
    bool ok[4];
    Slot sq[4], xq[4], rq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = base + q * 256 + (int)threadIdx.x;
      ok[q] = idx < total;
      at[q] = h_bn_slot(min(idx, total - 1), HW, n0, CG, g);
      sq[q] = s[at[q]];
      if constexpr (SUMS == 2) xq[q] = x[at[q]];
      if constexpr (GX && REF) rq[q] = ref[at[q]];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float sv[G];
      h_unpack<PREC>(sq[q], sv);
      if constexpr (SUMS >= 1) {
#pragma unroll
        for (int j = 0; j < G; ++j) sv[j] = ok[q] ? sv[j] : 0.f;
      }
      if constexpr (SUMS == 2) {
        float xv[G];
        h_unpack<PREC>(xq[q], xv);
#pragma unroll
        for (int j = 0; j < G; ++j) weighted[j] = fmaf(sv[j], xv[j] - mu[j], weighted[j]);
      }
      if constexpr (SUMS >= 1) {
#pragma unroll
        for (int j = 0; j < G; ++j) plain[j] += sv[j];
      }
      if constexpr (GX) {
#pragma unroll
        for (int j = 0; j < G; ++j) sv[j] = j < live ? sv[j] * a[j] : 0.f;
        if constexpr (REF) {
#pragma unroll
          for (int j = 0; j < G; ++j) sv[j] *= h_slot_positive<PREC>(rq[q], j) ? 1.f : slope;
        }
        if (ok[q]) gx[at[q]] = h_pack<PREC>(sv);
      }
    }
  }
  if constexpr (SUMS >= 1) {
    // the workgroup's V sums with ONE barrier (every wave's butterfly first, then the four waves in a fixed order: thread i holds
    // sum i), then the workgroups of the group in part order through the workspace, in the same tree (split_finish.h)
    __shared__ float waves[4][V];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int parts = (int)gridDim.y;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float p = wave_sum(plain[j]);
      if (lane == 0) waves[wave][j] = p;
      if constexpr (SUMS == 2) {
        const float w = wave_sum(weighted[j]);
        if (lane == 0) waves[wave][G + j] = w;
      }
    }
    __syncthreads();
    float mine = 0.f;                                        // thread i < V: sum i of this workgroup's images
    if (tid < V) mine = (waves[0][tid] + waves[1][tid]) + (waves[2][tid] + waves[3][tid]);
    if (!ordered_lane_finish<LaneSums, V>(mine, partial + (int64_t)g * parts * V, (int)blockIdx.y, parts, tickets + g, waves)) return;
    // thread j adds sum s of channel j to g_beta, thread G + j the weighted sum to g_gamma
    const int j = tid < G ? tid : tid - G;
    if (tid >= V || j >= live) return;
    const int c = first + j;
    if (tid < G) { if (g_beta) g_beta[c] += mine; }
    else if (g_gamma) g_gamma[c] += inv_std[c] * mine;
  }
}

// What the four batch-statistics entry points check before any device work.
static int h_bn_arguments(int32_t N, int32_t C, int64_t HW, int32_t dtype, bool pointers, const char* what) {
  if (const int status = check_precision<0, 1, 2>(dtype, what)) return status;
  SRGAN_REQUIRE(pointers && N > 0 && C > 0 && HW > 0, SRGAN_EINVAL, what);
  const int64_t M = HW > ((int64_t)1 << 24) ? HW : (int64_t)N * HW;      // values per channel (no overflow: N < 2^31)
  SRGAN_REQUIRE(M >= 2, SRGAN_EINVAL, what);
  // the partial counts are carried as fp32; this also keeps a workgroup's chunk inside 32-bit indices
  SRGAN_REQUIRE(M <= ((int64_t)1 << 24), SRGAN_ERANGE, what);
  return SRGAN_OK;
}

struct HBnGrid : RowFinishGrid { int group, CG; };

// Images per workgroup as the NCHW kernels choose them, a slot counted as its 16 bytes = four fp32 elements.
static HBnGrid h_bn_grid(int32_t N, int32_t C, int64_t HW, int32_t dtype) {
  HBnGrid grid;
  grid.group = slot_channels(dtype);
  grid.CG = channel_groups(C, dtype);
  grid.per = images_per_workgroup(N, grid.CG, HW * 4);
  grid.parts = (N + grid.per - 1) / grid.per;
  return grid;
}

// Records of the live profile: kinds 20 .. 23 as batch_norm_train.hip, 24 the frozen backward; the algorithmic bytes from the
// element size.
static int h_bn_bracket(int slot, hipStream_t stream, int32_t N, int32_t C, int64_t HW, int32_t dtype, LaunchKind kind, const HBnGrid& grid,
                        double tensors) {
  const double element = dtype == 0 ? 4.0 : 2.0;
  return profile_bracket_end_bytes(slot, stream, C, (int64_t)N * HW, 0, kind, 256, grid.per, grid.parts,
                                   element * tensors * (double)N * C * (double)HW, 0);
}

// The modes of h_frozen_norm_bwd_kernel that a call can ask for: gx alone (SUMS 0), sums alone with or without the gamma sums,
// both; the mask reference counts only where gx is written (the GX = false forms with REF are compiled here and never chosen).
template <int PREC, bool GX, int SUMS>
static auto h_frozen_kernel(bool masked) {
  return masked && GX ? h_frozen_norm_bwd_kernel<PREC, GX, SUMS, true> : h_frozen_norm_bwd_kernel<PREC, GX, SUMS, false>;
}

int h_frozen_norm_bwd_run(const void* s, const void* x, const float* mean, const float* inv_std, const float* gamma, const void* ref,
                          float slope, void* gx, float* g_gamma, float* g_beta, int32_t N, int32_t C, int64_t HW, int32_t dtype,
                          hipStream_t stream) {
  const char* what = "srgan_h_frozen_norm_bwd arguments";
  if (const int status = check_precision<0, 1, 2>(dtype, what)) return status;
  SRGAN_REQUIRE(s && inv_std && gamma && N > 0 && C > 0 && HW > 0, SRGAN_EINVAL, what);
  SRGAN_REQUIRE(gx || g_gamma || g_beta, SRGAN_EINVAL, what);
  SRGAN_REQUIRE(x || !g_gamma, SRGAN_EINVAL, what);
  // max_tensor_elements; this also keeps a workgroup's chunk (at most N * HW slots) inside 32-bit indices
  SRGAN_REQUIRE(HW <= (((int64_t)1 << 31) - 1) / ((int64_t)N * C), SRGAN_ERANGE, "srgan_h_frozen_norm_bwd tensor size (2^31 - 1 elements)");
  HBnGrid grid = h_bn_grid(N, C, HW, dtype);
  const int sums = g_gamma ? 2 : (g_beta ? 1 : 0);
  // a workgroup that reduces pays for its g (2 g) trees, its partials and its ticket whatever it read: at least 4096 slots each
  // while that leaves 256 workgroups
  while (sums && grid.per < N && (int64_t)grid.per * HW < 4096 && (int64_t)grid.CG * ((N + 2 * grid.per - 1) / (2 * grid.per)) >= 256)
    grid.per *= 2;
  grid.parts = (N + grid.per - 1) / grid.per;
  if (sums) {
    if (const int status = row_finish_grid(grid.CG, N, sums * grid.group, g_h_bn_tickets, stream, "srgan_h_frozen_norm_bwd grid", &grid)) return status;
  } else {
    SRGAN_REQUIRE(grid.parts <= 65535, SRGAN_ERANGE, "srgan_h_frozen_norm_bwd grid");
  }
  const int slot = profile_bracket_begin(stream);
  const int status = launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    constexpr int PREC = decltype(prec)::value;
    const bool masked = ref != nullptr;
    const auto kernel = gx ? (sums == 2   ? h_frozen_kernel<PREC, true, 2>(masked)
                              : sums == 1 ? h_frozen_kernel<PREC, true, 1>(masked)
                                          : h_frozen_kernel<PREC, true, 0>(masked))
                           : (sums == 2 ? h_frozen_kernel<PREC, false, 2>(masked) : h_frozen_kernel<PREC, false, 1>(masked));
    hipLaunchKernelGGL(kernel, dim3(grid.CG, grid.parts), dim3(256), 0, stream, (const Slot*)s, (const Slot*)x, mean, inv_std, gamma,
                       (const Slot*)ref, slope, (Slot*)gx, g_gamma, g_beta, N, C, (int)HW, grid.per, grid.partial, grid.tickets);
  });
  h_bn_bracket(slot, stream, N, C, HW, dtype, KIND_H_FROZEN_NORM_BWD, grid, 1.0 + (sums == 2) + (gx != nullptr) + (gx && ref));
  return status;
}

}  // namespace srgan

using namespace srgan;

extern "C" {

int srgan_h_batch_norm_stats(const void* x, float* mean, float* inv_std, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, float momentum, float eps, int32_t N, int32_t C, int64_t HW,
                             int32_t dtype, void* stream) {
  if (const int status = h_bn_arguments(N, C, HW, dtype, x && mean && inv_std, "srgan_h_batch_norm_stats arguments")) return status;
  SRGAN_REQUIRE(eps >= 0.f, SRGAN_EINVAL, "srgan_h_batch_norm_stats arguments");
  hipStream_t s = (hipStream_t)stream;
  HBnGrid grid = h_bn_grid(N, C, HW, dtype);
  if (const int status = row_finish_grid(grid.CG, N, 3 * grid.group, g_h_bn_tickets, s, "srgan_h_batch_norm_stats grid", &grid)) return status;
  const int slot = profile_bracket_begin(s);
  const int status = launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_bn_stats_kernel<decltype(prec)::value>, dim3(grid.CG, grid.parts), dim3(256), 0, s, (const Slot*)x, mean, inv_std,
                       running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), momentum, eps, N, C, (int)HW,
                       grid.per, grid.partial, grid.tickets);
  });
  h_bn_bracket(slot, s, N, C, HW, dtype, KIND_BN_STATS, grid, 1.0);
  return status;
}

int srgan_h_batch_norm_fwd(const void* x, const float* mean, const float* inv_std, const float* gamma, const float* beta,
                           float slope, void* y, int32_t N, int32_t C, int64_t HW, int32_t dtype, void* stream) {
  if (const int status = h_bn_arguments(N, C, HW, dtype, x && mean && inv_std && gamma && beta && y, "srgan_h_batch_norm_fwd arguments"))
    return status;
  hipStream_t s = (hipStream_t)stream;
  const HBnGrid grid = h_bn_grid(N, C, HW, dtype);
  SRGAN_REQUIRE(grid.parts <= 65535, SRGAN_ERANGE, "srgan_h_batch_norm_fwd grid");
  const int slot = profile_bracket_begin(s);
  const int status = launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_bn_fwd_kernel<decltype(prec)::value>, dim3(grid.CG, grid.parts), dim3(256), 0, s, (const Slot*)x, mean, inv_std,
                       gamma, beta, slope, (Slot*)y, N, C, (int)HW, grid.per);
  });
  h_bn_bracket(slot, s, N, C, HW, dtype, KIND_BN_FWD, grid, 2.0);
  return status;
}

int srgan_h_batch_norm_bwd_reduce(const void* s, const void* x, const float* mean, const float* inv_std, float* sums,
                                  float* g_gamma, float* g_beta, int32_t N, int32_t C, int64_t HW, int32_t dtype, void* stream) {
  if (const int status = h_bn_arguments(N, C, HW, dtype, s && x && mean && inv_std && sums, "srgan_h_batch_norm_bwd_reduce arguments"))
    return status;
  hipStream_t st = (hipStream_t)stream;
  HBnGrid grid = h_bn_grid(N, C, HW, dtype);
  if (const int status = row_finish_grid(grid.CG, N, 2 * grid.group, g_h_bn_tickets, st, "srgan_h_batch_norm_bwd_reduce grid", &grid)) return status;
  const int slot = profile_bracket_begin(st);
  const int status = launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_bn_bwd_reduce_kernel<decltype(prec)::value>, dim3(grid.CG, grid.parts), dim3(256), 0, st, (const Slot*)s,
                       (const Slot*)x, mean, inv_std, sums, g_gamma, g_beta, N, C, (int)HW, grid.per, grid.partial, grid.tickets);
  });
  h_bn_bracket(slot, st, N, C, HW, dtype, KIND_BN_BWD_REDUCE, grid, 2.0);
  return status;
}

int srgan_h_batch_norm_bwd_apply(const void* s, const void* x, const float* mean, const float* inv_std, const float* gamma,
                                 const float* sums, const void* ref, float slope, void* gx, int32_t N, int32_t C, int64_t HW,
                                 int32_t dtype, void* stream) {
  if (const int status = h_bn_arguments(N, C, HW, dtype, s && x && mean && inv_std && gamma && sums && gx,
                                        "srgan_h_batch_norm_bwd_apply arguments"))
    return status;
  hipStream_t st = (hipStream_t)stream;
  const HBnGrid grid = h_bn_grid(N, C, HW, dtype);
  SRGAN_REQUIRE(grid.parts <= 65535, SRGAN_ERANGE, "srgan_h_batch_norm_bwd_apply grid");
  const float inv_count = (float)(1.0 / ((double)N * (double)HW));
  const int slot = profile_bracket_begin(st);
  const int status = launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_bn_bwd_apply_kernel<decltype(prec)::value>, dim3(grid.CG, grid.parts), dim3(256), 0, st, (const Slot*)s,
                       (const Slot*)x, mean, inv_std, gamma, sums, (const Slot*)ref, slope, (Slot*)gx, N, C, (int)HW, grid.per, inv_count);
  });
  h_bn_bracket(slot, st, N, C, HW, dtype, KIND_BN_BWD_APPLY, grid, 3.0);
  return status;
}

int srgan_h_frozen_norm_bwd(const void* s, const void* x, const float* mean, const float* inv_std, const float* gamma,
                            const void* ref, float slope, void* gx, float* g_gamma, float* g_beta, int32_t N, int32_t C, int64_t HW,
                            int32_t dtype, void* stream) {
  return h_frozen_norm_bwd_run(s, x, mean, inv_std, gamma, ref, slope, gx, g_gamma, g_beta, N, C, HW, dtype, (hipStream_t)stream);
}

}  // extern "C"
