// blocked16_streaming.hip -- the HBM-bound kernels of the blocked data path (layout: blocked16.h), one thread per 16-byte slot.
//
// They serve what lies between the matrix kernels of the blocked networks: pack / unpack carry a tensor between fp32 NCHW and
// the blocked layout (the loss side stays fp32; pack can apply the mask by reference on the way in), add joins two gradient
// branches, the channel sums are the bias gradient of a fused convolution / linear layer, and the 2x2 max-pool with its
// backward and arg-max gather is VGG-16's pooling (reference age/vgg.py:76) in all three passes.
//
//   h_pack / h_unpack / h_add      dtype 0 (fp32, four channels per slot), 1 (bf16), 2 (fp16)
//   h_channel_sums (+ finish)      per-workgroup parts, added in part order (bit-reproducible): one launch with a ticket per
//                                  group (split_finish.h), two launches where the ordered finish is not available
//   h_maxpool / h_maxpool_bwd      16-bit only; the arg-max is recomputed (first maximum in scan order), never stored
#include <type_traits>
#include "blocked16.h"
#include "split_finish.h"

namespace srgan {

// fp32 NCHW -> blocked. One thread per slot (n, group, pixel): eight loads, each coalesced across the lanes along the
// plane.  Optional mask by reference (the gradient w.r.t. an activated tensor arrives here in fp32 from the loss side).
template <int PREC>
__global__ __launch_bounds__(256) void h_pack_kernel(const float* __restrict__ x, Slot* __restrict__ out,
                                                     const Slot* __restrict__ ref, float slope, int64_t slots, int32_t C,
                                                     int32_t CG, int32_t HW) {
  constexpr int G = HGroup<PREC>::N;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (int64_t)gridDim.x * 256) {
    const int pix = (int)(s % HW);
    const int64_t ng = s / HW;
    const int g = (int)(ng % CG);
    const int64_t n = ng / CG;
    float v[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int c = G * g + j;
      v[j] = c < C ? x[(n * C + c) * HW + pix] : 0.f;
    }
    if (ref) {
      const Slot r = ref[s];
#pragma unroll
      for (int j = 0; j < G; ++j) v[j] *= h_slot_positive<PREC>(r, j) ? 1.f : slope;
    }
    out[s] = h_pack<PREC>(v);
  }
}

template <int PREC>
__global__ __launch_bounds__(256) void h_unpack_kernel(const Slot* __restrict__ x, float* __restrict__ out, int64_t slots,
                                                       int32_t C, int32_t CG, int32_t HW) {
  constexpr int G = HGroup<PREC>::N;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (int64_t)gridDim.x * 256) {
    const int pix = (int)(s % HW);
    const int64_t ng = s / HW;
    const int g = (int)(ng % CG);
    const int64_t n = ng / CG;
    float v[G];
    h_unpack<PREC>(x[s], v);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int c = G * g + j;
      if (c < C) out[(n * C + c) * HW + pix] = v[j];
    }
  }
}

template <int PREC>
__global__ __launch_bounds__(256) void h_add_kernel(const Slot* __restrict__ a, const Slot* __restrict__ b,
                                                    Slot* __restrict__ out, int64_t slots) {
  constexpr int G = HGroup<PREC>::N;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (int64_t)gridDim.x * 256) {
    float x[G], y[G];
    h_unpack<PREC>(a[s], x);
    h_unpack<PREC>(b[s], y);
#pragma unroll
    for (int j = 0; j < G; ++j) x[j] += y[j];
    out[s] = h_pack<PREC>(x);
  }
}

// Channel sums (a bias gradient): part[(g * parts + part) * 8 + j] = sum over this block's share of (n, pixel) of channel
// 8g + j; h_channel_sums_finish_kernel adds the parts of a channel in part order into the fp32 gradient (bit-reproducible).
// `tickets` != NULL: ONE launch -- the group's last workgroup (a ticket per group and stream, split_finish.h) adds the parts in a
// fixed order and accumulates into `out` itself (the second launch was 47 launches of ~7 us per step of age-vgg-bf16).
__device__ unsigned int g_h_sum_tickets[SPLIT_TICKET_SETS * ROW_FINISH_ROWS];

template <int PREC>
__global__ __launch_bounds__(256) void h_channel_sums_kernel(const Slot* __restrict__ x, float* __restrict__ part, int32_t N,
                                                             int32_t CG, int32_t HW, int32_t parts, unsigned int* tickets,
                                                             float* __restrict__ out, int32_t C) {
  constexpr int G = HGroup<PREC>::N;
  __shared__ float scratch[4 * 8];
  __shared__ float finish_scratch[4];
  const int g = (int)blockIdx.x, part_id = (int)blockIdx.y;
  const int64_t total = (int64_t)N * HW;
  float sum[G];
#pragma unroll
  for (int j = 0; j < G; ++j) sum[j] = 0.f;
  for (int64_t i = (int64_t)part_id * 256 + threadIdx.x; i < total; i += (int64_t)parts * 256) {
    const int64_t n = i / HW;
    const int pix = (int)(i - n * HW);
    float v[G];
    h_unpack<PREC>(x[(n * CG + g) * HW + pix], v);
#pragma unroll
    for (int j = 0; j < G; ++j) sum[j] += v[j];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const float w = wave_sum(sum[j]);
    if (lane == 0) scratch[wave * 8 + j] = w;
  }
  __syncthreads();
  if (tickets == nullptr) {
    if (threadIdx.x < G) {
      const int j = threadIdx.x;
      part[((int64_t)g * parts + part_id) * 8 + j] = (scratch[j] + scratch[8 + j]) + (scratch[16 + j] + scratch[24 + j]);
    }
    return;
  }
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = j < G ? (scratch[j] + scratch[8 + j]) + (scratch[16 + j] + scratch[24 + j]) : 0.f;
  if (ordered_row_finish<8>(v, part + (int64_t)g * parts * 8, part_id, parts, tickets + g, finish_scratch)) {
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (g * G + j < C) out[g * G + j] += v[j];
  }
}

// `group` = channels per slot (8; 4 for the fp32 blocked form)
__global__ __launch_bounds__(256) void h_channel_sums_finish_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                    int32_t C, int32_t parts, int32_t group) {
  const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (c >= C) return;
  const float* mine = part + (int64_t)(c / group) * parts * 8 + (c % group);
  float total = 0.f;
  for (int s = 0; s < parts; ++s) total += mine[s * 8];
  out[c] += total;
}

// 2x2 / stride 2 max-pool (reference age/vgg.py:76).  The arg-max is not stored: every kernel that needs it finds the FIRST
// window position (scan order (0,0), (0,1), (1,0), (1,1): torch's tie rule) that holds the maximum.  With a NaN in the window
// this is NOT torch (which propagates it): `v > m` is false for a NaN on either side, so a NaN at position 0 stays and a NaN at
// positions 1 .. 3 is skipped (include/srgan_hip.h, NaN and mask rule; pinned by tests/test_blocked_streaming_gpu.py).
template <int PREC>
__device__ __forceinline__ void h_pool_window(const Slot* __restrict__ x, int64_t base, int32_t W, float (&m)[8], int (&at)[8]) {
  float v[4][8];
  h_unpack8<PREC>(x[base], v[0]);
  h_unpack8<PREC>(x[base + 1], v[1]);
  h_unpack8<PREC>(x[base + W], v[2]);
  h_unpack8<PREC>(x[base + W + 1], v[3]);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = v[0][j]; at[j] = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (v[q][j] > m[j]) { m[j] = v[q][j]; at[j] = q; }
  }
}

// mode 0: out = pool(x)             [pooled shape]
// mode 2: out = gather of `g` (input shape) at the arg-max of x      [pooled shape]   (the tangent of the double backward)
template <int PREC, int MODE>
__global__ __launch_bounds__(256) void h_maxpool_kernel(const Slot* __restrict__ x, const Slot* __restrict__ g,
                                                        Slot* __restrict__ out, int64_t planes, int32_t H, int32_t W) {
  const int OH = H / 2, OW = W / 2;
  const int64_t total = planes * OH * OW;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < total; s += (int64_t)gridDim.x * 256) {
    const int ox = (int)(s % OW);
    const int64_t rest = s / OW;
    const int oy = (int)(rest % OH);
    const int64_t plane = rest / OH;
    const int64_t base = (plane * H + 2 * oy) * W + 2 * ox;
    float m[8]; int at[8];
    h_pool_window<PREC>(x, base, W, m, at);
    if (MODE == 0) {
      out[s] = h_pack8<PREC>(m);
    } else {
      float v[4][8], r[8];
      h_unpack8<PREC>(g[base], v[0]);
      h_unpack8<PREC>(g[base + 1], v[1]);
      h_unpack8<PREC>(g[base + W], v[2]);
      h_unpack8<PREC>(g[base + W + 1], v[3]);
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = at[j] == 0 ? v[0][j] : (at[j] == 1 ? v[1][j] : (at[j] == 2 ? v[2][j] : v[3][j]));
      out[s] = h_pack8<PREC>(r);
    }
  }
}

// Backward: gx (input shape) = the pooled gradient placed at the arg-max, times the derivative of the activation that
// produced x (mask by x itself when `masked`): the gradient w.r.t. the PRE-activation tensor in one pass.
template <int PREC>
__global__ __launch_bounds__(256) void h_maxpool_bwd_kernel(const Slot* __restrict__ x, const Slot* __restrict__ gp,
                                                            Slot* __restrict__ gx, int64_t planes, int32_t H, int32_t W,
                                                            int masked, float slope) {
  const int OH = H / 2, OW = W / 2;
  const int64_t total = planes * OH * OW;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < total; s += (int64_t)gridDim.x * 256) {
    const int ox = (int)(s % OW);
    const int64_t rest = s / OW;
    const int oy = (int)(rest % OH);
    const int64_t plane = rest / OH;
    const int64_t base = (plane * H + 2 * oy) * W + 2 * ox;
    float m[8]; int at[8];
    h_pool_window<PREC>(x, base, W, m, at);
    float g[8];
    h_unpack8<PREC>(gp[s], g);
    if (masked) {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] *= h_positive_unpacked(m[j]) ? 1.f : slope;
    }
    float r[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) r[q][j] = at[j] == q ? g[j] : 0.f;
    gx[base] = h_pack8<PREC>(r[0]);
    gx[base + 1] = h_pack8<PREC>(r[1]);
    gx[base + W] = h_pack8<PREC>(r[2]);
    gx[base + W + 1] = h_pack8<PREC>(r[3]);
  }
}

}  // namespace srgan

using namespace srgan;

extern "C" {

int srgan_h_pack(const float* x, void* out, const void* mask_ref, float slope, int32_t N, int32_t C, int64_t HW, int dtype,
                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<0, 1, 2>(dtype, H16_OR_F32)) return status;
  SRGAN_REQUIRE(x && out && N >= 0 && C > 0 && HW > 0 && HW < ((int64_t)1 << 31), SRGAN_EINVAL, "srgan_h_pack arguments");
  const int CG = channel_groups(C, dtype);
  const int64_t slots = (int64_t)N * CG * HW;
  if (slots == 0) return SRGAN_OK;
  const dim3 grid(stream_grid(slots, 256));
  return launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_pack_kernel<decltype(prec)::value>, grid, dim3(256), 0, s, x, (Slot*)out, (const Slot*)mask_ref, slope, slots, C, CG, (int32_t)HW);
  });
}

int srgan_h_unpack(const void* x, float* out, int32_t N, int32_t C, int64_t HW, int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<0, 1, 2>(dtype, H16_OR_F32)) return status;
  SRGAN_REQUIRE(x && out && N >= 0 && C > 0 && HW > 0 && HW < ((int64_t)1 << 31), SRGAN_EINVAL, "srgan_h_unpack arguments");
  const int CG = channel_groups(C, dtype);
  const int64_t slots = (int64_t)N * CG * HW;
  if (slots == 0) return SRGAN_OK;
  const dim3 grid(stream_grid(slots, 256));
  return launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_unpack_kernel<decltype(prec)::value>, grid, dim3(256), 0, s, (const Slot*)x, out, slots, C, CG, (int32_t)HW);
  });
}

int srgan_h_add(const void* a, const void* b, void* out, int64_t slots, int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<0, 1, 2>(dtype, H16_OR_F32)) return status;
  SRGAN_REQUIRE(a && b && out && slots >= 0, SRGAN_EINVAL, "srgan_h_add arguments");
  if (slots == 0) return SRGAN_OK;
  const dim3 grid(stream_grid(slots, 256));
  return launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_add_kernel<decltype(prec)::value>, grid, dim3(256), 0, s, (const Slot*)a, (const Slot*)b, (Slot*)out, slots);
  });
}

// out[c] += sum over n and pixels of x[n, c, pixel]   (c < C; fp32; the bias gradient of a fused convolution / linear layer)
int srgan_h_channel_sums(const void* x, float* out, int32_t N, int32_t C, int64_t HW, int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<0, 1, 2>(dtype, H16_OR_F32)) return status;
  SRGAN_REQUIRE(x && out && N > 0 && C > 0 && HW > 0 && HW < ((int64_t)1 << 31), SRGAN_EINVAL, "srgan_h_channel_sums arguments");
  const int CG = channel_groups(C, dtype);
  const int64_t per_group = (int64_t)N * HW;
  int parts = (int)((per_group + 4095) / 4096);
  if (parts > 256) parts = 256;
  if (parts < 1) parts = 1;
  while (parts > 1 && (int64_t)parts * CG > 4096) parts >>= 1;
  unsigned int* tickets = nullptr;
  float* part = row_finish_workspace(CG, parts, 8, g_h_sum_tickets, s, &tickets);
  if (!part) {
    tickets = nullptr;
    part = partial_workspace((size_t)CG * parts * 8 * sizeof(float), s);
  }
  SRGAN_REQUIRE(part, SRGAN_EINVAL, "srgan_h_channel_sums: register a workspace for this stream first (srgan_set_workspace)");
  const dim3 grid((unsigned)CG, (unsigned)parts);
  return launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_channel_sums_kernel<decltype(prec)::value>, grid, dim3(256), 0, s, (const Slot*)x, part, N, CG, (int32_t)HW, parts, tickets, out, C);
    if (!tickets) hipLaunchKernelGGL(h_channel_sums_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, out, C, parts, slot_channels(dtype));
  });
}

// mode 0: out = maxpool2x2(x); mode 2: out = `g` gathered at the arg-max of x (both [planes][H/2][W/2] slots, planes = N * groups)
int srgan_h_maxpool2(const void* x, const void* g, void* out, int64_t planes, int32_t H, int32_t W, int mode, int dtype,
                     void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<1, 2>(dtype, H16_ONLY)) return status;
  SRGAN_REQUIRE(x && out && planes >= 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && (mode == 0 || (mode == 2 && g)),
                SRGAN_EINVAL, "srgan_h_maxpool2 arguments (even planes; mode 0 or 2)");
  const int64_t total = planes * (H / 2) * (W / 2);
  if (total == 0) return SRGAN_OK;
  const dim3 grid(stream_grid(total, 256));
  return launch_for_precision<1, 2>(dtype, [&](auto prec) {
    constexpr int PREC = decltype(prec)::value;
    if (mode == 0) hipLaunchKernelGGL((h_maxpool_kernel<PREC, 0>), grid, dim3(256), 0, s, (const Slot*)x, (const Slot*)g, (Slot*)out, planes, H, W);
    else hipLaunchKernelGGL((h_maxpool_kernel<PREC, 2>), grid, dim3(256), 0, s, (const Slot*)x, (const Slot*)g, (Slot*)out, planes, H, W);
  });
}

// gx (shape of x) = gp placed at the arg-max of x, times mask(x, slope) when `masked`
int srgan_h_maxpool2_bwd(const void* x, const void* gp, void* gx, int64_t planes, int32_t H, int32_t W, int masked, float slope,
                         int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<1, 2>(dtype, H16_ONLY)) return status;
  SRGAN_REQUIRE(x && gp && gx && planes >= 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, SRGAN_EINVAL,
                "srgan_h_maxpool2_bwd arguments");
  const int64_t total = planes * (H / 2) * (W / 2);
  if (total == 0) return SRGAN_OK;
  const dim3 grid(stream_grid(total, 256));
  return launch_for_precision<1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_maxpool_bwd_kernel<decltype(prec)::value>, grid, dim3(256), 0, s, (const Slot*)x, (const Slot*)gp, (Slot*)gx, planes, H, W, masked, slope);
  });
}

}  // extern "C"
