// crowd_full_image.hip -- the device side of the crowd application's full-image (sliding-window) inference, after the
// network: the float-mode bilinear resize of a density predicted below the patch resolution, and the overlap average of
// every window's density and uniformly spread count (reference crowd/srgan.py:332-395).  The windows themselves are cut
// by srgan_crowd_extract_windows (crowd_patches.hip).  Streaming kernels: a few bytes per pixel, HBM / latency bound.
#include "common.h"
#include "split_finish.h"

namespace srgan {

// out[b, oy, ox] of a [B, h, w] -> [B, P, P] upscale with half-pixel centres and clamped edges: the arithmetic of
// torch.nn.functional.interpolate(mode='bilinear', align_corners=False) (bilinear_source and bilinear_row_sample, common.h: the two
// horizontal lerps first).  Values are not rescaled: sums change.
template <int VEC>
__global__ __launch_bounds__(256) void crowd_resize_bilinear_kernel(const float* __restrict__ in, int h, int w, int P,
                                                                    int64_t runs, float* __restrict__ out) {
  const float scale_y = (float)h / (float)P, scale_x = (float)w / (float)P;
  for (int64_t run = (int64_t)blockIdx.x * 256 + threadIdx.x; run < runs; run += (int64_t)gridDim.x * 256) {
    const int64_t at = run * VEC;                 // (P % VEC == 0: a run never leaves its row)
    const int ox = (int)(at % P), oy = (int)((at / P) % P);
    const int64_t b = at / ((int64_t)P * P);
    int y0, y1;
    float ly;
    bilinear_source(scale_y, oy, h, y0, y1, ly);
    const float* top = in + (b * h + y0) * w;
    const float* bottom = in + (b * h + y1) * w;
    float v[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = bilinear_row_sample(top, bottom, ly, scale_x, ox + i, w);
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(out + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      out[at] = v[0];
    }
  }
}

// The overlap average as a GATHER: one thread per output pixel walks the windows that cover it in window-index order
// (y-major, then x: the order the host loop of CrowdExperiment.predict_full_example adds them in) from 0.0f, so the
// density map carries the host loop's bits.  Window (iy, ix) covers rows [ys[iy] - P/2, ys[iy] + P/2) and columns
// [xs[ix] - P/2, xs[ix] + P/2); a pixel no window covers divides by 1, as on the host.
//
// The scalar count = the sum over the pixels of count_sum / hits, in a fixed order: a thread adds its BLEND_PER_THREAD
// pixels (pixel = workgroup * 1024 + k * 256 + thread, k ascending: coalesced), the workgroup's 256 sums meet in the tree
// of block_sum_256, and the workgroups' sums meet through the stream's workspace in ordered_row_finish (split_finish.h:
// the last workgroup adds part t, t + 256, ... in thread t, then the same tree).  No atomics on data.
constexpr int BLEND_PER_THREAD = 4;
constexpr int BLEND_TILE = 256 * BLEND_PER_THREAD;
__device__ unsigned int g_blend_finish_tickets[SPLIT_TICKET_SETS * ROW_FINISH_ROWS];

__global__ __launch_bounds__(256) void crowd_blend_windows_kernel(const float* __restrict__ densities,
                                                                  const float* __restrict__ counts,
                                                                  const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
                                                                  int ny, int nx, int H, int W, int P,
                                                                  float* __restrict__ out_density, float* __restrict__ out_count,
                                                                  float* partial, unsigned int* ticket) {
  __shared__ float scratch[4];
  const int half = P / 2;
  const float patch_pixels = (float)(P * P);
  const int64_t plane = (int64_t)P * P, pixels = (int64_t)H * W;
  float mine = 0.f;
#pragma unroll
  for (int k = 0; k < BLEND_PER_THREAD; ++k) {
    const int64_t at = (int64_t)blockIdx.x * BLEND_TILE + k * 256 + threadIdx.x;
    if (at >= pixels) continue;
    const int py = (int)(at / W), px = (int)(at % W);
    float density_sum = 0.f, count_sum = 0.f;
    int hits = 0;
    for (int iy = 0; iy < ny; ++iy) {
      const int dy = py - (ys[iy] - half);
      if ((unsigned)dy >= (unsigned)P) continue;
      for (int ix = 0; ix < nx; ++ix) {
        const int dx = px - (xs[ix] - half);
        if ((unsigned)dx >= (unsigned)P) continue;
        const int window = iy * nx + ix;
        if (densities) density_sum += densities[window * plane + (int64_t)dy * P + dx];
        count_sum += counts[window] / patch_pixels;
        ++hits;
      }
    }
    const float covered = (float)(hits > 0 ? hits : 1);
    out_density[at] = density_sum / covered;
    mine += count_sum / covered;
  }
  float v[1] = {block_sum_256(mine, scratch)};
  __syncthreads();
  if (ordered_row_finish<1>(v, partial, (int)blockIdx.x, (int)gridDim.x, ticket, scratch)) *out_count = v[0];
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_crowd_resize_bilinear(const float* in, int32_t B, int32_t h, int32_t w, int32_t P, float* out,
                                           void* stream) {
  SRGAN_REQUIRE(in && out && B > 0 && h > 0 && w > 0 && P > 0, SRGAN_EINVAL, "srgan_crowd_resize_bilinear arguments");
  SRGAN_REQUIRE(P >= h && P >= w, SRGAN_EUNSUPPORTED, "srgan_crowd_resize_bilinear: downscaling is not implemented");
  SRGAN_REQUIRE((int64_t)B * P * P <= INT32_MAX, SRGAN_ERANGE, "srgan_crowd_resize_bilinear: more than 2^31 - 1 elements");
  const int64_t elements = (int64_t)B * P * P;
  if (P % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0)
    hipLaunchKernelGGL(crowd_resize_bilinear_kernel<4>, dim3(stream_grid(elements / 4, 256)), dim3(256), 0,
                       (hipStream_t)stream, in, h, w, P, elements / 4, out);
  else
    hipLaunchKernelGGL(crowd_resize_bilinear_kernel<1>, dim3(stream_grid(elements, 256)), dim3(256), 0, (hipStream_t)stream,
                       in, h, w, P, elements, out);
  return launch_status();
}

extern "C" int srgan_crowd_blend_windows(const float* densities, const float* counts, const int32_t* ys, int32_t ny,
                                         const int32_t* xs, int32_t nx, int32_t H, int32_t W, int32_t P,
                                         float* out_density, float* out_count, void* stream) {
  SRGAN_REQUIRE(counts && ys && xs && out_density && out_count && ny > 0 && nx > 0 && H > 0 && W > 0 && P > 0 && P % 2 == 0,
                SRGAN_EINVAL, "srgan_crowd_blend_windows arguments");
  SRGAN_REQUIRE((int64_t)H * W <= INT32_MAX && (int64_t)ny * nx * P * P <= INT32_MAX, SRGAN_ERANGE,
                "srgan_crowd_blend_windows: more than 2^31 - 1 elements");
  hipStream_t s = (hipStream_t)stream;
  const int parts = (int)(((int64_t)H * W + BLEND_TILE - 1) / BLEND_TILE);
  unsigned int* tickets = nullptr;
  float* partial = nullptr;
  if (parts > 1) {
    partial = row_finish_workspace(1, parts, 1, g_blend_finish_tickets, s, &tickets);
    SRGAN_REQUIRE(partial != nullptr, SRGAN_EUNSUPPORTED,
                  "srgan_crowd_blend_windows: the ordered count needs the stream's workspace (srgan_set_workspace)");
  }
  hipLaunchKernelGGL(crowd_blend_windows_kernel, dim3(parts), dim3(256), 0, s, densities, counts, ys, xs, ny, nx, H, W, P,
                     out_density, out_count, partial, tickets);
  return launch_status();
}
