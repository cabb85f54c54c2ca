// image_summaries.hip -- the pictures of a summary step, built where the batches already are (SRGAN_FEATURE_IMAGE_SUMMARIES):
// torchvision.utils.make_grid of one batch (reference age/srgan.py:73-90, driving/srgan.py:68-85, crowd/srgan.py:136-145) and
// the inferno heatmaps of the crowd map comparison (convert_density_maps_to_heatmaps, crowd/srgan.py:193-217).  Both are
// gathers: one thread owns an output pixel and writes it exactly once, so the output may hold anything before the call; no
// atomics, no fill in front.  HBM-bound passes of a few MB: plain coalesced loads and stores along x.
//
// The normalisation is current torchvision's: (clamp(x, low, high) - low) / max(high - low, 1e-5).  Releases old enough to
// take `range=` divided by (high - low + 1e-5) instead; the two differ by at most 1e-5 relative.
#include <cmath>

#include "launchers.h"

namespace srgan {

// out [3, GH, GW] <- images [N, C, H, W], C in {1, 3} (one channel is replicated).  xmaps == 0: N == 1, the image itself.
// cell_h = H + padding, cell_w = W + padding.  Pixel (y, x) lies in image k = (ry / cell_h) * xmaps + rx / cell_w, ry = y -
// padding, when ry, rx >= 0, the remainders are inside H x W and k < N; everything else is pad_value (not normalised).
__global__ __launch_bounds__(256) void image_grid_kernel(const float* __restrict__ images, int N, int C, int H, int W, int xmaps,
                                                         int padding, float pad_value, int normalize, float low, float high,
                                                         float span, int GH, int GW, int64_t elements,
                                                         float* __restrict__ out) {
  const int cell_h = H + padding, cell_w = W + padding;
  const int64_t plane = (int64_t)H * W;
  for (int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x; at < elements; at += (int64_t)gridDim.x * 256) {
    const int x = (int)(at % GW);
    const int64_t line = at / GW;
    const int y = (int)(line % GH), c = (int)(line / GH);
    int k = 0, iy = y, ix = x;
    bool inside = true;
    if (xmaps > 0) {
      const int ry = y - padding, rx = x - padding;
      inside = ry >= 0 && rx >= 0;
      if (inside) {
        iy = ry % cell_h;
        ix = rx % cell_w;
        const int cx = rx / cell_w;
        k = (ry / cell_h) * xmaps + cx;
        inside = iy < H && ix < W && cx < xmaps && k < N;
      }
    }
    float v = pad_value;
    if (inside) {
      v = images[((int64_t)k * C + (C == 1 ? 0 : c)) * plane + (int64_t)iy * W + ix];
      if (normalize) v = __fdiv_rn(__fsub_rn(fminf(fmaxf(v, low), high), low), span);
    }
    out[at] = v;
  }
}

// ranges[b, m] = {min, max} over labels[b] and predicted[b, m] together: workgroup b * M + m.
__global__ __launch_bounds__(256) void density_ranges_kernel(const float* __restrict__ labels, const float* __restrict__ predicted,
                                                             int M, int pixels, float* __restrict__ ranges) {
  __shared__ float scratch[2][4];
  const int pair = blockIdx.x;
  const float* label = labels + (int64_t)(pair / M) * pixels;
  const float* map = predicted + (int64_t)pair * pixels;
  float lo = label[0], hi = lo;
  for (int i = threadIdx.x; i < pixels; i += 256) {
    const float a = label[i], b = map[i];
    lo = fminf(lo, fminf(a, b));
    hi = fmaxf(hi, fmaxf(a, b));
  }
  block_min_max_256(lo, hi, scratch);
  if (threadIdx.x == 0) { ranges[2 * (int64_t)pair] = lo; ranges[2 * (int64_t)pair + 1] = hi; }
}

// Tile blockIdx.y = b * (M + 1) + slot: slot 0 is labels[b] under the range of pair (b, 0), slot 1 + m is predicted[b, m]
// under the range of pair (b, m).  A thread owns one pixel of the P x P tile and writes its three planes.  The map is resized
// with the arithmetic of srgan_crowd_resize_bilinear (bilinear_source / bilinear_row_sample), then matplotlib's Normalize and
// Colormap.__call__ on a float32 array: t = (v - vmin) / (vmax - vmin) (0 when the range is empty), entry (int)(t * entries),
// below 0 the first entry, at or above `entries` the last.
__global__ __launch_bounds__(256) void density_heatmaps_kernel(const float* __restrict__ labels, const float* __restrict__ predicted,
                                                               int M, int h, int w, int P, const float* __restrict__ lut,
                                                               int entries, const float* __restrict__ ranges,
                                                               float* __restrict__ tiles, int64_t tile_stride) {
  const int pixel = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (pixel >= P * P) return;
  const int b = (int)blockIdx.y / (M + 1), slot = (int)blockIdx.y % (M + 1);
  const int m = slot == 0 ? 0 : slot - 1;
  const int64_t pixels = (int64_t)h * w;
  const float* in = slot == 0 ? labels + b * pixels : predicted + ((int64_t)b * M + m) * pixels;
  const float vmin = ranges[2 * ((int64_t)b * M + m)], vmax = ranges[2 * ((int64_t)b * M + m) + 1];
  const int oy = pixel / P, ox = pixel % P;
  int y0, y1;
  float ly;
  bilinear_source((float)h / (float)P, oy, h, y0, y1, ly);
  const float v = bilinear_row_sample(in + (int64_t)y0 * w, in + (int64_t)y1 * w, ly, (float)w / (float)P, ox, w);
  const float t = vmax == vmin ? 0.f : __fdiv_rn(__fsub_rn(v, vmin), __fsub_rn(vmax, vmin));
  const float scaled = __fmul_rn(t, (float)entries);
  const int entry = scaled < 0.f ? 0 : (scaled >= (float)entries ? entries - 1 : (int)scaled);
  const int64_t plane = (int64_t)P * P;
  float* tile = tiles + b * tile_stride + (int64_t)slot * 3 * plane + pixel;
  tile[0] = lut[entry * 3];
  tile[plane] = lut[entry * 3 + 1];
  tile[2 * plane] = lut[entry * 3 + 2];
}

int image_grid_run(const float* images, int32_t N, int32_t C, int32_t H, int32_t W, int32_t nrow, int32_t padding, float pad_value,
                   int32_t normalize, float low, float high, float* out, hipStream_t stream) {
  const int xmaps = N == 1 ? 0 : (nrow < N ? nrow : N);
  const int64_t ymaps = xmaps ? ((int64_t)N + xmaps - 1) / xmaps : 1;
  const int64_t GH = xmaps ? ymaps * ((int64_t)H + padding) + padding : H;
  const int64_t GW = xmaps ? (int64_t)xmaps * ((int64_t)W + padding) + padding : W;
  SRGAN_REQUIRE(GH <= INT32_MAX && GW <= INT32_MAX && GH * GW <= INT32_MAX / 3, SRGAN_ERANGE,
                "srgan_image_grid: the grid has more than 2^31 - 1 elements");
  const int64_t elements = 3 * GH * GW;
  const float span = normalize ? fmaxf(high - low, 1e-5f) : 1.f;
  hipLaunchKernelGGL(image_grid_kernel, dim3(stream_grid(elements, 256)), dim3(256), 0, stream, images, N, C, H, W, xmaps,
                     xmaps ? padding : 0, pad_value, normalize, low, high, span, (int)GH, (int)GW, elements, out);
  return launch_status();
}

int density_heatmaps_run(const float* labels, const float* predicted, int32_t B, int32_t M, int32_t h, int32_t w, int32_t P,
                         const float* lut, int32_t lut_entries, float* tiles, int64_t tile_stride, float* ranges,
                         hipStream_t stream) {
  hipLaunchKernelGGL(density_ranges_kernel, dim3(B * M), dim3(256), 0, stream, labels, predicted, M, h * w, ranges);
  int status = launch_status();
  if (status != SRGAN_OK) return status;
  hipLaunchKernelGGL(density_heatmaps_kernel, dim3((P * P + 255) / 256, B * (M + 1)), dim3(256), 0, stream, labels, predicted,
                     M, h, w, P, lut, lut_entries, ranges, tiles, tile_stride);
  return launch_status();
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_image_grid(const float* images, int32_t N, int32_t C, int32_t H, int32_t W, int32_t nrow, int32_t padding,
                                float pad_value, int32_t normalize, float low, float high, float* out, void* stream) {
  SRGAN_REQUIRE(images && out && N >= 1 && (C == 1 || C == 3) && H >= 1 && W >= 1 && nrow >= 1 && padding >= 0, SRGAN_EINVAL,
                "srgan_image_grid arguments");
  SRGAN_REQUIRE(!normalize || (std::isfinite(low) && std::isfinite(high) && high >= low), SRGAN_EINVAL,
                "srgan_image_grid: normalize needs finite bounds with low <= high");
  return image_grid_run(images, N, C, H, W, nrow, padding, pad_value, normalize, low, high, out, (hipStream_t)stream);
}

extern "C" int srgan_density_heatmaps(const float* labels, const float* predicted, int32_t B, int32_t M, int32_t h, int32_t w,
                                      int32_t P, const float* lut, int32_t lut_entries, float* tiles, int64_t tile_stride,
                                      float* ranges, void* stream) {
  SRGAN_REQUIRE(labels && predicted && lut && tiles && ranges && B >= 1 && M >= 1 && h >= 1 && w >= 1 && P >= 1 &&
                lut_entries >= 1, SRGAN_EINVAL, "srgan_density_heatmaps arguments");
  SRGAN_REQUIRE(P >= h && P >= w, SRGAN_EUNSUPPORTED, "srgan_density_heatmaps: downscaling is not implemented");
  SRGAN_REQUIRE((int64_t)P * P <= INT32_MAX / 3 / ((int64_t)M + 1), SRGAN_ERANGE,
                "srgan_density_heatmaps: a row of tiles has more than 2^31 - 1 elements");
  SRGAN_REQUIRE(tile_stride >= ((int64_t)M + 1) * 3 * P * P, SRGAN_EINVAL,
                "srgan_density_heatmaps: tile_stride is shorter than the M + 1 tiles of an example");
  SRGAN_REQUIRE((int64_t)B * ((int64_t)M + 1) <= 65535 && tile_stride <= INT32_MAX / (int64_t)B &&
                (int64_t)B * M * h * w <= INT32_MAX && (int64_t)lut_entries * 3 <= INT32_MAX, SRGAN_ERANGE,
                "srgan_density_heatmaps: a tensor exceeds 2^31 - 1 elements (or more than 65535 tiles per call)");
  return density_heatmaps_run(labels, predicted, B, M, h, w, P, lut, lut_entries, tiles, tile_stride, ranges,
                              (hipStream_t)stream);
}
