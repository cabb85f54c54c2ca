// crowd_patches.hip -- training-batch assembly of the crowd application ON the device: for every
// example of the batch, the P x P patch around a given centre of a full scene that already lives in HBM as uint8 RGB
// (H, W, 3) + float label / map (H, W), optionally mirrored left-right, the image normalised to [-1, 1] and laid out
// planar.  This is ExtractPatchForPosition(allow_padded) -> RandomHorizontalFlip -> NegativeOneToOneNormalizeImage ->
// NumpyArraysToTorchTensors of the reference's 4-worker NumPy pipeline (crowd/data.py:41-128,370-453,
// crowd/shanghai_tech_data.py:76-104) in one HBM-bound kernel: 3 bytes + 8 bytes read, 20 bytes written per pixel.
// Pixels outside the scene are zero BEFORE normalisation (the reference pads the uint8 image), i.e. -1 afterwards.
// The same row body cuts the sliding windows of ONE scene for full-image inference (srgan_crowd_extract_windows: centres
// from two small tables instead of per-example pointer tables; 3 bytes read, 12 bytes written per pixel).
// srgan_crowd_draw_patches / srgan_crowd_extract_patches_indexed are the same batch with the host taken out: the positions
// come from the counter-based stream of philox.h and the tables are per scene, uploaded once.
#include "common.h"
#include "philox.h"

namespace srgan {

// `VEC` consecutive floats of one output row: one 16-byte store when VEC = 4 (the caller guarantees the alignment).
template <int VEC>
__device__ __forceinline__ void store_run(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = v[i];
  }
}

// Row `row` of the P x P patch centred on (cy, cx) of one scene -- the body both kernels below share.  The calling thread
// takes the runs of VEC columns first, first + step, ...; oi / ol / om point at the row's first element in the image
// plane 0 / the label / the map of the output (ol, om may be null).
template <int VEC>
__device__ __forceinline__ void patch_row(const uint8_t* __restrict__ image, const float* __restrict__ label,
                                          const float* __restrict__ map, int H, int W, int cy, int cx, bool flip, int P,
                                          int row, int first, int step, float* __restrict__ oi, float* __restrict__ ol,
                                          float* __restrict__ om) {
  const int half = P / 2;
  const int src_row = cy - half + row;
  const bool row_ok = (unsigned)src_row < (unsigned)H;
  const int64_t plane = (int64_t)P * P;
  for (int col = first * VEC; col < P; col += step * VEC) {
    float r[VEC], g[VEC], bl[VEC], lv[VEC], mv[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int src_col = cx - half + (flip ? P - 1 - (col + v) : col + v);
      const bool ok = row_ok && (unsigned)src_col < (unsigned)W;
      const int64_t at = ok ? (int64_t)src_row * W + src_col : 0;
      float pr = 0.f, pg = 0.f, pb = 0.f;
      if (ok) { pr = (float)image[at * 3]; pg = (float)image[at * 3 + 1]; pb = (float)image[at * 3 + 2]; }
      r[v] = pr / 127.5f - 1.f;
      g[v] = pg / 127.5f - 1.f;
      bl[v] = pb / 127.5f - 1.f;
      lv[v] = (ok && label) ? label[at] : 0.f;
      mv[v] = (ok && map) ? map[at] : 0.f;
    }
    store_run<VEC>(oi + col, r);
    store_run<VEC>(oi + plane + col, g);
    store_run<VEC>(oi + 2 * plane + col, bl);
    if (ol) store_run<VEC>(ol + col, lv);
    if (om) store_run<VEC>(om + col, mv);
  }
}

__global__ __launch_bounds__(256) void crowd_patches_kernel(const uint8_t* const* __restrict__ images,
                                                            const float* const* __restrict__ labels,
                                                            const float* const* __restrict__ maps,
                                                            const int32_t* __restrict__ heights,
                                                            const int32_t* __restrict__ widths,
                                                            const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
                                                            const int32_t* __restrict__ flips, int P,
                                                            float* __restrict__ out_images, float* __restrict__ out_labels,
                                                            float* __restrict__ out_maps) {
  const int b = blockIdx.y, row = blockIdx.x;
  const int64_t plane = (int64_t)P * P;
  patch_row<1>(images[b], labels ? labels[b] : nullptr, maps ? maps[b] : nullptr, heights[b], widths[b], ys[b], xs[b],
               flips[b] != 0, P, row, (int)threadIdx.x, 256, out_images + (int64_t)b * 3 * plane + (int64_t)row * P,
               out_labels ? out_labels + (int64_t)b * plane + (int64_t)row * P : nullptr,
               out_maps ? out_maps + (int64_t)b * plane + (int64_t)row * P : nullptr);
}

// Full-image inference: windows first, first + 1, ... of ONE scene, window i centred on (ys[i / nx], xs[i % nx]) -- the
// sliding-window order of the reference's ImageSlidingWindowDataset (crowd/data.py:521-560).  One wave per patch row, four
// rows per workgroup; with VEC = 4 a lane stores 16 bytes per plane and a wave 1 KiB of one row.
constexpr int WINDOW_ROWS = 4;
template <int VEC>
__global__ __launch_bounds__(256) void crowd_windows_kernel(const uint8_t* __restrict__ image, int H, int W,
                                                            const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
                                                            int nx, int first, int P, float* __restrict__ out_images) {
  const int row = (int)blockIdx.x * WINDOW_ROWS + ((int)threadIdx.x >> 6);
  if (row >= P) return;
  const int window = first + (int)blockIdx.y;
  patch_row<VEC>(image, nullptr, nullptr, H, W, ys[window / nx], xs[window % nx], false, P, row, (int)threadIdx.x & 63, 64,
                 out_images + (int64_t)blockIdx.y * 3 * P * P + (int64_t)row * P, nullptr, nullptr);
}

// Training batches without the host.  The draw: one thread per example, example e = first + i owns Philox block
// e of the draw; the 64-bit word (w1, w0) scaled to [0, length) by the high half of the 128-bit product picks a centre out of
// the running counts `starts`, a binary search finds its scene, bit 31 of w2 is the coin.
__global__ __launch_bounds__(256) void crowd_draw_patches_kernel(const int64_t* __restrict__ starts,
                                                                 const int32_t* __restrict__ heights,
                                                                 const int32_t* __restrict__ widths, int S, int P, int flip,
                                                                 int64_t first, int n, uint32_t draw,
                                                                 const uint32_t* __restrict__ state,
                                                                 int32_t* __restrict__ table) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  uint32_t w[4];
  draw_block_words((uint64_t)first + (uint64_t)i, draw, state[2], state[0], state[1], w);
  const uint64_t r = ((uint64_t)w[1] << 32) | w[0];
  const int64_t index = (int64_t)__umul64hi(r, (uint64_t)starts[S]);      // < length
  int lo = 0, hi = S - 1;                                                 // the largest s in [0, S) with starts[s] <= index
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (starts[mid] <= index) lo = mid; else hi = mid - 1;
  }
  const int64_t local = index - starts[lo];
  const int64_t columns = max(widths[lo] - P + 1, 1);      // (consistent tables: >= 1 for a scene that owns a centre)
  int32_t* entry = table + 4 * (int64_t)i;
  entry[0] = lo;
  entry[1] = P / 2 + (int)(local / columns);
  entry[2] = P / 2 + (int)(local % columns);
  entry[3] = flip ? (int)(w[2] >> 31) : 0;
}

// The cut: example b reads scene table[b][0] of the per-SCENE tables at centre (table[b][1], table[b][2]), mirrored when
// table[b][3] != 0.  The form of crowd_windows_kernel: one wave per patch row, four rows per workgroup, 16-byte stores with
// VEC = 4.  A scene outside [0, S) reads no table and no scene: H = W = 0 makes every pixel padding.
template <int VEC>
__global__ __launch_bounds__(256) void crowd_patches_indexed_kernel(const uint8_t* const* __restrict__ images,
                                                                    const float* const* __restrict__ labels,
                                                                    const float* const* __restrict__ maps,
                                                                    const int32_t* __restrict__ heights,
                                                                    const int32_t* __restrict__ widths, int S,
                                                                    const int32_t* __restrict__ table, int P,
                                                                    float* __restrict__ out_images,
                                                                    float* __restrict__ out_labels,
                                                                    float* __restrict__ out_maps) {
  const int row = (int)blockIdx.x * WINDOW_ROWS + ((int)threadIdx.x >> 6);
  if (row >= P) return;
  const int b = blockIdx.y;
  const int32_t* entry = table + 4 * (int64_t)b;
  const int scene = entry[0];
  const bool known = (unsigned)scene < (unsigned)S;
  const int64_t plane = (int64_t)P * P;
  patch_row<VEC>(known ? images[scene] : nullptr, known && labels ? labels[scene] : nullptr,
                 known && maps ? maps[scene] : nullptr, known ? heights[scene] : 0, known ? widths[scene] : 0, entry[1],
                 entry[2], entry[3] != 0, P, row, (int)threadIdx.x & 63, 64,
                 out_images + (int64_t)b * 3 * plane + (int64_t)row * P,
                 out_labels ? out_labels + (int64_t)b * plane + (int64_t)row * P : nullptr,
                 out_maps ? out_maps + (int64_t)b * plane + (int64_t)row * P : nullptr);
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_crowd_draw_patches(const int64_t* starts, const int32_t* heights, const int32_t* widths, int32_t S,
                                        int32_t P, int32_t flip, int64_t first, int32_t n, int32_t draw,
                                        const uint32_t* state, int32_t* table, void* stream) {
  SRGAN_REQUIRE(starts && heights && widths && state && table, SRGAN_EINVAL, "srgan_crowd_draw_patches pointers");
  SRGAN_REQUIRE(S >= 1 && P >= 2 && P % 2 == 0 && n >= 0 && draw >= 0, SRGAN_EINVAL, "srgan_crowd_draw_patches: S, P, n, draw");
  SRGAN_REQUIRE(first >= 0 && first <= INT64_MAX - n, SRGAN_EINVAL, "srgan_crowd_draw_patches: first");
  if (n == 0) return SRGAN_OK;
  hipLaunchKernelGGL(crowd_draw_patches_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, starts, heights,
                     widths, S, P, flip, first, n, (uint32_t)draw, state, table);
  return launch_status();
}

extern "C" int srgan_crowd_extract_patches_indexed(const void* const* images_u8, const float* const* labels,
                                                   const float* const* maps, const int32_t* heights, const int32_t* widths,
                                                   int32_t S, const int32_t* table, int32_t B, int32_t P, float* out_images,
                                                   float* out_labels, float* out_maps, void* stream) {
  SRGAN_REQUIRE(images_u8 && heights && widths && table && out_images && S >= 1 && B > 0 && P > 0 && P % 2 == 0 &&
                B <= 65535, SRGAN_EINVAL, "srgan_crowd_extract_patches_indexed arguments");
  SRGAN_REQUIRE(P <= 46340 && (int64_t)B * 3 * P * P <= INT32_MAX, SRGAN_ERANGE,
                "srgan_crowd_extract_patches_indexed: a tensor exceeds 2^31 - 1 elements");
  const dim3 grid((P + WINDOW_ROWS - 1) / WINDOW_ROWS, B);
  const uint8_t* const* images = reinterpret_cast<const uint8_t* const*>(images_u8);
  const uintptr_t bases = reinterpret_cast<uintptr_t>(out_images) | reinterpret_cast<uintptr_t>(out_labels) |
                          reinterpret_cast<uintptr_t>(out_maps);      // (a NULL output adds no bits)
  if (P % 4 == 0 && bases % 16 == 0)
    hipLaunchKernelGGL(crowd_patches_indexed_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, images, labels, maps, heights,
                       widths, S, table, P, out_images, out_labels, out_maps);
  else
    hipLaunchKernelGGL(crowd_patches_indexed_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, images, labels, maps, heights,
                       widths, S, table, P, out_images, out_labels, out_maps);
  return launch_status();
}

extern "C" int srgan_crowd_extract_patches(const void* const* images_u8, const float* const* labels,
                                           const float* const* maps, const int32_t* heights, const int32_t* widths,
                                           const int32_t* ys, const int32_t* xs, const int32_t* flips, int32_t B,
                                           int32_t P, float* out_images, float* out_labels, float* out_maps, void* stream) {
  SRGAN_REQUIRE(images_u8 && heights && widths && ys && xs && flips && out_images && B > 0 && P > 0 && P % 2 == 0 &&
                B <= 65535, SRGAN_EINVAL, "srgan_crowd_extract_patches arguments");
  hipLaunchKernelGGL(crowd_patches_kernel, dim3(P, B), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint8_t* const*>(images_u8), labels, maps, heights, widths, ys, xs, flips, P,
                     out_images, out_labels, out_maps);
  return launch_status();
}

extern "C" int srgan_crowd_extract_windows(const void* image_u8, int32_t H, int32_t W, const int32_t* ys, int32_t ny,
                                           const int32_t* xs, int32_t nx, int32_t first, int32_t count, int32_t P,
                                           float* out_images, void* stream) {
  SRGAN_REQUIRE(image_u8 && ys && xs && out_images && H > 0 && W > 0 && ny > 0 && nx > 0 && first >= 0 && count > 0 &&
                P > 0 && P % 2 == 0, SRGAN_EINVAL, "srgan_crowd_extract_windows arguments");
  SRGAN_REQUIRE((int64_t)first + count <= (int64_t)ny * nx, SRGAN_EINVAL, "srgan_crowd_extract_windows window range");
  SRGAN_REQUIRE(count <= 65535 && (int64_t)H * W * 3 <= INT32_MAX && (int64_t)count * 3 * P * P <= INT32_MAX, SRGAN_ERANGE,
                "srgan_crowd_extract_windows: a tensor exceeds 2^31 - 1 elements (or more than 65535 windows per call)");
  const dim3 grid((P + WINDOW_ROWS - 1) / WINDOW_ROWS, count);
  const uint8_t* image = static_cast<const uint8_t*>(image_u8);
  if (P % 4 == 0 && reinterpret_cast<uintptr_t>(out_images) % 16 == 0)
    hipLaunchKernelGGL(crowd_windows_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, image, H, W, ys, xs, nx, first, P,
                       out_images);
  else
    hipLaunchKernelGGL(crowd_windows_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, image, H, W, ys, xs, nx, first, P,
                       out_images);
  return launch_status();
}
