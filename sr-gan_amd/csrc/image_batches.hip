// image_batches.hip -- training-batch assembly for the applications whose database is a stack of equally sized frames
// with one scalar label each (age, driving): the frames live in HBM as uint8 or float [count, C, h, w] in the 0..255
// range, and one launch gathers the B frames an index list names, normalises them to [-1, 1] (reference
// utility.py:129-132), optionally resamples them to [H, W] (bilinear, half-pixel centres) and gathers their labels.  It is
// the reference's Dataset.__getitem__ + DataLoader collation (age/data.py:52-60, driving/data.py:44-51) as one HBM-bound
// data mover: no LDS, no atomics, no workspace.
#include "common.h"

namespace srgan {

constexpr int RUN = 4;      // output pixels per lane: one 16-byte store

// (v / 127.5) - 1 with an IEEE division and a separate subtraction: the bits of the reference's to_normalized_range on
// a CPU fp32 tensor.  (A multiplication by 1 / 127.5, or a fused multiply-add, rounds differently.)
__device__ __forceinline__ float normalised(float v) { return __fsub_rn(__fdiv_rn(v, 127.5f), 1.0f); }

// RUN consecutive elements of a row as floats: one 4-byte (uint8) / one 16-byte (float) load.  The address is only
// element-aligned in general (a frame of 3 x 5 x 7 floats starts anywhere), hence memcpy: the compiler emits the widest
// load the target allows for that alignment -- a single global_load_dword / _dwordx4 on gfx950.
__device__ __forceinline__ void load_run(const uint8_t* p, float (&v)[RUN]) {
  uint32_t bits;
  __builtin_memcpy(&bits, p, RUN);
#pragma unroll
  for (int i = 0; i < RUN; ++i) v[i] = (float)((bits >> (8 * i)) & 0xFFu);
}
__device__ __forceinline__ void load_run(const float* p, float (&v)[RUN]) { __builtin_memcpy(v, p, RUN * sizeof(float)); }

// Lane -> run `run` of the output: RUN consecutive pixels of one row of out_images [B, C, H, W] (the last run of a row
// whose width is no multiple of RUN is shorter and moves element by element).  Consecutive lanes take consecutive runs, so
// a wave reads and writes whole lines of a row.  Example b is frame order[first + b], clamped into [0, count): the host
// cannot check the index list.  The first B lanes also move the labels.
template <typename T, bool RESIZE>
__global__ __launch_bounds__(256) void image_batch_gather_kernel(const T* __restrict__ store, int count, int C, int h, int w,
                                                                 const float* __restrict__ labels,
                                                                 const int32_t* __restrict__ order, int64_t first, int B,
                                                                 int H, int W, int64_t runs, float* __restrict__ out_images,
                                                                 float* __restrict__ out_labels) {
  const int runs_per_row = (W + RUN - 1) / RUN;
  const int64_t frame = (int64_t)C * h * w;
  const float scale_y = (float)h / (float)H, scale_x = (float)w / (float)W;
  for (int64_t run = (int64_t)blockIdx.x * 256 + threadIdx.x; run < runs; run += (int64_t)gridDim.x * 256) {
    if (out_labels && run < B) out_labels[run] = labels[min(max(order[first + run], 0), count - 1)];
    const unsigned row = (unsigned)run / (unsigned)runs_per_row;       // (runs <= B * C * H * W < 2^31: 32-bit divisions)
    const int x = (int)((unsigned)run - row * (unsigned)runs_per_row) * RUN;
    const int y = (int)(row % (unsigned)H);
    const unsigned plane = row / (unsigned)H;            // b * C + c
    const int c = (int)(plane % (unsigned)C);
    const int b = (int)(plane / (unsigned)C);
    const int64_t index = min(max(order[first + b], 0), count - 1);
    const T* source = store + index * frame + (int64_t)c * h * w;
    float* out = out_images + (int64_t)row * W + x;
    const int valid = min(RUN, W - x);
    float v[RUN];
    if constexpr (!RESIZE) {
      const T* in = source + (int64_t)y * w + x;
      if (valid == RUN) {
        load_run(in, v);
      } else {
        for (int i = 0; i < valid; ++i) v[i] = (float)in[i];
      }
#pragma unroll
      for (int i = 0; i < RUN; ++i) v[i] = normalised(v[i]);
    } else {
      int y0, y1;
      float ly;
      bilinear_source(scale_y, y, h, y0, y1, ly);
      const T* top = source + (int64_t)y0 * w;
      const T* bottom = source + (int64_t)y1 * w;
#pragma unroll
      for (int i = 0; i < RUN; ++i) {
        int x0, x1;
        float lx;
        bilinear_source(scale_x, min(x + i, W - 1), w, x0, x1, lx);
        const float hx = 1.f - lx;
        v[i] = (1.f - ly) * (hx * normalised((float)top[x0]) + lx * normalised((float)top[x1])) +
               ly * (hx * normalised((float)bottom[x0]) + lx * normalised((float)bottom[x1]));
      }
    }
    if (valid == RUN) {
      __builtin_memcpy(out, v, RUN * sizeof(float));       // rows are 4-byte aligned in general: see load_run
    } else {
      for (int i = 0; i < valid; ++i) out[i] = v[i];
    }
  }
}

template <typename T>
void image_batch_gather_launch(const void* store, int32_t count, int32_t C, int32_t h, int32_t w, const float* labels,
                               const int32_t* order, int64_t first, int32_t B, int32_t H, int32_t W, float* out_images,
                               float* out_labels, hipStream_t stream) {
  const int64_t runs = (int64_t)B * C * H * ((W + RUN - 1) / RUN);
  const dim3 grid(stream_grid(runs, 256));
  if (H == h && W == w)
    hipLaunchKernelGGL((image_batch_gather_kernel<T, false>), grid, dim3(256), 0, stream, static_cast<const T*>(store), count,
                       C, h, w, labels, order, first, B, H, W, runs, out_images, out_labels);
  else
    hipLaunchKernelGGL((image_batch_gather_kernel<T, true>), grid, dim3(256), 0, stream, static_cast<const T*>(store), count,
                       C, h, w, labels, order, first, B, H, W, runs, out_images, out_labels);
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_image_batch_gather(const void* store, int store_dtype, int32_t count, int32_t C, int32_t h, int32_t w,
                                        const float* labels, const int32_t* order, int64_t first, int32_t B, int32_t H,
                                        int32_t W, float* out_images, float* out_labels, void* stream) {
  SRGAN_REQUIRE(store && order && out_images && count > 0 && C > 0 && h > 0 && w > 0 && first >= 0 && B > 0 && H > 0 && W > 0,
                SRGAN_EINVAL, "srgan_image_batch_gather arguments");
  SRGAN_REQUIRE(store_dtype == 0 || store_dtype == 1, SRGAN_EINVAL, "srgan_image_batch_gather: store_dtype is 0 (uint8) or 1 (float)");
  SRGAN_REQUIRE((labels == nullptr) == (out_labels == nullptr), SRGAN_EINVAL,
                "srgan_image_batch_gather: labels and out_labels are given together or not at all");
  SRGAN_REQUIRE((int64_t)C * h * w <= INT32_MAX && (int64_t)B * C * H * W <= INT32_MAX, SRGAN_EINVAL,
                "srgan_image_batch_gather: a frame or the batch exceeds 2^31 - 1 elements");
  if (store_dtype == 0)
    image_batch_gather_launch<uint8_t>(store, count, C, h, w, labels, order, first, B, H, W, out_images, out_labels,
                                       (hipStream_t)stream);
  else
    image_batch_gather_launch<float>(store, count, C, h, w, labels, order, first, B, H, W, out_images, out_labels,
                                     (hipStream_t)stream);
  return launch_status();
}
