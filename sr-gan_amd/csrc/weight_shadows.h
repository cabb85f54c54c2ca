// weight_shadows.h -- the layouts of the weight shadows: the operands that the blocked kernels (and the fp32 3x3 convolution's
// weight-image forms) read in place of the fp32 master weights, re-rounded from the masters behind every optimizer update.
//
// One device body per layout (one thread = one slot, or one 64 x 64 tile per workgroup) that blocked16_shadows.hip runs both
// from a single-layer kernel and from the batched launch of every shadow of a network (h_pack_batched_kernel), and HPackJob, one
// problem of that launch.  The kernel files that read a layout include this header for its constants and index functions.
#pragma once
#include "blocked16.h"

namespace srgan {

constexpr int K4_CK = 4;         // k-slots per chunk of the 4x4 / stride 2 family (blocked16_k4s2.hip)
constexpr int K4_TAPS = 4;

// conv weights (R x S taps) as the operand of the LDS-staged kernels: slot (chunk, tap, half g, row o) holds the 8 reduced
// channels chunk * 16 + g * 8 .. + 7 of row o at that tap.
template <int PREC>
__device__ __forceinline__ void h_pack_conv_weights_slot(const float* __restrict__ w, Slot* __restrict__ packed, int64_t slot,
                                                         int32_t CO, int32_t CI, int32_t R, int32_t S, int32_t base, int32_t so,
                                                         int32_t si, int32_t skh, int32_t skw) {
  const int T = R * S;
  const int o = (int)(slot % CO);
  const int64_t rest = slot / CO;
  const int g = (int)(rest & 1);
  const int64_t ct = rest >> 1;
  const int tap = (int)(ct % T), chunk = (int)(ct / T);
  const int kh = tap / S, kw = tap - kh * S;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = chunk * 16 + g * 8 + j;
    v[j] = c < CI ? w[base + o * so + c * si + kh * skh + kw * skw] : 0.f;
  }
  packed[slot] = h_pack8<PREC>(v);
}

// The fp32 weight image of a 3x3 convolution, the operand of conv3x3_lds_kernel's WIMG forms (conv3x3.hip):
//   img[(ci * 9 + tap) * CO_pad + o] = element (o, ci, tap / 3, tap % 3) at w[base + o * so + ci * si + kh * skh + kw * skw]
// with CO_pad = CO rounded up to 64 and ci running to CI rounded up to 8; rows o >= CO and channels ci >= CI are zeros, so a
// chunk's slice is read without a predicate.  One thread = one element (consecutive o: coalesced stores).
__host__ __device__ __forceinline__ int32_t conv3x3_image_co_pad(int32_t CO) { return (CO + 63) & ~63; }
__host__ __device__ __forceinline__ int64_t conv3x3_image_floats(int32_t CI, int32_t CO) {
  return (int64_t)((CI + 7) & ~7) * 9 * conv3x3_image_co_pad(CO);
}
__device__ __forceinline__ void conv3x3_image_element(const float* __restrict__ w, float* __restrict__ image, int64_t element,
                                                      int32_t CO, int32_t CI, int32_t base, int32_t so, int32_t si, int32_t skh,
                                                      int32_t skw) {
  const int co_pad = conv3x3_image_co_pad(CO);
  const int o = (int)(element % co_pad), row = (int)(element / co_pad);
  const int ci = row / 9, tap = row - ci * 9;
  const int kh = tap / 3, kw = tap - kh * 3;
  image[element] = (o < CO && ci < CI) ? w[base + o * so + ci * si + kh * skh + kw * skw] : 0.f;
}

// 4x4 / stride 2 weights as 2x2-tap operands (mode 0: "down", 1 .. 4: the "up" parity classes; layout in blocked16_k4s2.hip)
template <int PREC>
__device__ __forceinline__ void h_pack_k4s2_weights_slot(const float* __restrict__ w, Slot* __restrict__ packed, int64_t slot,
                                                         int32_t rows, int32_t reduced, int64_t row_stride, int64_t reduced_stride,
                                                         int32_t mode) {
  const int o = (int)(slot % rows);
  int64_t rest = slot / rows;
  const int j = (int)(rest % K4_CK); rest /= K4_CK;
  const int tap = (int)(rest % K4_TAPS);
  const int chunk = (int)(rest / K4_TAPS);
  const int a = tap >> 1, b = tap & 1;
  constexpr int G = HGroup<PREC>::N;
  int kh, kw, first;
  if (mode == 0) { kh = 2 * a + (j >> 1); kw = 2 * b + (j & 1); first = G * chunk; }
  else {
    const int ry = (mode - 1) >> 1, rx = (mode - 1) & 1;
    kh = ry == 0 ? 3 - 2 * a : 2 - 2 * a;
    kw = rx == 0 ? 3 - 2 * b : 2 - 2 * b;
    first = G * (K4_CK * chunk + j);
  }
  float v[G];
#pragma unroll
  for (int i = 0; i < G; ++i)
    v[i] = first + i < reduced ? w[o * row_stride + (int64_t)(first + i) * reduced_stride + kh * 4 + kw] : 0.f;
  packed[slot] = h_pack<PREC>(v);
}

// index of element i' of a flattened BLOCKED plane tensor ([C / 8][P][8]) in the flattened NCHW order ([C][P])
__host__ __device__ __forceinline__ int64_t h_plane_index(int64_t i, int32_t plane) {
  if (plane <= 1) return i;
  const int64_t slot = i >> 3;
  return ((slot / plane) * 8 + (i & 7)) * plane + slot % plane;
}

// The matrix shadows (linear layers, blocked16_gemm.hip).  out16[r][c] (row_slots slots per row) = src[map(r, row_plane) * rs +
// map(c, col_plane) * cs] for map(r) < rows_real, map(c) < cols_real, else 0.  One thread per slot of 8 consecutive c.
template <int PREC>
__device__ __forceinline__ void h_pack_matrix_slot(const float* __restrict__ src, Slot* __restrict__ out, int64_t slot,
                                                   int32_t row_slots, int64_t rows_real, int64_t cols_real, int64_t rs, int64_t cs,
                                                   int32_t row_plane, int32_t col_plane) {
  const int64_t r = slot / row_slots;
  const int64_t c0 = (slot % row_slots) * 8;
  const int64_t rr = h_plane_index(r, row_plane);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t cc = h_plane_index(c0 + j, col_plane);
    v[j] = (rr < rows_real && cc < cols_real) ? src[rr * rs + cc * cs] : 0.f;
  }
  out[slot] = h_pack8<PREC>(v);
}

// The same for rs == 1 (the TRANSPOSED shadow of a row-major matrix): one 64 x 64 tile (`tile_index`, row tiles fastest) of a
// WHOLE workgroup through LDS, so that both the fp32 reads (along r) and the 16-byte slot stores (along c) are coalesced.  The
// row pitch of 65 floats puts the 64 lanes of a column write (tile[c][r_load], r_load = lane) and of a row read (tile[8 s + j][r])
// on different banks.  Every thread of the workgroup must call it (one barrier).
template <int PREC>
__device__ __forceinline__ void h_pack_matrix_tile(const float* __restrict__ src, Slot* __restrict__ out, float (*tile)[65],
                                                   int tile_index, int64_t rows, int32_t row_slots, int64_t rows_real,
                                                   int64_t cols_real, int64_t cs, int32_t row_plane, int32_t col_plane,
                                                   int32_t tiles_r) {
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)(tile_index % tiles_r) * 64, c0 = (int64_t)(tile_index / tiles_r) * 64;
  const int r_load = tid & 63;
  const int64_t rr = h_plane_index(r0 + r_load, row_plane);
  const bool row_ok = r0 + r_load < rows && rr < rows_real;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c_local = (tid >> 6) + 4 * i;
    const int64_t cc = h_plane_index(c0 + c_local, col_plane);
    tile[c_local][r_load] = (row_ok && c0 + c_local < (int64_t)row_slots * 8 && cc < cols_real) ? src[cc * cs + rr] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int slot_local = tid & 7, r_local = (tid >> 3) + 32 * i;
    if (r0 + r_local >= rows || c0 / 8 + slot_local >= row_slots) continue;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[slot_local * 8 + j][r_local];
    out[(r0 + r_local) * row_slots + c0 / 8 + slot_local] = h_pack8<PREC>(v);
  }
}

// The bias rows of a seed transposed convolution (a linear map onto [Cout][plane], blocked16.py "linear_t"): fp32
// rows[(g * plane + p) * 8 + j] = bias[8 g + j] (0 from `channels` on) -- one thread = the 8 values of one (g, p); a copy.
__device__ __forceinline__ void h_bias_rows_slot(const float* __restrict__ bias, float* __restrict__ rows, int64_t slot,
                                                 int32_t channels, int32_t plane) {
  const int g = (int)(slot / plane);
  float4 v[2];
  float* f = reinterpret_cast<float*>(v);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = g * 8 + j < channels ? bias[g * 8 + j] : 0.f;
  reinterpret_cast<float4*>(rows + slot * 8)[0] = v[0];
  reinterpret_cast<float4*>(rows + slot * 8)[1] = v[1];
}

// one problem of the batched launch (80 bytes, filled on the host by srgan_h_pack_job_*); the kinds' numbers are part of it
enum HPackKind : int32_t {
  PACK_CONV_WEIGHTS = 0,            // h_pack_conv_weights_slot
  PACK_K4S2_WEIGHTS = 1,            // h_pack_k4s2_weights_slot
  PACK_MATRIX = 2,                  // h_pack_matrix_slot
  PACK_MATRIX_TILED = 3,            // h_pack_matrix_tile: one 64 x 64 tile per workgroup, slots = 256 x tiles
  PACK_BIAS_ROWS = 4,               // h_bias_rows_slot: packed = the fp32 bias rows
  PACK_CONV3X3_IMAGE = 5,           // conv3x3_image_element: slots = its floats, packed = the image
};
struct HPackJob {
  const float* w; Slot* packed;
  int64_t slots, first_block;       // this job's workgroups are [first_block, first_block + ceil(slots / 256))
  int32_t kind, prec;               // an HPackKind; prec = dtype
  int32_t p[10];                    // the body's integer arguments, in its order
};
static_assert(sizeof(HPackJob) == 80, "srgan_h_pack_job_bytes(): callers keep arrays of these");

}  // namespace srgan
