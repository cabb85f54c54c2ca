// common.h -- error plumbing and small device helpers shared by every translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
// The C ABI: every extern "C" definition is compiled against its declaration here.
#include "../../include/srgan_hip.h"

namespace srgan {

// Status convention of the C ABI (include/srgan_hip.h): 0 ok, <0 argument/shape error, >0 hipError_t.
enum { SRGAN_OK = 0, SRGAN_EINVAL = -1, SRGAN_EUNSUPPORTED = -2, SRGAN_ERANGE = -3 };

void set_error(const char* fmt, ...);      // runtime.hip: the thread-local message behind srgan_last_error()
const char* last_error();

#define SRGAN_HIP(expr)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      ::srgan::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return (int)e_;                                                                    \
    }                                                                                    \
  } while (0)

#define SRGAN_REQUIRE(cond, code, msg)                                                   \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      ::srgan::set_error("%s: requirement (%s) failed", msg, #cond);                     \
      return code;                                                                       \
    }                                                                                    \
  } while (0)

inline int launch_status() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("kernel launch failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  return SRGAN_OK;
}

// More than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize -- once per kernel AND per device (the
// attribute belongs to the device's copy of the function).  KERNEL is a template argument so that every kernel has its own
// record: a bit per device ordinal, set with an atomic OR, so that two host threads launching for the first time together at
// worst both set the (idempotent) attribute.  Returns the HIP status of what it had to call.  (static: the record stays a
// local symbol of the kernel's translation unit, not an export of the library.)
template <auto KERNEL>
static hipError_t allow_dynamic_lds(int bytes) {
  static std::atomic<uint64_t> configured{0};
  int device = 0;
  hipError_t status = hipGetDevice(&device);
  const uint64_t bit = (uint64_t)1 << (device & 63);
  if (status != hipSuccess || (configured.load(std::memory_order_acquire) & bit)) return status;
  status = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (status == hipSuccess) configured.fetch_or(bit, std::memory_order_release);
  return status;
}

// Zero-fills are kernels of this library, not hipMemsetAsync: a memset NODE of a captured HIP graph replayed wrongly for
// sizes that are not a multiple of 16 bytes (ROCm 7.2: 400 bytes left garbage behind), and the runtime's own fill kernel
// takes ~5 us per launch.  `count` / `width` in floats; rows `pitch` floats apart.
int zero_floats(float* p, int64_t count, hipStream_t stream);
int zero_rows(float* p, int64_t pitch, int64_t width, int64_t rows, hipStream_t stream);

// y = fma(x, a, b) is frozen batch-norm: a = inv_std * gamma, b = beta - mean * a.  Every kernel that evaluates the
// normalisation (forward, fused prologues, the mask recomputed in the backward) goes through this one function so
// that the sign of y -- the ReLU mask -- is bit-identical everywhere.
__device__ __forceinline__ void bn_coefficients(float mean, float inv_std, float gamma, float beta, float& a, float& b) {
  a = __fmul_rn(inv_std, gamma);
  b = __fsub_rn(beta, __fmul_rn(mean, a));
}

// Sum over the 32 lanes of each half of the wave, valid in lanes 16-31 / 48-63: four rotations inside the rows of 16
// (DPP row_ror) and one row broadcast (row_bcast:15 into rows 1 and 3) -- five VALU instructions, no LDS.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, true));
}
__device__ __forceinline__ float half_wave_sum(float v) {
  v += dpp_move<0x128, 0xF>(v);
  v += dpp_move<0x124, 0xF>(v);
  v += dpp_move<0x122, 0xF>(v);
  v += dpp_move<0x121, 0xF>(v);
  v += dpp_move<0x142, 0xA>(v);
  return v;
}

// Backward of relu(batch_norm_eval(x)) applied in the epilogue of a data-gradient kernel (pointwise.hip, conv3x3.hip):
// x is the tensor the normalisation read (batch stride x_bs, same channels as the kernel's output), bn = {mean,
// inv_std, gamma, beta}; g_gamma / g_beta (both or neither) are accumulated into.
struct BnBackwardEpilogue {
  const float* x; int64_t x_bs;
  const float* bn[4];
  float* g_gamma; float* g_beta;
  // Deferred form: the per-workgroup parameter sums go to this caller-owned region ([2][tiles][C] floats) and are NOT
  // reduced by the call -- a whole dense block's convolutions are reduced by one srgan_bn_partial_reduce_batched launch.
  float* partial_out;
};

// Source taps of one output coordinate of a bilinear resize with half-pixel centres and clamped edges -- the sampling rule
// of torch.nn.functional.interpolate(mode='bilinear', align_corners=False, antialias=False), up or down: scale = in / out
// in fp32, source = fma(scale, destination + 0.5, -0.5) clamped at 0 (one rounding, as torch's CPU kernel evaluates it:
// at 128 -> 192 a separately rounded product moves a tap weight by 1e-6); taps lo and hi (= lo at the far edge), weight w_hi.
__device__ __forceinline__ void bilinear_source(float scale, int destination, int extent, int& lo, int& hi, float& w_hi) {
  float source = __fmaf_rn(scale, (float)destination + 0.5f, -0.5f);
  source = source < 0.f ? 0.f : source;
  lo = min((int)source, extent - 1);
  hi = lo + (lo < extent - 1 ? 1 : 0);
  w_hi = source - (float)lo;
}

// One output element of a bilinear resize: the row taps (top / bottom rows of the source plane, weight ly of the bottom
// one) come from bilinear_source on the output row, the column taps are taken here; the two horizontal lerps first.  The
// resize arithmetic of srgan_crowd_resize_bilinear and of srgan_density_heatmaps -- stated once.  Equal extents: lx = ly = 0
// and the result is top[ox] itself.
__device__ __forceinline__ float bilinear_row_sample(const float* __restrict__ top, const float* __restrict__ bottom, float ly,
                                                     float scale_x, int ox, int w) {
  int x0, x1;
  float lx;
  bilinear_source(scale_x, ox, w, x0, x1, lx);
  const float hx = 1.f - lx;
  return (1.f - ly) * (hx * top[x0] + lx * top[x1]) + ly * (hx * bottom[x0] + lx * bottom[x1]);
}

// Grid for a grid-stride streaming kernel: enough blocks to fill 256 CUs x 8, never more than the work.
inline unsigned stream_grid(int64_t work_items, int per_block) {
  int64_t blocks = (work_items + per_block - 1) / per_block;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return (unsigned)blocks;
}

// Sum across the 64 lanes of a wavefront (DPP/shuffle butterfly); every lane returns the total.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) v += __shfl_xor(v, offset, 64);
  return v;
}

// Block-wide sum for 256-thread blocks; result valid in thread 0.
__device__ __forceinline__ float block_sum_256(float v, float* scratch4) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) scratch4[wave] = v;
  __syncthreads();
  float total = 0.f;
  if (threadIdx.x == 0) total = scratch4[0] + scratch4[1] + scratch4[2] + scratch4[3];
  return total;
}

// Largest and smallest value across the workgroup's 256 threads (valid in every thread): the wave's butterfly, then the four
// waves through LDS.  min / max are order-independent: any tree gives the same bits.
__device__ __forceinline__ void block_min_max_256(float& lo, float& hi, float (*scratch)[4]) {
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, offset, 64));
    hi = fmaxf(hi, __shfl_xor(hi, offset, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { scratch[0][wave] = lo; scratch[1][wave] = hi; }
  __syncthreads();
  lo = fminf(fminf(scratch[0][0], scratch[0][1]), fminf(scratch[0][2], scratch[0][3]));
  hi = fmaxf(fmaxf(scratch[1][0], scratch[1][1]), fmaxf(scratch[1][2], scratch[1][3]));
}

}  // namespace srgan
