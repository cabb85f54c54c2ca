// elementwise.hip -- HBM-bound streaming kernels: unary / binary maps, per-channel affine broadcast
// (frozen batch-norm, bias, row / column / scalar broadcasts) and channel-range copies (concat / slice).
// All are one read + one write per element (roofline: HBM ~6.3 TB/s achievable), float4 wide where every pointer of
// the call is 16-byte aligned (single floats otherwise: include/srgan_hip.h), grid-stride over at most 2048 workgroups.
#include "common.h"

namespace srgan {

enum UnaryOp { U_COPY = 0, U_NEG, U_ABS, U_SIGN, U_SQRT, U_EXP, U_LOG, U_LOG1P, U_SQUARE, U_RECIP, U_TANH, U_RELU,
               U_STEP, U_AFFINE, U_POW, U_LEAKY, U_SIGMOID, U_SOFTPLUS, U_ONE_MINUS_SQ, U_RSQRT, U_ACOS, U_CLAMP,
               U_IN_RANGE, U_COUNT };
enum BinaryOp { B_ADD = 0, B_SUB, B_MUL, B_DIV, B_DIV_SAFE, B_MAX, B_LEAKY_MASK_MUL, B_AXPY, B_COUNT };

template <int OP>
__device__ __forceinline__ float unary(float x, float p0, float p1) {
  switch (OP) {
    case U_COPY: return x;
    case U_NEG: return -x;
    case U_ABS: return fabsf(x);
    case U_SIGN: return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
    case U_SQRT: return sqrtf(x);
    case U_EXP: return expf(x);
    case U_LOG: return logf(x);
    case U_LOG1P: return log1pf(x);
    case U_SQUARE: return x * x;
    case U_RECIP: return 1.f / x;
    case U_TANH: return fabsf(x) >= 9.f ? copysignf(1.f, x) : tanhf(x);   // saturated from 9 on (1 - tanh(9) < 2^-24); NaN falls through
    case U_RELU: return x > 0.f ? x : 0.f;
    case U_STEP: return x > 0.f ? 1.f : 0.f;
    case U_AFFINE: return p0 * x + p1;
    case U_POW: return powf(x, p0);
    case U_LEAKY: return x > 0.f ? x : p0 * x;
    case U_SIGMOID: return 1.f / (1.f + expf(-x));
    case U_SOFTPLUS: return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
    case U_ONE_MINUS_SQ: return 1.f - x * x;
    case U_RSQRT: return 1.f / sqrtf(x);
    case U_ACOS: return acosf(x);
    case U_CLAMP: return x < p0 ? p0 : (x > p1 ? p1 : x);             // comparisons, not fminf / fmaxf: a NaN stays a NaN (torch.clamp)
    case U_IN_RANGE: return (x >= p0 && x <= p1) ? 1.f : 0.f;         // clamp's gradient mask, edges inclusive; NaN -> 0
  }
  return x;
}

template <int OP>
__device__ __forceinline__ float binary(float a, float b, float p0) {
  switch (OP) {
    case B_ADD: return a + b;
    case B_SUB: return a - b;
    case B_MUL: return a * b;
    case B_DIV: return a / b;
    case B_DIV_SAFE: return b == 0.f ? 0.f : a / b;
    case B_MAX: return fmaxf(a, b);
    case B_LEAKY_MASK_MUL: return b > 0.f ? a : p0 * a;
    case B_AXPY: return a + p0 * b;
  }
  return a;
}

template <int OP>
// (no __restrict__: these run in place for gradient accumulation and fills)
__global__ __launch_bounds__(256) void unary_kernel(const float* x, float* y, int64_t n, float p0, float p1) {
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
  if ((((uintptr_t)x | (uintptr_t)y) & 15) != 0) {       // a view that starts off a 16-byte boundary: single floats (uniform)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) y[i] = unary<OP>(x[i], p0, p1);
    return;
  }
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float4* y4 = reinterpret_cast<float4*>(y);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 v = x4[i];
    v.x = unary<OP>(v.x, p0, p1); v.y = unary<OP>(v.y, p0, p1);
    v.z = unary<OP>(v.z, p0, p1); v.w = unary<OP>(v.w, p0, p1);
    y4[i] = v;
  }
  const int64_t tail = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tail < n) y[tail] = unary<OP>(x[tail], p0, p1);
}

template <int OP>
__global__ __launch_bounds__(256) void binary_kernel(const float* a, const float* b, float* y, int64_t n, float p0) {
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
  if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 15) != 0) {       // as unary_kernel: single floats (uniform)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) y[i] = binary<OP>(a[i], b[i], p0);
    return;
  }
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  float4* y4 = reinterpret_cast<float4*>(y);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 u = a4[i], v = b4[i];
    float4 r;
    r.x = binary<OP>(u.x, v.x, p0); r.y = binary<OP>(u.y, v.y, p0);
    r.z = binary<OP>(u.z, v.z, p0); r.w = binary<OP>(u.w, v.w, p0);
    y4[i] = r;
  }
  const int64_t tail = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tail < n) y[tail] = binary<OP>(a[tail], b[tail], p0);
}

// y[i] = value, without reading y: the destination is usually fresh memory, and 0 * NaN is NaN.
__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ y, int64_t n, float value) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) y[i] = value;
}

// rows x width floats set to zero, rows `pitch` floats apart (pitch == width: one contiguous run).  16-byte stores
// where the row start is aligned, single floats at the ragged ends.
__global__ __launch_bounds__(256) void zero_rows_kernel(float* __restrict__ p, int64_t pitch, int64_t width, int64_t rows,
                                                        int blocks_per_row) {
  const int64_t row = (int64_t)blockIdx.x / blocks_per_row;
  const int part = (int)((int64_t)blockIdx.x - row * blocks_per_row);
  if (row >= rows) return;
  float* base = p + row * pitch;
  const int64_t head = min(width, (int64_t)((4 - (((uintptr_t)base >> 2) & 3)) & 3));       // floats before 16-byte alignment
  const int64_t quads = (width - head) >> 2;
  const int64_t tid = (int64_t)part * 256 + threadIdx.x, stride = (int64_t)blocks_per_row * 256;
  float4* aligned = reinterpret_cast<float4*>(base + head);
  for (int64_t i = tid; i < quads; i += stride) aligned[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < head) base[tid] = 0.f;
  const int64_t tail = head + 4 * quads;
  if (tid < width - tail) base[tail + tid] = 0.f;
}

int zero_rows(float* p, int64_t pitch, int64_t width, int64_t rows, hipStream_t stream) {
  if (width <= 0 || rows <= 0) return SRGAN_OK;
  if (pitch == width) { width *= rows; rows = 1; pitch = width; }
  int64_t per_row = (width / 4 + 255) / 256;                       // one float4 per thread, at most 2048 blocks in all
  if (per_row < 1) per_row = 1;
  const int64_t cap = rows >= 2048 ? 1 : 2048 / rows;
  if (per_row > cap) per_row = cap;
  SRGAN_REQUIRE(rows * per_row < ((int64_t)1 << 31), SRGAN_ERANGE, "zero-fill grid");
  hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)(rows * per_row)), dim3(256), 0, stream, p, pitch, width, rows,
                     (int)per_row);
  return launch_status();
}

int zero_floats(float* p, int64_t count, hipStream_t stream) { return zero_rows(p, count, count, 1, stream); }

template <int OP>
static int launch_unary(const float* x, float* y, int64_t n, float p0, float p1, hipStream_t s) {
  hipLaunchKernelGGL(unary_kernel<OP>, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, s, x, y, n, p0, p1);
  return launch_status();
}

template <int OP>
static int launch_binary(const float* a, const float* b, float* y, int64_t n, float p0, hipStream_t s) {
  hipLaunchKernelGGL(binary_kernel<OP>, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, s, a, b, y, n, p0);
  return launch_status();
}

// y[r, i] = (x[r, i] - mean[c]) * scale_a[c] * scale_b[c] + shift[c],  c = r % C, rows of length HW >= 1; every
// vector is optional (x defaults to 1).  Frozen batch-norm is ONE pass: mean = running mean, scale_a =
// 1/sqrt(var + eps), scale_b = gamma, shift = beta.  One workgroup per (row, segment): no per-element index math.
constexpr int AFF_SEG = 256 * 4 * 4;
__device__ __forceinline__ void chan_coefficients(const float* mean, const float* scale_a, const float* scale_b,
                                                  const float* shift, int c, float& a, float& b) {
  a = (scale_a ? scale_a[c] : 1.f) * (scale_b ? scale_b[c] : 1.f);
  b = __fsub_rn(shift ? shift[c] : 0.f, mean ? __fmul_rn(mean[c], a) : 0.f);   // bn_act_bwd recomputes exactly this
}

// RELU: y = max(y, 0) (fused frozen-batch-norm + ReLU forward).  mask: y = 0 where mask <= 0 (fused backward of the
// same pair: dL/dx = dL/dy * [y > 0] * scale).
template <bool RELU>
__global__ __launch_bounds__(256) void chan_affine_rows_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ scale_a,
                                                               const float* __restrict__ scale_b,
                                                               const float* __restrict__ shift,
                                                               const float* __restrict__ mask, float* __restrict__ y,
                                                               int C, int64_t HW, int segs, int64_t total_blocks,
                                                               int64_t x_bs, int64_t mask_bs, int64_t y_bs,
                                                               int accumulate) {
  // x / mask / y may be channel-slice views of wider buffers: image n starts at n * (its batch stride).
  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    const int64_t row = blk / segs;
    const int seg = (int)(blk - row * segs);
    const int64_t n = row / C;
    const int c = (int)(row - n * C);
    float a, b;
    chan_coefficients(mean, scale_a, scale_b, shift, c, a, b);
    const int64_t xb = n * x_bs + (int64_t)c * HW, mb = n * mask_bs + (int64_t)c * HW, yb = n * y_bs + (int64_t)c * HW;
    const int64_t beg = (int64_t)seg * AFF_SEG;
    const int64_t end = beg + AFF_SEG < HW ? beg + AFF_SEG : HW;
    for (int64_t i = beg + threadIdx.x; i < end; i += 256) {
      float v = fmaf(x ? x[xb + i] : 1.f, a, b);
      if (RELU) v = fmaxf(v, 0.f);
      if (mask) v = mask[mb + i] > 0.f ? v : 0.f;
      if (accumulate) y[yb + i] += v;
      else __builtin_nontemporal_store(v, y + yb + i);
    }
  }
}

template <bool RELU>
__global__ __launch_bounds__(256) void chan_affine_flat_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ scale_a,
                                                               const float* __restrict__ scale_b,
                                                               const float* __restrict__ shift,
                                                               const float* __restrict__ mask, float* __restrict__ y,
                                                               int C, int HW, int64_t n, int64_t x_bs, int64_t mask_bs,
                                                               int64_t y_bs, int accumulate) {
  const int64_t stride = (int64_t)gridDim.x * 256, image = (int64_t)C * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int64_t img = i / image, within = i - img * image;
    const int c = (int)(within / HW);
    float a, b;
    chan_coefficients(mean, scale_a, scale_b, shift, c, a, b);
    float v = fmaf(x ? x[img * x_bs + within] : 1.f, a, b);
    if (RELU) v = fmaxf(v, 0.f);
    if (mask) v = mask[img * mask_bs + within] > 0.f ? v : 0.f;
    float* dst = y + img * y_bs + within;
    *dst = accumulate ? *dst + v : v;
  }
}

// dst[n, d0 + c, :] (=, +=) src[n, s0 + c, :] for c < count: a contiguous run of count*HW floats per image.
template <typename I>      // element index type: 32-bit unless the tensor has > 2^31 elements (64-bit division is emulated)
__global__ __launch_bounds__(256) void copy_channels_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            int64_t src_image, int64_t dst_image, int64_t src_off,
                                                            int64_t dst_off, int64_t run, int N, int accumulate) {
  const I total = (I)(run * N), stride = (I)gridDim.x * 256, run_i = (I)run;
  for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const I n = i / run_i, r = i - n * run_i;
    const float v = src[(int64_t)n * src_image + src_off + r];
    float* d = dst + (int64_t)n * dst_image + dst_off + r;
    *d = accumulate ? *d + v : v;
  }
}

// out[b, f] = alpha[b] * u[b, f] + (1 - alpha[b]) * fake[b, f]   (reference srgan.py:365-366)
__global__ __launch_bounds__(256) void gp_interpolate_kernel(const float* __restrict__ u, const float* __restrict__ fake,
                                                             const float* __restrict__ alpha, float* __restrict__ out,
                                                             int64_t F, int segs, int64_t total_blocks) {
  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    const int64_t b = blk / segs;
    const int seg = (int)(blk - b * segs);
    const float a = alpha[b], na = 1.f - a;
    const int64_t base = b * F, beg = (int64_t)seg * AFF_SEG;
    const int64_t end = beg + AFF_SEG < F ? beg + AFF_SEG : F;
    for (int64_t i = beg + threadIdx.x; i < end; i += 256) out[base + i] = a * u[base + i] + na * fake[base + i];
  }
}

// Adam on a flat parameter arena, same operation order as torch.optim.Adam (single tensor path):
// g += wd * p;  m = lerp(m, g, 1 - b1);  v = b2 * v + (1 - b2) * g * g;
// p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)      (reference srgan.py:131-138 -> torch Adam defaults)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                   float beta1, float beta2, float eps, float weight_decay,
                                                   float bias_correction1, float bias_correction2_sqrt) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const float step_size = lr / bias_correction1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float grad = g[i];
    const float param = p[i];
    if (weight_decay != 0.f) grad = grad + weight_decay * param;
    float mi = m[i], vi = v[i];
    mi = mi + (grad - mi) * (1.f - beta1);
    vi = vi * beta2 + (1.f - beta2) * grad * grad;
    const float denom = sqrtf(vi) / bias_correction2_sqrt + eps;
    p[i] = param - step_size * (mi / denom);
    m[i] = mi;
    v[i] = vi;
  }
}

// The same update with the step count and its two bias corrections resident on the device, so that a HIP graph of a
// whole training iteration replays with a different count every time: ``state`` = {int32 step, float bias_correction1,
// float sqrt(bias_correction2)}; the first kernel advances it (in double, as the host path does), the second reads it.
__global__ void adam_advance_kernel(int32_t* __restrict__ state, float beta1, float beta2) {
  const int32_t step = state[0] + 1;
  state[0] = step;
  float* corrections = reinterpret_cast<float*>(state);
  corrections[1] = (float)(1.0 - pow((double)beta1, (double)step));
  corrections[2] = (float)sqrt(1.0 - pow((double)beta2, (double)step));
}

__global__ __launch_bounds__(256) void adam_counted_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                           float lr, float beta1, float beta2, float eps,
                                                           float weight_decay, const float* __restrict__ state) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const float bias_correction1 = state[1], bias_correction2_sqrt = state[2];
  const float step_size = lr / bias_correction1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float grad = g[i];
    const float param = p[i];
    if (weight_decay != 0.f) grad = grad + weight_decay * param;
    float mi = m[i], vi = v[i];
    mi = mi + (grad - mi) * (1.f - beta1);
    vi = vi * beta2 + (1.f - beta2) * grad * grad;
    const float denom = sqrtf(vi) / bias_correction2_sqrt + eps;
    p[i] = param - step_size * (mi / denom);
    m[i] = mi;
    v[i] = vi;
  }
}

// Gradient buckets on the wire in bf16 (parallel.py, data-parallel runs of the comm-sensitive configurations): fp32 ->
// bf16 with round-to-nearest-even (NaN kept quiet), 8 elements per thread (two float4 in, one 16-byte store out), and
// back.  HBM-bound: 6 B per element each way.
__device__ __forceinline__ uint32_t bf16_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;            // NaN
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
  const int64_t n8 = n >> 3, stride = (int64_t)gridDim.x * 256;
  const float4* s4 = reinterpret_cast<const float4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const float4 a = s4[2 * i], b = s4[2 * i + 1];
    uint4 o;
    o.x = bf16_bits(a.x) | (bf16_bits(a.y) << 16); o.y = bf16_bits(a.z) | (bf16_bits(a.w) << 16);
    o.z = bf16_bits(b.x) | (bf16_bits(b.y) << 16); o.w = bf16_bits(b.z) | (bf16_bits(b.w) << 16);
    d4[i] = o;
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 7)) {
    const int64_t i = (n8 << 3) + threadIdx.x;
    dst[i] = (uint16_t)bf16_bits(src[i]);
  }
}

__global__ __launch_bounds__(256) void unpack_bf16_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
  const int64_t n8 = n >> 3, stride = (int64_t)gridDim.x * 256;
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  float4* d4 = reinterpret_cast<float4*>(dst);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const uint4 v = s4[i];
    d4[2 * i] = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u),
                            __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
    d4[2 * i + 1] = make_float4(__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xffff0000u),
                                __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xffff0000u));
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 7)) {
    const int64_t i = (n8 << 3) + threadIdx.x;
    dst[i] = __uint_as_float((uint32_t)src[i] << 16);
  }
}

}  // namespace srgan

using namespace srgan;

extern "C" {

int srgan_ew_unary(int op, const float* x, float* y, int64_t n, float p0, float p1, void* stream) {
  SRGAN_REQUIRE(x && y && n >= 0 && op >= 0 && op < U_COUNT, SRGAN_EINVAL, "srgan_ew_unary arguments");
  if (n == 0) return SRGAN_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
#define CASE(OP) case OP: return launch_unary<OP>(x, y, n, p0, p1, s);
    CASE(U_COPY) CASE(U_NEG) CASE(U_ABS) CASE(U_SIGN) CASE(U_SQRT) CASE(U_EXP) CASE(U_LOG) CASE(U_LOG1P)
    CASE(U_SQUARE) CASE(U_RECIP) CASE(U_TANH) CASE(U_RELU) CASE(U_STEP) CASE(U_AFFINE) CASE(U_POW) CASE(U_LEAKY)
    CASE(U_SIGMOID) CASE(U_SOFTPLUS) CASE(U_ONE_MINUS_SQ) CASE(U_RSQRT)
    CASE(U_ACOS) CASE(U_CLAMP) CASE(U_IN_RANGE)
#undef CASE
  }
  return SRGAN_EINVAL;
}

int srgan_ew_binary(int op, const float* a, const float* b, float* y, int64_t n, float p0, void* stream) {
  SRGAN_REQUIRE(a && b && y && n >= 0 && op >= 0 && op < B_COUNT, SRGAN_EINVAL, "srgan_ew_binary arguments");
  if (n == 0) return SRGAN_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
#define CASE(OP) case OP: return launch_binary<OP>(a, b, y, n, p0, s);
    CASE(B_ADD) CASE(B_SUB) CASE(B_MUL) CASE(B_DIV) CASE(B_DIV_SAFE) CASE(B_MAX) CASE(B_LEAKY_MASK_MUL) CASE(B_AXPY)
#undef CASE
  }
  return SRGAN_EINVAL;
}

int srgan_fill(float* y, int64_t n, float value, void* stream) {
  SRGAN_REQUIRE(y && n >= 0, SRGAN_EINVAL, "srgan_fill arguments");
  if (n == 0) return SRGAN_OK;
  if (value == 0.f) return zero_floats(y, n, (hipStream_t)stream);
  hipLaunchKernelGGL(fill_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, y, n, value);
  return launch_status();
}

static int chan_affine_launch(const float* x, const float* mean, const float* scale_a, const float* scale_b,
                              const float* shift, const float* mask, int relu, float* y, int32_t N, int32_t C,
                              int64_t HW, hipStream_t s, int64_t x_bs = 0, int64_t mask_bs = 0, int64_t y_bs = 0,
                              int accumulate = 0) {
  const int64_t n = (int64_t)N * C * HW, dense = (int64_t)C * HW;
  if (x_bs == 0) x_bs = dense;
  if (mask_bs == 0) mask_bs = dense;
  if (y_bs == 0) y_bs = dense;
  if (HW >= 256) {
    const int segs = (int)((HW + AFF_SEG - 1) / AFF_SEG);
    const int64_t blocks = (int64_t)N * C * segs;
    const unsigned grid = (unsigned)(blocks < 65536 * 16 ? blocks : 65536 * 16);
    if (relu) hipLaunchKernelGGL(chan_affine_rows_kernel<true>, dim3(grid), dim3(256), 0, s, x, mean, scale_a, scale_b,
                                 shift, mask, y, C, HW, segs, blocks, x_bs, mask_bs, y_bs, accumulate);
    else hipLaunchKernelGGL(chan_affine_rows_kernel<false>, dim3(grid), dim3(256), 0, s, x, mean, scale_a, scale_b, shift,
                            mask, y, C, HW, segs, blocks, x_bs, mask_bs, y_bs, accumulate);
  } else {
    if (relu) hipLaunchKernelGGL(chan_affine_flat_kernel<true>, dim3(stream_grid(n, 256)), dim3(256), 0, s, x, mean,
                                 scale_a, scale_b, shift, mask, y, C, (int)HW, n, x_bs, mask_bs, y_bs, accumulate);
    else hipLaunchKernelGGL(chan_affine_flat_kernel<false>, dim3(stream_grid(n, 256)), dim3(256), 0, s, x, mean, scale_a,
                            scale_b, shift, mask, y, C, (int)HW, n, x_bs, mask_bs, y_bs, accumulate);
  }
  return launch_status();
}

int srgan_chan_affine(const float* x, const float* mean, const float* scale_a, const float* scale_b, const float* shift,
                      float* y, int32_t N, int32_t C, int64_t HW, void* stream) {
  SRGAN_REQUIRE(y && N > 0 && C > 0 && HW > 0, SRGAN_EINVAL, "srgan_chan_affine arguments");
  return chan_affine_launch(x, mean, scale_a, scale_b, shift, nullptr, 0, y, N, C, HW, (hipStream_t)stream);
}

int srgan_chan_affine_act(const float* x, const float* mean, const float* scale_a, const float* scale_b,
                          const float* shift, const float* mask, int relu, float* y, int32_t N, int32_t C, int64_t HW,
                          void* stream) {
  SRGAN_REQUIRE(y && N > 0 && C > 0 && HW > 0, SRGAN_EINVAL, "srgan_chan_affine_act arguments");
  return chan_affine_launch(x, mean, scale_a, scale_b, shift, mask, relu, y, N, C, HW, (hipStream_t)stream);
}

int srgan_chan_affine_act_strided(const float* x, const float* mean, const float* scale_a, const float* scale_b,
                                  const float* shift, const float* mask, int relu, float* y, int32_t N, int32_t C,
                                  int64_t HW, int64_t x_batch_stride, int64_t mask_batch_stride, int64_t y_batch_stride,
                                  int accumulate, void* stream) {
  SRGAN_REQUIRE(y && N > 0 && C > 0 && HW > 0, SRGAN_EINVAL, "srgan_chan_affine_act_strided arguments");
  return chan_affine_launch(x, mean, scale_a, scale_b, shift, mask, relu, y, N, C, HW, (hipStream_t)stream,
                            x_batch_stride, mask_batch_stride, y_batch_stride, accumulate);
}

int srgan_copy_channels(const float* src, int32_t src_channels, int32_t src_first, float* dst, int32_t dst_channels,
                        int32_t dst_first, int32_t count, int32_t N, int64_t HW, int accumulate, void* stream) {
  SRGAN_REQUIRE(src && dst && N > 0 && HW > 0 && count > 0, SRGAN_EINVAL, "srgan_copy_channels arguments");
  SRGAN_REQUIRE(src_first >= 0 && dst_first >= 0 && src_first + count <= src_channels &&
                dst_first + count <= dst_channels, SRGAN_EINVAL, "srgan_copy_channels channel ranges");
  const int64_t run = (int64_t)count * HW;
  if (run * N < ((int64_t)1 << 31) - ((int64_t)2048 * 256))
    hipLaunchKernelGGL(copy_channels_kernel<uint32_t>, dim3(stream_grid(run * N, 256 * 4)), dim3(256), 0, (hipStream_t)stream,
                       src, dst, (int64_t)src_channels * HW, (int64_t)dst_channels * HW, (int64_t)src_first * HW,
                       (int64_t)dst_first * HW, run, N, accumulate);
  else
    hipLaunchKernelGGL(copy_channels_kernel<int64_t>, dim3(stream_grid(run * N, 256 * 4)), dim3(256), 0, (hipStream_t)stream,
                       src, dst, (int64_t)src_channels * HW, (int64_t)dst_channels * HW, (int64_t)src_first * HW,
                       (int64_t)dst_first * HW, run, N, accumulate);
  return launch_status();
}

int srgan_gp_interpolate(const float* unlabeled, const float* fake, const float* alpha, float* out, int32_t B,
                         int64_t F, void* stream) {
  SRGAN_REQUIRE(unlabeled && fake && alpha && out && B > 0 && F > 0, SRGAN_EINVAL, "srgan_gp_interpolate arguments");
  const int segs = (int)((F + AFF_SEG - 1) / AFF_SEG);
  const int64_t blocks = (int64_t)B * segs;
  const unsigned grid = (unsigned)(blocks < 65536 * 16 ? blocks : 65536 * 16);
  hipLaunchKernelGGL(gp_interpolate_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, unlabeled, fake, alpha, out,
                     F, segs, blocks);
  return launch_status();
}

int srgan_pack_bf16(const float* src, uint16_t* dst, int64_t n, void* stream) {
  SRGAN_REQUIRE(src && dst && n >= 0, SRGAN_EINVAL, "srgan_pack_bf16 arguments");
  SRGAN_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, SRGAN_EINVAL, "srgan_pack_bf16: 16-byte aligned buffers");
  if (n == 0) return SRGAN_OK;
  hipLaunchKernelGGL(pack_bf16_kernel, dim3(stream_grid(n, 256 * 8)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
  return launch_status();
}

int srgan_unpack_bf16(const uint16_t* src, float* dst, int64_t n, void* stream) {
  SRGAN_REQUIRE(src && dst && n >= 0, SRGAN_EINVAL, "srgan_unpack_bf16 arguments");
  SRGAN_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, SRGAN_EINVAL, "srgan_unpack_bf16: 16-byte aligned buffers");
  if (n == 0) return SRGAN_OK;
  hipLaunchKernelGGL(unpack_bf16_kernel, dim3(stream_grid(n, 256 * 8)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
  return launch_status();
}

int srgan_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int32_t step, void* stream) {
  SRGAN_REQUIRE(p && g && m && v && n >= 0 && step >= 1, SRGAN_EINVAL, "srgan_adam_step arguments");
  if (n == 0) return SRGAN_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr,
                     beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2));
  return launch_status();
}

int srgan_adam_step_counted(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int32_t* state, void* stream) {
  SRGAN_REQUIRE(p && g && m && v && state && n >= 0, SRGAN_EINVAL, "srgan_adam_step_counted arguments");
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, beta1, beta2);
  if (n == 0) return launch_status();
  hipLaunchKernelGGL(adam_counted_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                     lr, beta1, beta2, eps, weight_decay, reinterpret_cast<const float*>(state));
  return launch_status();
}

}  // extern "C"
