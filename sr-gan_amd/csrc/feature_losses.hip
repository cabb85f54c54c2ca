// feature_losses.hip -- the correlation-matrix feature loss (reference srgan.py:511-535, feature_covariance_loss) without
// its F x F matrices.  With x = features [B, F] (fp32, row-major), per side (base / other):
//   m_i = mean of column i, xm = x - m, z_i = xm_i / ||xm_i||      (so C = Z Z^T is the clamped correlation matrix)
//   loss = sum_{i != j} | clamp(Cb_ij, -1, 1) - clamp(Co_ij, -1, 1) |
// The diagonal contributes exactly 0 (C_ii = 1 on both sides in exact arithmetic; the reference's fp32 diagonal is off by at
// most an ulp per feature).  An entry whose unclamped value lies strictly outside [-1, 1] is clamped and passes no gradient;
// a feature without variance gives 0 * inf = NaN in z, and from there in the loss and in every gradient.  The contract is at
// srgan_feature_corrcoef_l1_fwd in include/srgan_hip.h.
//
// Four kernels, no atomics and no cross-workgroup meeting inside a launch, so two launches on the same inputs give the same
// bits:
//   normalise   per side: column statistics (two passes: mean, then the centred sum of squares) and Z, transposed to
//               [Fp][Bp] with zero padding (Fp = F rounded up to 128, Bp = B rounded up to 32), so that the MFMA operands of
//               the Gram kernels are K-contiguous 16-byte loads
//   gram_fwd    a wave owns 32 features i and walks the 32-feature blocks j of its column split: both Gram tiles with
//               v_mfma_f32_32x32x2_f32 (K = batch), |difference| summed, r_i = sum_j G_ij C_ij summed; per-split partials
//   finish      the partial r_i and the partial losses added in split order / a fixed tree
//   gram_bwd    per requested side: the same walk over ALL j, the G tile formed in the accumulator layout -- which IS the B
//               operand layout of a second MFMA over k = j -- multiplied into Z_j for the wave's 128 examples, then the
//               row-wise epilogue dX = 2 g / ||xm_i|| * ((G Z)_i - r_i z_i)
// The tile T[j][i] = sum_b Z[j][b] Z[i][b] takes Z_j as the A operand and Z_i as the B operand: lane l then holds column
// i = l & 31 and rows j = mfma32_row(reg, l >> 5).
#include <math.h>
#include "common.h"
#include "mfma.h"

namespace srgan {
namespace {


constexpr int FL_TILE = 32;              // features per wave
constexpr int FL_GROUP = 128;            // features per workgroup (four waves)
constexpr int FL_BWD_CHUNKS = 4;         // 32-example chunks of the backward's second product per wave
constexpr int64_t FL_MAX_B = 8192, FL_MAX_F = (int64_t)1 << 20, FL_MAX_Z = (int64_t)1 << 26;

struct FeatureLossPlan {
  int64_t Fp, Bp;                        // padded extents of Z
  int j_blocks, per_split, splits;       // 32-feature column blocks, blocks per split, splits (grid.y of gram_fwd)
  int64_t z_floats, r_floats, loss_floats;
};

// The shape arithmetic of every launch and of the scratch query: one place.
FeatureLossPlan feature_loss_plan(int64_t B, int64_t F) {
  FeatureLossPlan p;
  p.Fp = (F + FL_GROUP - 1) / FL_GROUP * FL_GROUP;
  p.Bp = (B + 31) / 32 * 32;
  p.j_blocks = (int)((F + FL_TILE - 1) / FL_TILE);
  const int64_t groups = p.Fp / FL_GROUP;
  int64_t splits = (1024 + groups - 1) / groups;              // about 1024 workgroups: four per CU
  if (splits > p.j_blocks) splits = p.j_blocks;
  p.per_split = (int)((p.j_blocks + splits - 1) / splits);
  p.splits = (p.j_blocks + p.per_split - 1) / p.per_split;
  p.z_floats = 2 * p.Fp * p.Bp;
  p.r_floats = (int64_t)p.splits * 2 * p.Fp;
  p.loss_floats = p.Fp / FL_TILE * p.splits;
  return p;
}

int feature_loss_capacity(int64_t B, int64_t F, const char* what) {
  SRGAN_REQUIRE(B >= 2 && F >= 1, SRGAN_EINVAL, what);
  const int64_t Fp = (F + FL_GROUP - 1) / FL_GROUP * FL_GROUP, Bp = (B + 31) / 32 * 32;
  if (B > FL_MAX_B || F > FL_MAX_F || Fp * Bp > FL_MAX_Z) {
    set_error("%s: (B, F) = (%lld, %lld) is beyond the capacity B <= %lld, F <= %lld, "
              "round_up(F, 128) * round_up(B, 32) <= 2^26", what, (long long)B, (long long)F, (long long)FL_MAX_B,
              (long long)FL_MAX_F);
    return SRGAN_ERANGE;
  }
  return SRGAN_OK;
}

// grid (Fp / 64, 2 sides).  Lane = feature, the four waves share the examples; every sum is taken in a fixed order.
__global__ __launch_bounds__(256) void feature_normalise_kernel(const float* __restrict__ base, const float* __restrict__ other,
                                                                float* __restrict__ saved, float* __restrict__ zt, int B,
                                                                int64_t F, int64_t Fp, int64_t Bp) {
  __shared__ float sums[4][64];
  __shared__ float tile[64][65];
  const int side = (int)blockIdx.y, lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const float* __restrict__ x = side ? other : base;
  const int64_t f0 = (int64_t)blockIdx.x * 64, f = f0 + lane;
  const bool live = f < F;
  float s = 0.f;
  if (live) for (int b = wave; b < B; b += 4) s += x[(int64_t)b * F + f];
  sums[wave][lane] = s;
  __syncthreads();
  const float mean = ((sums[0][lane] + sums[1][lane]) + (sums[2][lane] + sums[3][lane])) / (float)B;
  __syncthreads();
  s = 0.f;
  if (live) for (int b = wave; b < B; b += 4) { const float d = x[(int64_t)b * F + f] - mean; s = fmaf(d, d, s); }
  sums[wave][lane] = s;
  __syncthreads();
  const float inv = live ? 1.f / sqrtf((sums[0][lane] + sums[1][lane]) + (sums[2][lane] + sums[3][lane])) : 0.f;
  if (live && wave == 0) {
    saved[((int64_t)side * 3 + 0) * F + f] = mean;
    saved[((int64_t)side * 3 + 1) * F + f] = inv;
  }
  float* __restrict__ z = zt + (int64_t)side * Fp * Bp;
  for (int64_t b0 = 0; b0 < Bp; b0 += 64) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t b = b0 + wave + 4 * i;
      tile[lane][wave + 4 * i] = (live && b < B) ? (x[b * F + f] - mean) * inv : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = wave + 4 * i;
      if (b0 + lane < Bp) z[(f0 + row) * Bp + b0 + lane] = tile[row][lane];        // f0 + row < Fp: Fp is a multiple of 128
    }
    __syncthreads();
  }
}

// Both Gram tiles T[j][i] of one (j block, i block): 16 batch elements per step, each lane two 16-byte loads per operand.
// Within a step MFMA t contracts k = {k0 + 8h + t} of the two lane halves h: A and B use the same map, so the order of k is
// the same for T[j][i] and T[i][j].
__device__ __forceinline__ void gram_tiles(const float* __restrict__ zb, const float* __restrict__ zo, int64_t Bp, int64_t j0,
                                           int64_t i0, int c, int h, f32x16& tb, f32x16& to) {
  const float* __restrict__ ab = zb + (j0 + c) * Bp + 8 * h;
  const float* __restrict__ bb = zb + (i0 + c) * Bp + 8 * h;
  const float* __restrict__ ao = zo + (j0 + c) * Bp + 8 * h;
  const float* __restrict__ bo = zo + (i0 + c) * Bp + 8 * h;
#pragma unroll
  for (int r = 0; r < 16; ++r) { tb[r] = 0.f; to[r] = 0.f; }
  for (int64_t k0 = 0; k0 < Bp; k0 += 16) {
    const float4 a0 = *reinterpret_cast<const float4*>(ab + k0), a1 = *reinterpret_cast<const float4*>(ab + k0 + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(bb + k0), b1 = *reinterpret_cast<const float4*>(bb + k0 + 4);
    const float4 c0 = *reinterpret_cast<const float4*>(ao + k0), c1 = *reinterpret_cast<const float4*>(ao + k0 + 4);
    const float4 d0 = *reinterpret_cast<const float4*>(bo + k0), d1 = *reinterpret_cast<const float4*>(bo + k0 + 4);
    tb = mfma32(a0.x, b0.x, tb);
    to = mfma32(c0.x, d0.x, to);
    tb = mfma32(a0.y, b0.y, tb);
    to = mfma32(c0.y, d0.y, to);
    tb = mfma32(a0.z, b0.z, tb);
    to = mfma32(c0.z, d0.z, to);
    tb = mfma32(a0.w, b0.w, tb);
    to = mfma32(c0.w, d0.w, to);
    tb = mfma32(a1.x, b1.x, tb);
    to = mfma32(c1.x, d1.x, to);
    tb = mfma32(a1.y, b1.y, tb);
    to = mfma32(c1.y, d1.y, to);
    tb = mfma32(a1.z, b1.z, tb);
    to = mfma32(c1.z, d1.z, to);
    tb = mfma32(a1.w, b1.w, tb);
    to = mfma32(c1.w, d1.w, to);
  }
}

// One entry: the clamped difference and the two masked sign factors.  Comparisons only (no fminf / fmaxf), so that a NaN
// stays a NaN in the value and in both factors.
__device__ __forceinline__ void entry_terms(float cb, float co, float& d, float& gb, float& go) {
  const float cbc = cb > 1.f ? 1.f : (cb < -1.f ? -1.f : cb);
  const float coc = co > 1.f ? 1.f : (co < -1.f ? -1.f : co);
  d = cbc - coc;
  const float g = d > 0.f ? 1.f : (d < 0.f ? -1.f : d);        // sign(d); 0 -> 0, NaN -> NaN
  gb = fabsf(cb) > 1.f ? 0.f : g;
  go = fabsf(co) > 1.f ? 0.f : -g;
}

// grid (Fp / 128, splits).  partial_r [splits][2][Fp], partial_loss [Fp / 32][splits].
__global__ __launch_bounds__(256) void feature_gram_fwd_kernel(const float* __restrict__ zt, float* __restrict__ partial_r,
                                                               float* __restrict__ partial_loss, int64_t F, int64_t Fp,
                                                               int64_t Bp, int j_blocks, int per_split, int splits) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int64_t i_wave = (int64_t)blockIdx.x * 4 + wave, i0 = i_wave * FL_TILE, i = i0 + c;
  const int split = (int)blockIdx.y;
  const float* __restrict__ zb = zt;
  const float* __restrict__ zo = zt + Fp * Bp;
  float loss = 0.f, rb = 0.f, ro = 0.f;
  if (i0 < F) {
    const int first = split * per_split, last = min(j_blocks, first + per_split);
    for (int jb = first; jb < last; ++jb) {
      const int64_t j0 = (int64_t)jb * FL_TILE;
      f32x16 tb, to;
      gram_tiles(zb, zo, Bp, j0, i0, c, h, tb, to);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t j = j0 + mfma32_row(r, h);
        if (j < F && i < F && j != i) {
          float d, gb, go;
          entry_terms(tb[r], to[r], d, gb, go);
          loss += fabsf(d);
          rb = fmaf(gb, tb[r], rb);
          ro = fmaf(go, to[r], ro);
        }
      }
    }
  }
  rb += __shfl_xor(rb, 32, 64);
  ro += __shfl_xor(ro, 32, 64);
  if (h == 0) {                                                  // i < Fp: the grid covers exactly Fp features
    partial_r[((int64_t)split * 2 + 0) * Fp + i] = rb;
    partial_r[((int64_t)split * 2 + 1) * Fp + i] = ro;
  }
  loss = wave_sum(loss);
  if (lane == 0) partial_loss[i_wave * splits + split] = loss;
}

// grid (ceil(F / 256) + 1): the first blocks add the r partials in split order, the last one the loss partials (thread t takes
// the parts t, t + 256, ..., then the tree of block_sum_256).
__global__ __launch_bounds__(256) void feature_finish_kernel(const float* __restrict__ partial_r, const float* __restrict__ partial_loss,
                                                             float* __restrict__ saved, float* __restrict__ loss, int64_t F,
                                                             int64_t Fp, int splits, int64_t loss_parts) {
  __shared__ float scratch4[4];
  if (blockIdx.x + 1 < gridDim.x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    float rb = 0.f, ro = 0.f;
    for (int s = 0; s < splits; ++s) {
      rb += partial_r[((int64_t)s * 2 + 0) * Fp + i];
      ro += partial_r[((int64_t)s * 2 + 1) * Fp + i];
    }
    saved[2 * F + i] = rb;
    saved[5 * F + i] = ro;
    return;
  }
  float mine = 0.f;
  for (int64_t part = threadIdx.x; part < loss_parts; part += 256) mine += partial_loss[part];
  const float total = block_sum_256(mine, scratch4);
  if (threadIdx.x == 0) loss[0] = total;
}

// grid (Fp / 128, ceil(B / 128)), one launch per requested side.  A wave: 32 features i, 128 examples, every j.
template <int SIDE>
__global__ __launch_bounds__(256) void feature_gram_bwd_kernel(const float* __restrict__ x, const float* __restrict__ zt,
                                                               const float* __restrict__ saved, const float* __restrict__ g,
                                                               float* __restrict__ grad, int B, int64_t F, int64_t Fp, int64_t Bp,
                                                               int j_blocks) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * FL_TILE, i = i0 + c;
  if (i0 >= F) return;                                           // (wave-uniform; no barrier follows)
  const int64_t b_first = (int64_t)blockIdx.y * (FL_BWD_CHUNKS * 32);
  const float* __restrict__ zb = zt;
  const float* __restrict__ zo = zt + Fp * Bp;
  const float* __restrict__ zs = SIDE ? zo : zb;
  f32x16 p[FL_BWD_CHUNKS];
#pragma unroll
  for (int q = 0; q < FL_BWD_CHUNKS; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) p[q][r] = 0.f;
  for (int jb = 0; jb < j_blocks; ++jb) {
    const int64_t j0 = (int64_t)jb * FL_TILE;
    f32x16 tb, to;
    gram_tiles(zb, zo, Bp, j0, i0, c, h, tb, to);
    float gv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t j = j0 + mfma32_row(r, h);
      float d, gb, go;
      entry_terms(tb[r], to[r], d, gb, go);
      gv[r] = (j < F && i < F && j != i) ? (SIDE ? go : gb) : 0.f;
    }
    // P[b][i] += sum_j Z[j][b] G[j][i]: MFMA r contracts the two rows j(r, h) this lane half holds -- gv[r] is already the B
    // operand; the A operand is Z[j(r, h)][b], 32 consecutive examples per lane half.  (j0 + 31 < Fp: rows of padding are 0.)
#pragma unroll
    for (int q = 0; q < FL_BWD_CHUNKS; ++q) {
      const int64_t bq = b_first + 32 * q;
      if (bq < Bp) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t j = j0 + mfma32_row(r, h);
          p[q] = mfma32(zs[j * Bp + bq + c], gv[r], p[q]);
        }
      }
    }
  }
  if (i >= F) return;
  const float mean = saved[((int64_t)SIDE * 3 + 0) * F + i], inv = saved[((int64_t)SIDE * 3 + 1) * F + i];
  const float r_i = saved[((int64_t)SIDE * 3 + 2) * F + i];
  const float factor = 2.f * g[0] * inv;
#pragma unroll
  for (int q = 0; q < FL_BWD_CHUNKS; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t b = b_first + 32 * q + mfma32_row(r, h);
      if (b < B) {
        const float z = (x[b * F + i] - mean) * inv;
        grad[b * F + i] = factor * (p[q][r] - r_i * z);
      }
    }
}

}  // namespace
}  // namespace srgan

using namespace srgan;

extern "C" {

int64_t srgan_feature_corrcoef_l1_scratch_bytes(int32_t B, int32_t F) {
  const int status = feature_loss_capacity(B, F, "srgan_feature_corrcoef_l1_scratch_bytes");
  if (status != SRGAN_OK) return status;
  const FeatureLossPlan p = feature_loss_plan(B, F);
  return (p.z_floats + p.r_floats + p.loss_floats) * (int64_t)sizeof(float);
}

int srgan_feature_corrcoef_l1_fwd(const float* base, const float* other, float* loss, float* saved, float* scratch, int32_t B,
                                  int32_t F, void* stream) {
  SRGAN_REQUIRE(base && other && loss && saved && scratch, SRGAN_EINVAL, "srgan_feature_corrcoef_l1_fwd pointers");
  SRGAN_REQUIRE(((uintptr_t)scratch & 15) == 0, SRGAN_EINVAL, "srgan_feature_corrcoef_l1_fwd: scratch 16-byte aligned");
  const int status = feature_loss_capacity(B, F, "srgan_feature_corrcoef_l1_fwd");
  if (status != SRGAN_OK) return status;
  const FeatureLossPlan p = feature_loss_plan(B, F);
  hipStream_t s = (hipStream_t)stream;
  float* zt = scratch;
  float* partial_r = zt + p.z_floats;
  float* partial_loss = partial_r + p.r_floats;
  hipLaunchKernelGGL(feature_normalise_kernel, dim3((unsigned)(p.Fp / 64), 2), dim3(256), 0, s, base, other, saved, zt, (int)B,
                     (int64_t)F, p.Fp, p.Bp);
  hipLaunchKernelGGL(feature_gram_fwd_kernel, dim3((unsigned)(p.Fp / FL_GROUP), (unsigned)p.splits), dim3(256), 0, s, zt, partial_r,
                     partial_loss, (int64_t)F, p.Fp, p.Bp, p.j_blocks, p.per_split, p.splits);
  hipLaunchKernelGGL(feature_finish_kernel, dim3((unsigned)((F + 255) / 256 + 1)), dim3(256), 0, s, partial_r, partial_loss, saved,
                     loss, (int64_t)F, p.Fp, p.splits, p.loss_floats);
  return launch_status();
}

int srgan_feature_corrcoef_l1_bwd(const float* base, const float* other, const float* saved, const float* scratch, const float* g,
                                  float* grad_base, float* grad_other, int32_t B, int32_t F, void* stream) {
  SRGAN_REQUIRE(base && other && saved && scratch && g, SRGAN_EINVAL, "srgan_feature_corrcoef_l1_bwd pointers");
  SRGAN_REQUIRE(((uintptr_t)scratch & 15) == 0, SRGAN_EINVAL, "srgan_feature_corrcoef_l1_bwd: scratch 16-byte aligned");
  const int status = feature_loss_capacity(B, F, "srgan_feature_corrcoef_l1_bwd");
  if (status != SRGAN_OK) return status;
  const FeatureLossPlan p = feature_loss_plan(B, F);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(p.Fp / FL_GROUP), (unsigned)((B + FL_BWD_CHUNKS * 32 - 1) / (FL_BWD_CHUNKS * 32)));
  if (grad_base)
    hipLaunchKernelGGL(feature_gram_bwd_kernel<0>, grid, dim3(256), 0, s, base, scratch, saved, g, grad_base, (int)B, (int64_t)F,
                       p.Fp, p.Bp, p.j_blocks);
  if (grad_other)
    hipLaunchKernelGGL(feature_gram_bwd_kernel<1>, grid, dim3(256), 0, s, other, scratch, saved, g, grad_other, (int)B, (int64_t)F,
                       p.Fp, p.Bp, p.j_blocks);
  return launch_status();
}

}  // extern "C"
