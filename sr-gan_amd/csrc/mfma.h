// mfma.h -- what every contraction kernel relies on about v_mfma_f32_32x32x* (gfx950, 64 lanes), stated once: the vector types
// of the operands, the C/D fragment layout, the instruction wrappers, the XCD band order of a grid and the flat view of a
// workgroup's accumulators.  Staging, epilogues and tile tables stay with their kernels.
#pragma once
#include <stdint.h>
#include <type_traits>
#include <hip/hip_runtime.h>

namespace srgan {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// C/D fragment of a 32 x 32 MFMA: a lane holds 16 accumulator registers of COLUMN lane & 31; register r of lane half
// lhi = lane >> 5 is ROW mfma32_row(r, lhi): four consecutive rows per register quad, the two halves interleaved in blocks of
// four, the quads 8 rows apart.  (A operand: row = lane & 31, B operand: column = lane & 31; the lane half selects k.)
// `first` = the index of the fragment's row 0 in whatever the caller counts (output channels of a tile, rows of a plane): the
// sum is formed left to right from it, in its type, as the kernels wrote it out (the compiler keeps the no-overflow facts of
// that order, and with them the address arithmetic behind it).
template <class T = int>
__host__ __device__ constexpr __forceinline__ T mfma32_row(int r, int lhi, T first = 0) { return first + (r & 3) + 8 * (r >> 2) + 4 * lhi; }
// The inverse: which register and which lane half hold row `row` (0..31) of the fragment.
__host__ __device__ constexpr __forceinline__ int mfma32_register(int row) { return (row & 3) + 4 * (row >> 3); }
__host__ __device__ constexpr __forceinline__ int mfma32_half(int row) { return (row >> 2) & 1; }

constexpr bool mfma32_rows_are_a_permutation() {
  unsigned seen = 0;
  for (int lhi = 0; lhi < 2; ++lhi)
    for (int r = 0; r < 16; ++r) {
      const int row = mfma32_row(r, lhi);
      if (row < 0 || row > 31 || ((seen >> row) & 1u)) return false;
      if (mfma32_register(row) != r || mfma32_half(row) != lhi) return false;
      seen |= 1u << row;
    }
  return seen == 0xFFFFFFFFu;
}
static_assert(mfma32_rows_are_a_permutation(), "the 32 (register, lane half) pairs hit rows 0..31 once each and the inverse inverts");

// v_mfma_f32_32x32x2_f32: c += A[32 x 2] B[2 x 32], one float of A and of B per lane (k = the lane half).
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// The 16-bit operand fragment of precision code PREC (1 = bf16, 2 = fp16): 8 consecutive k per lane, 16 bytes.
template <int PREC> using mfma_frag = typename std::conditional<PREC == 1, bf16x8, f16x8>::type;
// v_mfma_f32_32x32x16_bf16 / _f16: c += A[32 x 16] B[16 x 32], k = 8 * lane half + element.
template <int PREC>
__device__ __forceinline__ f32x16 mfma32(const mfma_frag<PREC>& a, const mfma_frag<PREC>& b, f32x16 c) {
  static_assert(PREC == 1 || PREC == 2, "bf16 (1) or fp16 (2)");
  if constexpr (PREC == 1) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// XCD-aware order of a one-dimensional grid of `grid` workgroups (a multiple of 8): the hardware places workgroup b on XCD
// b % 8, so logical tile (b % 8) * (grid / 8) + b / 8 gives every XCD one contiguous band of tiles -- neighbouring tiles
// (which share halo rows / columns, weight rows or the 128-byte lines of a 32-pixel tile row) then read them through ONE L2
// instead of two (round 2 PMC: 1.9x the algorithmic bytes without it).
__device__ __forceinline__ int xcd_band_order(int block, int grid) { return (block & 7) * (grid >> 3) + (block >> 3); }

// A workgroup's accumulators as one flat list, fragment by fragment (what split_finish_ordered's getter / setter walk).
// acc_flat(acc) is both at once: flat(i) reads accumulator i, flat(i, v) writes it.
template <int MI, int NI>
struct AccFlat2 {
  f32x16 (&acc)[MI][NI];
  __device__ __forceinline__ float operator()(int i) const { return acc[i / (NI * 16)][(i / 16) % NI][i % 16]; }
  __device__ __forceinline__ void operator()(int i, float v) const { acc[i / (NI * 16)][(i / 16) % NI][i % 16] = v; }
};
template <int MI>
struct AccFlat1 {
  f32x16 (&acc)[MI];
  __device__ __forceinline__ float operator()(int i) const { return acc[i / 16][i % 16]; }
  __device__ __forceinline__ void operator()(int i, float v) const { acc[i / 16][i % 16] = v; }
};
template <int MI, int NI>
__device__ __forceinline__ AccFlat2<MI, NI> acc_flat(f32x16 (&acc)[MI][NI]) { return {acc}; }
template <int MI>
__device__ __forceinline__ AccFlat1<MI> acc_flat(f32x16 (&acc)[MI]) { return {acc}; }

// (Zeroing the accumulators stays an element loop in each kernel: both a helper that takes the array by reference and the
// whole-vector form `c = f32x16{}` change the generated code of some kernels -- profiles/mfma_layout.md.)

}  // namespace srgan
