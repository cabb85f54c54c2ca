// crowd_evaluation.hip -- the sums behind the crowd application's evaluation scalars (reference crowd/srgan.py:149-191: count
// ME / MAE / MSE over the evaluated examples, kNN-map MAE / MSE over the first batch), taken ON the device from batches that
// already live in HBM: per batch 4 * B * HW bytes of labels and, with maps, 4 * B * (M + 1) * HW bytes more are read once and
// eight doubles are updated; nothing goes back to the host.  HBM-bound: per loaded map element two conversions, a subtraction,
// an absolute value, a product and two additions in fp64, far below what the loads cost.
//
// Two launches, no meeting of workgroups inside one: the partials kernel leaves one slot of three doubles per workgroup in the
// caller's scratch, the one-workgroup finish kernel adds the slots in a fixed order and updates the caller's sums.  No atomics
// on data, so two calls on the same inputs give the same bits.  Every accumulation is fp64 and every square is formed as a
// rounded product BEFORE it is added (no FMA contraction): each term is the one NumPy forms from the same fp32 inputs, only
// the order of the additions differs.
#include "evaluation_sums.h"

// hipcc compiles with -ffp-contract=fast, and this ROCm's __dmul_rn / __dadd_rn are a plain `*` / `+` that the compiler fuses
// like any other: contraction is switched off for every expression of this file instead (the pragma travels with the
// operations through inlining).  The kernels' code then has v_mul_f64 + v_add_f64 for the squares and no v_fma_f64 / v_fmac_f64;
// the GPU test has cases whose bits differ between the two forms.
#pragma clang fp contract(off)

namespace srgan {

constexpr int EVAL_CHUNK = 2048;      // plane elements per workgroup: two 16-byte loads per thread and operand
constexpr int EVAL_SLOT = 3;          // doubles per workgroup: sum of labels, sum |e|, sum e * e

__device__ __forceinline__ void map_term(float predicted, float map, double& abs_sum, double& square_sum) {
  const double e = (double)predicted - (double)map;
  abs_sum += fabs(e);
  const double square = e * e;          // rounded here; added below (no contraction in this file)
  square_sum += square;
}

// Workgroup blockIdx.x = example * chunks + chunk reduces elements [chunk * EVAL_CHUNK, ...) of the example's plane: the
// labels once, the map once (kept in registers) against each of the example's M predicted maps.  VEC: HW % 4 == 0 and every
// base pointer 16-byte aligned, so every plane and every chunk starts on 16 bytes.
template <bool VEC>
__global__ __launch_bounds__(256) void crowd_evaluation_partials_kernel(const float* __restrict__ labels,
                                                                        const float* __restrict__ predicted_maps,
                                                                        const float* __restrict__ maps, int M, int64_t HW,
                                                                        int chunks, double* __restrict__ slots) {
  __shared__ double scratch[EVAL_SLOT][4];
  const int64_t example = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x - example * chunks);
  const int64_t begin = (int64_t)chunk * EVAL_CHUNK;
  const int count = (int)(HW - begin < EVAL_CHUNK ? HW - begin : EVAL_CHUNK);       // >= 1: chunks = ceil(HW / EVAL_CHUNK)
  const float* label = labels + example * HW + begin;
  double v[EVAL_SLOT] = {0.0, 0.0, 0.0};
  if constexpr (VEC) {
    constexpr int RUNS = EVAL_CHUNK / (4 * 256);
    const int count4 = count >> 2;                                                  // HW % 4 == 0: no tail
    float4 m[RUNS];
#pragma unroll
    for (int j = 0; j < RUNS; ++j) {
      const int at = (int)threadIdx.x + 256 * j;
      m[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (at < count4) {
        const float4 l = reinterpret_cast<const float4*>(label)[at];
        v[0] += (((double)l.x + (double)l.y) + (double)l.z) + (double)l.w;
        if (maps) m[j] = reinterpret_cast<const float4*>(maps + example * HW + begin)[at];
      }
    }
    if (maps) {
      for (int c = 0; c < M; ++c) {
        const float4* predicted = reinterpret_cast<const float4*>(predicted_maps + (example * M + c) * HW + begin);
#pragma unroll
        for (int j = 0; j < RUNS; ++j) {
          const int at = (int)threadIdx.x + 256 * j;
          if (at < count4) {
            const float4 p = predicted[at];
            map_term(p.x, m[j].x, v[1], v[2]);
            map_term(p.y, m[j].y, v[1], v[2]);
            map_term(p.z, m[j].z, v[1], v[2]);
            map_term(p.w, m[j].w, v[1], v[2]);
          }
        }
      }
    }
  } else {
    constexpr int RUNS = EVAL_CHUNK / 256;
    float m[RUNS];
#pragma unroll
    for (int j = 0; j < RUNS; ++j) {
      const int at = (int)threadIdx.x + 256 * j;
      m[j] = 0.f;
      if (at < count) {
        v[0] += (double)label[at];
        if (maps) m[j] = maps[example * HW + begin + at];
      }
    }
    if (maps) {
      for (int c = 0; c < M; ++c) {
        const float* predicted = predicted_maps + (example * M + c) * HW + begin;
#pragma unroll
        for (int j = 0; j < RUNS; ++j) {
          const int at = (int)threadIdx.x + 256 * j;
          if (at < count) map_term(predicted[at], m[j], v[1], v[2]);
        }
      }
    }
  }
  block_sums_f64(v, scratch);
  if (threadIdx.x == 0) {
    double* slot = slots + (int64_t)blockIdx.x * EVAL_SLOT;
#pragma unroll
    for (int k = 0; k < EVAL_SLOT; ++k) slot[k] = v[k];
  }
}

// One workgroup, in a fixed order.  The 256 threads are 16 teams of 16 lanes; team g owns examples g, g + 16, ...  Lane s of
// a team adds the example's slots s, s + 16, ... in that order, the team's 16 label sums meet in a four-step butterfly, and the
// team's first lane forms the example's count difference and keeps the running sums over the team's examples (the map sums stay
// per lane).  The 256 threads' sums are then added by block_sums_f64 and thread 0 updates the caller's eight doubles (sums[7]
// is not touched).  At 512 x 512 / 16 an example has 128 slots: eight dependent loads per lane instead of 128.
constexpr int EVAL_TEAM = 16;
__global__ __launch_bounds__(256) void crowd_evaluation_finish_kernel(const float* __restrict__ predicted_counts,
                                                                      const double* __restrict__ slots, int B, int chunks,
                                                                      int with_maps, double map_terms, double* __restrict__ sums) {
  __shared__ double scratch[EVAL_SLOT][4];
  const int team = (int)threadIdx.x / EVAL_TEAM, lane = (int)threadIdx.x % EVAL_TEAM;
  double count[EVAL_SLOT] = {0.0, 0.0, 0.0}, map[EVAL_SLOT] = {0.0, 0.0, 0.0};
  for (int first = 0; first < B; first += 256 / EVAL_TEAM) {       // (uniform trip count: the shuffles see all 64 lanes)
    const int b = first + team;
    double label_sum = 0.0;
    if (b < B) {
      const double* slot = slots + (int64_t)b * chunks * EVAL_SLOT;
      for (int c = lane; c < chunks; c += EVAL_TEAM) {
        label_sum += slot[c * EVAL_SLOT];
        map[1] += slot[c * EVAL_SLOT + 1];
        map[2] += slot[c * EVAL_SLOT + 2];
      }
    }
#pragma unroll
    for (int offset = EVAL_TEAM / 2; offset > 0; offset >>= 1) label_sum += __shfl_xor(label_sum, offset, 64);
    if (b < B && lane == 0) {
      const double d = (double)predicted_counts[b] - label_sum;
      count[0] += d;
      count[1] += fabs(d);
      const double square = d * d;      // rounded here; added below (no contraction in this file)
      count[2] += square;
    }
  }
  block_sums_f64(count, scratch);
  if (with_maps) {          // (uniform over the workgroup)
    __syncthreads();        // the LDS words are reused
    block_sums_f64(map, scratch);
  }
  if (threadIdx.x == 0) {
    sums[0] += count[0];
    sums[1] += count[1];
    sums[2] += count[2];
    sums[3] += (double)B;
    if (with_maps) {
      sums[4] += map[1];
      sums[5] += map[2];
      sums[6] += map_terms;
    }
  }
}

static int64_t evaluation_chunks(int64_t HW) { return (HW + EVAL_CHUNK - 1) / EVAL_CHUNK; }

// Workgroups of one partials launch: 256 threads each, and a launch holds fewer than 2^32 threads.  (An evaluation batch at
// 512 x 512 / 16 is 2048 workgroups; only B in the millions with tiny planes comes near the limit.)
constexpr int64_t EVAL_MAX_WORKGROUPS = ((int64_t)1 << 24) - 1;

}  // namespace srgan

using namespace srgan;

extern "C" int64_t srgan_crowd_evaluation_scratch_bytes(int32_t B, int32_t M, int64_t HW) {
  const int64_t limit = ((int64_t)1 << 31) - 1;
  SRGAN_REQUIRE(B >= 0 && M >= 0 && HW >= 0, SRGAN_EINVAL, "srgan_crowd_evaluation_scratch_bytes arguments");
  const int64_t planes = (int64_t)B * (M > 1 ? M : 1);
  SRGAN_REQUIRE(planes == 0 || HW <= limit / planes, SRGAN_ERANGE,
                "srgan_crowd_evaluation_scratch_bytes: B * M * HW within max_tensor_elements (2^31 - 1)");
  const int64_t slots = (int64_t)B * evaluation_chunks(HW);
  SRGAN_REQUIRE(slots <= EVAL_MAX_WORKGROUPS, SRGAN_ERANGE,
                "srgan_crowd_evaluation_scratch_bytes: B * ceil(HW / 2048) workgroups within 2^24 - 1");
  return (slots > 0 ? slots : 1) * EVAL_SLOT * (int64_t)sizeof(double);
}

extern "C" int srgan_crowd_evaluation_sums(const float* predicted_counts, const float* labels, const float* predicted_maps,
                                           const float* maps, int32_t B, int32_t M, int64_t HW, double* sums, void* scratch,
                                           void* stream) {
  const int64_t limit = ((int64_t)1 << 31) - 1;
  SRGAN_REQUIRE(predicted_counts && labels && sums && scratch, SRGAN_EINVAL, "srgan_crowd_evaluation_sums: NULL pointer");
  SRGAN_REQUIRE((predicted_maps != nullptr) == (maps != nullptr), SRGAN_EINVAL,
                "srgan_crowd_evaluation_sums: predicted_maps and maps are given together or not at all");
  SRGAN_REQUIRE(B >= 0 && HW >= 0 && (!maps || M >= 1), SRGAN_EINVAL, "srgan_crowd_evaluation_sums arguments");
  SRGAN_REQUIRE((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(scratch)) % 8 == 0, SRGAN_EINVAL,
                "srgan_crowd_evaluation_sums: sums and scratch are 8-byte aligned");
  const int64_t planes = (int64_t)B * (maps ? M : 1);
  SRGAN_REQUIRE(planes == 0 || HW <= limit / planes, SRGAN_ERANGE,
                "srgan_crowd_evaluation_sums: B * M * HW within max_tensor_elements (2^31 - 1)");
  SRGAN_REQUIRE((int64_t)B * evaluation_chunks(HW) <= EVAL_MAX_WORKGROUPS, SRGAN_ERANGE,
                "srgan_crowd_evaluation_sums: B * ceil(HW / 2048) workgroups within 2^24 - 1");
  if (B == 0 || HW == 0) return SRGAN_OK;
  const int chunks = (int)evaluation_chunks(HW);
  const unsigned grid = (unsigned)((int64_t)B * chunks);        // <= EVAL_MAX_WORKGROUPS
  double* slots = static_cast<double*>(scratch);
  const uintptr_t bases = reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(predicted_maps) |
                          reinterpret_cast<uintptr_t>(maps);
  if (HW % 4 == 0 && bases % 16 == 0)
    hipLaunchKernelGGL(crowd_evaluation_partials_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, labels,
                       predicted_maps, maps, M, HW, chunks, slots);
  else
    hipLaunchKernelGGL(crowd_evaluation_partials_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, labels,
                       predicted_maps, maps, M, HW, chunks, slots);
  const int status = launch_status();
  if (status != SRGAN_OK) return status;
  hipLaunchKernelGGL(crowd_evaluation_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, predicted_counts, slots, B,
                     chunks, maps ? 1 : 0, (double)B * (double)(maps ? M : 0) * (double)HW, sums);
  return launch_status();
}
