// pointwise_ring.hip -- the 1x1 / stride 1 convolution with BOTH operands staged by LDS-DMA (round 4).
//
// Same contraction as pointwise.hip -- out[n, o, p] = sum_i w(o, i) * in[n, i, p] on NCHW data, reference
// crowd/models.py:340-341,369-370 and their data gradients -- for the shapes that dominate the 512 x 512 step: whole
// 128-row tiles of output channels, input channels in multiples of 32, planes in multiples of 64 / 128 pixels.  The
// calibration that led here is scratch/lab/gemm_lab.hip (profiles/r04_gemm_calibration.txt): on clean shapes the
// register-streamed structure of pointwise.hip tops out at 0.60-0.72 of the fp32 MFMA peak, this one at 0.67-0.78, and
// with the fused batch-norm prologue at 0.53-0.57 against 0.64-0.67.
//
//   * global_load_lds_dwordx4: a wave moves 1 KB per instruction straight into LDS (no VGPR round trip, no ds_write
//     pass); the loads of stage t + 1 are in flight during the whole matrix work of stage t, counted with
//     s_waitcnt vmcnt(N) and ONE raw s_barrier per 32-deep K stage (a __syncthreads() would drain the DMA queue).
//   * a workgroup owns 128 output rows x 128 (or 64) pixels; wave w owns rows 32w..32w+31 for ALL the pixels, so a
//     128-row convolution reads its activations exactly once, and the activation tile is shared through LDS.
//   * MFMA column block ni of a wave holds the pixels NI*j + ni: a lane's NI accumulators of one row are NI consecutive
//     pixels -- the B fragment is ONE ds_read_b128 / b64 per k step, and the tile leaves as float4 / float2 rows with no
//     trip through LDS; the batch-norm backward epilogue of a data gradient works on the same float4s.
//   * v_mfma_f32_32x32x2_f32 pairs two k per instruction (lanes 0-31 / 32-63); which two is free as long as A and B
//     agree.  Step 4g + t of a stage pairs k = 8g + t with k = 8g + 4 + t, so that with k-contiguous weights (the forward
//     convolution) a lane's four steps of a group come from ONE 16-byte read; the weight rows sit in LDS as 256-byte
//     bank rows whose 16-byte slots are XOR-swizzled by the bank-row index (applied to the DMA's SOURCE addresses: the
//     LDS image of an LDS-DMA is lane-linear) -- conflict-free ds_read_b128.  m-contiguous weights (the data gradient's
//     W^T) are staged as [k][128 rows] and read by conflict-free ds_read_b32.
//   * two stages of 32 channels (64 KB for the 128-pixel tile): two workgroups per CU interleave their barrier and
//     epilogue phases, which measured better than three or four stages at one workgroup per CU.
// Roofline: fp32 MFMA 157.3 TF/s; algorithmic bytes 4 * (CI + CO) per pixel (+ the epilogue streams of a fused data
// gradient).
#include "common.h"
#include "mfma.h"
#include "launchers.h"
#include "lds_dma.h"
#include <stdlib.h>
#include <type_traits>

namespace srgan {

struct RingParams {
  const float* in;      // [N, CI, HW], batch stride in_bs
  const float* w;       // A_KCONTIG: element (o, i) at w[o * w_ld + i]; otherwise at w[i * w_ld + o]
  float* out;           // [N, CO, HW], batch stride out_bs
  int32_t N, CI, CO, HW;
  int64_t in_bs, out_bs;
  int32_t w_ld;
  int32_t bpi;          // pixel blocks (of 32 * NI) per image
  int32_t tiles_m;      // 128-row tiles (the last one may hold 32, 64 or 96 rows)
  int32_t xcd_remap;
  int32_t mode;         // 0 store, 1 accumulate
  // FUSE 1: the input is relu(batch_norm_eval(in)), bn_* per INPUT channel.  FUSE 2: the output rows go through the
  // backward of relu(batch_norm_eval(epi_x)) (bn_* per OUTPUT row), see pointwise.hip
  const float* bn_mean; const float* bn_inv; const float* bn_gamma; const float* bn_beta;
  const float* epi_x; int64_t epi_x_bs;
  float* epi_partial; int32_t epi_cols;
  int32_t epi_ld;       // rows of the partial-sum region (CO, or the whole layer's rows when the launch covers a strip of them)
  // PAIR: two data gradients into the same rows in one pass.  The fields above describe the layer applied second; these
  // the one applied first (same N, CI, HW and batch strides; its bn_* are indexed by the same rows)
  const float* first_in; const float* first_w; int32_t first_w_ld;
  const float* first_bn_mean; const float* first_bn_inv; const float* first_bn_gamma; const float* first_bn_beta;
  float* first_partial; int32_t first_ld;
};

// NI: 32-pixel column blocks per wave (4: 128-pixel tile; 2 / 1: 64- / 32-pixel tiles for launches with few pixel blocks).
// FUSE: 0 plain, 1 batch-norm + ReLU prologue on the activations, 2 batch-norm + ReLU backward epilogue (NI = 4).
// PAIR (FUSE 2, accumulate): the data gradients of two consecutive dense layers into their common rows.  ONE K loop over
// the first layer's stages and then the second's; after the first layer's last stage its epilogue is applied to the
// accumulators and added into the prefetched old-gradient registers, which the second layer's epilogue then adds to and
// stores: x and the gradient buffer go through HBM once, and per element the sum is (old + r_first) + r_second, the bits
// of two launches.
template <int STAGES, int NI, bool A_KCONTIG, int FUSE, bool PAIR = false>
__global__ __launch_bounds__(256, 2) void pointwise_ring_kernel(const RingParams p) {
  constexpr int BK = 32;
  constexpr int A_BYTES = 128 * BK * 4, RB = 128 * NI, B_BYTES = BK * RB, C_BYTES = FUSE == 1 ? 4 * 512 : 0;
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES + C_BYTES;
  constexpr int QA = 4, QB = NI, RPI = 1024 / RB;
  constexpr int PER_STAGE = QA + QB + (FUSE == 1 ? 2 : 0);
  static_assert(FUSE != 2 || NI == 4, "the epilogue's partial sums are per 128-pixel block");
  static_assert(!PAIR || (FUSE == 2 && STAGES == 2 && !A_KCONTIG), "the pair is a fused data gradient on the two-stage ring");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = (int)blockIdx.x;
  if (p.xcd_remap) bid = xcd_band_order(bid, (int)gridDim.x);     // the row tiles of a pixel block on one XCD
  const int tm = bid % p.tiles_m, cb = bid / p.tiles_m;
  const int n = cb / p.bpi, pix0 = (cb - n * p.bpi) * (32 * NI);
  const int m0 = tm * 128;
  const uint32_t lds0 = ring_lds_address(smem);
  const int nst1 = p.CI / BK;                                               // K stages of one layer
  const int nst = PAIR ? 2 * nst1 : nst1;

  // ---- DMA sources ----
  // B: instruction q of wave w covers the RPI k rows (w * QB + q) * RPI .. of the stage, RB bytes each
  const char* in_block = (const char*)(p.in + (int64_t)n * p.in_bs + pix0);
  const int b_row = lane / (RB / 16), b_col = lane % (RB / 16);
  const uint32_t b_lane = (uint32_t)(b_row * p.HW + 4 * b_col) * 4u;
  // (PAIR: ONE lane offset, row 2 * (wave * QA + q) + lhi of a stage through the scalar base and the lane's half -- its K
  // loop has no registers for four, let alone eight)
  uint32_t a_lane[PAIR ? 1 : QA];
  if constexpr (PAIR) {
    a_lane[0] = (uint32_t)(min(m0 + 4 * l31, p.CO - 4)) * 4u;
  } else if (A_KCONTIG) {
    // weight rows of 32 floats; a 256-byte bank row holds two of them = 16 slots of 16 bytes, slot' = slot ^ (bank row & 15)
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const int br = lane >> 4, sp = lane & 15;
      const int bank_row = 16 * wave + 4 * q + br;
      const int s = sp ^ (bank_row & 15);
      a_lane[q] = (uint32_t)(min(m0 + 2 * bank_row + (s >> 3), p.CO - 1) * p.w_ld + 4 * (s & 7)) * 4u;
    }
  } else {
#pragma unroll
    for (int q = 0; q < QA; ++q)
      a_lane[q] = (uint32_t)(((wave * QA + q) * 2 + lhi) * p.w_ld + min(m0 + 4 * l31, p.CO - 4)) * 4u;
  }
  const char* first_block = PAIR ? (const char*)(p.first_in + (int64_t)n * p.in_bs + pix0) : nullptr;
  auto issue_pair_weights = [&](const float* w, int32_t w_ld, int stage, uint32_t slot) {
    const char* wb = (const char*)w + (int64_t)stage * BK * w_ld * 4;
    const uint32_t at = a_lane[0] + (uint32_t)(lhi * w_ld) * 4u;
#pragma unroll
    for (int q = 0; q < QA; ++q)
      ring_glds16(wb + (int64_t)((wave * QA + q) * 2) * w_ld * 4, at, slot + (uint32_t)((wave * QA + q) * 1024));
  };
  // the last row tile may be partial (CO is a multiple of 32: whole waves): its surplus waves stage their share of the
  // operands (clamped rows) and keep the barriers, but skip the matrix work and the stores
  const bool active = m0 + 32 * wave < p.CO;
  // FUSE 1: a wave's own table of the stage's batch-norm vectors [mean: 32][inv_std: 32][gamma: 32][beta: 32]
  const float* c_lane0 = (lhi ? p.bn_inv : p.bn_mean) + l31;
  const float* c_lane1 = (lhi ? p.bn_beta : p.bn_gamma) + l31;
  auto issue = [&](int stage) {
    const uint32_t slot = lds0 + (uint32_t)(stage % STAGES) * STAGE_BYTES;
    if constexpr (PAIR) {
      if (stage < nst1) {                                                     // the first layer's operands
        const char* xb = first_block + (int64_t)(stage * BK + wave * QB * RPI) * p.HW * 4;
#pragma unroll
        for (int q = 0; q < QB; ++q)
          ring_glds16(xb + (int64_t)(q * RPI) * p.HW * 4, b_lane, slot + A_BYTES + (uint32_t)((wave * QB + q) * RPI) * RB);
        issue_pair_weights(p.first_w, p.first_w_ld, stage, slot);
        return;
      }
      stage -= nst1;
    }
    const char* xb = in_block + (int64_t)(stage * BK + wave * QB * RPI) * p.HW * 4;
#pragma unroll
    for (int q = 0; q < QB; ++q)
      ring_glds16(xb + (int64_t)(q * RPI) * p.HW * 4, b_lane, slot + A_BYTES + (uint32_t)((wave * QB + q) * RPI) * RB);
    if constexpr (PAIR) {
      issue_pair_weights(p.w, p.w_ld, stage, slot);
    } else {
      const char* wb = (const char*)p.w + (A_KCONTIG ? (int64_t)stage * BK * 4 : (int64_t)stage * BK * p.w_ld * 4);
#pragma unroll
      for (int q = 0; q < QA; ++q)
        ring_glds16(wb, a_lane[q], slot + (A_KCONTIG ? (uint32_t)(4096 * wave + 1024 * q) : (uint32_t)((wave * QA + q) * 1024)));
    }
    if (FUSE == 1) {
      ring_glds4(c_lane0 + stage * BK, slot + A_BYTES + B_BYTES + wave * 512);
      ring_glds4(c_lane1 + stage * BK, slot + A_BYTES + B_BYTES + wave * 512 + 256);
    }
  };

  // ---- fragment read offsets inside a stage slot ----
  uint32_t a_read[4];
  if (A_KCONTIG) {
    const int row = 32 * wave + l31, bank_row = row >> 1;
#pragma unroll
    for (int g = 0; g < 4; ++g) a_read[g] = (uint32_t)(bank_row * 256 + ((((row & 1) * 8 + 2 * g + lhi) ^ (bank_row & 15)) * 16));
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) a_read[g] = (uint32_t)((8 * g + 4 * lhi) * 512 + (32 * wave + l31) * 4);
  }
  const uint32_t b_read = (uint32_t)(A_BYTES + (4 * lhi) * RB + l31 * (4 * NI));
  const uint32_t c_read = (uint32_t)(A_BYTES + B_BYTES + wave * 512 + 16 * lhi);

  f32x16 acc[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;

  // One group = four MFMA steps = the k values 8g + 4*lhi + 0..3 of the stage.  The fragments of group g + 1 are read into
  // a second register set while group g's matrix work issues.
  struct Group { float a[4]; float b[4][NI]; f32x4 mean, inv, gamma, beta; };
  auto load_group = [&](Group& f, const char* slot, int g) {
    if (A_KCONTIG) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(slot + a_read[g]);
      f.a[0] = v.x; f.a[1] = v.y; f.a[2] = v.z; f.a[3] = v.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) f.a[q] = *reinterpret_cast<const float*>(slot + a_read[g] + q * 512);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (NI == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(slot + b_read + (8 * g + q) * RB);
        f.b[q][0] = v.x; f.b[q][1] = v.y; f.b[q][2] = v.z; f.b[q][3] = v.w;
      } else if constexpr (NI == 2) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(slot + b_read + (8 * g + q) * RB);
        f.b[q][0] = v.x; f.b[q][1] = v.y;
      } else {
        f.b[q][0] = *reinterpret_cast<const float*>(slot + b_read + (8 * g + q) * RB);
      }
    }
    if (FUSE == 1) {
      f.mean = *reinterpret_cast<const f32x4*>(slot + c_read + 32 * g);
      f.inv = *reinterpret_cast<const f32x4*>(slot + c_read + 128 + 32 * g);
      f.gamma = *reinterpret_cast<const f32x4*>(slot + c_read + 256 + 32 * g);
      f.beta = *reinterpret_cast<const f32x4*>(slot + c_read + 384 + 32 * g);
    }
  };
  auto compute_group = [&](const Group& f) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float b[NI];
      if (FUSE == 1) {
        float ca, cb;
        bn_coefficients(f.mean[q], f.inv[q], f.gamma[q], f.beta[q], ca, cb);     // the forward's own (a, b): same ReLU mask
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) b[ni] = fmaxf(fmaf(f.b[q][ni], ca, cb), 0.f);
      } else {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) b[ni] = f.b[q][ni];
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) acc[ni] = mfma32(f.a[q], b[ni], acc[ni]);
    }
  };

  // ---- epilogue operands ----
  const int64_t row0 = m0 + 32 * wave + 4 * lhi;                       // + mfma32_row(r, 0)
  float* out_lane = p.out + (int64_t)n * p.out_bs + row0 * p.HW + pix0 + NI * l31;
  // FUSE 2: the epilogue's own streams -- x for the mask, the accumulated gradient -- are requested while the K loop runs
  // (after the stage-1 / stage-2 DMAs: 128 registers that this kernel has to spare at two workgroups per CU).  The pass
  // moves 4 * (128 + 3 * rows) bytes per pixel for 2 * 128 * rows FLOP: HBM-bound, so what matters is that the loads of
  // a tile overlap its matrix phase instead of following it.
  const float* x_lane = FUSE == 2 ? p.epi_x + (int64_t)n * p.epi_x_bs + row0 * p.HW + pix0 + 4 * l31 : nullptr;
  f32x4 xs[FUSE == 2 ? 16 : 1], olds[FUSE == 2 ? 16 : 1];
  // the lane's rows of x and of the gradient, `local` = 0 .. 3, 8 .. 11, ...  (PAIR: wave-uniform row bases and ONE lane
  // offset, opaque at each use so that the addresses are formed there -- its K loop has no registers to carry thirty-two
  // 64-bit row addresses, which is what hoisting them makes of the prefetches and the stores)
  const uint32_t lane_at = (uint32_t)(4 * lhi * p.HW + 4 * l31);
  const int64_t wave_at = (int64_t)(m0 + 32 * wave) * p.HW + pix0;
  auto pair_row = [&](int64_t wave_rows, int local) {                       // (offsets, not pointers: those stay global)
    uint32_t at = lane_at;
    int64_t plane = p.HW;
    asm volatile("" : "+s"(wave_rows), "+s"(plane), "+v"(at));
    return (wave_rows + local * plane) + at;
  };
  auto x_row = [&](int local) {
    if constexpr (PAIR) return reinterpret_cast<const f32x4*>(p.epi_x + pair_row((int64_t)n * p.epi_x_bs + wave_at, local));
    else return reinterpret_cast<const f32x4*>(x_lane + (int64_t)local * p.HW);
  };
  auto out_row = [&](int local) {
    if constexpr (PAIR) return reinterpret_cast<f32x4*>(p.out + pair_row((int64_t)n * p.out_bs + wave_at, local));
    else return reinterpret_cast<f32x4*>(out_lane + (int64_t)local * p.HW);
  };
  const bool prefetch = FUSE == 2 && STAGES == 2 && (PAIR || nst >= 3) && active;          // (PAIR: at least four stages)
  const bool accumulate = PAIR || p.mode == 1;
  // out (=, +=) acc * [fma(x, a, b) > 0] * a per row; per row the sums of the masked values and of masked * (x - mean)
  // over the tile's 128 pixels (complete inside this wave: five DPP adds per value), one partial per (pixel block, row).
  // The rows' [128][4] tables (a, b, mean) take the first ring slot once the K loop is over; a PAIR's two tables have
  // 2 x 2 KB of their own behind the ring (its first epilogue runs while DMAs are in flight) and are written up front:
  // the K loop's first barrier publishes them.
  float* table = reinterpret_cast<float*>(smem + (PAIR ? STAGES * STAGE_BYTES : 0));
  float* table_first = table + 512;
  auto fill_table = [&](float* rows, const float* mean, const float* inv, const float* gamma, const float* beta) {
    if (tid < 128) {
      const int o = min(m0 + tid, p.CO - 1);
      const float mu = mean[o];
      float a, b;
      bn_coefficients(mu, inv[o], gamma[o], beta[o], a, b);
      rows[tid * 4 + 0] = a; rows[tid * 4 + 1] = b; rows[tid * 4 + 2] = mu;
    }
  };
  const bool sums_wanted = FUSE == 2 && p.epi_partial != nullptr;
  float* partial = FUSE == 2 ? p.epi_partial + (int64_t)cb * p.epi_ld + row0 : nullptr;
  // the lane's half of the wave for an epilogue's offsets (PAIR: found again where it is used, from an opaque zero, so
  // that no offset derived from it is carried through the K loop -- the last two registers that did not fit)
  auto epilogue_half = [&]() {
    if constexpr (PAIR) {
      unsigned zero = 0;
      asm volatile("" : "+v"(zero));
      return (int)(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero)) >> 5);
    } else {
      return lhi;
    }
  };
  // row r of the lane (local row mfma32_row(r, 0) of the wave): its table entry and its masked accumulators
  auto masked_row = [&](const float* rows, int half, int r, int local, f32x4& t) {
    t = *reinterpret_cast<const f32x4*>(rows + (32 * wave + 4 * half + local) * 4);
    const f32x4 x = xs[r];
    f32x4 v;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) v[ni] = fmaf(x[ni], t.x, t.y) > 0.f ? acc[ni % NI][r] : 0.f;      // (FUSE 2: NI = 4)
    return v;
  };
  auto row_sums = [&](const f32x4& v, const f32x4& x, float mean, float* plain_to, float* centred_to, uint32_t at) {
    const float plain = half_wave_sum((v.x + v.y) + (v.z + v.w));
    const float centred = half_wave_sum((v.x * (x.x - mean) + v.y * (x.y - mean)) + (v.z * (x.z - mean) + v.w * (x.w - mean)));
    if (l31 == 31) {
      plain_to[at] = plain;
      centred_to[at] = centred;
    }
  };
  // v * a + old in ONE rounding per element, spelled out: a launch per layer and a PAIR must round alike
  auto scaled_add = [](const f32x4& v, float a, const f32x4& old) {
    f32x4 sum;
    sum.x = __builtin_fmaf(v.x, a, old.x); sum.y = __builtin_fmaf(v.y, a, old.y);
    sum.z = __builtin_fmaf(v.z, a, old.z); sum.w = __builtin_fmaf(v.w, a, old.w);
    return sum;
  };
  if constexpr (PAIR) {
    fill_table(table_first, p.first_bn_mean, p.first_bn_inv, p.first_bn_gamma, p.first_bn_beta);
    fill_table(table, p.bn_mean, p.bn_inv, p.bn_gamma, p.bn_beta);
  }

  for (int s = 0; s < STAGES - 1 && s < nst; ++s) issue(s);
  for (int t = 0; t < nst; ++t) {
    // stage t has landed once at most the (STAGES - 2) younger stages of this wave are still in flight (plus, FUSE 2, the 16
    // prefetch loads issued behind stage t's DMAs); the barrier also tells that every wave is done reading the slot that is
    // refilled next
    if (FUSE == 2 && prefetch && (t == 1 || (t == 2 && accumulate))) ring_wait_and_barrier<16>();
    else if (nst - 1 - t >= STAGES - 2) ring_wait_and_barrier<PER_STAGE * (STAGES - 2)>();
    else ring_wait_and_barrier<0>();
    if (t + STAGES - 1 < nst) issue(t + STAGES - 1);
    if constexpr (FUSE == 2) {
      if (prefetch && t == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xs[r] = *x_row(mfma32_row(r, 0));
      }
      if (prefetch && t == 1 && accumulate) {
#pragma unroll
        for (int r = 0; r < 16; ++r) olds[r] = *out_row(mfma32_row(r, 0));
      }
    }
    if (!active) continue;
    const char* slot = smem + (t % STAGES) * STAGE_BYTES;
    Group f0, f1;
    load_group(f0, slot, 0);
    load_group(f1, slot, 1);
    compute_group(f0);
    load_group(f0, slot, 2);
    compute_group(f1);
    load_group(f1, slot, 3);
    compute_group(f0);
    compute_group(f1);
    if constexpr (PAIR) {
      if (t == nst1 - 1) {
        // the first layer is complete (x and the old gradient landed with this stage's vmcnt(0)): its epilogue into the old
        // gradient's registers, and the accumulators start over for the second layer
        // (wave-uniform bases and one lane offset: sixteen rows' 64-bit addresses would be kept across the whole K loop)
        float* plain_to = p.first_partial + (int64_t)cb * p.first_ld + m0 + 32 * wave;
        float* centred_to = plain_to + (int64_t)p.epi_cols * p.first_ld;
        const int half = epilogue_half();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int local = mfma32_row(r, 0);
          f32x4 e;
          const f32x4 v = masked_row(table_first, half, r, local, e);
          olds[r] = scaled_add(v, e.x, olds[r]);
          if (sums_wanted) row_sums(v, xs[r], e.z, plain_to, centred_to, (uint32_t)(4 * half + local));
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) acc[ni][r] = 0.f;
          if ((r & 1) == 1) __builtin_amdgcn_sched_barrier(0);             // two rows at a time: no spare registers
        }
      }
    }
  }

  // ---- epilogue: a lane holds NI consecutive pixels of 16 rows ----
  if constexpr (FUSE == 2) {
    if constexpr (!PAIR) {
      __syncthreads();                                                  // (no DMA in flight: the last stage waited vmcnt(0))
      fill_table(table, p.bn_mean, p.bn_inv, p.bn_gamma, p.bn_beta);
      __syncthreads();
    }
    if (!active) return;
    const int half = epilogue_half();
    auto rows = [&](auto accumulating) {
#pragma unroll
      for (int batch = 0; batch < 4; ++batch) {                         // four rows at a time: loads first, stores last
        if (!PAIR && !prefetch) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            xs[4 * batch + e] = *x_row(mfma32_row(4 * batch + e, 0));
            if constexpr (decltype(accumulating)::value) olds[4 * batch + e] = *out_row(e + 8 * batch);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * batch + e, local = e + 8 * batch;
          f32x4 t;
          const f32x4 v = masked_row(table, half, r, local, t);
          f32x4* dst = out_row(local);
          if constexpr (decltype(accumulating)::value) *dst = scaled_add(v, t.x, olds[r]);
          else __builtin_nontemporal_store(v * t.x, dst);
          if constexpr (PAIR) {
            float* plain_to = p.epi_partial + (int64_t)cb * p.epi_ld + m0 + 32 * wave;
            if (sums_wanted) row_sums(v, xs[r], t.z, plain_to, plain_to + (int64_t)p.epi_cols * p.epi_ld, (uint32_t)(4 * half + local));
          } else {
            if (sums_wanted) row_sums(v, xs[r], t.z, partial, partial + (int64_t)p.epi_cols * p.epi_ld, (uint32_t)local);
          }
        }
        __builtin_amdgcn_sched_barrier(0);                               // keeps a batch's loads from joining the previous one's
      }
    };
    if (accumulate) rows(std::true_type{});
    else rows(std::false_type{});
    return;
  }
  if (!active) return;
  if (p.mode == 1) {
    // accumulate: the sixteen rows' old values in one batch, then the stores (loads and stores return through one in-order
    // counter, vmcnt: `+=` row by row made every load wait for the store in front of it)
    float previous[16][NI];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* src = out_lane + (int64_t)mfma32_row(r, 0) * p.HW;
      if constexpr (NI == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src);
        previous[r][0] = v.x; previous[r][1] = v.y; previous[r][2] = v.z; previous[r][3] = v.w;
      } else if constexpr (NI == 2) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(src);
        previous[r][0] = v.x; previous[r][1] = v.y;
      } else {
        previous[r][0] = *src;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float* dst = out_lane + (int64_t)mfma32_row(r, 0) * p.HW;
      if constexpr (NI == 4) {
        f32x4 v;
        v.x = previous[r][0] + acc[0][r]; v.y = previous[r][1] + acc[1][r]; v.z = previous[r][2] + acc[2][r]; v.w = previous[r][3] + acc[3][r];
        *reinterpret_cast<f32x4*>(dst) = v;
      } else if constexpr (NI == 2) {
        f32x2 v;
        v.x = previous[r][0] + acc[0][r]; v.y = previous[r][1] + acc[1][r];
        *reinterpret_cast<f32x2*>(dst) = v;
      } else {
        *dst = previous[r][0] + acc[0][r];
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float* dst = out_lane + (int64_t)mfma32_row(r, 0) * p.HW;
    if constexpr (NI == 4) {
      f32x4 v;
      v.x = acc[0][r]; v.y = acc[1][r]; v.z = acc[2][r]; v.w = acc[3][r];
      __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst));             // consumed by a later kernel
    } else if constexpr (NI == 2) {
      f32x2 v;
      v.x = acc[0][r]; v.y = acc[1][r];
      __builtin_nontemporal_store(v, reinterpret_cast<f32x2*>(dst));
    } else {
      __builtin_nontemporal_store(acc[0][r], dst);
    }
  }
}

// Whether the LDS-DMA kernel takes the 128-row tiles of this convolution (the caller sends the remaining rows, if any,
// to pointwise_kernel); *tile_pixels = 128, 64 or 32.  Everything the DMA addresses must be 16-byte aligned.
bool pointwise_ring_eligible(const float* in, int64_t in_bs, const float* w, int32_t w_so, int32_t w_si, const float* bias,
                             const float* out, int64_t out_bs, int32_t N, int32_t CI, int32_t CO, int32_t HW, bool fused_pro,
                             const BnBackwardEpilogue* epilogue, int* tile_pixels) {
  if (bias || CO < 128 || CO % 32 != 0 || CI % 32 != 0 || CI < 32 || HW % 32 != 0) return false;
  if (!(w_si == 1 && w_so % 4 == 0) && !(w_so == 1 && w_si % 4 == 0)) return false;
  if ((((uintptr_t)in | (uintptr_t)w | (uintptr_t)out) & 15) || (in_bs & 3) || (out_bs & 3)) return false;
  // A data gradient with the batch-norm backward epilogue moves 4 * (128 + 3 * rows) bytes per pixel for 2 * 128 * rows
  // FLOP: HBM-bound on either kernel.  Here the epilogue's x / old-gradient rows are requested during the K loop and the
  // last row tile may be partial (no second launch): 37.5 ms per step against 39.9 ms on pointwise_kernel (profiles/r04e).
  static const bool no_epilogue = getenv("SRGAN_NO_PW_RING_EPILOGUE") != nullptr;
  if (epilogue && (no_epilogue || HW % 128 != 0 || (((uintptr_t)epilogue->x) & 15) || (epilogue->x_bs & 3))) return false;
  // Few pixel blocks: narrower tiles multiply the workgroups (16 images of 32 x 32 pixels, 128 rows: 43 us on the 128-pixel
  // tile = half the CUs idle, 30 us on the 64-pixel tile); the epilogue's partial sums are per 128-pixel block.
  constexpr int narrow_below = 512, slim_below = 384, min_blocks = 192;
  const int64_t tiles = (int64_t)N * ((CO + 127) / 128);
  int pixels = 128;
  if (epilogue) pixels = 128;
  else if (HW % 128 != 0 || tiles * (HW / 128) < narrow_below) pixels = 64;
  if (!epilogue && (HW % 64 != 0 || (pixels == 64 && tiles * (HW / 64) < slim_below))) pixels = 32;
  // too few workgroups even so: the K-split kernel / short tiles of pointwise.hip do better
  if (tiles * (HW / pixels) < min_blocks) return false;
  (void)fused_pro;
  *tile_pixels = pixels;
  return true;
}

template <int NI, bool A_KCONTIG, int FUSE, bool PAIR = false>
static int launch_ring(const RingParams& p, unsigned blocks, hipStream_t stream) {
  constexpr int STAGES = 2;
  constexpr int bytes = STAGES * (128 * 32 * 4 + 32 * 128 * NI + (FUSE == 1 ? 2048 : 0)) + (PAIR ? 2 * 2048 : 0);
  constexpr auto kernel = pointwise_ring_kernel<STAGES, NI, A_KCONTIG, FUSE, PAIR>;
  SRGAN_HIP(allow_dynamic_lds<kernel>(bytes));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), bytes, stream, p);
  return launch_status();
}

// Every row of the convolution (the last 128-row tile may be partial); *rows_done = the rows it covered.
int pointwise_ring_run(const float* in, int64_t in_bs, const float* w, int32_t w_so, int32_t w_si, float* out, int64_t out_bs,
                       int32_t N, int32_t CI, int32_t CO, int32_t HW, int accumulate, hipStream_t stream,
                       const float* const* bn, const BnBackwardEpilogue* epilogue, float* epi_partial, int32_t epi_cols,
                       int tile_pixels, int32_t* rows_done) {
  RingParams p;
  p.in = in; p.w = w; p.out = out;
  p.N = N; p.CI = CI; p.CO = CO; p.HW = HW; p.in_bs = in_bs; p.out_bs = out_bs;
  const bool k_contiguous = w_si == 1;
  p.w_ld = k_contiguous ? w_so : w_si;
  p.tiles_m = (CO + 127) / 128;
  p.bpi = HW / tile_pixels;
  p.mode = accumulate == 1 ? 1 : 0;
  p.bn_mean = p.bn_inv = p.bn_gamma = p.bn_beta = nullptr;
  p.epi_x = nullptr; p.epi_x_bs = 0; p.epi_partial = nullptr; p.epi_cols = 0; p.epi_ld = CO;
  p.first_in = p.first_w = nullptr; p.first_w_ld = 0; p.first_partial = nullptr; p.first_ld = 0;
  p.first_bn_mean = p.first_bn_inv = p.first_bn_gamma = p.first_bn_beta = nullptr;
  if (bn) { p.bn_mean = bn[0]; p.bn_inv = bn[1]; p.bn_gamma = bn[2]; p.bn_beta = bn[3]; }
  if (epilogue) {
    p.bn_mean = epilogue->bn[0]; p.bn_inv = epilogue->bn[1]; p.bn_gamma = epilogue->bn[2]; p.bn_beta = epilogue->bn[3];
    p.epi_x = epilogue->x; p.epi_x_bs = epilogue->x_bs; p.epi_partial = epi_partial; p.epi_cols = epi_cols;
  }
  const int64_t blocks = (int64_t)N * p.bpi * p.tiles_m;
  SRGAN_REQUIRE(blocks < ((int64_t)1 << 31), SRGAN_ERANGE, "pointwise ring grid");
  p.xcd_remap = (p.tiles_m > 1 && blocks % 8 == 0) ? 1 : 0;
  *rows_done = CO;
  const unsigned grid = (unsigned)blocks;
  const int fuse = epilogue ? 2 : (bn ? 1 : 0);
  if (fuse == 2) return k_contiguous ? launch_ring<4, true, 2>(p, grid, stream) : launch_ring<4, false, 2>(p, grid, stream);
  if (tile_pixels == 32) {
    if (fuse == 1) return k_contiguous ? launch_ring<1, true, 1>(p, grid, stream) : launch_ring<1, false, 1>(p, grid, stream);
    return k_contiguous ? launch_ring<1, true, 0>(p, grid, stream) : launch_ring<1, false, 0>(p, grid, stream);
  }
  if (tile_pixels == 64) {
    if (fuse == 1) return k_contiguous ? launch_ring<2, true, 1>(p, grid, stream) : launch_ring<2, false, 1>(p, grid, stream);
    return k_contiguous ? launch_ring<2, true, 0>(p, grid, stream) : launch_ring<2, false, 0>(p, grid, stream);
  }
  if (fuse == 1) return k_contiguous ? launch_ring<4, true, 1>(p, grid, stream) : launch_ring<4, false, 1>(p, grid, stream);
  return k_contiguous ? launch_ring<4, true, 0>(p, grid, stream) : launch_ring<4, false, 0>(p, grid, stream);
}

// ---- two consecutive dense layers' fused data gradients (norm1 -> relu1 -> conv1 backward, accumulated into the block's
// gradient buffer) with ONE pass over their common rows.  Layer A = l + 1 writes the rows [0, rows_A), layer B = l the rows
// [0, rows_B), rows_B = rows_A - 32, and B's 3x3 data gradient reads the rows [rows_B, rows_A) with A's contribution in
// them.  So A's last 32 rows run first, on their own (the strip: the FUSE 2 kernel on one 32-row tile, reached through
// pointer offsets), and once B's gradient exists one PAIR launch applies A and then B to the rows [0, rows_B).

// Whether a pair takes this form: both layers on the LDS-DMA kernel by themselves (the per-layer launches then give the
// same bits), 128 input channels each (four K stages per layer), at least one whole row tile in common.  Pointers may be
// null (a geometry-only query).
bool pointwise_ring_pair_eligible(const float* in_a, const float* in_b, int64_t in_bs, const float* w_a, const float* w_b,
                                  const float* x, int64_t x_bs, const float* out, int64_t out_bs, int32_t N, int32_t CI,
                                  int32_t rows_a, int32_t rows_b, int32_t HW) {
  if (CI != 128 || rows_a != rows_b + 32 || rows_b < 128 || HW % 128 != 0 || x_bs != out_bs) return false;
  // The strip is launch-bound (15 us whatever its size), the pair saves about a sixth of two per-layer launches: on the
  // 16 x 16 planes of the last crowd block (16 images: 26 us per layer) strip + pair came to 59.7 us against 52.0 us, a tie at
  // 48 images, and a gain from 16 384 pixels upwards (profiles/paired_data_gradient.md) -- smaller launches stay per layer.
  constexpr int64_t pair_min_pixels = 16384;
  if ((int64_t)N * HW < pair_min_pixels) return false;
  if ((int64_t)N * (HW / 128) * ((rows_b + 127) / 128) >= ((int64_t)1 << 31)) return false;
  const BnBackwardEpilogue epilogue{x, x_bs, {nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr, nullptr};
  int pixels_a = 0, pixels_b = 0;
  return pointwise_ring_eligible(in_a, in_bs, w_a, 1, rows_a, nullptr, out, out_bs, N, CI, rows_a, HW, false, &epilogue, &pixels_a) &&
         pointwise_ring_eligible(in_b, in_bs, w_b, 1, rows_b, nullptr, out, out_bs, N, CI, rows_b, HW, false, &epilogue, &pixels_b) &&
         pixels_a == 128 && pixels_b == 128;
}

static RingParams fused_gradient_params(const float* in, int64_t in_bs, const float* w, int32_t w_ld, float* out, int64_t out_bs,
                                        int32_t N, int32_t CI, int32_t rows, int32_t HW, const BnBackwardEpilogue& epilogue,
                                        int64_t row0, int32_t partial_ld) {
  RingParams p;
  p.in = in; p.w = w + row0; p.out = out + row0 * HW;
  p.N = N; p.CI = CI; p.CO = rows; p.HW = HW; p.in_bs = in_bs; p.out_bs = out_bs;
  p.w_ld = w_ld;
  p.tiles_m = (rows + 127) / 128;
  p.bpi = HW / 128;
  p.mode = 1;
  p.bn_mean = epilogue.bn[0] + row0; p.bn_inv = epilogue.bn[1] + row0; p.bn_gamma = epilogue.bn[2] + row0; p.bn_beta = epilogue.bn[3] + row0;
  p.epi_x = epilogue.x + row0 * HW; p.epi_x_bs = epilogue.x_bs;
  p.epi_partial = epilogue.partial_out ? epilogue.partial_out + row0 : nullptr;
  p.epi_cols = N * p.bpi; p.epi_ld = partial_ld;
  p.first_in = p.first_w = nullptr; p.first_w_ld = 0; p.first_partial = nullptr; p.first_ld = 0;
  p.first_bn_mean = p.first_bn_inv = p.first_bn_gamma = p.first_bn_beta = nullptr;
  p.xcd_remap = (p.tiles_m > 1 && ((int64_t)N * p.bpi * p.tiles_m) % 8 == 0) ? 1 : 0;
  return p;
}

// The strip: the rows [row0, CO) of one layer's fused data gradient, accumulated (row0 a multiple of 32; CO - row0 <= 128).
// The partial sums land in the layer's own region, whose rows are CO wide.
int pointwise_ring_strip_run(const float* in, int64_t in_bs, const float* w, float* out, int64_t out_bs, int32_t N, int32_t CI,
                             int32_t CO, int32_t row0, int32_t HW, const BnBackwardEpilogue& epilogue, hipStream_t stream) {
  const int32_t rows = CO - row0;
  const RingParams p = fused_gradient_params(in, in_bs, w, CO, out, out_bs, N, CI, rows, HW, epilogue, row0, CO);
  const int profile_slot = profile_bracket_begin(stream);
  const int status = launch_ring<4, false, 2>(p, (unsigned)(N * p.bpi), stream);
  const int64_t pixels = (int64_t)N * HW;
  profile_bracket_end(profile_slot, stream, rows, pixels, CI, KIND_POINTWISE_RING, 128, 128, 1, 0, 0, (CI + 2 * (int64_t)rows) * pixels);
  return status;
}

// The pair: layer A's and then layer B's contribution to the rows [0, rows_b); both layers' partial sums or neither's.
int pointwise_ring_pair_run(const float* in_a, const float* w_a, int32_t rows_a, const BnBackwardEpilogue& epilogue_a,
                            const float* in_b, const float* w_b, int32_t rows_b, const BnBackwardEpilogue& epilogue_b,
                            int64_t in_bs, float* out, int64_t out_bs, int32_t N, int32_t CI, int32_t HW, hipStream_t stream) {
  RingParams p = fused_gradient_params(in_b, in_bs, w_b, rows_b, out, out_bs, N, CI, rows_b, HW, epilogue_b, 0, rows_b);
  p.first_in = in_a; p.first_w = w_a; p.first_w_ld = rows_a;
  p.first_bn_mean = epilogue_a.bn[0]; p.first_bn_inv = epilogue_a.bn[1]; p.first_bn_gamma = epilogue_a.bn[2]; p.first_bn_beta = epilogue_a.bn[3];
  p.first_partial = epilogue_a.partial_out; p.first_ld = rows_a;
  const int profile_slot = profile_bracket_begin(stream);
  const int status = launch_ring<4, false, 2, true>(p, (unsigned)((int64_t)N * p.bpi * p.tiles_m), stream);
  // what the launch executes: K = both layers' channels; x and the old gradient are read once
  const int64_t pixels = (int64_t)N * HW;
  profile_bracket_end(profile_slot, stream, rows_b, pixels, 2 * CI, KIND_POINTWISE_RING, 128, 128, 1, 0, 0,
                      (2 * (int64_t)CI + 2 * (int64_t)rows_b) * pixels);
  return status;
}

}  // namespace srgan
