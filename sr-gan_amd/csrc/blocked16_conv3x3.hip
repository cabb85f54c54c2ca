// blocked16_conv3x3.hip -- the 3x3 / stride 1 / pad 1 convolution of the 16-bit data path (layout: blocked16.h), from packed
// weights (the conv-weight shadows of blocked16_shadows.hip).
//
// It serves VGG-16's convolution stack (reference age/vgg.py:28-53,70-84: conv3x3 + bias -> ReLU) in every pass that is a
// convolution: the forward, the data gradient (the same kernel on the flipped, transposed shadow) and the linearised forward of
// the penalty's double backward.  The activation is FUSED: the epilogue adds the bias and applies relu / leaky_relu before the
// 16-bit store (epi 1), or multiplies by the derivative of the activation that produced the reference tensor (epi 2, `mask by
// reference`: the sign pattern of the activated tensor itself), so neither the pre-activation tensor nor the un-masked gradient
// ever exists in HBM.
//
//   hconv3x3_kernel       register-staged operands, one or two LDS stages, optional K split with an ordered finish
//   hconv3x3_dma_kernel   the same tiles with LDS-DMA staging in a ring: the 64-row tiles with an unsplit K
//   hconv3_plan           the tile shape and K split of a call (SRGAN_H_CONV_NI forces the pixel tile, SRGAN_H_DMA_RING the staging)
#include <type_traits>
#include <stdlib.h>
#include "blocked16.h"
#include "launchers.h"
#include "split_finish.h"

namespace srgan {

struct HConv3Params {
  const Slot* in; const Slot* wp; Slot* out; const float* bias; const Slot* ref;
  float slope;
  int32_t epi;                 // 0 plain, 1 bias (optional) + leaky(slope), 2 multiply by mask(ref, slope)
  int32_t N, CGI, CGO, CO, C_real, H, W;      // CO = rows of the packed weights (>= 8 * CGO is not required: rows beyond are zero)
  int32_t chunks, chunks_per_split;
  int32_t tiles_x, tiles_y, tiles_m;
  float* split_ws; unsigned int* split_tickets;
  int32_t xcd_remap;
};

__device__ unsigned int g_hconv3_split_tickets[SPLIT_TICKET_SETS * SPLIT_TICKET_TILES];

// The BM bias values of a workgroup's rows into LDS, at the kernel's start (the barrier behind it is nowhere near the epilogue's
// stores: a barrier in front of the epilogue would make the four waves' stores wait for the slowest wave's last MFMA).
template <int BM>
__device__ __forceinline__ void hconv3_stage_bias(const float* bias, int epi, int C_real, int m0, float* bias_rows) {
  if (epi == 1 && bias != nullptr) {
    if ((int)threadIdx.x < BM) bias_rows[threadIdx.x] = m0 + (int)threadIdx.x < C_real ? bias[m0 + threadIdx.x] : 0.f;
    __syncthreads();
  }
}

// Epilogue of the 3x3 kernels.  C/D fragment: column = pixel (lane & 31), rows mfma32_row(r, lane >> 5): registers
// 4q .. 4q + 3 are four CONSECUTIVE output channels = 8 bytes of the pixel's slot of group (m0 + 32 mi) / 8 + q; the 32 lanes of
// a half cover 32 consecutive slots (with the other half: 512 contiguous bytes per store instruction).
template <int BM, int NI, int TW, int ROWS, int PREC>
__device__ __forceinline__ void hconv3_epilogue(const HConv3Params& p, f32x16 (&acc)[BM / 32][NI], int n0, int y0, int x0, int m0,
                                                int wave, int l31, int lhi, const float* bias_rows) {
  constexpr int MI = BM / 32;
  const int HW = p.H * p.W;
  // bias_rows: the tile's bias values in LDS (hconv3_stage_bias at the kernel's start).  Read per value from global memory
  // inside the loops below they were 4 dependent loads per quad -- 128 VMEM instructions per wave at 64 rows x 512 pixels, 25 us
  // of a 59 us launch (conv1_1, batch 128: scratch/h_conv_bench.py).
  const bool with_bias = p.epi == 1 && p.bias != nullptr;
  float4 bias4[MI][4];              // this lane's rows are the same for every pixel column: read once
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd)
      bias4[mi][qd] = with_bias ? *reinterpret_cast<const float4*>(&bias_rows[mi * 32 + 8 * qd + 4 * lhi]) : make_float4(0.f, 0.f, 0.f, 0.f);
  // epi 2: the mask references of a pixel column are loaded in ONE batch in front of its stores.  On this ISA loads and stores
  // return through one in-order counter (vmcnt): interleaved load - use - store, every load waited for the stores in front of it
  // (32 round trips per wave at 64 rows x 512 pixels: 102 us for the data gradient of a layer whose forward took 69).
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int q = (wave * NI + ni) * 32 + l31;
    const int n = n0 + q / (ROWS * TW), y = y0 + (q / TW) % ROWS, x = x0 + q % TW;
    if (n >= p.N || y >= p.H || x >= p.W) continue;
    const int64_t pixel = (int64_t)n * p.CGO * HW + y * p.W + x;
    uint2 refs[MI][4];
    if (p.epi == 2) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const int group = (m0 + mi * 32) / 8 + qd;
          refs[mi][qd] = group < p.CGO ? *(reinterpret_cast<const uint2*>(p.ref + pixel + (int64_t)group * HW) + lhi) : uint2{0u, 0u};
        }
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int qp = 0; qp < 2; ++qp) {
        // two register quads = this lane's half (channels 4 lhi .. 4 lhi + 3) of the slots of groups g0 and g0 + 1
        const int g0 = (m0 + mi * 32) / 8 + 2 * qp;
        uint2 packed[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int qd = 2 * qp + h;
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = acc[mi][ni][4 * qd + j];
          if (p.epi == 1) {
            const float4 b4 = bias4[mi][qd];
            v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : v[j] * p.slope;
          } else if (p.epi == 2) {
            const uint2 r = refs[mi][qd];
            v[0] *= h_mask(r.x & 0xFFFFu, p.slope); v[1] *= h_mask(r.x >> 16, p.slope);
            v[2] *= h_mask(r.y & 0xFFFFu, p.slope); v[3] *= h_mask(r.y >> 16, p.slope);
          }
          packed[h].x = h_pack2<PREC>(v[0], v[1]);
          packed[h].y = h_pack2<PREC>(v[2], v[3]);
        }
        // v_permlane32_swap: the upper half-wave's value of the first operand changes places with the lower half-wave's of the
        // second.  Before: lane l (< 32) holds channels 0-3 of (g0, pixel l) and of (g0 + 1, pixel l), lane l + 32 channels 4-7 of
        // both.  After: lane l holds the WHOLE slot of (g0, pixel l), lane l + 32 the whole slot of (g0 + 1, pixel l): one
        // 16-byte store per lane (2 x 512 contiguous bytes per instruction) instead of two 8-byte stores (0-7 % per launch).
        const auto first = __builtin_amdgcn_permlane32_swap(packed[0].x, packed[1].x, false, false);
        const auto second = __builtin_amdgcn_permlane32_swap(packed[0].y, packed[1].y, false, false);
        const int group = g0 + lhi;
        if (group < p.CGO) {
          uint4 whole;
          whole.x = first[0]; whole.y = second[0]; whole.z = first[1]; whole.w = second[1];
          *reinterpret_cast<uint4*>(p.out + pixel + (int64_t)group * HW) = whole;
        }
      }
    }
  }
}

// One workgroup (4 waves) = BM output channels x P = 128 * NI pixels.  The pixel tile is IMG x ROWS x TW with
// IMG * ROWS * TW = P: a ROWS x 32 band of one image on wide planes, whole small images side by side on the 16 / 8 / 4
// pixel planes of VGG's later stages (a one-image tile would leave most MFMA columns outside the image there).  Per
// 16-channel chunk the halo patch [2 groups][IMG][(ROWS + 2) x (TW + 2)] and the weight slice [9 taps][2 groups][BM] are
// staged in LDS as operand slots (register-staged: the next chunk's 16-byte loads are in flight during the current
// chunk's 9 * MI * NI MFMAs) and every fragment is one ds_read_b128.
// STAGES = 2: two LDS stages, one barrier per chunk; STAGES = 1 (the 512-pixel tiles, whose two stages would not fit two
// workgroups per CU): one stage, the next chunk waits in registers, two barriers per (twice as long) chunk.
template <int BM, int NI, int TW, int ROWS, int PREC, int STAGES = 2>
__global__ __launch_bounds__(256, 2) void hconv3x3_kernel(const HConv3Params p) {
  constexpr int P = 128 * NI, IMG = P / (ROWS * TW), PW = TW + 2, PH = ROWS + 2, PLANE = PH * PW;
  static_assert(IMG * ROWS * TW == P && IMG >= 1, "the pixel tile is IMG x ROWS x TW");
  constexpr int MI = BM / 32;
  constexpr int PATCH_G = IMG * PLANE, PATCH_Q = 2 * PATCH_G, WT_Q = 18 * BM, STAGE_Q = PATCH_Q + WT_Q;
  constexpr int NP = (PATCH_Q + 255) / 256, NW = (WT_Q + 255) / 256;
  __shared__ Slot lds[STAGES * STAGE_Q];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  int block = blockIdx.x;
  if (p.xcd_remap) block = xcd_band_order(block, (int)gridDim.x);
  const int logical_block = block;
  const int tm = block % p.tiles_m; block /= p.tiles_m;
  const int tx = block % p.tiles_x; block /= p.tiles_x;
  const int ty = block % p.tiles_y;
  const int n0 = (block / p.tiles_y) * IMG;
  const int m0 = tm * BM, y0 = ty * ROWS, x0 = tx * TW;
  __shared__ __attribute__((aligned(16))) float bias_rows[BM];
  hconv3_stage_bias<BM>(p.bias, p.epi, p.C_real, m0, bias_rows);
  const int cbeg = (int)blockIdx.y * p.chunks_per_split;
  const int cend = min(p.chunks, cbeg + p.chunks_per_split);
  const int HW = p.H * p.W;

  int poff[NP], pgrp[NP], woff[NW];
#pragma unroll
  for (int e = 0; e < NP; ++e) {
    const int flat = e * 256 + tid;
    const int g = flat / PATCH_G, rest = flat - g * PATCH_G;
    const int img = rest / PLANE, pix = rest - img * PLANE;
    const int py = pix / PW, px = pix - py * PW;
    const int y = y0 - 1 + py, x = x0 - 1 + px;
    const bool ok = flat < PATCH_Q && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W && n0 + img < p.N;
    poff[e] = ok ? img * p.CGI * HW + y * p.W + x : -1;
    pgrp[e] = g;
  }
#pragma unroll
  for (int e = 0; e < NW; ++e) {
    const int flat = e * 256 + tid;
    const int o = flat % BM, tg = flat / BM;
    const bool ok = flat < WT_Q && (m0 + o) < p.CO;
    woff[e] = ok ? tg * p.CO + m0 + o : -1;
  }
  const Slot* in_n = p.in + (int64_t)n0 * p.CGI * HW;

  Slot rp[NP], rw[NW];
  auto fetch = [&](int c) {                                 // raw loads only: validity is applied at stage time
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      const int g = 2 * c + pgrp[e];
      const bool ok = poff[e] >= 0 && g < p.CGI;
      rp[e] = in_n[ok ? g * HW + poff[e] : 0];
    }
#pragma unroll
    for (int e = 0; e < NW; ++e) rw[e] = p.wp[(int64_t)c * (18 * p.CO) + (woff[e] >= 0 ? woff[e] : 0)];
  };
  auto stage = [&](int c, Slot* stage_base) {
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      const int flat = e * 256 + tid;
      Slot v = rp[e];
      if (!(poff[e] >= 0 && 2 * c + pgrp[e] < p.CGI)) v = Slot{{0u, 0u, 0u, 0u}};
      if (flat < PATCH_Q) stage_base[flat] = v;
    }
#pragma unroll
    for (int e = 0; e < NW; ++e) {
      const int flat = e * 256 + tid;
      Slot v = rw[e];
      if (woff[e] < 0) v = Slot{{0u, 0u, 0u, 0u}};
      if (flat < WT_Q) stage_base[PATCH_Q + flat] = v;
    }
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  int b_lane[NI];                                           // this lane's pixel of column block ni in the patch (window origin)
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int q = (wave * NI + ni) * 32 + l31;
    b_lane[ni] = lhi * PATCH_G + (q / (ROWS * TW)) * PLANE + ((q / TW) % ROWS) * PW + q % TW;
  }
  const int a_lane = PATCH_Q + lhi * BM + l31;              // + tap * 2 * BM + mi * 32

  auto multiply = [&](const Slot* st) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap % 3;
      Slot a[MI], b[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi] = st[a_lane + tap * 2 * BM + mi * 32];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) b[ni] = st[b_lane[ni] + kh * PW + kw];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = h_mfma<PREC>(a[mi], b[ni], acc[mi][ni]);
    }
  };
  if (cbeg < cend) {
    fetch(cbeg);
    if constexpr (STAGES == 2) {
      stage(cbeg, lds);
      __syncthreads();
      int cur = 0;
      for (int c = cbeg; c < cend; ++c) {
        const bool more = c + 1 < cend;
        if (more) fetch(c + 1);
        multiply(lds + cur * STAGE_Q);
        if (more) stage(c + 1, lds + (cur ^ 1) * STAGE_Q);     // the other stage: everyone left it at the previous barrier
        __syncthreads();
        cur ^= 1;
      }
    } else {
      for (int c = cbeg; c < cend; ++c) {
        if (c > cbeg) __syncthreads();                          // the previous chunk's fragment reads are done
        stage(c, lds);
        __syncthreads();
        if (c + 1 < cend) fetch(c + 1);
        multiply(lds);
      }
    }
  }

  if (gridDim.y > 1) {       // K split, ordered finish: the tile's last workgroup goes on with the sum of all slices, in slice order
    constexpr int COUNT = MI * NI * 16;
    if (!split_finish_ordered<COUNT, 256>(p.split_ws + (int64_t)logical_block * gridDim.y * (COUNT * 256), (int)blockIdx.y,
                                          (int)gridDim.y, p.split_tickets + logical_block,
                                          acc_flat(acc), acc_flat(acc)))
      return;
  }

  hconv3_epilogue<BM, NI, TW, ROWS, PREC>(p, acc, n0, y0, x0, m0, wave, l31, lhi, bias_rows);
}

// ---- the same convolution with LDS-DMA staging (global_load_lds_dwordx4: HBM / L2 -> LDS without passing the registers) -----
// The register-staged kernel above has ONE chunk in flight per workgroup and pays a ds_write phase per chunk; the counters
// (profiles/r06f) show its waves parked on memory 46 % of the time at 1.4x the algorithmic HBM bytes: latency, not bandwidth.
// Here a chunk's patch and weight slots are fetched by DMA into a ring of RING stages, RING - 1 chunks ahead, with no staging
// registers and no LDS-write instructions.  An LDS-DMA writes lane-linearly (wave-uniform LDS base + lane * 16) from PER-LANE
// global addresses, and the stage image [patch slots, rounded up to whole 64-slot instructions][weight slots][padding to a
// multiple of four instructions] is linear in the staging index, so instruction i of a chunk is "slots 64 i .. 64 i + 63" and
// the halo gather lives entirely in the lanes' source addresses; slots that are padding (outside the image, beyond the
// channels) read a 16-byte block of zeros in global memory.  Wave w issues instructions w, w + 4, ...: every wave exactly
// L = TP / 4, so `s_waitcnt vmcnt(L * chunks left in flight)` is exact; one raw s_barrier per chunk (a __syncthreads() would
// drain the DMA queue).  No K split (the small layers keep the register-staged kernel).
__device__ Slot g_h_zero_slots[4];
const Slot* h_zero_slots() { return reinterpret_cast<const Slot*>(device_tickets(g_h_zero_slots)); }

template <int BM, int NI, int TW, int ROWS, int PREC, int RING>
__global__ __launch_bounds__(256, RING == 2 ? 2 : 1) void hconv3x3_dma_kernel(const HConv3Params p, const Slot* zero) {
  constexpr int P = 128 * NI, IMG = P / (ROWS * TW), PW = TW + 2, PH = ROWS + 2, PLANE = PH * PW;
  static_assert(IMG * ROWS * TW == P && IMG >= 1, "the pixel tile is IMG x ROWS x TW");
  constexpr int MI = BM / 32;
  constexpr int PATCH_G = IMG * PLANE, PATCH_Q = 2 * PATCH_G, WT_Q = 18 * BM;
  constexpr int PATCH_I = (PATCH_Q + 63) / 64, WT_I = WT_Q / 64, T = PATCH_I + WT_I, TP = (T + 3) / 4 * 4, L = TP / 4;
  constexpr int WT_OFF = PATCH_I * 64, STAGE_Q = TP * 64;
  static_assert(WT_Q % 64 == 0, "whole weight instructions");
  extern __shared__ __attribute__((aligned(16))) Slot ring[];

  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int block = blockIdx.x;
  if (p.xcd_remap) block = xcd_band_order(block, (int)gridDim.x);
  const int tm = block % p.tiles_m; block /= p.tiles_m;
  const int tx = block % p.tiles_x; block /= p.tiles_x;
  const int ty = block % p.tiles_y;
  const int n0 = (block / p.tiles_y) * IMG;
  const int m0 = tm * BM, y0 = ty * ROWS, x0 = tx * TW;
  __shared__ __attribute__((aligned(16))) float bias_rows[BM];
  const int HW = p.H * p.W;
  const uint32_t lds0 = h_lds_address(ring);

  // this lane's source of instruction wave + 4 e: an offset (slots) from the input of image n0 (patch; + group * HW + the chunk's
  // 2 * HW * c) or from the packed weights (+ 18 * CO * c); kind 0 patch group 0, 1 patch group 1, 2 weights, 3 zeros
  int off[L], kind[L];
#pragma unroll
  for (int e = 0; e < L; ++e) {
    const int i = wave + 4 * e;
    off[e] = 0; kind[e] = 3;
    if (i < PATCH_I) {
      const int flat = i * 64 + lane;
      const int g = flat / PATCH_G, rest = flat - g * PATCH_G;
      const int img = rest / PLANE, pix = rest - img * PLANE;
      const int py = pix / PW, px = pix - py * PW;
      const int y = y0 - 1 + py, x = x0 - 1 + px;
      const bool ok = flat < PATCH_Q && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W && n0 + img < p.N;
      if (ok) { off[e] = (img * p.CGI + g) * HW + y * p.W + x; kind[e] = g; }
    } else if (i < T) {
      const int flat = (i - PATCH_I) * 64 + lane;
      const int o = flat % BM, tg = flat / BM;
      if (m0 + o < p.CO) { off[e] = tg * p.CO + m0 + o; kind[e] = 2; }
    }
  }
  const Slot* in_n = p.in + (int64_t)n0 * p.CGI * HW;
  auto issue = [&](int c, int stage) {
#pragma unroll
    for (int e = 0; e < L; ++e) {
      const Slot* src = zero;
      if (kind[e] == 2) src = p.wp + ((int64_t)c * (18 * p.CO) + off[e]);
      else if (kind[e] < 2 && 2 * c + kind[e] < p.CGI) src = in_n + ((int64_t)c * (2 * HW) + off[e]);
      h_glds16(src, lds0 + (uint32_t)((stage * STAGE_Q + (wave + 4 * e) * 64) * 16));
    }
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  int b_lane[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int q = ((tid >> 6) * NI + ni) * 32 + l31;
    b_lane[ni] = lhi * PATCH_G + (q / (ROWS * TW)) * PLANE + ((q / TW) % ROWS) * PW + q % TW;
  }
  const int a_lane = WT_OFF + lhi * BM + l31;

  const int chunks = p.chunks;
#pragma unroll
  for (int d = 0; d < RING - 1; ++d)
    if (d < chunks) issue(d, d);
  hconv3_stage_bias<BM>(p.bias, p.epi, p.C_real, m0, bias_rows);           // behind the first chunk's requests, not in front of them
  int stage = 0;
  for (int c = 0; c < chunks; ++c) {
    // chunk c has landed (this wave's part: vmcnt; everybody's: the barrier), and everybody is done reading the stage that
    // chunk c + RING - 1 goes into (it held chunk c - 1)
    if (RING == 3 && c + 1 < chunks) h_dma_wait_and_barrier<L>();
    else h_dma_wait_and_barrier<0>();
    if (c + RING - 1 < chunks) issue(c + RING - 1, (stage + RING - 1) % RING);
    const Slot* st = ring + stage * STAGE_Q;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap % 3;
      Slot a[MI], b[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi] = st[a_lane + tap * 2 * BM + mi * 32];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) b[ni] = st[b_lane[ni] + kh * PW + kw];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = h_mfma<PREC>(a[mi], b[ni], acc[mi][ni]);
    }
    stage = stage + 1 == RING ? 0 : stage + 1;
  }
  hconv3_epilogue<BM, NI, TW, ROWS, PREC>(p, acc, n0, y0, x0, m0, tid >> 6, l31, lhi, bias_rows);
}

struct HConv3Plan { int bm, ni, tw, rows, tiles_x, tiles_y, tiles_m, tiles_n, split, chunks_per; int64_t blocks; };

static bool hconv3_plan(int32_t N, int32_t CGI, int32_t CO_rows, int32_t H, int32_t W, HConv3Plan& plan) {
  // tile width and the image rows of a 128 * NI pixel tile (NI = 1, 2, 4; 0 = that tile does not exist for the plane)
  int tw, rows_for_ni[5] = {0, 0, 0, 0, 0};
  if (W > 16) { tw = 32; rows_for_ni[1] = 4; rows_for_ni[2] = 8; rows_for_ni[4] = 16; }
  else if (W == 8 && H == 8) { tw = 8; rows_for_ni[1] = rows_for_ni[2] = rows_for_ni[4] = 8; }   // whole images side by side
  else if (W == 4 && H == 4) { tw = 4; rows_for_ni[1] = 4; }                                      // (32 KB of LDS per stage at NI = 2)
  else { tw = 16; rows_for_ni[1] = 8; rows_for_ni[2] = 16; if (H == 16) rows_for_ni[4] = 16; }    // (NI = 4: two whole images)
  plan.tw = tw;
  plan.bm = CO_rows > 32 ? 64 : 32;
  plan.tiles_m = (CO_rows + plan.bm - 1) / plan.bm;
  auto count = [&](int ni) {
    const int rows = rows_for_ni[ni];
    const int img = 128 * ni / (rows * tw);
    const int64_t tx = (W + tw - 1) / tw, ty = img > 1 ? 1 : (H + rows - 1) / rows, tn = (N + img - 1) / img;
    return tx * ty * tn * plan.tiles_m;
  };
  // the largest pixel tile that still gives two workgroups per CU: the weight slice of a chunk (18 KB at 64 rows) is staged once
  // per tile, and the L2 -> LDS stream, not the matrix pipe, bounds these kernels
  int ni = 1;
  if (rows_for_ni[4] && plan.bm == 64 && count(4) >= 512) ni = 4;
  else if (rows_for_ni[2] && count(2) >= 512) ni = 2;
  if (const char* forced = getenv("SRGAN_H_CONV_NI")) {          // tests: every tile shape on small tensors
    const int want = atoi(forced);
    if ((want == 1 || want == 2 || want == 4) && rows_for_ni[want] && (want != 4 || plan.bm == 64)) ni = want;
  }
  plan.ni = ni;
  plan.rows = rows_for_ni[ni];
  const int img = 128 * ni / (plan.rows * tw);
  plan.tiles_x = (W + tw - 1) / tw;
  plan.tiles_y = img > 1 ? 1 : (H + plan.rows - 1) / plan.rows;
  plan.tiles_n = (N + img - 1) / img;
  plan.blocks = count(ni);
  if (plan.blocks >= ((int64_t)1 << 31)) return false;
  const int chunks = (CGI + 1) / 2;
  int split = 1;
  if (plan.blocks < 384 && chunks >= 4 && plan.blocks <= SPLIT_TICKET_TILES) {
    split = (int)((512 + plan.blocks - 1) / plan.blocks);
    if (split > chunks / 2) split = chunks / 2;
    if (split > 16) split = 16;
  }
  plan.chunks_per = (chunks + split - 1) / split;
  plan.split = (chunks + plan.chunks_per - 1) / plan.chunks_per;
  return true;
}

template <int BM, int NI, int PREC>
static void hconv3_launch_tiles(const HConv3Params& p, int tw, dim3 grid, hipStream_t stream) {
  if constexpr (NI == 4) {
    if (tw == 32) hipLaunchKernelGGL((hconv3x3_kernel<BM, 4, 32, 16, PREC, 1>), grid, dim3(256), 0, stream, p);
    else if (tw == 16) hipLaunchKernelGGL((hconv3x3_kernel<BM, 4, 16, 16, PREC, 1>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((hconv3x3_kernel<BM, 4, 8, 8, PREC, 1>), grid, dim3(256), 0, stream, p);
  } else {
    if (tw == 32) hipLaunchKernelGGL((hconv3x3_kernel<BM, NI, 32, 4 * NI, PREC>), grid, dim3(256), 0, stream, p);
    else if (tw == 16) hipLaunchKernelGGL((hconv3x3_kernel<BM, NI, 16, 8 * NI, PREC>), grid, dim3(256), 0, stream, p);
    else if (tw == 8) hipLaunchKernelGGL((hconv3x3_kernel<BM, NI, 8, 8, PREC>), grid, dim3(256), 0, stream, p);
    else if constexpr (NI == 1) hipLaunchKernelGGL((hconv3x3_kernel<BM, 1, 4, 4, PREC>), grid, dim3(256), 0, stream, p);
  }
}

template <int PREC>
static void hconv3_launch(const HConv3Params& p, const HConv3Plan& plan, dim3 grid, hipStream_t stream) {
  if (plan.bm == 64) {
    if (plan.ni == 4) hconv3_launch_tiles<64, 4, PREC>(p, plan.tw, grid, stream);
    else if (plan.ni == 2) hconv3_launch_tiles<64, 2, PREC>(p, plan.tw, grid, stream);
    else hconv3_launch_tiles<64, 1, PREC>(p, plan.tw, grid, stream);
  } else {
    if (plan.ni == 2) hconv3_launch_tiles<32, 2, PREC>(p, plan.tw, grid, stream);
    else hconv3_launch_tiles<32, 1, PREC>(p, plan.tw, grid, stream);
  }
}

// ---- launchers of the LDS-DMA ring kernel (64-row tiles, unsplit K) -------------------------------------------------------
template <int NI, int TW, int ROWS, int PREC, int RING>
static int hconv3_dma_launch_one(const HConv3Params& p, dim3 grid, hipStream_t stream, const Slot* zero) {
  constexpr int P = 128 * NI, IMG = P / (ROWS * TW), PLANE = (ROWS + 2) * (TW + 2);
  constexpr int PATCH_I = (2 * IMG * PLANE + 63) / 64, T = PATCH_I + 18, TP = (T + 3) / 4 * 4;
  constexpr int bytes = RING * TP * 64 * 16;
  static_assert(bytes <= 160 * 1024, "the ring fits the CU's LDS");
  constexpr auto kernel = hconv3x3_dma_kernel<64, NI, TW, ROWS, PREC, RING>;
  SRGAN_HIP(allow_dynamic_lds<kernel>(bytes));
  hipLaunchKernelGGL(kernel, grid, dim3(256), bytes, stream, p, zero);
  return SRGAN_OK;
}

template <int PREC, int RING>
static int hconv3_dma_launch(const HConv3Params& p, const HConv3Plan& plan, dim3 grid, hipStream_t stream, const Slot* zero) {
  const int tw = plan.tw;
  if (plan.ni == 4) {
    if (tw == 32) return hconv3_dma_launch_one<4, 32, 16, PREC, RING>(p, grid, stream, zero);
    if (tw == 16) return hconv3_dma_launch_one<4, 16, 16, PREC, RING>(p, grid, stream, zero);
    return hconv3_dma_launch_one<4, 8, 8, PREC, RING>(p, grid, stream, zero);
  }
  if (plan.ni == 2) {
    if (tw == 32) return hconv3_dma_launch_one<2, 32, 8, PREC, RING>(p, grid, stream, zero);
    if (tw == 16) return hconv3_dma_launch_one<2, 16, 16, PREC, RING>(p, grid, stream, zero);
    return hconv3_dma_launch_one<2, 8, 8, PREC, RING>(p, grid, stream, zero);
  }
  if (tw == 32) return hconv3_dma_launch_one<1, 32, 4, PREC, RING>(p, grid, stream, zero);
  if (tw == 16) return hconv3_dma_launch_one<1, 16, 8, PREC, RING>(p, grid, stream, zero);
  if (tw == 8) return hconv3_dma_launch_one<1, 8, 8, PREC, RING>(p, grid, stream, zero);
  return hconv3_dma_launch_one<1, 4, 4, PREC, RING>(p, grid, stream, zero);
}

}  // namespace srgan

using namespace srgan;

extern "C" {

// out[N, C_out, H, W] = epi(conv3x3 / stride 1 / pad 1 of x[N, C_in, H, W] with packed weights of `rows` rows [+ bias]).
// epi 0: plain; 1: + bias (may be NULL), then leaky_relu(slope) (slope 0 = relu, 1 = identity); 2: times mask(ref, slope), ref
// of the output's shape.  C_out = the channels the output tensor stores (rows of the packed weights may be fewer or more).
int srgan_h_conv3x3(const void* x, const void* packed, const float* bias, const void* ref, float slope, int epi, void* out,
                    int32_t N, int32_t C_in, int32_t C_out, int32_t rows, int32_t H, int32_t W, int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<1, 2>(dtype, H16_ONLY)) return status;
  SRGAN_REQUIRE(x && packed && out && N > 0 && C_in > 0 && C_out > 0 && rows > 0 && H > 0 && W > 0 && epi >= 0 && epi <= 2 &&
                (epi != 2 || ref), SRGAN_EINVAL, "srgan_h_conv3x3 arguments");
  HConv3Params p;
  p.in = (const Slot*)x; p.wp = (const Slot*)packed; p.out = (Slot*)out; p.bias = bias; p.ref = (const Slot*)ref;
  p.slope = slope; p.epi = epi;
  p.N = N; p.CGI = (C_in + 7) / 8; p.CGO = (C_out + 7) / 8; p.CO = rows; p.C_real = C_out; p.H = H; p.W = W;
  p.chunks = (p.CGI + 1) / 2;
  SRGAN_REQUIRE((int64_t)N * (p.CGI > p.CGO ? p.CGI : p.CGO) * H * W < ((int64_t)1 << 31), SRGAN_ERANGE, "srgan_h_conv3x3 tensor size");
  HConv3Plan plan;
  const int rows_needed = p.CGO * 8 < rows ? p.CGO * 8 : rows;       // output rows that are stored
  SRGAN_REQUIRE(hconv3_plan(N, p.CGI, rows_needed, H, W, plan), SRGAN_EUNSUPPORTED, "srgan_h_conv3x3 plane size");
  p.tiles_x = plan.tiles_x; p.tiles_y = plan.tiles_y; p.tiles_m = plan.tiles_m;
  p.chunks_per_split = plan.chunks_per;
  p.split_ws = nullptr; p.split_tickets = nullptr;
  int split = plan.split;
  if (split > 1) {
    int ticket_set = -1;
    const int64_t accumulators = (int64_t)(plan.bm / 32) * plan.ni * 16 * 256;
    float* ws = split_workspace(plan.blocks, split, accumulators, 0, s, &ticket_set);
    unsigned int* tickets = ws ? device_tickets(g_hconv3_split_tickets) : nullptr;
    if (ws && tickets) {
      p.split_ws = ws;
      p.split_tickets = tickets + (size_t)ticket_set * SPLIT_TICKET_TILES;
    } else {
      split = 1;
      p.chunks_per_split = p.chunks;
    }
  }
  p.xcd_remap = (plan.blocks % 8 == 0 && plan.blocks >= 64) ? 1 : 0;
  const dim3 grid((unsigned)plan.blocks, (unsigned)split, 1);
  // LDS-DMA ring for 64-row tiles with an unsplit K.  SRGAN_H_DMA_RING: 0 = off (register staging), 2 / 3 = that many stages;
  // default two stages = two workgroups per CU.  Measured (profiles/r06h_*, scratch/h_conv_bench.py): three stages -- two chunks
  // in flight but ONE workgroup per CU -- lose 25-40 %; two stages equal the register-staged kernel on the wide planes and gain
  // 15-20 % on the 16 x 16 / 8 x 8 planes of the stacked pass.  With the staging switched off altogether the loop reaches
  // 950-1160 TF/s: fragment reads and matrix work, not the operand stream, are the larger part of what is left.
  static const int ring_env = getenv("SRGAN_H_DMA_RING") ? atoi(getenv("SRGAN_H_DMA_RING")) : -1;
  const int ring = ring_env >= 0 ? ring_env : 2;
  const Slot* zero = (ring == 2 || ring == 3) && split == 1 && plan.bm == 64
                         ? h_zero_slots() : nullptr;
  const int slot = profile_bracket_begin(s);
  int launched = SRGAN_OK;
  if (!for_precision<1, 2>(dtype, [&](auto prec) {
        constexpr int PREC = decltype(prec)::value;
        if (!zero) hconv3_launch<PREC>(p, plan, grid, s);
        else if (ring == 3) launched = hconv3_dma_launch<PREC, 3>(p, plan, grid, s, zero);
        else launched = hconv3_dma_launch<PREC, 2>(p, plan, grid, s, zero);
      }))
    launched = check_precision<>(dtype, "srgan_h_conv3x3 launch");
  if (launched != SRGAN_OK) {
    profile_bracket_end(slot, s, 0, 0, 0, KIND_HCONV3X3, plan.bm, plan.ni * 128, split);      // close the bracket this call opened
    return launched;
  }
  const int status = launch_status();
  const double pixels = (double)N * H * W;
  profile_bracket_end_bytes(slot, s, rows_needed, (int64_t)pixels, (int64_t)p.CGI * 8 * 9, KIND_HCONV3X3, plan.bm, plan.ni * 128, split,
                            2.0 * (pixels * p.CGI * 8 + pixels * p.CGO * 8 * (epi == 2 ? 2 : 1) + (double)rows * p.CGI * 8 * 9), dtype);
  return status;
}

}  // extern "C"
