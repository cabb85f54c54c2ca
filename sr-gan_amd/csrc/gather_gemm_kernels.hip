// gather_gemm_kernels.hip -- the MFMA contraction kernel behind every convolution / linear pass that has no kernel of its
// own, its VALU siblings for skinny shapes, their launcher (gg_run_group) and srgan_gemm.  The convolution entry points that
// route to it are in conv_dispatch.hip.
//
// One 256-thread workgroup (4 wavefronts of 64) owns a BM x BN tile of C.  Per K-step of 16 the tile's A
// (BM x 16) and B (16 x BN) slices are gathered from HBM into registers (next step's loads are issued
// before the current step's MFMAs so HBM latency hides under the matrix pipe), written to LDS as
// [k][m] / [k][n] rows padded by one word (conflict-free ds_read_b32 for the MFMA operand pattern), and
// consumed by v_mfma_f32_32x32x2_f32: exact fp32, 157 TF/s peak on gfx950.  Lanes map to C columns, so
// stores are 128-byte runs along the contiguous (pixel) dimension of NCHW.
//
// Roofline (MI355X_MICROARCH.md): fp32 MFMA 157.3 TF/s; the gather adds ~30 VALU ops per staged element,
// which overlaps with the 64-cycle MFMAs of the other waves on the SIMD.
#include "common.h"
#include "mfma.h"
#include "split_finish.h"
#include "gather_gemm.h"
#include "conv_plan.h"
#include "launchers.h"
#include <stdlib.h>
#include <type_traits>
#include <vector>

namespace srgan {

constexpr int GG_BK = 32;   // K-slice alignment of split-K chunks (the largest per-config BK)

// BK is 16 for the 128x128 and 32x256 tiles (keeps VGPR + AGPR <= 256: two workgroups per CU so that one's staging
// overlaps the other's MFMAs) and 32 for the smaller tiles (half the barriers per FLOP).
// The 16-byte staged (VEC) variants need few registers, so they take K-slices of 32: twice the MFMA work per barrier
// and per load round trip.
template <int BM, int BN, bool VEC>
struct TileBK { static constexpr int value = (BM * BN >= 128 * 128 || BN >= 256) ? 16 : 32; };

// VEC: both operands are staged with 16-byte loads along their contiguous direction (groups of 4 consecutive k or
// m/n that share one address decode): the 1x1 convolutions and linear layers, i.e. plain GEMMs on NCHW data.
// The host (vec_eligible) guarantees that every group is 16-byte aligned and entirely valid or entirely invalid.
// PREC: 0 = v_mfma_f32_32x32x2_f32 (exact fp32, 157 TF/s peak); 1 / 2 = v_mfma_f32_32x32x16_bf16 / _f16 (2.5 PF/s peak):
// lane l of a fragment holds row / column l & 31 and k = 8 * (l >> 5) .. + 7 of a 16-deep step.  The tiles in LDS are
// OPERAND-TYPED (round 3): stage() rounds the fp32 values it fetched and writes them as [row][k] with k contiguous and a
// row stride of BK + 8 elements (80 / 48 bytes: the sixteen lanes of a ds_read_b128 group hit sixteen different bank
// quads), so a fragment is ONE ds_read_b128 -- it used to be eight ds_read_b32 of fp32 values plus eight conversions per
// fragment, which kept the kernel at 66-79 TF/s in the bf16 mode, below its own fp32 rate.  Accumulation is fp32 and the
// C/D fragment layout is the same, so fetch and epilogue are shared.  The mixed-precision modes of BASELINE.json configs
// 2 and 5.
template <int BM, int BN, int WGM, bool AKF, bool BKF, bool VEC, int PREC = 0>
__global__ __launch_bounds__(256, 2) void gg_mfma_kernel(const GatherGemm p) {
  constexpr int BK = TileBK<BM, BN, VEC>::value;
  constexpr int WGN = 4 / WGM;
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int MI = WM / 32, NI = WN / 32;
  constexpr int G = VEC ? 4 : 1;                                  // elements per staged group
  constexpr int AG = BM * BK / G, BG = BN * BK / G;               // groups per tile
  constexpr int EA = (AG + 255) / 256, EB = (BG + 255) / 256;     // groups per thread
  constexpr int LDA = BM + (VEC ? 4 : 1), LDB = BN + (VEC ? 4 : 1);
  static_assert(MI >= 1 && NI >= 1, "tile too small for 4 waves");
  __shared__ __attribute__((aligned(16))) float lds[BK * LDA + BK * LDB];
  float* As = lds;
  float* Bs = lds + BK * LDA;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_m = (p.M + BM - 1) / BM;
  const int m0 = (int)(blockIdx.x % tiles_m) * BM, n0 = (int)(blockIdx.x / tiles_m) * BN;
  const int kbeg = (int)blockIdx.y * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);

  // Per-thread staging coordinates (first element of each group).  With k-fast staging consecutive lanes walk k
  // (the operand's contiguous direction), otherwise they walk m / n.
  int a_kk[EA], a_ml[EA], b_kk[EB], b_nl[EB];
  bool a_on[EA], b_on[EB];
#pragma unroll
  for (int e = 0; e < EA; ++e) {
    const int flat = e * 256 + tid;
    a_on[e] = (AG % 256 == 0) || flat < AG;
    a_kk[e] = AKF ? (flat % (BK / G)) * G : flat / (BM / (AKF ? 1 : G));
    a_ml[e] = AKF ? flat / (BK / G) : (flat % (BM / G)) * G;
  }
#pragma unroll
  for (int e = 0; e < EB; ++e) {
    const int flat = e * 256 + tid;
    b_on[e] = (BG % 256 == 0) || flat < BG;
    b_kk[e] = BKF ? (flat % (BK / G)) * G : flat / (BN / (BKF ? 1 : G));
    b_nl[e] = BKF ? flat / (BK / G) : (flat % (BN / G)) * G;
  }
  // Loop-invariant halves of the address computation.
  Side a_m[AKF ? EA : 1], b_n[BKF ? EB : 1];
#pragma unroll
  for (int e = 0; e < (AKF ? EA : 1); ++e) a_m[e] = decode(p.am, m0 + a_ml[e]);
#pragma unroll
  for (int e = 0; e < (BKF ? EB : 1); ++e) b_n[e] = decode(p.bn, n0 + b_nl[e]);

  float ra[EA][G], rb[EB][G];
  // With m/n-fast scalar staging every lane of a wavefront works on the same k (tile rows are >= 64 wide), so the
  // k-side decode (two constant divisions + affine maps) is hoisted to the scalar unit via readfirstlane; the vector
  // unit only adds the per-lane half and tests the halo.
  constexpr bool A_UNIFORM_K = !VEC && !AKF && BM >= 64;
  constexpr bool B_UNIFORM_K = !VEC && !BKF && BN >= 64;
  // Loads are unconditional (the offset of an out-of-range element is clamped to 0) and their results are NOT touched
  // until stage(): the validity bits travel separately and the zeroing happens at the LDS write.  Any use of a loaded
  // value inside fetch() makes the compiler wait for the whole slice before the MFMAs it is meant to overlap with.
  uint32_t a_ok = 0u, b_ok = 0u;
  auto load_group = [&](const float* base, uint32_t off, bool ok, float (&dst)[G]) {
    if (VEC) {
      const float4 v = *reinterpret_cast<const float4*>(base + (ok ? off : 0u));
      dst[0] = v.x; dst[G > 1 ? 1 : 0] = v.y; dst[G > 2 ? 2 : 0] = v.z; dst[G > 3 ? 3 : 0] = v.w;
      if (G == 1) dst[0] = v.x;
    } else {
      dst[0] = base[ok ? off : 0u];
    }
  };
  auto fetch = [&](int k0) {
    a_ok = 0u; b_ok = 0u;
#pragma unroll
    for (int e = 0; e < EA; ++e) {
      const int k = k0 + ((A_UNIFORM_K) ? __builtin_amdgcn_readfirstlane(a_kk[e]) : a_kk[e]);
      const Side sk = decode(p.ak, k);
      const Side sm = a_m[AKF ? e : 0];
      const bool ok = a_on[e] & sk.valid & (k < kend) & sm.valid;
      a_ok |= (ok ? 1u : 0u) << e;
      load_group(p.A, sm.off + sk.off, ok, ra[e]);
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      const int k = k0 + ((B_UNIFORM_K) ? __builtin_amdgcn_readfirstlane(b_kk[e]) : b_kk[e]);
      const Side sk = decode(p.bk, k);
      const Side sn = b_n[BKF ? e : 0];
      bool ok = b_on[e] & sk.valid & (k < kend) & sn.valid;
      if (!VEC) ok = ok & ((uint32_t)(sk.h + sn.h) < (uint32_t)p.hlim) & ((uint32_t)(sk.w + sn.w) < (uint32_t)p.wlim);
      b_ok |= (ok ? 1u : 0u) << e;
      load_group(p.B, sk.off + sn.off, ok, rb[e]);
    }
  };
  using half_t = typename std::conditional<PREC == 2, _Float16, __bf16>::type;
  typedef half_t half4_t __attribute__((ext_vector_type(4)));
  constexpr int LDK = BK + 8;                                     // PREC: elements per operand-typed LDS row
  half_t* As16 = reinterpret_cast<half_t*>(lds);
  half_t* Bs16 = As16 + BM * LDK;
  static_assert(PREC == 0 || (BM + BN) * (BK + 8) * 2 <= (BK * LDA + BK * LDB) * 4, "the typed tiles fit the fp32 allocation");
  auto stage_typed = [&](half_t* tile, const float (&v)[G], int row, int kk, bool kfast) {
    if (kfast && VEC) {
      half4_t packed;
#pragma unroll
      for (int i = 0; i < 4; ++i) packed[i] = (half_t)v[G > i ? i : 0];
      *reinterpret_cast<half4_t*>(&tile[row * LDK + kk]) = packed;      // four consecutive k of one row: 8 aligned bytes
    } else if (kfast) {
      tile[row * LDK + kk] = (half_t)v[0];
    } else {
#pragma unroll
      for (int i = 0; i < G; ++i) tile[(row + i) * LDK + kk] = (half_t)v[i];   // G consecutive rows at one k
    }
  };
  auto stage = [&]() {
    if constexpr (PREC != 0) {
#pragma unroll
      for (int e = 0; e < EA; ++e) {
        if (!a_on[e]) continue;
        const bool ok = (a_ok >> e) & 1u;
        float v[G];
#pragma unroll
        for (int i = 0; i < G; ++i) v[i] = ok ? ra[e][i] : 0.f;
        stage_typed(As16, v, a_ml[e], a_kk[e], AKF);
      }
#pragma unroll
      for (int e = 0; e < EB; ++e) {
        if (!b_on[e]) continue;
        const bool ok = (b_ok >> e) & 1u;
        float v[G];
#pragma unroll
        for (int i = 0; i < G; ++i) v[i] = ok ? rb[e][i] : 0.f;
        stage_typed(Bs16, v, b_nl[e], b_kk[e], BKF);
      }
      return;
    }
#pragma unroll
    for (int e = 0; e < EA; ++e) {
      if (!a_on[e]) continue;
      const bool ok = (a_ok >> e) & 1u;
      float v[G];
#pragma unroll
      for (int i = 0; i < G; ++i) v[i] = ok ? ra[e][i] : 0.f;
      if (VEC && !AKF) {
        *reinterpret_cast<float4*>(&As[a_kk[e] * LDA + a_ml[e]]) = make_float4(v[0], v[G > 1 ? 1 : 0], v[G > 2 ? 2 : 0],
                                                                                v[G > 3 ? 3 : 0]);
      } else {
#pragma unroll
        for (int i = 0; i < G; ++i) As[(a_kk[e] + (AKF ? i : 0)) * LDA + a_ml[e] + (AKF ? 0 : i)] = v[i];
      }
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      if (!b_on[e]) continue;
      const bool ok = (b_ok >> e) & 1u;
      float v[G];
#pragma unroll
      for (int i = 0; i < G; ++i) v[i] = ok ? rb[e][i] : 0.f;
      if (VEC && !BKF) {
        *reinterpret_cast<float4*>(&Bs[b_kk[e] * LDB + b_nl[e]]) = make_float4(v[0], v[G > 1 ? 1 : 0], v[G > 2 ? 2 : 0],
                                                                                v[G > 3 ? 3 : 0]);
      } else {
#pragma unroll
        for (int i = 0; i < G; ++i) Bs[(b_kk[e] + (BKF ? i : 0)) * LDB + b_nl[e] + (BKF ? 0 : i)] = v[i];
      }
    }
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int wm0 = (wave / WGN) * WM, wn0 = (wave % WGN) * WN;
  const int l31 = lane & 31, lhi = lane >> 5;

  if (kbeg < kend) {
    fetch(kbeg);
    stage();
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
      const bool more = k0 + BK < kend;
      if (more) fetch(k0 + BK);
      if constexpr (PREC != 0) {
        static_assert(PREC == 0 || BK % 16 == 0, "16-deep MFMA steps");
        using frag = mfma_frag<PREC>;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 16) {
          frag a[MI], b[NI];                   // one ds_read_b128 each: 8 consecutive k of this lane's row / column
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
            a[mi] = *reinterpret_cast<const frag*>(&As16[(wm0 + mi * 32 + l31) * LDK + kk + 8 * lhi]);
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            b[ni] = *reinterpret_cast<const frag*>(&Bs16[(wn0 + ni * 32 + l31) * LDK + kk + 8 * lhi]);
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = mfma32<PREC>(a[mi], b[ni], acc[mi][ni]);
        }
      } else
#pragma unroll
      for (int kk = 0; kk < BK; kk += 2) {
        float a[MI], b[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) a[mi] = As[(kk + lhi) * LDA + wm0 + mi * 32 + l31];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) b[ni] = Bs[(kk + lhi) * LDB + wn0 + ni * 32 + l31];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = mfma32(a[mi], b[ni], acc[mi][ni]);
      }
      __syncthreads();
      if (more) {
        stage();
        __syncthreads();
      }
    }
  }

  // Epilogue: C/D fragment of the 32x32 MFMA: column = lane & 31, row = mfma32_row(r, lane >> 5).
  int mode = p.mode;
  if (mode >= GG_ORDERED_STORE) {     // K split, ordered finish: the tile's last workgroup goes on with the sum of all slices
    constexpr int COUNT = MI * NI * 16;
    if (!split_finish_ordered<COUNT, 256>(p.partial + (int64_t)blockIdx.x * gridDim.y * (COUNT * 256), (int)blockIdx.y,
                                          (int)gridDim.y, p.tickets + blockIdx.x,
                                          acc_flat(acc), acc_flat(acc)))
      return;
    mode -= GG_ORDERED_STORE;
  }
  const bool add_bias = p.bias != nullptr && (blockIdx.y == 0 || p.mode >= GG_ORDERED_STORE);
  Side sn[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) sn[ni] = decode(p.cn, n0 + wn0 + ni * 32 + l31);
  // bias values in front of every store (a load behind a store waits for it: one in-order vmcnt)
  float row_bias_all[MI][16], col_bias[NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const Side sm = decode(p.cm, mfma32_row(r, lhi, m0 + wm0 + mi * 32));
      row_bias_all[mi][r] = (add_bias && !p.bias_cols && sm.valid) ? p.bias[sm.c] : 0.f;
    }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) col_bias[ni] = (add_bias && p.bias_cols && sn[ni].valid) ? p.bias[sn[ni].c] : 0.f;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      // accumulate (every weight gradient: the arena sums four backward passes): the 4 x NI old values of a register quad in
      // one batch in front of their stores -- loads and stores return through one in-order counter (vmcnt), so `*dst += v`
      // per element made every load wait for the store in front of it
      float previous[4][NI];
      if (mode == GG_ACCUMULATE) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int i = mfma32_row(4 * rq + rr, lhi, m0 + wm0 + mi * 32);
          const Side sm = decode(p.cm, i);
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            previous[rr][ni] = (sm.valid && sn[ni].valid) ? p.C[(uint32_t)(sm.off + sn[ni].off)] : 0.f;
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = 4 * rq + rr;
        const int i = mfma32_row(r, lhi, m0 + wm0 + mi * 32);
        const Side sm = decode(p.cm, i);
        if (!sm.valid) continue;
        const float row_bias = row_bias_all[mi][r];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          if (!sn[ni].valid) continue;
          const float v = (acc[mi][ni][r] + row_bias) + col_bias[ni];
          if (mode == GG_PARTIAL) {
            p.partial[((int64_t)blockIdx.y * p.M + i) * p.N + (n0 + wn0 + ni * 32 + l31)] = v;
            continue;
          }
          float* dst = p.C + (uint32_t)(sm.off + sn[ni].off);
          if (mode == GG_STORE) *dst = v;
          else if (mode == GG_ACCUMULATE) *dst = previous[rr][ni] + v;
          else unsafeAtomicAdd(dst, v);
        }
      }
    }
  }
}

// Direct form for very skinny outputs (M <= 2: single-channel map heads, count
// layers): one thread per C element, lanes along columns, A broadcast.  HBM/L2-bound, no matrix core.
__global__ __launch_bounds__(256) void gg_direct_kernel(const GatherGemm p) {
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const int i = (int)blockIdx.y;
  const int kbeg = (int)blockIdx.z * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);
  const Side am = decode(p.am, i), cm = decode(p.cm, i);
  const Side bn = decode(p.bn, j), cn = decode(p.cn, j);
  if (!cn.valid || !cm.valid) return;
  float acc = 0.f;
  for (int k = kbeg; k < kend; ++k) {
    const Side ak = decode(p.ak, k), bk = decode(p.bk, k);
    acc = fmaf(gg_a(p, am, ak), gg_b(p, bk, bn), acc);
  }
  if (p.bias != nullptr && blockIdx.z == 0) acc += p.bias[p.bias_cols ? cn.c : cm.c];
  if (p.mode == GG_PARTIAL) {
    p.partial[((int64_t)blockIdx.z * p.M + i) * p.N + j] = acc;
    return;
  }
  float* dst = p.C + (uint32_t)(cm.off + cn.off);
  if (p.mode == GG_STORE) *dst = acc;
  else if (p.mode == GG_ACCUMULATE) *dst += acc;
  else unsafeAtomicAdd(dst, acc);
}

// A few output rows (M <= MR: RGB image gradients of the stem, the generator's 3-channel output layer) over a very
// wide N: the MFMA tile would spend 29 of its 32 rows on padding (4.5 TF/s measured).  One thread per column keeps
// MR accumulators.  Everything that depends only on k -- the decoded B-side offset / coordinates and the MR values
// of A -- is tabulated in LDS once per 256-k chunk and read back as broadcasts, so each gathered B element costs one
// vector load, two LDS broadcasts and ~12 VALU instructions, branch-free.
template <int MR>
__global__ __launch_bounds__(256) void gg_rows_kernel(const GatherGemm p) {
  constexpr int KC = 256;
  __shared__ int4 ktab[KC];                  // {B offset, h, w, -} of k
  __shared__ float atab[KC * MR];            // A[i, k] for the MR rows
  const int tid = (int)threadIdx.x;
  const int j = (int)blockIdx.x * 256 + tid;
  const bool col_ok = j < p.N;
  const int jc = col_ok ? j : p.N - 1;
  const Side bn = decode(p.bn, jc), cn = decode(p.cn, jc);
  const int kbeg = (int)blockIdx.y * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);
  const bool lane_ok = col_ok && bn.valid;
  float acc[MR];
#pragma unroll
  for (int i = 0; i < MR; ++i) acc[i] = 0.f;

  for (int k0 = kbeg; k0 < kend; k0 += KC) {
    __syncthreads();
    {
      const int k = k0 + tid;
      const bool k_ok = k < kend;
      const Side bk = decode(p.bk, k_ok ? k : kbeg), ak = decode(p.ak, k_ok ? k : kbeg);
      // an invalid k gets a row coordinate that fails every bounds test
      ktab[tid] = make_int4((int)bk.off, (k_ok && bk.valid) ? bk.h : -0x40000000, bk.w, 0);
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const Side am = decode(p.am, i < p.M ? i : 0);
        const bool ok = k_ok && i < p.M && am.valid && ak.valid;
        const float v = p.A[ok ? am.off + ak.off : 0u];
        atab[tid * MR + i] = ok ? v : 0.f;
      }
    }
    __syncthreads();
    const int kc = min(KC, kend - k0);
#pragma unroll 8
    for (int kk = 0; kk < kc; ++kk) {
      const int4 t = ktab[kk];
      // bitwise, not short-circuit: no divergent branches around the table reads
      const bool ok = (int)lane_ok & (int)((uint32_t)(t.y + bn.h) < (uint32_t)p.hlim) &
                      (int)((uint32_t)(t.z + bn.w) < (uint32_t)p.wlim);
      const float v = p.B[ok ? (uint32_t)t.x + bn.off : 0u];
      const float b = ok ? v : 0.f;
#pragma unroll
      for (int i = 0; i < MR; ++i) acc[i] = fmaf(atab[kk * MR + i], b, acc[i]);
    }
  }
  if (!col_ok || !cn.valid) return;
  const bool add_bias = p.bias != nullptr && blockIdx.y == 0;
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    if (i >= p.M) break;
    const Side cm = decode(p.cm, i);
    if (!cm.valid) continue;
    float v = acc[i];
    if (add_bias) v += p.bias[p.bias_cols ? cn.c : cm.c];
    if (p.mode == GG_PARTIAL) {
      p.partial[((int64_t)blockIdx.y * p.M + i) * p.N + j] = v;
      continue;
    }
    float* dst = p.C + (uint32_t)(cm.off + cn.off);
    if (p.mode == GG_STORE) *dst = v;
    else if (p.mode == GG_ACCUMULATE) *dst += v;
    else unsafeAtomicAdd(dst, v);
  }
}

// A tiny output (M, N <= 8) over a very long K (weight gradients of the k = stride map-head transposed convolutions:
// 8 x 4 outputs, K = all pixels of the batch): lanes along K.  Every thread walks its share of k with an M x N block
// of accumulators (M + N loads, M*N FMAs per k), the workgroup reduces the 64 sums once (shuffles, then LDS) and adds
// them with M*N atomics.  The MFMA tile did this at 0.3 TF/s: 32 x 128 tiles that are 97 % padding.
__global__ __launch_bounds__(256) void gg_dot_kernel(const GatherGemm p) {
  __shared__ float red[4][64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  Side am[8], bn[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { am[i] = decode(p.am, i < p.M ? i : 0); am[i].valid = am[i].valid && i < p.M; }
#pragma unroll
  for (int j = 0; j < 8; ++j) { bn[j] = decode(p.bn, j < p.N ? j : 0); bn[j].valid = bn[j].valid && j < p.N; }
  const int stride = (int)gridDim.x * 256;
  for (int k = (int)blockIdx.x * 256 + tid; k < p.K; k += stride) {
    const Side ak = decode(p.ak, k), bk = decode(p.bk, k);
    float a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool ok = am[i].valid && ak.valid;
      const float v = p.A[ok ? am[i].off + ak.off : 0u];
      a[i] = ok ? v : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = (int)bn[j].valid & (int)bk.valid & (int)((uint32_t)(bk.h + bn[j].h) < (uint32_t)p.hlim) &
                      (int)((uint32_t)(bk.w + bn[j].w) < (uint32_t)p.wlim);
      const float v = p.B[ok ? bk.off + bn[j].off : 0u];
      b[j] = ok ? v : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
  }
  // wave reduction of each of the 64 sums, then the four waves through LDS
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = acc[i][j];
#pragma unroll
      for (int offset = 32; offset > 0; offset >>= 1) v += __shfl_xor(v, offset, 64);
      if (lane == 0) red[wave][i * 8 + j] = v;
    }
  __syncthreads();
  if (tid < 64) {
    const int i = tid >> 3, j = tid & 7;
    if (i < p.M && j < p.N) {
      const Side cm = decode(p.cm, i), cn = decode(p.cn, j);
      if (cm.valid && cn.valid) {
        float v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        if (p.bias != nullptr && blockIdx.x == 0) v += p.bias[p.bias_cols ? cn.c : cm.c];
        float* dst = p.C + (uint32_t)(cm.off + cn.off);
        if (p.mode == GG_PARTIAL) p.partial[((int64_t)blockIdx.x * p.M + i) * p.N + j] = v;
        else if (gridDim.x > 1) unsafeAtomicAdd(dst, v);
        else if (p.mode == GG_ACCUMULATE) *dst += v;
        else *dst = v;
      }
    }
  }
}

// Second stage of a split-K launch whose output is small (M*N up to a few thousand): thousands of workgroups adding into
// the same few cache lines serialise in L2 (measured: 310 us for a 20x48 output from 1024 K-slices), so the slices are
// stored to a workspace and summed here, no atomics, no pre-zeroing.  A workgroup owns 16 consecutive outputs; its 16
// slice-lanes per output walk the slices with four independent loads in flight each (a single dependent chain over 128
// slices cost 64 us of pure load latency), then 16-lane shuffle reductions.
__global__ __launch_bounds__(256) void gg_reduce_partials_kernel(const GatherGemm p, const float* __restrict__ ws) {
  const int o = (int)threadIdx.x & 15, lane_z = (int)threadIdx.x >> 4;      // 16 outputs x 16 slice-lanes
  const int64_t mn = (int64_t)p.M * p.N;
  const int64_t idx = (int64_t)blockIdx.x * 16 + o;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (idx < mn) {
    int z = lane_z;
    for (; z + 48 < p.split_k; z += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += ws[(int64_t)(z + 16 * u) * mn + idx];
    }
    for (; z < p.split_k; z += 16) acc[0] += ws[(int64_t)z * mn + idx];
  }
  float total = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  // lanes of one output are 16 apart (lane = lane_z * 16 + o): combine across lane_z within the wave, then across waves
  total += __shfl_xor(total, 16, 64);
  total += __shfl_xor(total, 32, 64);
  __shared__ float scratch[4][16];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  if (lane < 16) scratch[wave][lane] = total;
  __syncthreads();
  if (threadIdx.x >= 16 || idx >= mn) return;
  total = (scratch[0][o] + scratch[1][o]) + (scratch[2][o] + scratch[3][o]);
  const int i = (int)(idx / p.N), j = (int)(idx - (int64_t)i * p.N);
  const Side sm = decode(p.cm, i), sn = decode(p.cn, j);
  if (!sm.valid || !sn.valid) return;
  float* dst = p.C + (uint32_t)(sm.off + sn.off);
  *dst = p.mode == GG_ACCUMULATE ? *dst + total : total;
}

// The same second stage for outputs of any size (weight gradients of the strided / transposed convolutions: up to a few
// hundred thousand outputs x up to a few hundred slices): one thread per output, consecutive threads on consecutive
// outputs (coalesced over every slice), the slices added in slice order -- four loads in flight, one fixed order.
__global__ __launch_bounds__(256) void gg_reduce_partials_wide_kernel(const GatherGemm p, const float* __restrict__ ws) {
  const int64_t mn = (int64_t)p.M * p.N;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= mn) return;
  float total = ws[idx];
  int z = 1;
  for (; z + 3 < p.split_k; z += 4) {
    const float a = ws[(int64_t)z * mn + idx], b = ws[(int64_t)(z + 1) * mn + idx];
    const float c = ws[(int64_t)(z + 2) * mn + idx], d = ws[(int64_t)(z + 3) * mn + idx];
    total = (((total + a) + b) + c) + d;
  }
  for (; z < p.split_k; ++z) total += ws[(int64_t)z * mn + idx];
  const int i = (int)(idx / p.N), j = (int)(idx - (int64_t)i * p.N);
  const Side sm = decode(p.cm, i), sn = decode(p.cn, j);
  if (!sm.valid || !sn.valid) return;
  float* dst = p.C + (uint32_t)(sm.off + sn.off);
  *dst = p.mode == GG_ACCUMULATE ? *dst + total : total;
}

__device__ unsigned int g_gg_split_tickets[SPLIT_TICKET_SETS * SPLIT_TICKET_TILES];

// ------------------------------------------------------------------------------------------- launcher
// (GGConfig, gg_prepare and gg_launch are private to this file: other translation units go through gg_run_group)
namespace { struct GGConfig { LaunchKind kind; int bm, bn; int tiles; }; }   // kind: one of the four KIND_GG_*
constexpr int GG_TILE_TARGET = 1024;      // workgroups a launch aims for (4 per CU): choose_config's tile, choose_split's K split

static GGConfig choose_config(const GatherGemm& p, int force) {
  GGConfig c;
  // M <= 2 (single-channel map heads, count layers): the direct form; from 3 rows up (RGB image gradients, generator
  // output) the MFMA tile wins even at 3/32 row utilisation because the direct form is VALU/latency bound.
  if ((p.M <= 2 && force != 2) || force == 1) {
    c.kind = KIND_GG_DIRECT; c.bm = 1; c.bn = 256;
    c.tiles = p.M * ((p.N + 255) / 256);
    return c;
  }
  if (force == 0 && p.M <= 8 && p.N <= 8 && p.K >= 65536) {     // lanes along K
    c.kind = KIND_GG_DOT; c.bm = 8; c.bn = 8;
    c.tiles = 1;
    return c;
  }
  if (force == 0 && p.M <= 8 && p.N >= 4096) {     // the few-rows kernel
    c.kind = KIND_GG_ROWS; c.bm = p.M <= 4 ? 4 : 8; c.bn = 256;
    c.tiles = (p.N + 255) / 256;
    return c;
  }
  c.kind = KIND_GG_MFMA;
  // Largest tile that still yields >= target workgroups (4 per CU: staging of one hides under the MFMAs of the
  // others); otherwise the smallest tile of the class, topped up by split-K in choose_split.
  static const int candidates[3][3][2] = {{{128, 128}, {128, 64}, {64, 64}},     // M > 64
                                          {{64, 128}, {64, 64}, {64, 64}},        // 32 < M <= 64
                                          {{32, 256}, {32, 128}, {32, 128}}};     // M <= 32
  const int cls = p.M > 64 ? 0 : (p.M > 32 ? 1 : 2);
  // Long-K problems (weight gradients: K = pixels) get their parallelism from split-K anyway, so they take the
  // largest tile: at 64 x 64 the operand stream (16 FLOP/B) is HBM-bound at ~80 TF/s.
  if (p.K >= 131072 && p.M >= 96 && p.N >= 96) {
    c.bm = 128; c.bn = 128;
    c.tiles = ((p.M + 127) / 128) * ((p.N + 127) / 128);
    return c;
  }
  for (int i = 0; i < 3; ++i) {
    c.bm = candidates[cls][i][0];
    c.bn = candidates[cls][i][1];
    c.tiles = ((p.M + c.bm - 1) / c.bm) * ((p.N + c.bn - 1) / c.bn);
    if (c.tiles >= GG_TILE_TARGET) break;
  }
  return c;
}

static void choose_split(GatherGemm& p, const GGConfig& c, bool allow_split) {
  p.split_k = 1;
  p.k_per_split = p.K > 0 ? ((p.K + GG_BK - 1) / GG_BK) * GG_BK : GG_BK;
  constexpr int target = GG_TILE_TARGET;
  if (!allow_split || p.K < 128 || c.tiles * 4 >= target * 3) return;
  const int want = (target + c.tiles - 1) / c.tiles;
  const int max_split = p.K / 64;
  int split = want < max_split ? want : max_split;
  if (split <= 1) return;
  int per = (p.K + split - 1) / split;
  per = ((per + GG_BK - 1) / GG_BK) * GG_BK;
  p.k_per_split = per;
  p.split_k = (p.K + per - 1) / per;
}

// The staging orders of one tile and operand type: lanes along k or along m / n, per operand.
template <int BM, int BN, int WGM, bool VEC, int PREC>
static void launch_mfma_staged(const GatherGemm& p, dim3 grid, hipStream_t stream) {
  if (p.a_kfast && p.b_kfast) hipLaunchKernelGGL((gg_mfma_kernel<BM, BN, WGM, true, true, VEC, PREC>), grid, dim3(256), 0, stream, p);
  else if (p.a_kfast) hipLaunchKernelGGL((gg_mfma_kernel<BM, BN, WGM, true, false, VEC, PREC>), grid, dim3(256), 0, stream, p);
  else if (p.b_kfast) hipLaunchKernelGGL((gg_mfma_kernel<BM, BN, WGM, false, true, VEC, PREC>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((gg_mfma_kernel<BM, BN, WGM, false, false, VEC, PREC>), grid, dim3(256), 0, stream, p);
}

// Can a Dec3 be walked in aligned groups of 4 consecutive indices with unit element stride?
static bool dec_vec_fast(const Dec3& d) {
  const int32_t B = (int32_t)d.div_b.d, A = (int32_t)(d.div_ab.d / d.div_b.d);
  if (d.limit % 4 || d.off0 % 4) return false;
  if (B > 1) return d.off_b == 1 && B % 4 == 0 && d.off_a % 4 == 0 && d.off_c % 4 == 0;
  if (A > 1) return d.off_a == 1 && A % 4 == 0 && d.off_c % 4 == 0;
  return d.off_c == 1;
}

static bool dec_vec_slow(const Dec3& d) {
  const int32_t B = (int32_t)d.div_b.d, A = (int32_t)(d.div_ab.d / d.div_b.d);
  // strides of extent-1 components are never applied
  return d.off_c % 4 == 0 && (A == 1 || d.off_a % 4 == 0) && (B == 1 || d.off_b % 4 == 0) && d.off0 % 4 == 0;
}

// Both operands 16-byte stageable (1x1 convolutions / linear layers on contiguous data, no halo).
static bool vec_eligible(const GatherGemm& p) {
  if (p.hlim != 1 || p.wlim != 1) return false;
  if (((uintptr_t)p.A | (uintptr_t)p.B) & 15) return false;
  const bool a = p.a_kfast ? (dec_vec_fast(p.ak) && dec_vec_slow(p.am)) : (dec_vec_fast(p.am) && dec_vec_slow(p.ak));
  const bool b = p.b_kfast ? (dec_vec_fast(p.bk) && dec_vec_slow(p.bn)) : (dec_vec_fast(p.bn) && dec_vec_slow(p.bk));
  return a && b && p.K % 4 == 0;
}

template <int BM, int BN, int WGM>
static void launch_mfma(const GatherGemm& p, dim3 grid, hipStream_t stream) {
  if (p.precision == 1) launch_mfma_staged<BM, BN, WGM, false, 1>(p, grid, stream);        // (scalar staging only)
  else if (p.precision == 2) launch_mfma_staged<BM, BN, WGM, false, 2>(p, grid, stream);
  else if (vec_eligible(p)) launch_mfma_staged<BM, BN, WGM, true, 0>(p, grid, stream);
  else launch_mfma_staged<BM, BN, WGM, false, 0>(p, grid, stream);
}

// The launch's accumulators per workgroup for the ordered finish (see gg_mfma_kernel: MI x NI fragments of 16 per lane).
static int64_t mfma_tile_floats(const GGConfig& c) { return (int64_t)c.bm * c.bn; }

// Plans one launch: fills split_k / k_per_split and how its K slices are combined (p.use_partial, a SplitCombine); returns
// whether the launch needs a zeroed (or live) C because it combines them with fp32 atomics -- only when the stream has
// no workspace (or SRGAN_ATOMIC_SPLIT=1): otherwise the slices meet in a fixed order, through the workspace.
static bool gg_prepare(GatherGemm& p, int force, GGConfig* out, hipStream_t stream) {
  p.tickets = nullptr;
  GGConfig c = choose_config(p, force);
  if (c.kind == KIND_GG_DOT) {             // workgroups of 256 k-lanes, ~16 k per thread
    int groups = (p.K + 4095) / 4096;
    if (groups > 1024) groups = 1024;
    p.split_k = groups; p.k_per_split = p.K;
  } else {
    choose_split(p, c, true);
  }
  if (out) *out = c;
  p.use_partial = GG_COMBINE_ATOMIC;
  if (p.split_k <= 1) return false;
  const int64_t mn = (int64_t)p.M * p.N;
  const bool fits = (size_t)mn * p.split_k * sizeof(float) <= workspace_capacity();
  // (up to 4096 outputs: at 960 outputs x 1024 slices the atomics still serialised -- 310 us for 36 MB of operands)
  if (c.kind == KIND_GG_MFMA && p.split_k >= 16 && mn <= 4096 && fits) {
    p.use_partial = GG_COMBINE_PARTIAL_TINY;
    return false;
  }
  const bool have_workspace = !split_atomics_forced() && partial_workspace(1, stream) != nullptr;
  if (have_workspace) {
    // few slices of an MFMA launch: the tile's last workgroup adds them (one launch); many slices, or the VALU kernels:
    // partial outputs + a second kernel that adds the slices of every output in slice order
    int set = -1;
    if (c.kind == KIND_GG_MFMA && p.split_k <= 16 &&
        split_workspace(c.tiles, p.split_k, mfma_tile_floats(c), 0, stream, &set) != nullptr) {
      p.use_partial = GG_COMBINE_ORDERED;
      return false;
    }
    if (fits) {
      p.use_partial = (c.kind == KIND_GG_MFMA && mn <= 4096) ? GG_COMBINE_PARTIAL_TINY : GG_COMBINE_PARTIAL_WIDE;
      return false;
    }
  }
  return true;
}

static int gg_launch_unprofiled(const GatherGemm& p, const GGConfig& c, hipStream_t stream) {
  if (p.M <= 0 || p.N <= 0) return SRGAN_OK;
  if (p.split_k > 1 && (p.use_partial == GG_COMBINE_PARTIAL_TINY || p.use_partial == GG_COMBINE_PARTIAL_WIDE)) {
    // every slice stores its partial output to the workspace, a second kernel adds the slices in slice order
    SRGAN_REQUIRE(p.mode == GG_STORE || p.mode == GG_ACCUMULATE, SRGAN_EINVAL, "partial-sum launch mode");
    const int64_t mn = (int64_t)p.M * p.N;
    float* ws = partial_workspace((size_t)mn * p.split_k * sizeof(float), stream);
    SRGAN_REQUIRE(ws != nullptr, SRGAN_EINVAL,
                  "split-K workspace: call srgan_set_workspace(ptr, >= srgan_workspace_bytes(), stream) for this stream first");
    GatherGemm q = p;
    q.mode = GG_PARTIAL; q.partial = ws; q.use_partial = GG_COMBINE_ATOMIC;
    const int status = gg_launch_unprofiled(q, c, stream);
    if (status != SRGAN_OK) return status;
    if (p.use_partial == GG_COMBINE_PARTIAL_TINY)
      hipLaunchKernelGGL(gg_reduce_partials_kernel, dim3((unsigned)((mn + 15) / 16)), dim3(256), 0, stream, p, ws);
    else
      hipLaunchKernelGGL(gg_reduce_partials_wide_kernel, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, stream, p, ws);
    return launch_status();
  }
  if (p.split_k > 1 && p.use_partial == GG_COMBINE_ORDERED) {
    SRGAN_REQUIRE(c.kind == KIND_GG_MFMA && (p.mode == GG_STORE || p.mode == GG_ACCUMULATE), SRGAN_EINVAL, "ordered split launch mode");
    int set = -1;
    float* ws = split_workspace(c.tiles, p.split_k, mfma_tile_floats(c), 0, stream, &set);
    unsigned int* tickets = ws ? device_tickets(g_gg_split_tickets) : nullptr;
    SRGAN_REQUIRE(ws != nullptr && tickets != nullptr, SRGAN_EINVAL, "ordered split-K: the stream's workspace went away");
    GatherGemm q = p;
    q.mode = p.mode == GG_ACCUMULATE ? GG_ORDERED_ACCUMULATE : GG_ORDERED_STORE;
    q.partial = ws; q.tickets = tickets + (size_t)set * SPLIT_TICKET_TILES; q.use_partial = GG_COMBINE_ATOMIC;
    return gg_launch_unprofiled(q, c, stream);
  }
  if (c.kind == KIND_GG_DIRECT) {
    dim3 grid((p.N + 255) / 256, p.M, p.split_k);
    SRGAN_REQUIRE(p.M <= 65535 && p.split_k <= 65535, SRGAN_ERANGE, "direct gather-gemm grid");
    hipLaunchKernelGGL(gg_direct_kernel, grid, dim3(256), 0, stream, p);
    return launch_status();
  }
  dim3 grid(c.tiles, p.split_k, 1);
  SRGAN_REQUIRE(p.split_k <= 65535, SRGAN_ERANGE, "split-k grid");
  if (c.kind == KIND_GG_DOT) {
    hipLaunchKernelGGL(gg_dot_kernel, dim3(p.split_k), dim3(256), 0, stream, p);
    return launch_status();
  }
  if (c.kind == KIND_GG_ROWS) {
    if (c.bm == 4) hipLaunchKernelGGL(gg_rows_kernel<4>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(gg_rows_kernel<8>, grid, dim3(256), 0, stream, p);
    return launch_status();
  }
  if (c.bm == 128 && c.bn == 128) launch_mfma<128, 128, 2>(p, grid, stream);
  else if (c.bm == 128 && c.bn == 64) launch_mfma<128, 64, 2>(p, grid, stream);
  else if (c.bm == 64 && c.bn == 128) launch_mfma<64, 128, 2>(p, grid, stream);
  else if (c.bm == 64 && c.bn == 64) launch_mfma<64, 64, 2>(p, grid, stream);
  else if (c.bm == 32 && c.bn == 256) launch_mfma<32, 256, 1>(p, grid, stream);
  else launch_mfma<32, 128, 1>(p, grid, stream);
  return launch_status();
}

static int gg_launch(const GatherGemm& p, const GGConfig& c, hipStream_t stream) {
  if (p.M <= 0 || p.N <= 0) return SRGAN_OK;
  const int slot = profile_bracket_begin(stream);
  const int status = gg_launch_unprofiled(p, c, stream);
  profile_bracket_end(slot, stream, p.M, p.N, p.K, c.kind, c.bm, c.bn, p.split_k, p.a_kfast, p.b_kfast, p.b_unique,
                      c.kind == KIND_GG_MFMA ? p.precision : 0);
  return status;
}

// Runs a group of plans that together define one output tensor (launchers.h): c_rows rows of c_width floats, c_pitch apart.
int gg_run_group(std::vector<GatherGemm>& plans, float* c_base, int64_t c_pitch, int64_t c_width, int64_t c_rows, int accumulate,
                 int force, hipStream_t stream) {
  std::vector<GGConfig> configs(plans.size());
  bool any_atomic = false;
  for (size_t i = 0; i < plans.size(); ++i) any_atomic |= gg_prepare(plans[i], force, &configs[i], stream);
  if (any_atomic && !accumulate) {          // (a strided view -- a channel slice of a wider buffer -- is zeroed row by row)
    const int status = c_pitch == c_width ? zero_floats(c_base, c_width * c_rows, stream)
                                          : zero_rows(c_base, c_pitch, c_width, c_rows, stream);
    if (status != SRGAN_OK) return status;
  }
  for (size_t i = 0; i < plans.size(); ++i) {
    GatherGemm& p = plans[i];
    if (p.split_k > 1 && p.use_partial == GG_COMBINE_ATOMIC) p.mode = GG_ATOMIC;
    else p.mode = accumulate ? GG_ACCUMULATE : GG_STORE;
    const int status = gg_launch(p, configs[i], stream);
    if (status != SRGAN_OK) return status;
  }
  return SRGAN_OK;
}

}  // namespace srgan

// ------------------------------------------------------------------------------------------- C ABI
using namespace srgan;

extern "C" {

int srgan_gemm_f32(int32_t M, int32_t N, int32_t K, const float* A, int64_t sai, int64_t sak, const float* B,
                   int64_t sbk, int64_t sbj, float* C, int64_t sci, int64_t scj, const float* bias,
                   int32_t bias_on_columns, int accumulate, int force_kernel, void* stream) {
  return srgan_gemm(M, N, K, A, sai, sak, B, sbk, sbj, C, sci, scj, bias, bias_on_columns, accumulate, force_kernel, 0, stream);
}

int srgan_gemm(int32_t M, int32_t N, int32_t K, const float* A, int64_t sai, int64_t sak, const float* B,
               int64_t sbk, int64_t sbj, float* C, int64_t sci, int64_t scj, const float* bias,
               int32_t bias_on_columns, int accumulate, int force_kernel, int compute_dtype, void* stream) {
  SRGAN_REQUIRE(M > 0 && N > 0 && K >= 0 && A && B && C, SRGAN_EINVAL, "srgan_gemm_f32 arguments");
  SRGAN_REQUIRE(compute_dtype >= 0 && compute_dtype <= 2, SRGAN_EINVAL, "srgan_gemm compute_dtype");
  if (compute_dtype) force_kernel = 2;
  const int64_t lim = (int64_t)1 << 31;
  SRGAN_REQUIRE(M * sai + K * sak < lim && K * sbk + N * sbj < lim && M * sci + N * scj < lim, SRGAN_ERANGE,
                "srgan_gemm_f32 extents");
  // C must be a dense M x N matrix in one of the two orientations so that it can be zeroed for split-K.
  SRGAN_REQUIRE((scj == 1 && sci == N) || (sci == 1 && scj == M), SRGAN_EUNSUPPORTED, "srgan_gemm_f32 dense C");
  GatherGemm p = plan_gemm(M, N, K, A, (int32_t)sai, (int32_t)sak, B, (int32_t)sbk, (int32_t)sbj, C, (int32_t)sci,
                           (int32_t)scj, bias, bias_on_columns);
  if (sci == 1 && scj != 1) {   // make the lane dimension the contiguous one
    p = gg_transposed(p);
    choose_staging(p);
  }
  p.precision = compute_dtype;
  std::vector<GatherGemm> plans{p};
  return gg_run_group(plans, C, (int64_t)M * N, (int64_t)M * N, 1, accumulate, force_kernel, (hipStream_t)stream);
}

}  // extern "C"
