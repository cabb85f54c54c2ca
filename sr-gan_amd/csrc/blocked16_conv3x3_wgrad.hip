// blocked16_conv3x3_wgrad.hip -- the weight gradient of the 3x3 / stride 1 / pad 1 convolution of the 16-bit data path
// (VGG-16's convolution stack, reference age/vgg.py:28-53,70-84; the forward and the data gradient are blocked16_conv3x3.hip).
// The gradient is fp32 in the master weights' own order [CO][CI][3][3] and accumulates (+=): Adam and the masters stay fp32.
//
//   hwgrad3x3_kernel          gw += gy (x) x over pixels, all nine taps: ds_read_b64_tr_b16 operands, partial blocks per walker
//   hwgrad3x3_finish_kernel   the partial blocks added in walker order into gw (bit-reproducible)
#include <type_traits>
#include "blocked16.h"
#include "launchers.h"
#include "split_finish.h"

namespace srgan {

//   gw[co, ci, kh, kw] +=sum_{n, y, x} gy[n, co, y, x] * x[n, ci, y + kh - 1, x + kw - 1]        (fp32, [CO][CI][3][3])
// M = co, N = ci, K = pixels: both operands are reduced over the pixel index, which the blocked layout does NOT keep
// contiguous per channel -- the fragments come from LDS through ds_read_b64_tr_b16 (blocked16.h).  A workgroup (4 waves) owns
// a 64 x 64 (co x ci) block of gw for ALL nine taps: wave (mi, ni) keeps nine 32 x 32 accumulators (144 registers) while the
// workgroup walks its share of the 64-pixel tiles; per tile the gy slots [8 groups][64 pixels] and the x halo patch
// [8 groups][IMG][(ROWS + 2) x (TW + 2)] are staged once (register-staged, one LDS stage) and all nine taps read them: per
// 16-pixel step one A fragment and nine shifted B fragments, two transpose reads each.  The walkers of a block leave their
// accumulators in the caller's workspace in thread order; hwgrad3x3_finish_kernel adds them in walker order into gw.
struct HWgrad3Params {
  const Slot* x; const Slot* gy; float* partial;
  int32_t N, CGX, CGY, H, W;
  int32_t tiles_ci, tiles_x, tiles_y, tiles_n, pixel_tiles, walkers;
};

constexpr int HWGRAD_P = 64;      // pixels per staged tile (128 needs 44+ staging registers next to the 144 accumulators: spills)
constexpr int h_pad_stride(int slots) { return ((slots + 15) / 16) * 16 + 4; }     // = 4 slots (mod 16): the two groups of a
                                                                                  // transpose read land 64 bytes apart
// MB = 32-row blocks of output channels per workgroup: 2 (64 x 64 block, 4 waves, two workgroups per CU) or 4 (128 x 64 block,
// 8 waves = two per SIMD in one workgroup: the x patch, two thirds of the staged bytes, is then shared by twice the matrix work).
template <int TW, int ROWS, int PREC, int MB>
__global__ __launch_bounds__(128 * MB, 2) void hwgrad3x3_kernel(const HWgrad3Params p) {
  constexpr int THREADS = 128 * MB;
  constexpr int P = HWGRAD_P, IMG = P / (ROWS * TW), PW = TW + 2, PH = ROWS + 2, PLANE = PH * PW;
  static_assert(IMG * ROWS * TW == P && IMG >= 1, "the pixel tile is IMG x ROWS x TW");
  constexpr int GS = h_pad_stride(P), XS = h_pad_stride(IMG * PLANE);       // group strides of the two LDS images (slots)
  constexpr int GQ = 4 * MB * P, XQ = 8 * IMG * PLANE;                      // slots staged per tile
  constexpr int NG = GQ / THREADS, NX = (XQ + THREADS - 1) / THREADS;
  __shared__ Slot lds[4 * MB * GS + 8 * XS];
  Slot* gs = lds;
  Slot* xs = lds + 4 * MB * GS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mi = wave >> 1, ni = wave & 1;
  const int tci = (int)blockIdx.x % p.tiles_ci, tco = (int)blockIdx.x / p.tiles_ci;
  const int walker = (int)blockIdx.y;
  const int HW = p.H * p.W;

  // staging ownership: gy slot e * THREADS + tid -> (group, tile pixel); x slot -> (group, image, patch position); the index
  // arithmetic (compile-time divisors) is redone where it is used instead of being kept in registers
  Slot rg[NG], rx[NX];
  uint32_t okg = 0, okx = 0;
  auto fetch = [&](int tile) {
    const int tx = tile % p.tiles_x;
    const int rest_t = tile / p.tiles_x;
    const int ty = rest_t % p.tiles_y;
    const int n0 = (rest_t / p.tiles_y) * IMG;
    const int y0 = ty * ROWS, x0 = tx * TW;
    okg = okx = 0;
#pragma unroll
    for (int e = 0; e < NG; ++e) {
      const int flat = e * THREADS + tid;
      const int grp = flat / P, q = flat % P;
      const int n = n0 + q / (ROWS * TW), y = y0 + (q / TW) % ROWS, x = x0 + q % TW;
      const int group = tco * (4 * MB) + grp;
      const bool ok = n < p.N && y < p.H && x < p.W && group < p.CGY;
      okg |= (ok ? 1u : 0u) << e;
      rg[e] = p.gy[ok ? ((int64_t)n * p.CGY + group) * HW + y * p.W + x : 0];
    }
#pragma unroll
    for (int e = 0; e < NX; ++e) {
      const int flat = e * THREADS + tid;
      const int grp = flat / (IMG * PLANE), rest = flat - grp * (IMG * PLANE);
      const int img = rest / PLANE, pix = rest % PLANE;
      const int n = n0 + img, y = y0 - 1 + pix / PW, x = x0 - 1 + pix % PW;
      const int group = tci * 8 + grp;
      const bool ok = flat < XQ && n < p.N && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W && group < p.CGX;
      okx |= (ok ? 1u : 0u) << e;
      rx[e] = p.x[ok ? ((int64_t)n * p.CGX + group) * HW + y * p.W + x : 0];
    }
  };

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // Fragment addressing (blocked16.h, h_tr_read): 16-lane group G = lane >> 4: row block rb = G & 1 (channels 16 rb .. of the
  // wave's 32), k half = G >> 1 (pixels 8 khalf .. of the 16-pixel step); within the group lane s = 4 j + u supplies pixel j
  // of its quad, channels 4 u .. 4 u + 3.
  const int G = lane >> 4, rb = G & 1, khalf = G >> 1, s = lane & 15, j = s >> 2, u = s & 3;
  constexpr int HALF = TW >= 16 ? 8 : (TW == 8 ? PW : 2 * PW);     // patch offset of pixel 8 of a 16-pixel step
  constexpr int QUAD = TW >= 8 ? 4 : PW;                           // ... of the second quad of a half
  const uint32_t a_base = h_lds_address(gs) + (uint32_t)(((4 * mi + 2 * rb + (u >> 1)) * GS + 8 * khalf + j) * 16 + (u & 1) * 8);
  const uint32_t b_base = h_lds_address(xs) + (uint32_t)(((4 * ni + 2 * rb + (u >> 1)) * XS + khalf * HALF + j) * 16 + (u & 1) * 8);

  // a wave whose 32 x 32 block lies entirely beyond the channels that exist (3 input channels: conv1_1) only helps staging
  const bool active = (tco * (32 * MB) + mi * 32) < p.CGY * 8 && (tci * 64 + ni * 32) < p.CGX * 8;
  int tile = walker;
  if (tile < p.pixel_tiles) fetch(tile);
  for (; tile < p.pixel_tiles; tile += p.walkers) {
    __syncthreads();                        // the previous tile's reads are done
#pragma unroll
    for (int e = 0; e < NG; ++e) {
      const int flat = e * THREADS + tid;
      Slot v = rg[e];
      if (!((okg >> e) & 1u)) v = Slot{{0u, 0u, 0u, 0u}};
      gs[(flat / P) * GS + flat % P] = v;
    }
#pragma unroll
    for (int e = 0; e < NX; ++e) {
      const int flat = e * THREADS + tid;
      const int grp = flat / (IMG * PLANE), rest = flat - grp * (IMG * PLANE);
      Slot v = rx[e];
      if (!((okx >> e) & 1u)) v = Slot{{0u, 0u, 0u, 0u}};
      if (flat < XQ) xs[grp * XS + rest] = v;
    }
    __syncthreads();
    const int next = tile + p.walkers;
    if (next < p.pixel_tiles) fetch(next);
    if (active)
#pragma unroll 2
    for (int t = 0; t < P / 16; ++t) {       // (not fully unrolled: the scheduler otherwise hoists the transpose reads of many steps and spills)
      const int pix = 16 * t;                                                        // first pixel of the step (tile order)
      const int origin = ((pix / (ROWS * TW)) * PH + (pix / TW) % ROWS) * PW + pix % TW;   // its window origin in the patch
      Slot a;
      const uint2 a0 = h_tr_read(a_base + pix * 16), a1 = h_tr_read(a_base + (pix + 4) * 16);
      a.v[0] = a0.x; a.v[1] = a0.y; a.v[2] = a1.x; a.v[3] = a1.y;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int shift = origin + (tap / 3) * PW + tap % 3;
        Slot b;
        const uint2 b0 = h_tr_read(b_base + shift * 16), b1 = h_tr_read(b_base + (shift + QUAD) * 16);
        b.v[0] = b0.x; b.v[1] = b0.y; b.v[2] = b1.x; b.v[3] = b1.y;
        acc[tap] = h_mfma<PREC>(a, b, acc[tap]);
      }
    }
  }

  float* mine = p.partial + ((int64_t)blockIdx.x * p.walkers + walker) * (9 * 16 * THREADS) + tid;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[(t * 16 + r) * THREADS] = acc[t][r];
}

// gw[co][ci][tap] += sum over the walkers of the block's partial accumulators, in a FIXED order.  One workgroup per (block,
// output channel): the 64 input channels x 9 taps of that row are 576 consecutive floats of gw.  Lane l of every wave reads
// input channel l of each tap -- two 128-byte runs of the partial block per (walker, tap), whole lines: the first version gave a
// workgroup 64 consecutive gw elements = 7 of a line's 32 floats and fetched every line 4.5 times (18 GB per step, PMC
// profiles/r06f) -- the four waves add the walkers w = wave, wave + 4, ... and the four sums meet as (0 + 1) + (2 + 3); the
// row leaves through LDS in gw's own order.  The read index undoes the accumulator layout: wave = (co' / 32) * 2 + ci' / 32,
// C/D row co' % 32 = mfma32_row(r, lane >> 5), column ci' % 32 = lane & 31.
__global__ __launch_bounds__(256) void hwgrad3x3_finish_kernel(const float* __restrict__ partial, float* __restrict__ gw,
                                                               int32_t CO, int32_t CI, int32_t tiles_ci, int32_t walkers,
                                                               int32_t block_rows) {
  __shared__ float sums[4][9][64];
  const int lane = (int)threadIdx.x & 63, part = (int)threadIdx.x >> 6;
  const int block = (int)blockIdx.x / block_rows, row = (int)blockIdx.x % block_rows;
  const int tco = block / tiles_ci, tci = block % tiles_ci;
  const int co = tco * block_rows + row;
  if (co >= CO) return;
  const int threads = 4 * block_rows;
  const int64_t per_walker = (int64_t)9 * 16 * threads;              // accumulators of one workgroup
  const int r32 = row & 31, lhi = mfma32_half(r32), r = mfma32_register(r32);
  const int thread = ((row >> 5) * 2 + (lane >> 5)) * 64 + lhi * 32 + (lane & 31);
  const float* base = partial + (int64_t)block * walkers * per_walker + r * threads + thread;
  float total[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) total[t] = 0.f;
  // four walkers' loads in flight per wave, added in walker order (the sum is the one-at-a-time loop's, bit for bit): the
  // single-block layers have 512 walkers = 128 dependent round trips per wave
  for (int w0 = part; w0 < walkers; w0 += 16) {
    float v[4][9];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int w = w0 + 4 * d;
#pragma unroll
      for (int t = 0; t < 9; ++t) v[d][t] = w < walkers ? base[(int64_t)w * per_walker + t * 16 * threads] : 0.f;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (w0 + 4 * d < walkers)
#pragma unroll
        for (int t = 0; t < 9; ++t) total[t] += v[d][t];
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) sums[part][t][lane] = total[t];
  __syncthreads();
  float previous[3];                        // read all, then write all (loads wait for the stores in front of them: one vmcnt)
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int i = (int)threadIdx.x + 256 * e, ci_local = i / 9, tap = i - ci_local * 9, ci = tci * 64 + ci_local;
    previous[e] = (i < 576 && ci < CI) ? gw[((int64_t)co * CI + ci) * 9 + tap] : 0.f;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int i = (int)threadIdx.x + 256 * e, ci_local = i / 9, tap = i - ci_local * 9, ci = tci * 64 + ci_local;
    if (i < 576 && ci < CI)
      gw[((int64_t)co * CI + ci) * 9 + tap] = previous[e] + ((sums[0][tap][ci_local] + sums[1][tap][ci_local]) + (sums[2][tap][ci_local] + sums[3][tap][ci_local]));
  }
}

template <int TW, int ROWS, int PREC>
static void hwgrad3_launch(const HWgrad3Params& p, int mb, dim3 grid, hipStream_t stream) {
  if (mb == 4) hipLaunchKernelGGL((hwgrad3x3_kernel<TW, ROWS, PREC, 4>), grid, dim3(512), 0, stream, p);
  else hipLaunchKernelGGL((hwgrad3x3_kernel<TW, ROWS, PREC, 2>), grid, dim3(256), 0, stream, p);
}

}  // namespace srgan

using namespace srgan;

extern "C" {

// gw[C_out][C_in][3][3] (fp32) += the weight gradient of a 3x3 / s1 / p1 convolution from x[N, C_in, H, W] and gy[N, C_out, H, W]
int srgan_h_conv3x3_wgrad(const void* x, const void* gy, float* gw, int32_t N, int32_t C_in, int32_t C_out, int32_t H, int32_t W,
                          int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<1, 2>(dtype, H16_ONLY)) return status;
  SRGAN_REQUIRE(x && gy && gw && N > 0 && C_in > 0 && C_out > 0 && H > 0 && W > 0, SRGAN_EINVAL, "srgan_h_conv3x3_wgrad arguments");
  HWgrad3Params p;
  p.x = (const Slot*)x; p.gy = (const Slot*)gy;
  p.N = N; p.CGX = (C_in + 7) / 8; p.CGY = (C_out + 7) / 8; p.H = H; p.W = W;
  int tw, rows;
  if (W > 16) { tw = 32; rows = 2; }
  else if (W == 8 && H == 8) { tw = 8; rows = 8; }
  else if (W == 4 && H == 4) { tw = 4; rows = 4; }
  else { tw = 16; rows = 4; }
  const int img = HWGRAD_P / (rows * tw);
  p.tiles_x = (W + tw - 1) / tw;
  p.tiles_y = img > 1 ? 1 : (H + rows - 1) / rows;
  p.tiles_n = (N + img - 1) / img;
  p.pixel_tiles = p.tiles_x * p.tiles_y * p.tiles_n;
  p.tiles_ci = (C_in + 63) / 64;
  const int mb = C_out >= 128 ? 4 : 2;                // 128- or 64-row blocks of gw
  const int tiles_co = (C_out + 32 * mb - 1) / (32 * mb);
  const int blocks = p.tiles_ci * tiles_co;
  // Walkers per block: enough workgroups to occupy the chip, but every walker leaves its accumulators (147 / 295 KB) as a partial
  // block that the finish reads back -- 1024 / blocks walkers made that traffic (and the finish's serial walker loop) the larger
  // part of the launch on both ends of VGG (1 block x 1024 walkers; 64 blocks x 16 walkers: 151 MB each, profiles/r06b_*).
  // (64-row blocks run two workgroups per CU: where a walker still gets a long run of tiles -- the 64-channel layers on 64 x 64
  // planes: one block, 8192+ tiles -- all 512 slots are filled; elsewhere 320, for the partial traffic)
  const int target = mb == 4 ? 256 : ((int64_t)p.pixel_tiles >= (int64_t)16 * 512 * blocks ? 512 : 320);
  int walkers = (target + blocks - 1) / blocks;
  if (walkers > p.pixel_tiles) walkers = p.pixel_tiles;
  if (walkers < 1) walkers = 1;
  p.walkers = walkers;
  const int threads = 128 * mb;
  p.partial = partial_workspace((size_t)blocks * walkers * 9 * 16 * threads * sizeof(float), s);
  SRGAN_REQUIRE(p.partial, SRGAN_EINVAL, "srgan_h_conv3x3_wgrad: register a workspace for this stream first (srgan_set_workspace)");
  const dim3 grid((unsigned)blocks, (unsigned)walkers);
  const int slot = profile_bracket_begin(s);
  const int64_t elements = (int64_t)C_out * C_in * 9;
  const int status = launch_for_precision<1, 2>(dtype, [&](auto prec) {
    constexpr int PREC = decltype(prec)::value;
    if (tw == 32) hwgrad3_launch<32, 2, PREC>(p, mb, grid, s);
    else if (tw == 16) hwgrad3_launch<16, 4, PREC>(p, mb, grid, s);
    else if (tw == 8) hwgrad3_launch<8, 8, PREC>(p, mb, grid, s);
    else hwgrad3_launch<4, 4, PREC>(p, mb, grid, s);
    hipLaunchKernelGGL(hwgrad3x3_finish_kernel, dim3((unsigned)(blocks * 32 * mb)), dim3(256), 0, s, p.partial, gw,
                       C_out, C_in, p.tiles_ci, walkers, 32 * mb);
  });
  const double pixels = (double)N * H * W;
  profile_bracket_end_bytes(slot, s, C_out, (int64_t)C_in * 9, (int64_t)pixels, KIND_HWGRAD3X3, 32 * mb, 64, walkers,
                            2.0 * pixels * (p.CGX + p.CGY) * 8 + 8.0 * (double)elements, dtype);
  return status;
}

}  // extern "C"
