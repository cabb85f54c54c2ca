// blocked16_shadows.hip -- the weight shadows: every operand that is rounded or re-ordered from the fp32 master weights once per
// optimizer step (layouts and device bodies: weight_shadows.h).
//
//   conv weights          R x S taps in operand slots, forward or flipped + transposed   VGG-16's 3x3 stack (blocked16_conv3x3.hip)
//   4x4 / stride 2        "down", or the four parity classes "up"                        the DCGAN stages (blocked16_k4s2.hip)
//   matrix                a 16-bit matrix, optionally transposed / in blocked plane order   the linear layers (blocked16_gemm.hip)
//   bias rows             a bias repeated over a blocked plane, fp32                     the seed transposed convolution
//   3x3 weight image      fp32, padded rows                                              conv3x3.hip's weight-image forms
//
// Each kind is one HPackKind.  ONE host function per kind derives its job(s) -- the body's arguments -- from an entry point's
// arguments; the kind's single-layer entry point launches its kernel from the job's fields, its srgan_h_pack_job_* filler adds
// the first workgroup and copies the job out for h_pack_batched_kernel, which runs the same bodies for a whole network in one
// launch.
#include <type_traits>
#include <string.h>
#include "weight_shadows.h"

namespace srgan {

// ---------------------------------------------------------------------------------------------------- single-layer kernels
// A convolution's weights in operand slots, rounded once per optimizer step (the "16-bit shadow" of the fp32 masters):
//   packed[((chunk * T + tap) * 2 + group) * CO + o] = the 8 channels chunk * 16 + group * 8 ... + 7 of tap `tap` of output
//   channel o, element (o, c, kh, kw) at w[base + o * so + c * si + kh * skh + kw * skw]   (zero beyond CI)
// T = R * S taps.  The data gradient's shadow is the same call with the channel roles swapped and mirrored taps (base at the
// last tap, negative tap strides).
template <int PREC>
__global__ __launch_bounds__(256) void h_pack_conv_weights_kernel(const float* __restrict__ w, Slot* __restrict__ packed,
                                                                  int64_t slots, int32_t CO, int32_t CI, int32_t R, int32_t S,
                                                                  int32_t base, int32_t so, int32_t si, int32_t skh, int32_t skw) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= slots) return;
  h_pack_conv_weights_slot<PREC>(w, packed, slot, CO, CI, R, S, base, so, si, skh, skw);
}

__global__ __launch_bounds__(256) void conv3x3_image_kernel(const float* __restrict__ w, float* __restrict__ image, int64_t floats,
                                                            int32_t CO, int32_t CI, int32_t base, int32_t so, int32_t si,
                                                            int32_t skh, int32_t skw) {
  const int64_t element = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (element >= floats) return;
  conv3x3_image_element(w, image, element, CO, CI, base, so, si, skh, skw);
}

// (G = channels per slot: 8, or 4 for the fp32 form)
// mode 0 ("down"): slot (chunk, tap = 2a + b, j = 2 qy + qx, o) = G reduced channels G chunk .. of w[o][.][2a + qy][2b + qx]
// mode 1 + 2 ry + rx ("up", one output parity class): slot (chunk, tap, j, o) = 8 reduced channels 8 (4 chunk + j) .. of
//   w[.][o][kh(ry, a)][kw(rx, b)]
// element (row o, reduced r, kh, kw) at w[o * row_stride + r * reduced_stride + kh * 4 + kw]
template <int PREC>
__global__ __launch_bounds__(256) void h_pack_k4s2_weights_kernel(const float* __restrict__ w, Slot* __restrict__ packed,
                                                                  int64_t slots, int32_t rows, int32_t reduced, int64_t row_stride,
                                                                  int64_t reduced_stride, int32_t mode) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= slots) return;
  h_pack_k4s2_weights_slot<PREC>(w, packed, slot, rows, reduced, row_stride, reduced_stride, mode);
}

// out16[r][c] (pitch ld elements, ld % 8 == 0) = src[map(r, row_plane) * rs + map(c, col_plane) * cs] for map(r) < rows_real,
// map(c) < cols_real, else 0.  One thread per slot of 8 consecutive c (body: h_pack_matrix_slot).
template <int PREC>
__global__ __launch_bounds__(256) void h_pack_matrix_kernel(const float* __restrict__ src, Slot* __restrict__ out, int64_t slots,
                                                            int32_t row_slots, int64_t rows_real, int64_t cols_real, int64_t rs,
                                                            int64_t cs, int32_t row_plane, int32_t col_plane) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= slots) return;
  h_pack_matrix_slot<PREC>(src, out, slot, row_slots, rows_real, cols_real, rs, cs, row_plane, col_plane);
}

// The same for a row stride of 1 (the TRANSPOSED shadow of a row-major matrix: consecutive output rows are consecutive source
// addresses): a 64 x 64 tile goes through LDS, so both the fp32 reads (along r) and the 16-byte slot stores (along c) are
// coalesced -- the one-thread-per-slot kernel read eight floats a row pitch apart and fetched every line seven times
// (4.1 GB per step for VGG-16's two large linear layers, PMC profiles/r06f).  Body: h_pack_matrix_tile.
template <int PREC>
__global__ __launch_bounds__(256) void h_pack_matrix_transposed_kernel(const float* __restrict__ src, Slot* __restrict__ out,
                                                                       int64_t rows, int32_t row_slots, int64_t rows_real,
                                                                       int64_t cols_real, int64_t cs, int32_t row_plane,
                                                                       int32_t col_plane, int32_t tiles_r) {
  __shared__ float tile[64][65];
  h_pack_matrix_tile<PREC>(src, out, tile, (int)blockIdx.x, rows, row_slots, rows_real, cols_real, cs, row_plane, col_plane, tiles_r);
}

// ---------------------------------------------------------------------------------------------------- the batched launch
// Every weight shadow of one network in ONE launch: a workgroup finds its job by bisection over the jobs' first blocks
// (wave-uniform), then runs that job's body.  A step of the driving configuration re-rounds 80 operands, of the VGG
// configuration 52: as single launches they were 0.45 / 0.34 ms of 5 us kernels with the launch gaps on top.  The matrix shadows
// (linear layers) and the seed layer's bias rows are jobs too, so a refresh writes only fixed addresses and can be captured in a
// HIP graph.  The transposed-matrix body stages a 64 x 65 fp32 tile in LDS (16.6 KB per workgroup for every job kind: eight
// 256-thread workgroups per CU, the wave limit, still fit in the 160 KB of a gfx950 CU).
__global__ __launch_bounds__(256) void h_pack_batched_kernel(const HPackJob* __restrict__ jobs, int32_t count) {
  __shared__ float tile[64][65];
  int lo = 0, hi = count - 1;
  const int64_t block = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_block <= block) lo = mid; else hi = mid - 1;
  }
  const HPackJob job = jobs[lo];
  const int64_t slot = (block - job.first_block) * 256 + threadIdx.x;
  if (slot >= job.slots) return;
  const int32_t* q = job.p;
  if (job.kind == PACK_CONV_WEIGHTS) {
    if (job.prec == 1) h_pack_conv_weights_slot<1>(job.w, job.packed, slot, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
    else h_pack_conv_weights_slot<2>(job.w, job.packed, slot, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
  } else if (job.kind == PACK_K4S2_WEIGHTS) {
    if (job.prec == 0) h_pack_k4s2_weights_slot<0>(job.w, job.packed, slot, q[0], q[1], q[2], q[3], q[4]);
    else if (job.prec == 1) h_pack_k4s2_weights_slot<1>(job.w, job.packed, slot, q[0], q[1], q[2], q[3], q[4]);
    else h_pack_k4s2_weights_slot<2>(job.w, job.packed, slot, q[0], q[1], q[2], q[3], q[4]);
  } else if (job.kind == PACK_MATRIX) {
    if (job.prec == 1) h_pack_matrix_slot<1>(job.w, job.packed, slot, q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
    else h_pack_matrix_slot<2>(job.w, job.packed, slot, q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
  } else if (job.kind == PACK_MATRIX_TILED) {       // the whole workgroup (slots = 256 x tiles: no thread returned above)
    const int tile_index = (int)(block - job.first_block);
    if (job.prec == 1) h_pack_matrix_tile<1>(job.w, job.packed, tile, tile_index, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]);
    else h_pack_matrix_tile<2>(job.w, job.packed, tile, tile_index, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]);
  } else if (job.kind == PACK_BIAS_ROWS) {
    h_bias_rows_slot(job.w, reinterpret_cast<float*>(job.packed), slot, q[0], q[1]);
  } else {
    conv3x3_image_element(job.w, reinterpret_cast<float*>(job.packed), slot, q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
  }
}

// ---------------------------------------------------------------------------------------------------- one job function per kind
static HPackJob new_job(HPackKind kind, int prec, const float* w, void* packed) {
  HPackJob job;
  memset(&job, 0, sizeof(job));
  job.w = w; job.packed = (Slot*)packed; job.kind = kind; job.prec = prec;
  return job;
}

static int64_t job_blocks(const HPackJob& job) { return (job.slots + 255) / 256; }

// what a filler does with `count` jobs derived by the functions below: workgroups from `first_block` on, in order, copied out to
// the caller's (host) array; the workgroups they take
static int64_t write_jobs(void* out, int64_t first_block, HPackJob* jobs, int count) {
  int64_t blocks = 0;
  for (int i = 0; i < count; ++i) {
    jobs[i].first_block = first_block + blocks;
    blocks += job_blocks(jobs[i]);
  }
  memcpy(out, jobs, count * sizeof(HPackJob));
  return blocks;
}

// one conv-weight operand of w[K][C][R][S]; transposed: rows = C, taps mirrored
static HPackJob conv_weights_job(const float* w, void* packed, int32_t K, int32_t C, int32_t R, int32_t S, int transposed, int dtype) {
  HPackJob job = new_job(PACK_CONV_WEIGHTS, dtype, w, packed);
  const int rows = transposed ? C : K, reduced = transposed ? K : C;
  job.slots = srgan_h_conv_weight_slots(rows, reduced, R, S);
  job.p[0] = rows; job.p[1] = reduced; job.p[2] = R; job.p[3] = S;
  job.p[4] = transposed ? R * S - 1 : 0;                    // base
  job.p[5] = transposed ? R * S : C * R * S;                // row stride
  job.p[6] = transposed ? C * R * S : R * S;                // reduced-channel stride
  job.p[7] = transposed ? -S : S; job.p[8] = transposed ? -1 : 1;
  return job;
}

// one weight image of conv2d weights w[K][C][3][3]; transposed: the data gradient's operand (rows = C, reduced = K, taps
// mirrored) -- the strides conv3x3_run is called with for that direction
static HPackJob conv3x3_image_job(const float* w, float* image, int32_t K, int32_t C, int transposed) {
  HPackJob job = new_job(PACK_CONV3X3_IMAGE, 0, w, image);
  const int rows = transposed ? C : K, reduced = transposed ? K : C;
  job.slots = conv3x3_image_floats(reduced, rows);
  job.p[0] = rows; job.p[1] = reduced;
  job.p[2] = transposed ? 8 : 0;                            // base
  job.p[3] = transposed ? 9 : C * 9;                        // row stride
  job.p[4] = transposed ? C * 9 : 9;                        // reduced-channel stride
  job.p[5] = transposed ? -3 : 3; job.p[6] = transposed ? -1 : 1;
  return job;
}

// the operand(s) of w[A][B][4][4]: one job "down" (rows A), four "up" (rows B: the output parity classes, class-major in
// `packed`); the number written to `jobs`.  p = the body's (rows, reduced, row_stride, reduced_stride, mode).  The strides are
// the job's 32-bit integers for the single-layer call too: B * 16 < 2^31, a weight tensor below 8 GB per row of A.
static int k4s2_weights_jobs(HPackJob (&jobs)[4], const float* w, void* packed, int32_t A, int32_t B, int direction, int dtype) {
  const int count = direction ? 4 : 1;
  const int64_t slots = srgan_h_k4s2_weight_slots(A, B, direction, dtype) / count;
  for (int cls = 0; cls < count; ++cls) {
    HPackJob& job = jobs[cls] = new_job(PACK_K4S2_WEIGHTS, dtype, w, (Slot*)packed + cls * slots);
    job.slots = slots;
    job.p[0] = direction ? B : A; job.p[1] = direction ? A : B;
    job.p[2] = direction ? 16 : B * 16; job.p[3] = direction ? B * 16 : 16; job.p[4] = direction ? 1 + cls : 0;
  }
  return count;
}

// A matrix shadow is written by the tile-transposing body where its rows are consecutive source addresses, else by the
// one-thread-per-slot body; the tiles of the former (row tiles fastest).
static bool matrix_shadow_is_tiled(int64_t row_stride, int64_t col_stride) { return row_stride == 1 && col_stride != 1; }
struct MatrixTiles { int64_t tiles_r, tiles; };
static MatrixTiles matrix_shadow_tiles(int64_t rows, int64_t row_slots) {
  const int64_t tiles_r = (rows + 63) / 64, tiles = tiles_r * ((row_slots * 8 + 63) / 64);
  return {tiles_r, tiles};
}

// The matrix shadow srgan_h_pack_matrix writes, as one job.  The job keeps its integers in 32 bits: the caller has checked that
// every extent and stride is below 2^31 and that the tiles fit.
static HPackJob matrix_job(const float* src, void* out, int64_t rows, int64_t cols, int64_t rows_real, int64_t cols_real,
                           int64_t row_stride, int64_t col_stride, int32_t row_plane, int32_t col_plane, int dtype) {
  const int64_t row_slots = (cols + 7) / 8;
  const bool tiled = matrix_shadow_is_tiled(row_stride, col_stride);
  HPackJob job = new_job(tiled ? PACK_MATRIX_TILED : PACK_MATRIX, dtype, src, out);
  if (tiled) {
    const MatrixTiles t = matrix_shadow_tiles(rows, row_slots);
    job.slots = t.tiles * 256;
    job.p[0] = (int32_t)rows; job.p[1] = (int32_t)row_slots; job.p[2] = (int32_t)rows_real; job.p[3] = (int32_t)cols_real;
    job.p[4] = (int32_t)col_stride; job.p[5] = row_plane; job.p[6] = col_plane; job.p[7] = (int32_t)t.tiles_r;
  } else {
    job.slots = rows * row_slots;
    job.p[0] = (int32_t)row_slots; job.p[1] = (int32_t)rows_real; job.p[2] = (int32_t)cols_real; job.p[3] = (int32_t)row_stride;
    job.p[4] = (int32_t)col_stride; job.p[5] = row_plane; job.p[6] = col_plane;
  }
  return job;
}

// fp32 rows[ceil(channels / 8) * plane * 8]: rows[(g * plane + p) * 8 + j] = bias[8 g + j], 0 from `channels` on (the bias of every
// output row of a seed transposed convolution in the blocked order).  Batched only: there is no single-layer entry point.
static HPackJob bias_rows_job(const float* bias, float* rows, int32_t channels, int32_t plane) {
  HPackJob job = new_job(PACK_BIAS_ROWS, 0, bias, rows);
  job.slots = (int64_t)(channels + 7) / 8 * plane;
  job.p[0] = channels; job.p[1] = plane;
  return job;
}

}  // namespace srgan

using namespace srgan;

extern "C" {

// ---- sizes
// Slots of a packed convolution weight tensor of CO rows, CI reduced channels and R x S taps.
int64_t srgan_h_conv_weight_slots(int32_t CO, int32_t CI, int32_t R, int32_t S) {
  return (int64_t)((CI + 15) / 16) * R * S * 2 * CO;
}

// 16-byte slots of one operand of a [A][B][4][4] weight tensor: direction 0 "down" (rows = A: the strided convolution's forward /
// a transposed convolution's data gradient), 1 "up" (rows = B, all four output parity classes, class-major).
int64_t srgan_h_k4s2_weight_slots(int32_t A, int32_t B, int direction, int dtype) {
  if (direction == 0) return (int64_t)channel_groups(B, dtype) * K4_TAPS * K4_CK * A;
  return (int64_t)4 * ((channel_groups(A, dtype) + K4_CK - 1) / K4_CK) * K4_TAPS * K4_CK * B;
}

// floats of the fp32 weight image of a 3x3 convolution (layout: conv3x3_image_element)
int64_t srgan_conv3x3_image_floats(int32_t CI, int32_t CO) {
  return (CI > 0 && CO > 0) ? conv3x3_image_floats(CI, CO) : 0;
}

int32_t srgan_h_pack_job_bytes(void) { return (int32_t)sizeof(HPackJob); }

// ---- each kind's single-layer call, and its filler for the batched form: the caller keeps a device array of jobs
// (srgan_h_pack_job_bytes() each), filled on the host with the arguments of the single-layer calls, and launches them all at
// once.  A filler writes its jobs at `jobs` (host memory) with workgroups from `first_block` on and returns the number of
// workgroups they take (< 0: error).  Both check the shared arguments alike unless a comment says otherwise.

// transposed = 0: the forward operand of conv2d weights w[K][C][R][S] (rows = K, reduced = C).
// transposed = 1: the data-gradient operand (rows = C, reduced = K, taps mirrored).   (Any non-zero value is 1, in both.)
int srgan_h_pack_conv_weights(const float* w, void* packed, int32_t K, int32_t C, int32_t R, int32_t S, int transposed, int dtype,
                              void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<1, 2>(dtype, H16_ONLY)) return status;
  SRGAN_REQUIRE(w && packed && K > 0 && C > 0 && R > 0 && S > 0, SRGAN_EINVAL, "srgan_h_pack_conv_weights arguments");
  const HPackJob job = conv_weights_job(w, packed, K, C, R, S, transposed, dtype);
  const dim3 grid((unsigned)job_blocks(job));
  const int32_t* q = job.p;
  return launch_for_precision<1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_pack_conv_weights_kernel<decltype(prec)::value>, grid, dim3(256), 0, s, job.w, job.packed, job.slots, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
  });
}

int64_t srgan_h_pack_job_conv_weights(void* jobs, int64_t first_block, const float* w, void* packed, int32_t K, int32_t C, int32_t R,
                                      int32_t S, int transposed, int dtype) {
  if (const int status = check_precision<1, 2>(dtype, H16_ONLY)) return status;
  SRGAN_REQUIRE(jobs && first_block >= 0 && w && packed && K > 0 && C > 0 && R > 0 && S > 0, SRGAN_EINVAL,
                "srgan_h_pack_job_conv_weights arguments");
  HPackJob job = conv_weights_job(w, packed, K, C, R, S, transposed, dtype);
  return write_jobs(jobs, first_block, &job, 1);
}

int srgan_h_pack_k4s2_weights(const float* w, void* packed, int32_t A, int32_t B, int direction, int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<0, 1, 2>(dtype, H_ANY)) return status;
  SRGAN_REQUIRE(w && packed && A > 0 && B > 0 && (direction == 0 || direction == 1), SRGAN_EINVAL, "srgan_h_pack_k4s2_weights arguments");
  HPackJob jobs[4];
  const int count = k4s2_weights_jobs(jobs, w, packed, A, B, direction, dtype);
  return launch_for_precision<0, 1, 2>(dtype, [&](auto prec) {
    for (int cls = 0; cls < count; ++cls) {
      const HPackJob& job = jobs[cls];
      const int32_t* q = job.p;
      hipLaunchKernelGGL(h_pack_k4s2_weights_kernel<decltype(prec)::value>, dim3((unsigned)job_blocks(job)), dim3(256), 0, s, job.w, job.packed, job.slots, q[0], q[1], (int64_t)q[2], (int64_t)q[3], q[4]);
    }
  });
}

// (the dtype message names the filler, the single call's is H_ANY: the status is the same)
int64_t srgan_h_pack_job_k4s2_weights(void* jobs, int64_t first_block, const float* w, void* packed, int32_t A, int32_t B,
                                      int direction, int dtype, int32_t* jobs_written) {
  if (const int status = check_precision<0, 1, 2>(dtype, "srgan_h_pack_job_k4s2_weights dtype")) return status;
  SRGAN_REQUIRE(jobs && first_block >= 0 && w && packed && A > 0 && B > 0 && (direction == 0 || direction == 1) && jobs_written,
                SRGAN_EINVAL, "srgan_h_pack_job_k4s2_weights arguments");
  HPackJob made[4];
  *jobs_written = k4s2_weights_jobs(made, w, packed, A, B, direction, dtype);
  return write_jobs(jobs, first_block, made, *jobs_written);
}

// out16[rows][cols] (row pitch = ceil(cols / 8) slots) = src[map(r, row_plane) * row_stride + map(c, col_plane) * col_stride],
// zero where the mapped index is outside [rows_real) x [cols_real).  map(i, P) = the NCHW-flattened index of element i of a
// flattened blocked plane tensor with P pixels (P <= 1: identity).
// The single call takes 64-bit extents and strides, which a job cannot hold, so it keeps a launch of its own (with the job's
// rule for the body and its tile counts) and its own answers: no check of the strides, planes and real extents, and
// SRGAN_ERANGE for a row too long.
int srgan_h_pack_matrix(const float* src, void* out, int64_t rows, int64_t cols, int64_t rows_real, int64_t cols_real,
                        int64_t row_stride, int64_t col_stride, int32_t row_plane, int32_t col_plane, int dtype,
                        void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (const int status = check_precision<1, 2>(dtype, H16_ONLY)) return status;
  SRGAN_REQUIRE(src && out && rows > 0 && cols > 0, SRGAN_EINVAL, "srgan_h_pack_matrix arguments");
  const int64_t row_slots = (cols + 7) / 8, slots = rows * row_slots;
  SRGAN_REQUIRE(row_slots < ((int64_t)1 << 31), SRGAN_ERANGE, "srgan_h_pack_matrix row length");
  if (matrix_shadow_is_tiled(row_stride, col_stride)) {
    const MatrixTiles t = matrix_shadow_tiles(rows, row_slots);
    const dim3 tgrid((unsigned)t.tiles);
    return launch_for_precision<1, 2>(dtype, [&](auto prec) {
      hipLaunchKernelGGL(h_pack_matrix_transposed_kernel<decltype(prec)::value>, tgrid, dim3(256), 0, s, src, (Slot*)out, rows, (int32_t)row_slots, rows_real, cols_real, col_stride, row_plane, col_plane, (int32_t)t.tiles_r);
    });
  }
  const dim3 grid((unsigned)((slots + 255) / 256));
  return launch_for_precision<1, 2>(dtype, [&](auto prec) {
    hipLaunchKernelGGL(h_pack_matrix_kernel<decltype(prec)::value>, grid, dim3(256), 0, s, src, (Slot*)out, slots, (int32_t)row_slots, rows_real, cols_real, row_stride, col_stride, row_plane, col_plane);
  });
}

// ... and the filler's: everything must fit the job's 32 bits, SRGAN_EINVAL where it does not.
int64_t srgan_h_pack_job_matrix(void* jobs, int64_t first_block, const float* src, void* out, int64_t rows, int64_t cols,
                                int64_t rows_real, int64_t cols_real, int64_t row_stride, int64_t col_stride, int32_t row_plane,
                                int32_t col_plane, int dtype) {
  if (const int status = check_precision<1, 2>(dtype, H16_ONLY)) return status;
  const int64_t limit = (int64_t)1 << 31;
  SRGAN_REQUIRE(jobs && first_block >= 0 && src && out && rows > 0 && cols > 0 && rows < limit && cols < limit && rows_real >= 0 &&
                rows_real < limit && cols_real >= 0 && cols_real < limit && row_stride > 0 && row_stride < limit && col_stride > 0 &&
                col_stride < limit && row_plane >= 0 && col_plane >= 0, SRGAN_EINVAL, "srgan_h_pack_job_matrix arguments");
  HPackJob job = matrix_job(src, out, rows, cols, rows_real, cols_real, row_stride, col_stride, row_plane, col_plane, dtype);
  SRGAN_REQUIRE(job.kind != PACK_MATRIX_TILED || job_blocks(job) < limit / 256, SRGAN_EINVAL, "srgan_h_pack_job_matrix size");
  return write_jobs(jobs, first_block, &job, 1);
}

int64_t srgan_h_pack_job_bias_rows(void* jobs, int64_t first_block, const float* bias, float* rows, int32_t channels, int32_t plane) {
  SRGAN_REQUIRE(jobs && first_block >= 0 && bias && rows && channels > 0 && plane > 0 &&
                (int64_t)(channels + 7) / 8 * plane < ((int64_t)1 << 31), SRGAN_EINVAL, "srgan_h_pack_job_bias_rows arguments");
  HPackJob job = bias_rows_job(bias, rows, channels, plane);
  return write_jobs(jobs, first_block, &job, 1);
}

// transposed = 0: the forward operand of conv2d weights w[K][C][3][3] (CO = K, CI = C); 1: the data gradient's (CO = C, CI = K)
int srgan_h_pack_conv3x3_image(const float* w, float* image, int32_t K, int32_t C, int transposed, void* stream) {
  SRGAN_REQUIRE(w && image && K > 0 && C > 0 && (transposed == 0 || transposed == 1) && (((uintptr_t)image) & 15) == 0 &&
                (int64_t)K * C * 9 < ((int64_t)1 << 31), SRGAN_EINVAL, "srgan_h_pack_conv3x3_image arguments");
  const HPackJob job = conv3x3_image_job(w, image, K, C, transposed);
  const int32_t* q = job.p;
  hipLaunchKernelGGL(conv3x3_image_kernel, dim3((unsigned)job_blocks(job)), dim3(256), 0, (hipStream_t)stream, job.w, image,
                     job.slots, q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
  return launch_status();
}

int64_t srgan_h_pack_job_conv3x3_image(void* jobs, int64_t first_block, const float* w, float* image, int32_t K, int32_t C,
                                       int transposed) {
  SRGAN_REQUIRE(jobs && first_block >= 0 && w && image && K > 0 && C > 0 && (transposed == 0 || transposed == 1) &&
                (((uintptr_t)image) & 15) == 0 && (int64_t)K * C * 9 < ((int64_t)1 << 31), SRGAN_EINVAL,
                "srgan_h_pack_job_conv3x3_image arguments");
  HPackJob job = conv3x3_image_job(w, image, K, C, transposed);
  return write_jobs(jobs, first_block, &job, 1);
}

int srgan_h_pack_batched(const void* jobs_device, int32_t count, int64_t blocks, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  SRGAN_REQUIRE(jobs_device && count > 0 && blocks > 0 && blocks < ((int64_t)1 << 31), SRGAN_EINVAL, "srgan_h_pack_batched arguments");
  hipLaunchKernelGGL(h_pack_batched_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const HPackJob*)jobs_device, count);
  return launch_status();
}

}  // extern "C"
