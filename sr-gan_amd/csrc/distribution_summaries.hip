// distribution_summaries.hip -- what the coefficient application logs about distributions at a summary step, computed where
// the predictions already are (SRGAN_FEATURE_DISTRIBUTION_SUMMARIES; contracts in include/srgan_hip.h): the 1-D Wasserstein
// distance of two sample sets (reference coefficient/srgan.py:56-64), Gaussian kernel-density curves and the line chart that
// shows them (coefficient/presentation.py:19-55).  Summary-step work of a few thousand values: one workgroup sorts, the other
// kernels are gathers; nothing here is tuned beyond coalesced loads and stores.  Every fp32 operation whose rounding the tests'
// restatement repeats is spelled with the _rn intrinsics, so that the compiler does not contract it into an fma.
#include <cmath>

#include "bn_train.h"
#include "launchers.h"

namespace srgan {

constexpr int WASSERSTEIN_THREADS = 1024;
// keys [P] floats, the threads' partial sums [1024] floats, the threads' tag counts [1024] ints, tags [P] bytes
inline int wasserstein_lds_bytes(int P) { return 5 * P + 8 * WASSERSTEIN_THREADS; }

// One workgroup; P = the power of two >= n + m (>= 2).  Thread t owns the sorted positions [t * E, (t + 1) * E), E = max(P / 1024,
// 1): its gaps k (between x[k] and x[k + 1], k + 1 < n + m) are added in order, then the 1024 partial sums in a halving tree.
__global__ __launch_bounds__(WASSERSTEIN_THREADS) void wasserstein_kernel(const float* __restrict__ u, int n,
                                                                          const float* __restrict__ v, int m, int P,
                                                                          float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char wasserstein_lds[];
  float* keys = (float*)wasserstein_lds;
  float* partial = keys + P;
  int* counts = (int*)(partial + WASSERSTEIN_THREADS);
  unsigned char* tags = (unsigned char*)(counts + WASSERSTEIN_THREADS);
  const int t = threadIdx.x, N = n + m;
  for (int i = t; i < P; i += WASSERSTEIN_THREADS) {
    float key = INFINITY;
    unsigned char tag = 0;
    if (i < n) {
      key = u[i];
      tag = 1;
    } else if (i < N) {
      key = v[i - n];
    }
    keys[i] = key;
    tags[i] = tag;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P / 2; i += WASSERSTEIN_THREADS) {
        const int a = 2 * i - (i & (j - 1)), b = a + j;      // bit j of a is clear; a, b < P
        const float ka = keys[a], kb = keys[b];
        if ((a & k) == 0 ? ka > kb : ka < kb) {
          keys[a] = kb;
          keys[b] = ka;
          const unsigned char ta = tags[a];
          tags[a] = tags[b];
          tags[b] = ta;
        }
      }
      __syncthreads();
    }
  }
  const int E = P >= WASSERSTEIN_THREADS ? P / WASSERSTEIN_THREADS : 1;
  const int begin = min(t * E, P), end = min(begin + E, P);
  int own = 0;
  for (int k = begin; k < end; ++k) own += tags[k];
  counts[t] = own;
  __syncthreads();
  for (int offset = 1; offset < WASSERSTEIN_THREADS; offset <<= 1) {      // inclusive scan of the threads' counts
    const int before = t >= offset ? counts[t - offset] : 0;
    __syncthreads();
    counts[t] += before;
    __syncthreads();
  }
  int cu = counts[t] - own;
  float sum = 0.f;
  for (int k = begin; k < end; ++k) {
    cu += tags[k];
    if (k + 1 < N) {
      const int cv = k + 1 - cu;
      const int64_t difference = (int64_t)cu * m - (int64_t)cv * n;
      const float weight = (float)(difference < 0 ? -difference : difference);
      sum = __fadd_rn(sum, __fmul_rn(weight, __fsub_rn(keys[k + 1], keys[k])));
    }
  }
  partial[t] = sum;
  for (int stride = WASSERSTEIN_THREADS / 2; stride > 0; stride >>= 1) {
    __syncthreads();
    if (t < stride) partial[t] = __fadd_rn(partial[t], partial[t + stride]);
  }
  if (t == 0) out[0] = __fdiv_rn(partial[0], (float)((int64_t)n * m));
}

// stats[c] = (count, min, max, h) of curve c = samples[offsets[c] .. offsets[c + 1]): workgroup c.  Each thread runs Welford's
// update over its samples (every 256th, in order); the threads meet in the fixed tree of bn_train.h.
__global__ __launch_bounds__(256) void kde_stats_kernel(const float* __restrict__ samples, const int32_t* __restrict__ offsets,
                                                        float factor, float* __restrict__ stats) {
  __shared__ float extrema[2][4];
  __shared__ Moments waves[4];
  const int c = blockIdx.x;
  const int begin = offsets[c], end = offsets[c + 1];
  Moments own{0.f, 0.f, 0.f};
  float lo = INFINITY, hi = -INFINITY;
  for (int i = begin + (int)threadIdx.x; i < end; i += 256) {
    const float x = samples[i];
    own.n += 1.f;
    const float delta = x - own.mean;
    own.mean += delta / own.n;
    own.m2 += delta * (x - own.mean);
    lo = fminf(lo, x);
    hi = fmaxf(hi, x);
  }
  block_min_max_256(lo, hi, extrema);
  const Moments all = block_moments_256(own, waves);
  if (threadIdx.x == 0) {
    float h = 0.f;
    if (all.n >= 2.f) {
      h = __fmul_rn(factor, __fsqrt_rn(__fdiv_rn(all.m2, all.n - 1.f)));
      if (!(h > 0.f) || !isfinite(h)) h = 0.f;
    }
    float* row = stats + 4 * (int64_t)c;
    row[0] = all.n;
    row[1] = all.n > 0.f ? lo : 0.f;
    row[2] = all.n > 0.f ? hi : 0.f;
    row[3] = h;
  }
}

// support[c, g] and density[c, g]: workgroup (x, c) owns 256 grid points of curve c, one per thread; the curve's samples pass
// through LDS 256 at a time and every thread adds their kernels in stored order.
__global__ __launch_bounds__(256) void kde_evaluate_kernel(const float* __restrict__ samples, const int32_t* __restrict__ offsets,
                                                           int G, float cut, const float* __restrict__ stats,
                                                           float* __restrict__ support, float* __restrict__ density) {
  __shared__ float tile[256];
  const int c = blockIdx.y, g = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const float* row = stats + 4 * (int64_t)c;
  const float count = row[0], h = row[3];
  const int64_t at = (int64_t)c * G + g;
  if (h == 0.f) {      // the whole workgroup: an invalid curve
    if (g < G) support[at] = density[at] = 0.f;
    return;
  }
  const float reach = __fmul_rn(cut, h);
  const float lo = __fsub_rn(row[1], reach), top = __fadd_rn(row[2], reach);
  const float step = __fdiv_rn(__fsub_rn(top, lo), (float)(G - 1));
  const float s = __fadd_rn(lo, __fmul_rn((float)g, step));
  const float inverse_h = __fdiv_rn(1.f, h);
  const float scale = __fdiv_rn(1.f, __fmul_rn(__fmul_rn(count, h), 2.5066282746310002f));
  const int begin = offsets[c], end = offsets[c + 1];
  float sum = 0.f;
  for (int base = begin; base < end; base += 256) {
    __syncthreads();
    if (base + (int)threadIdx.x < end) tile[threadIdx.x] = samples[base + threadIdx.x];
    __syncthreads();
    const int held = min(256, end - base);
    for (int i = 0; i < held; ++i) {
      const float z = __fmul_rn(__fsub_rn(s, tile[i]), inverse_h);
      sum = __fadd_rn(sum, expf(__fmul_rn(__fmul_rn(-0.5f, z), z)));
    }
  }
  if (g < G) {
    support[at] = s;
    density[at] = __fmul_rn(sum, scale);
  }
}

struct FrameAxes { float x_lo, x_scale, y_hi, y_scale; };      // px = (x - x_lo) * x_scale - 0.5, py = (y_hi - y) * y_scale - 0.5

__device__ __forceinline__ void composite(float (&colour)[3], const float* __restrict__ line, float coverage) {
  const float a = fminf(fmaxf(coverage, 0.f), 1.f);
#pragma unroll
  for (int channel = 0; channel < 3; ++channel) colour[channel] = colour[channel] * (1.f - a) + line[channel] * a;
}

// One pixel per thread (grid-stride).  The vertices are the same for every thread of a wave: uniform loads.
__global__ __launch_bounds__(256) void curve_frame_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ offsets,
                                                          int C, const float* __restrict__ colours, const float* __restrict__ widths,
                                                          int H, int W, FrameAxes axes, const float* __restrict__ background,
                                                          const float* __restrict__ grid_colour, const float* __restrict__ x_ticks,
                                                          int n_x, const float* __restrict__ y_ticks, int n_y,
                                                          float* __restrict__ out) {
  const int pixels = H * W;
  for (int pixel = (int)blockIdx.x * 256 + (int)threadIdx.x; pixel < pixels; pixel += (int)gridDim.x * 256) {
    const float cy = (float)(pixel / W), cx = (float)(pixel % W);
    float colour[3] = {background[0], background[1], background[2]};
    for (int i = 0; i < n_x; ++i) composite(colour, grid_colour, 1.f - fabsf((x_ticks[i] - axes.x_lo) * axes.x_scale - 0.5f - cx));
    for (int i = 0; i < n_y; ++i) composite(colour, grid_colour, 1.f - fabsf((axes.y_hi - y_ticks[i]) * axes.y_scale - 0.5f - cy));
    for (int k = 0; k < C; ++k) {
      const int begin = offsets[k], end = offsets[k + 1];
      if (end - begin < 2) continue;
      float nearest = INFINITY;      // squared
      float ax = (vertices[2 * (int64_t)begin] - axes.x_lo) * axes.x_scale - 0.5f;
      float ay = (axes.y_hi - vertices[2 * (int64_t)begin + 1]) * axes.y_scale - 0.5f;
      for (int j = begin + 1; j < end; ++j) {
        const float bx = (vertices[2 * (int64_t)j] - axes.x_lo) * axes.x_scale - 0.5f;
        const float by = (axes.y_hi - vertices[2 * (int64_t)j + 1]) * axes.y_scale - 0.5f;
        const float dx = bx - ax, dy = by - ay, qx = cx - ax, qy = cy - ay;      // relative to the segment's first vertex
        const float length2 = dx * dx + dy * dy;
        const float along = length2 > 0.f ? fminf(fmaxf((qx * dx + qy * dy) / length2, 0.f), 1.f) : 0.f;
        const float ex = qx - along * dx, ey = qy - along * dy;
        nearest = fminf(nearest, ex * ex + ey * ey);
        ax = bx;
        ay = by;
      }
      composite(colour, colours + 3 * (int64_t)k, 0.5f + 0.5f * widths[k] - sqrtf(nearest));
    }
    out[pixel] = colour[0];
    out[(int64_t)pixels + pixel] = colour[1];
    out[2 * (int64_t)pixels + pixel] = colour[2];
  }
}

int wasserstein_run(const float* u, int32_t n, const float* v, int32_t m, float* out, hipStream_t stream) {
  int P = 2;
  while (P < n + m) P <<= 1;
  SRGAN_HIP(allow_dynamic_lds<wasserstein_kernel>(wasserstein_lds_bytes(SRGAN_WASSERSTEIN_MAX_VALUES)));
  hipLaunchKernelGGL(wasserstein_kernel, dim3(1), dim3(WASSERSTEIN_THREADS), wasserstein_lds_bytes(P), stream, u, n, v, m, P, out);
  return launch_status();
}

int kde_curves_run(const float* samples, const int32_t* offsets, int32_t C, int32_t G, float factor, float cut, float* support,
                   float* density, float* stats, hipStream_t stream) {
  hipLaunchKernelGGL(kde_stats_kernel, dim3(C), dim3(256), 0, stream, samples, offsets, factor, stats);
  int status = launch_status();
  if (status != SRGAN_OK) return status;
  hipLaunchKernelGGL(kde_evaluate_kernel, dim3((G + 255) / 256, C), dim3(256), 0, stream, samples, offsets, G, cut, stats,
                     support, density);
  return launch_status();
}

int curve_frame_run(const float* vertices, const int32_t* offsets, int32_t C, const float* colours, const float* widths, int32_t H,
                    int32_t W, float x_lo, float x_hi, float y_lo, float y_hi, const float* background, const float* grid_colour,
                    const float* x_ticks, int32_t n_x, const float* y_ticks, int32_t n_y, float* out, hipStream_t stream) {
  const FrameAxes axes{x_lo, (float)W / (x_hi - x_lo), y_hi, (float)H / (y_hi - y_lo)};
  hipLaunchKernelGGL(curve_frame_kernel, dim3(stream_grid((int64_t)H * W, 256)), dim3(256), 0, stream, vertices, offsets, C, colours,
                     widths, H, W, axes, background, grid_colour, x_ticks, n_x, y_ticks, n_y, out);
  return launch_status();
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_wasserstein_1d(const float* u, int32_t n, const float* v, int32_t m, float* out, void* stream) {
  SRGAN_REQUIRE(u && v && out && n >= 1 && m >= 1, SRGAN_EINVAL, "srgan_wasserstein_1d arguments");
  SRGAN_REQUIRE((int64_t)n + m <= SRGAN_WASSERSTEIN_MAX_VALUES, SRGAN_EUNSUPPORTED,
                "srgan_wasserstein_1d: more than SRGAN_WASSERSTEIN_MAX_VALUES values (one workgroup sorts them in LDS)");
  return wasserstein_run(u, n, v, m, out, (hipStream_t)stream);
}

extern "C" int srgan_kde_curves(const float* samples, const int32_t* offsets, int32_t C, int32_t G, float factor, float cut,
                                float* support, float* density, float* stats, void* stream) {
  SRGAN_REQUIRE(samples && offsets && support && density && stats && C >= 1 && G >= 2, SRGAN_EINVAL, "srgan_kde_curves arguments");
  SRGAN_REQUIRE(std::isfinite(factor) && factor > 0.f && std::isfinite(cut) && cut >= 0.f, SRGAN_EINVAL,
                "srgan_kde_curves: factor must be positive and cut non-negative, both finite");
  SRGAN_REQUIRE(C <= 65535 && (int64_t)C * G <= INT32_MAX, SRGAN_ERANGE,
                "srgan_kde_curves: more than 65535 curves or 2^31 - 1 grid points per call");
  return kde_curves_run(samples, offsets, C, G, factor, cut, support, density, stats, (hipStream_t)stream);
}

extern "C" int srgan_curve_frame(const float* vertices, const int32_t* offsets, int32_t C, const float* colours,
                                 const float* widths, int32_t H, int32_t W, float x_lo, float x_hi, float y_lo, float y_hi,
                                 const float* background, const float* grid_colour, const float* x_ticks, int32_t n_x,
                                 const float* y_ticks, int32_t n_y, float* out, void* stream) {
  SRGAN_REQUIRE(background && grid_colour && out && H >= 1 && W >= 1 && C >= 0 && n_x >= 0 && n_y >= 0, SRGAN_EINVAL,
                "srgan_curve_frame arguments");
  SRGAN_REQUIRE((C == 0 || (vertices && offsets && colours && widths)) && (n_x == 0 || x_ticks) && (n_y == 0 || y_ticks),
                SRGAN_EINVAL, "srgan_curve_frame: a NULL array with a count above 0");
  SRGAN_REQUIRE(std::isfinite(x_lo) && std::isfinite(x_hi) && std::isfinite(y_lo) && std::isfinite(y_hi) && x_hi > x_lo &&
                y_hi > y_lo, SRGAN_EINVAL, "srgan_curve_frame: the axes need finite bounds with lo < hi");
  SRGAN_REQUIRE((int64_t)H * W <= INT32_MAX / 3, SRGAN_ERANGE, "srgan_curve_frame: the frame has more than 2^31 - 1 elements");
  return curve_frame_run(vertices, offsets, C, colours, widths, H, W, x_lo, x_hi, y_lo, y_hi, background, grid_colour, x_ticks,
                         n_x, y_ticks, n_y, out, (hipStream_t)stream);
}
