// summary_histogram.hip -- the histogram record of a summary step, taken where the tensor already is
// (SRGAN_FEATURE_SUMMARY_HISTOGRAM; contract in include/srgan_hip.h).  The tensors a GAN run wants histograms of are the flat
// parameter and gradient arenas, 20 to 137 M floats: the kernel reads them twice and 8 * (5 + 2 * bins + 1) bytes go to the
// host, instead of 4 * n.
//
// Two launches inside the one call:
//   moments   min / max / sum / sum of squares / count of the FINITE elements.  Every workgroup reduces its spans to one value
//             of five doubles; the workgroups meet in the stream's workspace through ordered_lane_finish (split_finish.h): the
//             one that draws the last ticket adds all parts in a fixed order, writes out[0..4] and zeroes the counters.  No
//             floating-point atomics: two runs give the same bits.
//   counts    every workgroup forms the edges in LDS from out[0..4] (the same fp64 operations in each, so the same edges),
//             finds every finite element's bin by an estimate that it then corrects against those stored edges, counts in LDS
//             with 32-bit integer atomics (up to 32 counters per bin, a lane adds to counter lane % copies: a summary tensor
//             has most of its elements in a few bins, and 64 lanes on one LDS word serialise) and adds its non-zero
//             totals to 64-bit integer counters that live in the counts'
//             own slots of `out` (integer sums are order-independent).  The workgroup that draws the last ticket
//             (counters_complete_after_adds, split_finish.h) writes the edges and turns the counters into doubles in place.
// Without a workspace registered for the stream (or with SRGAN_ATOMIC_SPLIT set) there are no tickets: one workgroup does each
// launch's work alone, with the same results for the counts, edges, min and max (the sums then differ in their order only).
//
// Per element one load, a handful of fp64 operations and one LDS atomic; profiles/summary_events.md has the times, beside
// what two reads of the tensor take at the copy rate.
#include "split_finish.h"

// lo + i * width must be the two roundings NumPy float64 arithmetic makes, not one fused one (hipcc compiles with
// -ffp-contract=fast; the pragma travels with the operations through inlining).
#pragma clang fp contract(off)

namespace srgan {

constexpr int HIST_THREADS = 256;
constexpr int HIST_RUNS = 4;                                     // 16-byte loads in flight per thread
constexpr int HIST_SPAN4 = HIST_THREADS * HIST_RUNS;             // float4 per span: a span is 4096 floats
constexpr int HIST_MAX_WORKGROUPS = 2048;                        // 256 CUs x 8; the spans beyond are taken grid-stride
constexpr int HIST_MAX_BINS = 1024;
constexpr int HIST_LOCAL_WORDS = 4096;                           // LDS counters of a workgroup: `copies` per bin, see below
constexpr int HIST_MAX_COPIES = 32;

__device__ unsigned int histogram_tickets[SPLIT_TICKET_SETS * ROW_FINISH_ROWS];

__device__ __forceinline__ bool is_finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// f(x) for every element of x[0..n): workgroup w takes the spans w, w + gridDim.x, ... of the 16-byte aligned body with
// float4 loads, and workgroup 0 the at most 3 + 3 single floats before and behind the body.  Both launches walk the tensor
// through this one function, so both see the same elements whatever the pointer's alignment.
template <typename F>
__device__ __forceinline__ void for_each_element(const float* __restrict__ x, int64_t n, F f) {
  const int64_t to_boundary = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(x) >> 2) & 3)) & 3);
  const int64_t head = to_boundary < n ? to_boundary : n;
  const int64_t n4 = (n - head) >> 2;
  const int tail = (int)((n - head) & 3);
  const float4* body = reinterpret_cast<const float4*>(x + head);
  // (the next span's loads are issued before this span's elements are worked on)
  float4 v[HIST_RUNS], next[HIST_RUNS];
  bool have[HIST_RUNS], have_next[HIST_RUNS];
  auto load = [&](int64_t span, float4 (&into)[HIST_RUNS], bool (&loaded)[HIST_RUNS]) {
#pragma unroll
    for (int j = 0; j < HIST_RUNS; ++j) {
      const int64_t at = span * HIST_SPAN4 + j * HIST_THREADS + (int)threadIdx.x;
      loaded[j] = at < n4;                        // false for every j once the span lies behind the body
      if (loaded[j]) into[j] = body[at];
    }
  };
  load(blockIdx.x, next, have_next);
  for (int64_t span = blockIdx.x; span * HIST_SPAN4 < n4; span += gridDim.x) {
#pragma unroll
    for (int j = 0; j < HIST_RUNS; ++j) { v[j] = next[j]; have[j] = have_next[j]; }
    load(span + gridDim.x, next, have_next);
#pragma unroll
    for (int j = 0; j < HIST_RUNS; ++j)
      if (have[j]) { f(v[j].x); f(v[j].y); f(v[j].z); f(v[j].w); }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < (int)head + tail) {
    const int t = (int)threadIdx.x;
    f(t < (int)head ? x[t] : x[head + 4 * n4 + (t - (int)head)]);
  }
}

// The moments of a set of finite floats; count == 0 marks the empty set (lo / hi are then ignored), so the all-zero value is
// the neutral element that ordered_lane_finish asks for.
struct HistMoments { double lo, hi, sum, squares, count; };

struct HistMomentOps {
  using Value = HistMoments;
  static __device__ __forceinline__ HistMoments combine(const HistMoments& a, const HistMoments& b) {
    if (a.count == 0.0) return b;
    if (b.count == 0.0) return a;
    return HistMoments{b.lo < a.lo ? b.lo : a.lo, b.hi > a.hi ? b.hi : a.hi, a.sum + b.sum, a.squares + b.squares, a.count + b.count};
  }
  // The xor butterfly: every lane ends with the wave's value (each step combines the same two operands in both lanes; +, min
  // and max are commutative, so both lanes get the same bits).
  static __device__ __forceinline__ HistMoments wave(HistMoments v) {
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) {
      HistMoments other;
      other.lo = __shfl_xor(v.lo, offset, 64);
      other.hi = __shfl_xor(v.hi, offset, 64);
      other.sum = __shfl_xor(v.sum, offset, 64);
      other.squares = __shfl_xor(v.squares, offset, 64);
      other.count = __shfl_xor(v.count, offset, 64);
      const bool first = ((int)threadIdx.x & offset) == 0;          // the lower lane's value is the left operand in both
      v = first ? combine(v, other) : combine(other, v);
    }
    return v;
  }
  static __device__ __forceinline__ HistMoments four(const HistMoments& w0, const HistMoments& w1, const HistMoments& w2,
                                                     const HistMoments& w3) {
    return combine(combine(w0, w1), combine(w2, w3));
  }
};

// out[0..4] and the zeroed counters are written by the workgroup that holds the total.  `counters` = the counts' slots of
// `out`, used as 64-bit integers until the second launch converts them.
__global__ __launch_bounds__(HIST_THREADS) void histogram_moments_kernel(const float* __restrict__ x, int64_t n, int bins,
                                                                         float* partial, unsigned int* ticket, double* out) {
  __shared__ HistMoments scratch[4][1];
  HistMoments mine{0.0, 0.0, 0.0, 0.0, 0.0};
  float lo = 0.f, hi = 0.f;
  unsigned int count = 0;               // a thread sees fewer than 2^31 / 256 elements
  for_each_element(x, n, [&](float value) {
    if (!is_finite_bits(value)) return;
    lo = (count == 0 || value < lo) ? value : lo;
    hi = (count == 0 || value > hi) ? value : hi;
    const double wide = (double)value;
    mine.sum += wide;
    mine.squares += wide * wide;        // exact: 48 significant bits
    ++count;
  });
  mine.lo = (double)lo;
  mine.hi = (double)hi;
  mine.count = (double)count;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  mine = HistMomentOps::wave(mine);
  if (lane == 0) scratch[wave][0] = mine;
  __syncthreads();
  if (threadIdx.x == 0) mine = HistMomentOps::four(scratch[0][0], scratch[1][0], scratch[2][0], scratch[3][0]);
  __syncthreads();                      // scratch is reused by the finish
  if (!ordered_lane_finish<HistMomentOps, 1>(mine, partial, (int)blockIdx.x, (int)gridDim.x, ticket, scratch)) return;
  if (threadIdx.x == 0) {
    const bool any = mine.count != 0.0;
    out[0] = any ? mine.lo + 0.0 : 0.0;           // (+ 0.0: a zero minimum or maximum is reported as +0.0)
    out[1] = any ? mine.hi + 0.0 : 0.0;
    out[2] = any ? mine.sum : 0.0;
    out[3] = any ? mine.squares : 0.0;
    out[4] = mine.count;
  }
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(out + 5 + bins + 1);
  for (int i = (int)threadIdx.x; i < bins; i += HIST_THREADS)
    __hip_atomic_store(counters + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(HIST_THREADS) void histogram_counts_kernel(const float* __restrict__ x, int64_t n, int bins,
                                                                        unsigned int* ticket, double* out) {
  __shared__ double edges[HIST_MAX_BINS + 1];
  __shared__ unsigned int local[HIST_LOCAL_WORDS];
  double* out_edges = out + 5;
  if (out[4] == 0.0) {                  // no finite element: the counters are zero bits already, which is +0.0
    if (blockIdx.x == 0)
      for (int i = (int)threadIdx.x; i <= bins; i += HIST_THREADS) out_edges[i] = 0.0;
    return;
  }
  double lo = out[0], hi = out[1];
  if (lo == hi) { lo -= 0.5; hi += 0.5; }
  const double width = (hi - lo) / (double)bins;
  // counter (bin, copy) is local[bin * copies + copy]: copies = the largest power of two <= 32 with bins * copies <= 4096
  int copies = HIST_MAX_COPIES;
  while (bins * copies > HIST_LOCAL_WORDS) copies >>= 1;
  const int copy = (int)threadIdx.x & (copies - 1);
  for (int i = (int)threadIdx.x; i <= bins; i += HIST_THREADS) edges[i] = i < bins ? lo + (double)i * width : hi;
  for (int i = (int)threadIdx.x; i < bins * copies; i += HIST_THREADS) local[i] = 0u;
  __syncthreads();
  const double per_width = (double)bins / (hi - lo);
  for_each_element(x, n, [&](float value) {
    if (!is_finite_bits(value)) return;
    const double wide = (double)value;
    const double estimate = (wide - lo) * per_width;            // in [0, bins] up to rounding; NaN when hi - lo rounds to 0
    int bin = estimate >= 0.0 ? (estimate < (double)bins ? (int)estimate : bins - 1) : 0;
    while (bin > 0 && wide < edges[bin]) --bin;                 // the comparison against the stored edges decides
    while (bin < bins - 1 && wide >= edges[bin + 1]) ++bin;
    atomicAdd(&local[bin * copies + copy], 1u);
  });
  __syncthreads();
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(out + 5 + bins + 1);
  // (the returning form, and its result kept alive: the add has been performed when the value is back, before the ticket)
  unsigned long long seen = 0;
  for (int i = (int)threadIdx.x; i < bins; i += HIST_THREADS) {
    unsigned int mine = 0u;               // fewer than 2^32: a workgroup sees at most 2^31 elements
    for (int c = 0; c < copies; ++c) mine += local[i * copies + ((c + i) & (copies - 1))];        // (+ i: the lanes on different banks)
    if (mine) seen += __hip_atomic_fetch_add(counters + i, (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("" ::"v"(seen));
  if (!counters_complete_after_adds(ticket, (int)gridDim.x)) return;
  for (int i = (int)threadIdx.x; i <= bins; i += HIST_THREADS) {
    out_edges[i] = edges[i];
    if (i < bins) {
      const unsigned long long total = __hip_atomic_load(counters + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double as_double = (double)total;                   // exact below 2^53
      __hip_atomic_store(counters + i, (unsigned long long)__double_as_longlong(as_double), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_tensor_histogram(const float* x, int64_t n, int32_t bins, double* out, void* stream) {
  SRGAN_REQUIRE(out != nullptr && n >= 0 && (x != nullptr || n == 0), SRGAN_EINVAL, "srgan_tensor_histogram: NULL pointer or n < 0");
  SRGAN_REQUIRE(bins >= 1 && bins <= HIST_MAX_BINS, SRGAN_EINVAL, "srgan_tensor_histogram: bins within [1, 1024]");
  SRGAN_REQUIRE(reinterpret_cast<uintptr_t>(x) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0, SRGAN_EINVAL,
                "srgan_tensor_histogram: x is 4-byte and out 8-byte aligned");
  SRGAN_REQUIRE(n <= ((int64_t)1 << 31) - 1, SRGAN_ERANGE, "srgan_tensor_histogram: n within max_tensor_elements (2^31 - 1)");
  constexpr int VALUES = sizeof(HistMoments) / sizeof(float);
  const int64_t spans = (n / 4 + HIST_SPAN4 - 1) / HIST_SPAN4;
  int parts = (int)(spans < 1 ? 1 : (spans > HIST_MAX_WORKGROUPS ? HIST_MAX_WORKGROUPS : spans));
  unsigned int* ticket = nullptr;
  float* partial = parts > 1 ? row_finish_workspace(1, parts, VALUES, histogram_tickets, (hipStream_t)stream, &ticket) : nullptr;
  if (!partial) parts = 1;              // no workspace for this stream: one workgroup, no tickets
  hipLaunchKernelGGL(histogram_moments_kernel, dim3(parts), dim3(HIST_THREADS), 0, (hipStream_t)stream, x, n, (int)bins, partial,
                     ticket, out);
  const int status = launch_status();
  if (status != SRGAN_OK) return status;
  hipLaunchKernelGGL(histogram_counts_kernel, dim3(parts), dim3(HIST_THREADS), 0, (hipStream_t)stream, x, n, (int)bins, ticket, out);
  return launch_status();
}
