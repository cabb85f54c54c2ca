// regression_evaluation.hip -- the sums behind the age and driving applications' evaluation scalars (reference
// age/srgan.py:92-107, driving/srgan.py:87-104: MAE / MSE, NMAE over the label range), taken ON the device from one batch of
// predictions and labels that already live in HBM: six of the caller's eight doubles are updated and nothing goes back to the
// host.  In the SGAN case (reference age/sgan.py:22-26, utility.py:147-151) a row holds K class logits and the prediction is
// the bin value of the first maximal logit, picked here.
//
// One launch of one workgroup: an evaluation batch is at most a few thousand rows of at most a few logits, so the launch is
// latency, not bandwidth.  Thread t takes rows t, t + 256, ... in that order and the 256 running sums meet in a fixed tree
// (evaluation_sums.h): no atomics, no scratch, two calls on the same inputs give the same bits.  Every accumulation is fp64 and
// every square is formed as a rounded product BEFORE it is added: each term is the one NumPy forms from the same fp32 inputs,
// only the order of the additions differs.
#include "evaluation_sums.h"

// hipcc compiles with -ffp-contract=fast: contraction is switched off for every expression of this file, as in
// crowd_evaluation.hip (the GPU test has cases whose bits differ between a fused and a rounded square).
#pragma clang fp contract(off)

namespace srgan {

constexpr int REGRESSION_EVAL_SUMS = 3;                                // sum d, sum |d|, sum d * d
constexpr int64_t REGRESSION_EVAL_MAX_ELEMENTS = (int64_t)1 << 22;     // B * K of one call: at most 2^14 loads per thread
constexpr int REGRESSION_EVAL_MAX_BINS = 1024;

// bins == nullptr: the prediction of row b is predictions[b * row_stride].  Otherwise it is bins[j], j the LOWEST index of the
// row's maximum (`>` keeps the first of equal values, and +0.0 == -0.0), as torch.max(dim=1) picks it.
__global__ __launch_bounds__(256) void regression_evaluation_kernel(const float* __restrict__ predictions, int64_t row_stride,
                                                                    int K, const float* __restrict__ bins,
                                                                    const float* __restrict__ labels, int B,
                                                                    double* __restrict__ sums) {
  __shared__ double scratch[REGRESSION_EVAL_SUMS][4];
  __shared__ float extremes[2][4];
  double v[REGRESSION_EVAL_SUMS] = {0.0, 0.0, 0.0};
  float lo = INFINITY, hi = -INFINITY;
  for (int b = (int)threadIdx.x; b < B; b += 256) {
    const float* row = predictions + (int64_t)b * row_stride;
    float prediction = row[0];
    if (bins) {
      int best = 0;
      for (int j = 1; j < K; ++j) {
        const float logit = row[j];
        if (logit > prediction) {
          prediction = logit;
          best = j;
        }
      }
      prediction = bins[best];
    }
    const float label = labels[b];
    const double d = (double)prediction - (double)label;
    v[0] += d;
    v[1] += fabs(d);
    const double square = d * d;          // rounded here; added below (no contraction in this file)
    v[2] += square;
    lo = fminf(lo, label);
    hi = fmaxf(hi, label);
  }
  block_sums_f64(v, scratch);
  block_min_max_256(lo, hi, extremes);    // (fp32 labels: their minimum and maximum are exact in fp32)
  if (threadIdx.x == 0) {
    sums[0] += v[0];
    sums[1] += v[1];
    sums[2] += v[2];
    sums[3] += (double)B;
    sums[4] = fmin(sums[4], (double)lo);
    sums[5] = fmax(sums[5], (double)hi);
  }
}

}  // namespace srgan

using namespace srgan;

extern "C" int srgan_regression_evaluation_sums(const float* predictions, int64_t row_stride, int32_t K, const float* bins,
                                                const float* labels, int32_t B, double* sums, void* stream) {
  SRGAN_REQUIRE(predictions && labels && sums, SRGAN_EINVAL, "srgan_regression_evaluation_sums: NULL pointer");
  SRGAN_REQUIRE(B >= 0 && K >= 1, SRGAN_EINVAL, "srgan_regression_evaluation_sums arguments");
  SRGAN_REQUIRE(bins || K == 1, SRGAN_EINVAL, "srgan_regression_evaluation_sums: K > 1 logits per row need the bins");
  SRGAN_REQUIRE(row_stride >= K, SRGAN_EINVAL, "srgan_regression_evaluation_sums: a row holds its K values");
  SRGAN_REQUIRE(reinterpret_cast<uintptr_t>(sums) % 8 == 0, SRGAN_EINVAL,
                "srgan_regression_evaluation_sums: sums is 8-byte aligned");
  SRGAN_REQUIRE(K <= REGRESSION_EVAL_MAX_BINS && (int64_t)B * K <= REGRESSION_EVAL_MAX_ELEMENTS, SRGAN_ERANGE,
                "srgan_regression_evaluation_sums: K within 1024 and B * K within 2^22 (one workgroup walks the batch)");
  if (B == 0) return SRGAN_OK;
  hipLaunchKernelGGL(regression_evaluation_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, predictions, row_stride,
                     (int)K, bins, labels, (int)B, sums);
  return launch_status();
}
