// launchers.h -- the host functions one translation unit defines and another calls, declared once, with the names they
// share: the launch kinds of the live profile (LaunchKind) and the operands of a convolution route (Conv3Weights, the
// batch-norm helpers).  Default arguments live here only.  (The workspace registry -- partial_workspace, workspace_index,
// workspace_register, workspace_capacity -- is in split_finish.h, the error string and the zero-fills in common.h and
// h_zero_slots in blocked16.h.)
#pragma once
#include <vector>
#include "common.h"
#include "gather_gemm.h"

namespace srgan {

// The `kind` column of srgan_profile_report, one entry per kernel family that brackets its launches.  The numbers are part
// of the report's format (bench.py and tests/contraction_cases.py print them by number): they never change.
enum LaunchKind {
  KIND_GG_DIRECT = 0,           // gather_gemm_kernels.hip: one thread per output (M <= 2)
  KIND_GG_MFMA = 1,             //   the generic MFMA tile
  KIND_CONV3X3_LDS = 2,         // conv3x3.hip (also the k4 / s2 classes)
  KIND_POINTWISE = 3,           // pointwise.hip
  KIND_CONV3X3_WGRAD = 4,       // conv3x3_wgrad.hip, single and grouped
  KIND_GG_ROWS = 5,             // gather_gemm_kernels.hip: a few output rows over a wide N
  KIND_POINTWISE_WGRAD = 6,     // pointwise_wgrad.hip, single and grouped
  // 7 is unused (a retired kernel's number; kept free so that old reports stay readable)
  KIND_POINTWISE_KSPLIT = 8,    // pointwise_ksplit.hip
  KIND_GG_DOT = 9,              // gather_gemm_kernels.hip: lanes along K
  KIND_STEM7X7_FWD = 10,        // stem7x7.hip
  KIND_STEM7X7_WGRAD = 11,
  KIND_STEM7X7_BWD_DATA = 12,
  KIND_POINTWISE_RING = 13,     // pointwise_ring.hip
  KIND_HCONV3X3 = 14,           // blocked16_conv3x3.hip: forward and data gradient
  KIND_HWGRAD3X3 = 15,          // blocked16_conv3x3_wgrad.hip
  KIND_HGEMM = 16,              // blocked16_gemm.hip
  KIND_HLINEAR_WGRAD = 17,
  KIND_HCONV4X4S2 = 18,         // blocked16_k4s2.hip
  KIND_HWGRAD4X4S2 = 19,
  KIND_BN_STATS = 20,           // batch_norm_train.hip and blocked16_batch_norm.hip: 0 FLOP, algorithmic bytes only
  KIND_BN_FWD = 21,
  KIND_BN_BWD_REDUCE = 22,
  KIND_BN_BWD_APPLY = 23,
  KIND_H_FROZEN_NORM_BWD = 24,  // blocked16_batch_norm.hip
};

// Kernels that do their FLOPs on the vector unit: everything else counts towards the profile's MFMA FLOPs.
inline bool launch_kind_is_valu(LaunchKind kind) {
  return kind == KIND_GG_DIRECT || kind == KIND_GG_ROWS || kind == KIND_GG_DOT || kind == KIND_STEM7X7_BWD_DATA;
}

// profile.hip: the bench's live event bracket around a contraction launch (-1 from begin(): profiling off).
// The _bytes form states the launch's algorithmic bytes itself (and counts its FLOPs as MFMA FLOPs whatever the kind).
int profile_bracket_begin(hipStream_t stream);
int profile_bracket_end(int slot, hipStream_t stream, int64_t M, int64_t N, int64_t K, LaunchKind kind, int bm, int bn, int split,
                        int akf = 0, int bkf = 0, int64_t b_unique = 0, int precision = 0);
int profile_bracket_end_bytes(int slot, hipStream_t stream, int64_t M, int64_t N, int64_t K, LaunchKind kind, int bm, int bn, int split,
                              double bytes, int precision);

// gather_gemm_kernels.hip: runs a group of plans that together define one output tensor of `c_rows` rows of `c_width` floats,
// `c_pitch` floats apart (dense: pitch == width).  `accumulate` adds into the existing contents; otherwise the output is
// (over)written, and zeroed first where a plan adds its K slices with atomics.  force: 0 auto, 1 direct, 2 mfma.
int gg_run_group(std::vector<GatherGemm>& plans, float* c_base, int64_t c_pitch, int64_t c_width, int64_t c_rows, int accumulate,
                 int force, hipStream_t stream);

// The four coefficient vectors of a fused norm -> relu prologue, in the order the kernels take them; and the batch-norm
// backward epilogue of a data gradient (common.h) from the same struct.
struct BnVectors { const float* v[4]; };
inline BnVectors bn_vectors(const srgan_bn_relu* bn) {
  return bn ? BnVectors{{bn->mean, bn->inv_std, bn->gamma, bn->beta}} : BnVectors{{nullptr, nullptr, nullptr, nullptr}};
}
inline BnBackwardEpilogue bn_backward_epilogue(const srgan_bn_relu* bn, const float* x, int64_t x_bs, float* g_gamma, float* g_beta,
                                               float* partial_out) {
  return BnBackwardEpilogue{x, x_bs, {bn->mean, bn->inv_std, bn->gamma, bn->beta}, g_gamma, g_beta, partial_out};
}

// conv3x3.hip: 3x3 / stride 1 / pad 1, the LDS-halo kernel.
// A stride-2 class of a k4 / s2 / p1 transposed convolution as a 2x2 sub-window of the 3x3 kernel (see conv3x3_run).
struct Conv3Placement { int32_t taps, out_plane, out_sy, out_sx, out_off; };
constexpr int CONV3_MIN_WIDTH = 7;        // narrowest plane of the kernel (the 14- and 7-wide planes at 224)
// How the kernel walks its weights: element (o, i, kh, kw) of the 3x3 window at w[base + o * so + i * si + kh * skh + kw * skw];
// `image`: the operand's weight image (weight_shadows.h), fused fp32 forms only.
struct Conv3Weights { const float* w; int32_t base, so, si, skh, skw; const float* image; };
// The forward taps of a [K, C, 3, 3] weight (o = k, i = c).
inline Conv3Weights conv3_forward_taps(const float* w, int32_t C, const float* image = nullptr) {
  return Conv3Weights{w, 0, C * 9, 9, 3, 1, image};
}
// The flipped taps of the same weight for the data gradient (o = c, i = k).
inline Conv3Weights conv3_flipped_taps(const float* w, int32_t C, const float* image = nullptr) {
  return Conv3Weights{w, 8, 9, C * 9, -3, -1, image};
}
// The stride class (a, b) of the data gradient of a [K, C, 4, 4] k4 / s2 / p1 weight: output pixel (2q + a, 2r + b) of the
// H x W gradient meets the taps kh = 3 + a - 2i, kw = 3 + b - 2j only -- a 2x2 sub-window of the 3x3 kernel, stored with
// stride 2.  Fills the class's placement.
inline Conv3Weights conv3_k4s2_class(const float* w, int32_t C, int a, int b, int32_t H, int32_t W, Conv3Placement* placement) {
  *placement = Conv3Placement{(0x01B << (3 * a)) << b, H * W, 2 * W, 2, a * W + b};
  return Conv3Weights{w, (3 + a) * 4 + (3 + b), 16, C * 16, -8, -2, nullptr};
}
int conv3x3_splits(int32_t N, int32_t CI, int32_t CO, int32_t H, int32_t W, int precision = 0);
bool conv3x3_epilogue_supported(int32_t N, int32_t CI, int32_t CO, int32_t H, int32_t W);
int64_t conv3x3_epilogue_tiles(int32_t N, int32_t CI, int32_t CO, int32_t H, int32_t W);
int conv3x3_run(const float* in, int64_t in_bs, const Conv3Weights& weights, const float* bias, float* out, int64_t out_bs, int32_t N,
                int32_t CI, int32_t CO, int32_t H, int32_t W, int accumulate, hipStream_t stream, const float* const* bn = nullptr,
                const BnBackwardEpilogue* epilogue = nullptr, int precision = 0, const Conv3Placement* placement = nullptr);

// A grouped weight-gradient launch (conv3x3_wgrad.hip, pointwise_wgrad.hip) asks for this many times the resident
// workgroups, shared out over its problems.
constexpr int GROUP_OVERSUBSCRIPTION = 4;

// conv3x3_wgrad.hip: the weight gradient of a 3x3 / stride 1 / pad 1 convolution, single and grouped.
int conv3x3_wgrad_run(const float* x, int64_t x_bs, const float* gy, int64_t gy_bs, float* gw, int32_t N, int32_t CI,
                      int32_t CO, int32_t H, int32_t W, int accumulate, hipStream_t stream, const float* const* bn = nullptr,
                      int precision = 0);
int conv3x3_wgrad_group_plan(int64_t x_off, int64_t x_bs, int64_t gy_off, int64_t gy_bs, float* gw, int64_t gw_off, int32_t N, int32_t CI,
                             int32_t CO, int32_t H, int32_t W, const float* const* bn, int32_t group, int64_t partial_offset, void* job_out,
                             int32_t* grid_x, int32_t* grid_y, int32_t* ragged, int64_t* partial_floats);
int conv3x3_wgrad_group_run(const void* jobs, int32_t count, int32_t grid_x, int32_t grid_y, int32_t ragged,
                            const float* x_base, const float* gy_base, float* gw_base, int64_t flops_mn, int64_t pixels,
                            int64_t elements, int64_t partial_floats, hipStream_t stream);

// pointwise.hip: 1x1 / stride 1, the register-streamed kernel, and the reduction of the deferred batch-norm parameter sums.
int pointwise_run(const float* in, int64_t in_bs, const float* w, int32_t w_so, int32_t w_si, const float* bias, float* out,
                  int64_t out_bs, int32_t N, int32_t CI, int32_t CO, int32_t HW, int accumulate, hipStream_t stream,
                  const float* const* bn = nullptr, const BnBackwardEpilogue* epilogue = nullptr,
                  int* plan_only_split = nullptr);
int64_t pointwise_epilogue_tiles(int32_t N, int32_t HW);
void bn_partial_reduce_run(const float* partial, int tiles, int CO, const float* inv_std, float* g_gamma, float* g_beta,
                           hipStream_t stream);
int bn_partial_reduce_batched_run(const srgan_bn_reduce_job* jobs, int count, int max_channels, int max_tiles,
                                  const float* scratch, hipStream_t stream);

// pointwise_ring.hip: the pointwise convolution with both operands staged by LDS-DMA.
bool pointwise_ring_eligible(const float* in, int64_t in_bs, const float* w, int32_t w_so, int32_t w_si, const float* bias,
                             const float* out, int64_t out_bs, int32_t N, int32_t CI, int32_t CO, int32_t HW, bool fused_pro,
                             const BnBackwardEpilogue* epilogue, int* tile_pixels);
int pointwise_ring_run(const float* in, int64_t in_bs, const float* w, int32_t w_so, int32_t w_si, float* out, int64_t out_bs,
                       int32_t N, int32_t CI, int32_t CO, int32_t HW, int accumulate, hipStream_t stream,
                       const float* const* bn, const BnBackwardEpilogue* epilogue, float* epi_partial, int32_t epi_cols,
                       int tile_pixels, int32_t* rows_done);
// Two consecutive dense layers' fused data gradients in one pass over their common rows (pointwise_ring.hip): layer A's
// rows [row0, CO) on their own (the strip), then A and B together on B's rows (the pair).
bool pointwise_ring_pair_eligible(const float* in_a, const float* in_b, int64_t in_bs, const float* w_a, const float* w_b,
                                  const float* x, int64_t x_bs, const float* out, int64_t out_bs, int32_t N, int32_t CI,
                                  int32_t rows_a, int32_t rows_b, int32_t HW);
int pointwise_ring_strip_run(const float* in, int64_t in_bs, const float* w, float* out, int64_t out_bs, int32_t N, int32_t CI,
                             int32_t CO, int32_t row0, int32_t HW, const BnBackwardEpilogue& epilogue, hipStream_t stream);
int pointwise_ring_pair_run(const float* in_a, const float* w_a, int32_t rows_a, const BnBackwardEpilogue& epilogue_a,
                            const float* in_b, const float* w_b, int32_t rows_b, const BnBackwardEpilogue& epilogue_b,
                            int64_t in_bs, float* out, int64_t out_bs, int32_t N, int32_t CI, int32_t HW, hipStream_t stream);

// pointwise_ksplit.hip: the pointwise convolution for few pixels and many input channels (K split over the grid).
bool pointwise_ksplit_wanted(int32_t N, int32_t K, int32_t M, int32_t HW, bool fused_bn);
int pointwise_ksplit_run(const float* in, int64_t in_bs, const float* w, const float* bias, float* out, int64_t out_bs,
                         int32_t N, int32_t K, int32_t M, int32_t HW, int accumulate, hipStream_t stream,
                         const float* const* bn);

// pointwise_wgrad.hip: the weight gradient of a 1x1 / stride 1 convolution, single and grouped.
bool pointwise_wgrad_enabled();
int pointwise_wgrad_run(const float* x, int64_t x_bs, const float* gy, int64_t gy_bs, float* gw, int32_t N, int32_t CI,
                        int32_t CO, int32_t HW, int accumulate, hipStream_t stream, const float* const* bn = nullptr);
int pointwise_wgrad_group_plan(int64_t x_off, int64_t x_bs, int64_t gy_off, int64_t gy_bs, float* gw, int64_t gw_off, int32_t N, int32_t CI,
                               int32_t CO, int32_t HW, const float* const* bn, int32_t group, int64_t group_weights, int64_t partial_offset,
                               void* job_out, int32_t* grid_x, int32_t* grid_y, int32_t* ragged, int64_t* partial_floats);
int pointwise_wgrad_group_run(const void* jobs, int32_t count, int32_t grid_x, int32_t grid_y, int32_t ragged, int32_t fused_bn,
                              const float* x_base, const float* gy_base, float* gw_base, int64_t flops_mn, int64_t pixels,
                              int64_t elements, int64_t partial_floats, hipStream_t stream);

// batch_norm_train.hip: training-mode batch normalisation (batch statistics), fp32 NCHW.  `sums` = [2][C]: sum g', sum g' * xhat.
int bn_train_stats_run(const float* x, float* mean, float* inv_std, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, float momentum, float eps, int32_t N, int32_t C, int64_t HW,
                       hipStream_t stream);
int bn_train_fwd_run(const float* x, const float* mean, const float* inv_std, const float* gamma, const float* beta, float slope,
                     float* y, int32_t N, int32_t C, int64_t HW, hipStream_t stream);
int bn_train_bwd_reduce_run(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                            const float* beta, float slope, float* sums, float* g_gamma, float* g_beta, int32_t N, int32_t C,
                            int64_t HW, hipStream_t stream);
int bn_train_bwd_apply_run(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                           const float* beta, float slope, const float* sums, float* gx, int32_t N, int32_t C, int64_t HW,
                           hipStream_t stream);

// blocked16_batch_norm.hip: the backward of a norm with given statistics on blocked tensors (contract: srgan_h_frozen_norm_bwd).
int h_frozen_norm_bwd_run(const void* s, const void* x, const float* mean, const float* inv_std, const float* gamma, const void* ref,
                          float slope, void* gx, float* g_gamma, float* g_beta, int32_t N, int32_t C, int64_t HW, int32_t dtype,
                          hipStream_t stream);

// stem7x7.hip: the DenseNet stem's 7x7 / stride 2 convolution, all three passes.
bool stem7x7_geometry(int32_t C, int32_t K, int32_t R, int32_t S, int32_t sh, int32_t sw, int32_t ph, int32_t pw);
int stem7x7_fwd_run(const float* x, int64_t x_bs, const float* w, float* y, int64_t y_bs, int32_t N, int32_t H, int32_t W,
                    int32_t K, int32_t OH, int32_t OW, hipStream_t stream);
int stem7x7_wgrad_run(const float* x, int64_t x_bs, const float* gy, int64_t gy_bs, float* gw, int32_t N, int32_t H, int32_t W,
                      int32_t K, int32_t OH, int32_t OW, int accumulate, hipStream_t stream);
int stem7x7_bwd_data_run(const float* gy, int64_t gy_bs, const float* w, float* gx, int64_t gx_bs, int32_t N, int32_t H,
                         int32_t W, int32_t K, int32_t OH, int32_t OW, hipStream_t stream);


// image_summaries.hip: the image grid and the crowd map heatmaps of a summary step (contracts: srgan_image_grid,
// srgan_density_heatmaps; arguments already checked).
int image_grid_run(const float* images, int32_t N, int32_t C, int32_t H, int32_t W, int32_t nrow, int32_t padding, float pad_value,
                   int32_t normalize, float low, float high, float* out, hipStream_t stream);
int density_heatmaps_run(const float* labels, const float* predicted, int32_t B, int32_t M, int32_t h, int32_t w, int32_t P,
                         const float* lut, int32_t lut_entries, float* tiles, int64_t tile_stride, float* ranges,
                         hipStream_t stream);

// distribution_summaries.hip: the Wasserstein distance, the kernel-density curves and the line chart of a coefficient summary
// step (contracts: srgan_wasserstein_1d, srgan_kde_curves, srgan_curve_frame; arguments already checked).
int wasserstein_run(const float* u, int32_t n, const float* v, int32_t m, float* out, hipStream_t stream);
int kde_curves_run(const float* samples, const int32_t* offsets, int32_t C, int32_t G, float factor, float cut, float* support,
                   float* density, float* stats, hipStream_t stream);
int curve_frame_run(const float* vertices, const int32_t* offsets, int32_t C, const float* colours, const float* widths, int32_t H,
                    int32_t W, float x_lo, float x_hi, float y_lo, float y_hi, const float* background, const float* grid_colour,
                    const float* x_ticks, int32_t n_x, const float* y_ticks, int32_t n_y, float* out, hipStream_t stream);

}  // namespace srgan
