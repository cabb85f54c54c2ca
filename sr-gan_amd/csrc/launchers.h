// launchers.h -- the host functions one translation unit defines and another calls, declared once.  Default arguments
// live here only.  (The workspace registry -- partial_workspace, workspace_index -- is in split_finish.h, the zero-fills
// in common.h and h_zero_slots in blocked16.h.)
#pragma once
#include "common.h"

namespace srgan {

// gather_gemm_kernels.hip: the bench's live event bracket around a contraction launch (-1 from begin(): profiling off).
// The _bytes form states the launch's algorithmic bytes itself.
int profile_bracket_begin(hipStream_t stream);
int profile_bracket_end(int slot, hipStream_t stream, int64_t M, int64_t N, int64_t K, int kind, int bm, int bn, int split,
                        int akf = 0, int bkf = 0, int64_t b_unique = 0, int precision = 0);
int profile_bracket_end_bytes(int slot, hipStream_t stream, int64_t M, int64_t N, int64_t K, int kind, int bm, int bn, int split,
                              double bytes, int precision);

// conv3x3.hip: 3x3 / stride 1 / pad 1, the LDS-halo kernel.
// A stride-2 class of a k4 / s2 / p1 transposed convolution as a 2x2 sub-window of the 3x3 kernel (see conv3x3_run).
struct Conv3Placement { int32_t taps, out_plane, out_sy, out_sx, out_off; };
int conv3x3_splits(int32_t N, int32_t CI, int32_t CO, int32_t H, int32_t W, int precision = 0);
bool conv3x3_epilogue_supported(int32_t N, int32_t CI, int32_t CO, int32_t H, int32_t W);
int64_t conv3x3_epilogue_tiles(int32_t N, int32_t CI, int32_t CO, int32_t H, int32_t W);
int conv3x3_run(const float* in, int64_t in_bs, const float* w, int32_t w_base, int32_t w_so, int32_t w_si, int32_t w_skh,
                int32_t w_skw, const float* bias, float* out, int64_t out_bs, int32_t N, int32_t CI, int32_t CO, int32_t H,
                int32_t W, int accumulate, hipStream_t stream, const float* const* bn = nullptr,
                const BnBackwardEpilogue* epilogue = nullptr, int precision = 0, const Conv3Placement* placement = nullptr,
                const float* w_image = nullptr);      // w_image: the operand's weight image (blocked16.h), fused fp32 forms only

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
