/* srgan_hip.h -- C ABI of libsrgan_hip.so: the MI355X (gfx950) compute layer of the SRGAN/SGAN training step.
 *
 * The reference (golmschenk/sr-gan) is pure Python on PyTorch and has NO FFI of its own: its
 * arithmetic is reached through torch.nn / torch.nn.functional / torch.optim call sites.  Each entry point
 * below therefore cites the reference call site(s) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns int: 0 = ok, < 0 = argument / shape error (-1 invalid, -2 unsupported,
 *     -3 out of range), > 0 = hipError_t.  srgan_last_error() returns a thread-local message.
 *   - pointers are DEVICE pointers to contiguous fp32 (int32 for arg-max), borrowed for the call only;
 *     the library never allocates or frees device memory.  The one block it keeps between calls is the split-K
 *     workspace the CALLER registers per (device, stream) with srgan_set_workspace (below); a contraction that
 *     needs it on a stream without one fails with -1 and a message.  Activations are NCHW, conv weights
 *     [K, C, R, S], transposed-conv weights [Cin, Cout, R, S] (torch layouts).
 *   - alignment: any 4-byte-aligned fp32 pointer is accepted (a view may start at any element of a buffer) unless an
 *     entry point states otherwise (srgan_pack_bf16 / srgan_unpack_bf16, the fused pooling calls, the workspace);
 *     16-byte alignment of every pointer of a call selects the 16-byte vector paths of the streaming kernels, anything
 *     else their single-float loops, with the same results.
 *   - thread safety: calls may come from several host threads (the registry and the profile state are locked,
 *     srgan_last_error is thread-local); two threads must not launch on the SAME stream with the same workspace
 *     concurrently, as with any stream-ordered resource.
 *   - collectives: thin RCCL entry points (srgan_comm_*, srgan_all_reduce_sum, srgan_reduce_scatter_sum,
 *     srgan_all_gather, srgan_broadcast, at the end of this file) carry the data-parallel exchange for a caller without
 *     torch.distributed; they are the Python host's default device transport as well (sr-gan_amd/parallel.py: torch.distributed
 *     keeps the rendezvous and the host-side control messages; `SRGAN_ABI_COLLECTIVES=0` puts the device collectives back on
 *     torch.distributed's "nccl" backend = the same RCCL over xGMI), see INTEGRATION.md.
 *   - `stream` is a hipStream_t (NULL = default stream); every call is asynchronous on it.
 *   - `accumulate` != 0 adds into the existing output (gradient accumulation across the four
 *     discriminator backward passes, reference srgan.py:280-295) instead of overwriting it.
 *   - tensors are limited to < 2^31 elements.
 *   - `force_kernel`: 0 = automatic choice, 1 = direct VALU form, 2 = MFMA form (used by tests to
 *     cross-check the two implementations).
 */
#ifndef SRGAN_HIP_H
#define SRGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int srgan_version(void);               /* 110 = ABI 1.1 (see "ABI history" in INTEGRATION.md; 100 = ABI 1.0) */
/* 16 hex digits: sha256 over the kernel sources this library was compiled from (sr-gan_amd/_build.py source_id()).
 * The Python loader refuses a library whose id differs from the sources next to it: a stale prebuilt .so must not
 * silently run old kernels under new parity tests. */
const char* srgan_build_id(void);
const char* srgan_last_error(void);

/* ---- capabilities, caller-owned workspace -------------------------------------------------------------------
 * srgan_capabilities fills the struct below (pass sizeof(srgan_capabilities_t)); SRGAN_DTYPE_* / SRGAN_FEATURE_*
 * are bit masks.  Reference analogue: none (torch picks kernels internally); SURVEY.md 8b asks for the query. */
#define SRGAN_DTYPE_F32 0x1u            /* fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32): the parity path */
#define SRGAN_DTYPE_BF16 0x2u           /* bf16 MFMA operands, fp32 accumulate (v_mfma_f32_32x32x16_bf16) */
#define SRGAN_DTYPE_F16 0x4u            /* fp16 MFMA operands, fp32 accumulate (v_mfma_f32_32x32x16_f16) */
#define SRGAN_FEATURE_FUSED_BNRELU 0x1u /* norm -> relu -> conv evaluated inside the convolution kernels */
#define SRGAN_FEATURE_SPLITK_WORKSPACE 0x2u
#define SRGAN_FEATURE_LIVE_PROFILE 0x4u
#define SRGAN_FEATURE_BLOCKED16 0x8u    /* ABI 1.1: the srgan_h_* entry points (16-bit storage in the blocked layout) */
#define SRGAN_FEATURE_BATCHED_SHADOWS 0x10u /* ABI 1.1, additive: srgan_h_pack_job_matrix / _bias_rows (every shadow kind in
                                                srgan_h_pack_batched) */
#define SRGAN_FEATURE_CROWD_FULL_IMAGE 0x20u /* ABI 1.1, additive: srgan_crowd_extract_windows / _resize_bilinear /
                                                 _blend_windows (full-image crowd inference on the device) */
#define SRGAN_FEATURE_IMAGE_BATCHES 0x40u /* ABI 1.1, additive: srgan_image_batch_gather (training batches gathered on the
                                             device from a resident database of frames) */
#define SRGAN_FEATURE_BATCH_NORM_TRAIN 0x80u /* ABI 1.1, additive: srgan_batch_norm_train_* (batch statistics, fp32 NCHW) */
#define SRGAN_FEATURE_BLOCKED_BATCH_NORM 0x100u /* ABI 1.1, additive: srgan_h_batch_norm_* (batch statistics on blocked
                                                  tensors, dtype 0 / 1 / 2) */
#define SRGAN_FEATURE_BLOCKED_FROZEN_NORM 0x200u /* ABI 1.1, additive: srgan_h_frozen_norm_bwd (the backward, to first and
                                                   second order, of a norm with given statistics on blocked tensors) */
#define SRGAN_FEATURE_DEVICE_DRAWS 0x400u /* ABI 1.1, additive: srgan_random_fill / srgan_random_advance (an iteration's random
                                             tensors from a counter-based generator on the device) */
#define SRGAN_FEATURE_IMAGE_SUMMARIES 0x800u /* ABI 1.1, additive: srgan_image_grid / srgan_density_heatmaps (a summary step's
                                               image grids and crowd map heatmaps built on the device) */
#define SRGAN_FEATURE_DISTRIBUTION_SUMMARIES 0x1000u /* ABI 1.1, additive: srgan_wasserstein_1d / srgan_kde_curves /
                                                        srgan_curve_frame (the coefficient application's distribution summaries
                                                        built on the device) */
#define SRGAN_FEATURE_CONV3X3_WEIGHT_IMAGE 0x2000u /* ABI 1.1, additive: srgan_conv3x3_image_floats / srgan_h_pack_conv3x3_image /
                                                      srgan_h_pack_job_conv3x3_image and the *_image forms of the fused fp32 3x3
                                                      calls (weights staged from a per-step packed image) */
#define SRGAN_FEATURE_DROPOUT 0x4000u /* ABI 1.1, additive: srgan_dropout (inverted dropout whose mask is regenerated from the
                                         device draws' counter-based stream, never stored) */
#define SRGAN_FEATURE_FEATURE_LOSSES 0x8000u /* ABI 1.1, additive: srgan_feature_corrcoef_l1_fwd / _bwd / _scratch_bytes (the
                                                correlation-matrix feature loss, fused) and unary ops 20-22 (acos, clamp,
                                                in_range) */
#define SRGAN_FEATURE_CROWD_EVALUATION 0x10000u /* ABI 1.1, additive: srgan_crowd_evaluation_sums / _scratch_bytes (the sums
                                                   behind the crowd evaluation scalars, from batches resident on the device) */
#define SRGAN_FEATURE_SUMMARY_HISTOGRAM 0x20000u /* ABI 1.1, additive: srgan_tensor_histogram (the histogram record of a device
                                                    tensor: moments, edges and counts of its finite elements) */
#define SRGAN_FEATURE_REGRESSION_EVALUATION 0x40000u /* ABI 1.1, additive: srgan_regression_evaluation_sums (the sums behind
                                                        the age / driving evaluation scalars, from a batch on the device) */
#define SRGAN_FEATURE_CROWD_PATCH_DRAWS 0x80000u /* ABI 1.1, additive: srgan_crowd_draw_patches /
                                                    srgan_crowd_extract_patches_indexed (the crowd loader's patch positions drawn
                                                    on the device; the cut over per-scene tables) */
#define SRGAN_FEATURE_EPOCH_ORDER 0x100000u /* ABI 1.1, additive: srgan_epoch_order / srgan_argsort_u64 /
                                               srgan_epoch_batch_indices (the resident image loaders' epoch order drawn on
                                               the device; a batch's index table cut from it by the step held in a state) */
typedef struct srgan_capabilities_t {
  int32_t abi_version;          /* = srgan_version() */
  int32_t struct_bytes;         /* sizeof(srgan_capabilities_t) as the library was built */
  char arch[16];                /* "gfx950" */
  uint32_t dtypes;              /* SRGAN_DTYPE_* */
  uint32_t features;            /* SRGAN_FEATURE_* */
  int64_t workspace_bytes;      /* = srgan_workspace_bytes() */
  int64_t max_tensor_elements;  /* 2^31 - 1 */
} srgan_capabilities_t;
int srgan_capabilities(srgan_capabilities_t* out, int32_t out_bytes);
/* Every sum that several workgroups of one launch share -- the K slices of a split contraction, the workers of a weight
 * gradient, per-channel parameter sums, per-example loss sums -- goes through a workspace: the workgroups leave their
 * partial tiles there and the last one (or a second launch) adds them in a fixed order (round 5: no fp32 atomics on data,
 * bit-reproducible results; round 2 used it only for tiny split-K outputs).  The caller owns that memory: register one
 * block of >= srgan_workspace_bytes() bytes (256 MiB; 16-byte aligned, device memory) per (current device, stream) before
 * the first launch on that stream; NULL unregisters.  Launches on one stream are ordered, so one block per stream is
 * enough.  A stream without a workspace still computes: the sums then meet through fp32 atomics. */
int64_t srgan_workspace_bytes(void);
int srgan_set_workspace(void* workspace, int64_t bytes, void* stream);
/* Round 5: a contraction that splits K over several workgroups (few output tiles: the small planes) finishes in a FIXED
 * order on a stream that has a workspace: every slice leaves its partial tile there, the tile's last workgroup adds the
 * slices in slice order and stores -- one launch, no zero-filled output, bit-identical from run to run (the reference's CPU
 * path is repeatable; fp32 atomics are not).  Returns 1 when launches on `stream` do so, 0 when they fall back to fp32
 * atomics into a zero-filled output (no workspace registered, or SRGAN_ATOMIC_SPLIT=1). */
int srgan_split_is_ordered(void* stream);

/* ---- convolution ------------------------------------------------------------------------------------------
 * Geometry of y = conv2d(x, w): x [N,C,H,W], w [K,C,R,S], y [N,K,OH,OW].  Batch strides (elements) allow a
 * channel-slice view of a wider buffer; 0 means dense. */
typedef struct srgan_conv_desc {
  int32_t N, C, H, W;
  int32_t K, R, S;
  int32_t stride_h, stride_w, pad_h, pad_w;
  int32_t OH, OW;
  int64_t x_batch_stride, y_batch_stride;
  int32_t compute_dtype;   /* SRGAN_COMPUTE_*: the MFMA operand type of this pass */
} srgan_conv_desc;

/* Mixed precision (BASELINE.json configs 2 and 5: "bf16", "fp16 with fp32 GP"; the reference itself is fp32-only).
 * Tensors stay fp32 in HBM -- activations, weights (the master copy), gradients, Adam moments -- and accumulation is
 * fp32; with SRGAN_COMPUTE_BF16 / _F16 the two operands of every contraction are rounded to bf16 / fp16 when the MFMA
 * fragments are formed (v_mfma_f32_32x32x16_bf16 / _f16, 16x the fp32 matrix rate).  The choice is per call, so a
 * caller keeps e.g. the gradient-penalty chain in SRGAN_COMPUTE_F32 while the rest of the step runs in fp16.  The
 * specialised fp32 kernels (fused batch-norm forms included: srgan_conv2d_bnrelu_supported then returns 0) are not
 * used in these modes; fp32 remains the parity path (1e-3), the mixed modes are tested against it with their own,
 * stated tolerances (tests/test_mixed_precision_gpu.py). */
#define SRGAN_COMPUTE_F32 0
#define SRGAN_COMPUTE_BF16 1
#define SRGAN_COMPUTE_F16 2

/* y = conv2d(x, w) + bias[k] (bias may be NULL).
 * Replaces torch.nn.Conv2d.forward at reference crowd/models.py:340-345,369,770-775,1072,1134-1135;
 * age/models.py:24,61-65; age/vgg.py:78. */
int srgan_conv2d_fwd(const srgan_conv_desc* desc, const float* x, const float* w, const float* bias, float* y,
                     int force_kernel, void* stream);

/* gx = d(conv2d)/dx applied to gy, + bias[c] (bias may be NULL).  Also IS the forward of
 * torch.nn.ConvTranspose2d (weight [Cin=K, Cout=C, R, S], input = gy, output = gx): reference
 * age/models.py:16-21,37-41, crowd/models.py:132-136,768-769.  As a backward pass it replaces autograd's
 * conv backward-to-input reached from reference srgan.py:280-295,304 and the create_graph pass of
 * srgan.py:368-370. */
int srgan_conv2d_bwd_data(const srgan_conv_desc* desc, const float* gy, const float* w, const float* bias, float* gx,
                          int accumulate, int force_kernel, void* stream);

/* gw = d(conv2d)/dw applied to gy (reduction over batch and output pixels). */
int srgan_conv2d_bwd_weight(const srgan_conv_desc* desc, const float* x, const float* gy, float* gw, int accumulate,
                            int force_kernel, void* stream);

/* Convolutions whose input is relu(batch_norm_eval(x)) evaluated ON THE FLY inside the kernel (the DenseNet
 * norm -> relu -> conv triples, reference crowd/models.py:338-345): the normalised tensor is never written to HBM.
 * Zero padding applies to the activated tensor, as in the reference sequence.  Supported geometries: 1x1 / stride 1 /
 * unpadded on images of a multiple of 32 pixels, and 3x3 / stride 1 / pad 1 with W >= 16 (weight gradient: W % 4 ==
 * 0, C >= 32; forward: C <= 512); srgan_conv2d_bnrelu_supported(desc, pass) (pass 0 forward, 1 data gradient,
 * 2 weight gradient) returns 1 when the fused form exists, otherwise the caller materialises the activation
 * (srgan_chan_affine_act) and uses the plain entry points.  Results are identical to that two-step form up to
 * summation order.
 * srgan_conv2d_bwd_data_bnrelu is the backward of the triple w.r.t. x in one kernel: gx (=, +=)
 * conv_bwd_data(gy, w) * [batch_norm(x) > 0] * inv_std * gamma, with x and gx sharing desc->x_batch_stride (gx may be
 * a channel-slice view that is accumulated into), plus -- when g_gamma / g_beta are given (both or neither) -- the
 * batch-norm parameter gradients accumulated into them.  Equals srgan_conv2d_bwd_data followed by srgan_bn_act_bwd. */
typedef struct srgan_bn_relu { const float* mean; const float* inv_std; const float* gamma; const float* beta; } srgan_bn_relu;
int srgan_conv2d_bnrelu_supported(const srgan_conv_desc* desc, int pass);
int srgan_conv2d_fwd_bnrelu(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* w,
                            const float* bias, float* y, void* stream);
/* Small problems split K over the grid and add their partial results with fp32 atomics into a zeroed y: one extra
 * zero-fill launch per convolution.  srgan_conv2d_fwd_bnrelu_splits(desc) tells how many K splits the forward of this
 * geometry uses (1: plain stores; -1: no fused form); a caller that hands over y ALREADY ZERO (one fill for the outputs
 * of a whole dense block) calls srgan_conv2d_fwd_bnrelu_into_zeros, which skips the per-call zero-fill. */
int srgan_conv2d_fwd_bnrelu_splits(const srgan_conv_desc* desc);
int srgan_conv2d_fwd_bnrelu_into_zeros(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* w,
                                       const float* bias, float* y, void* stream);
int srgan_conv2d_bwd_data_bnrelu(const srgan_conv_desc* desc, const float* gy, const float* w, const srgan_bn_relu* bn,
                                 const float* x, float* gx, float* g_gamma, float* g_beta, int accumulate, void* stream);
int srgan_conv2d_bwd_weight_bnrelu(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* gy,
                                   float* gw, int accumulate, void* stream);
/* Deferred parameter gradients of srgan_conv2d_bwd_data_bnrelu: the per-workgroup sums behind g_gamma / g_beta are left in
 * a caller-owned region of 2 * srgan_conv2d_bwd_data_bnrelu_tiles(desc) * C floats instead of being reduced by a small
 * kernel after EVERY convolution (597 launches per training step); one srgan_bn_partial_reduce_batched call then
 * reduces the regions of many convolutions (a DenseNet block's backward pass: two per layer).  `jobs_device` is a table in
 * DEVICE memory; partial_offset is in floats from `scratch`.  Offsets and pointers are stable from step to step, so the
 * caller builds the table once per block. */
typedef struct srgan_bn_reduce_job {
  int64_t partial_offset;
  int32_t tiles, channels;
  const float* inv_std;
  float* g_gamma;
  float* g_beta;
} srgan_bn_reduce_job;
int64_t srgan_conv2d_bwd_data_bnrelu_tiles(const srgan_conv_desc* desc);
int srgan_conv2d_bwd_data_bnrelu_partials(const srgan_conv_desc* desc, const float* gy, const float* w, const srgan_bn_relu* bn,
                                          const float* x, float* gx, float* partials, int accumulate, void* stream);
int srgan_bn_partial_reduce_batched(const srgan_bn_reduce_job* jobs_device, int32_t count, int32_t max_channels, int32_t max_tiles,
                                    const float* scratch, void* stream);
/* Two consecutive layers of a dense block, A (desc_a: C rows) and B (desc_b: C - 32 rows, otherwise the same descriptor),
 * accumulate their 1x1 data gradients (srgan_conv2d_bwd_data_bnrelu_partials with accumulate = 1, same x and gx) into
 * almost the same rows.  Where srgan_conv2d_bwd_data_bnrelu_pair_supported answers 1 (both on the LDS-DMA kernel, K = 128,
 * B's C >= 128, H * W a multiple of 128, N * H * W >= 16384, equal batch strides) the two calls can be replaced by
 *   srgan_conv2d_bwd_data_bnrelu_strip: A's contribution to its last 32 rows [C - 32, C), which B's 3x3 data gradient
 *     reads (issued where A's call stood), and
 *   srgan_conv2d_bwd_data_bnrelu_pair: A's and then B's contribution to the rows [0, C - 32) in ONE pass over x and gx
 *     (issued where B's call stood),
 * with BIT-IDENTICAL gx and partial-sum regions (partials_a / partials_b: each layer's own region as above; both NULL =
 * no parameter sums).  Pointers the kernel cannot take (16-byte alignment): SRGAN_EUNSUPPORTED. */
int srgan_conv2d_bwd_data_bnrelu_pair_supported(const srgan_conv_desc* desc_a, const srgan_conv_desc* desc_b);
int srgan_conv2d_bwd_data_bnrelu_strip(const srgan_conv_desc* desc_a, const srgan_conv_desc* desc_b, const float* gy, const float* w,
                                       const srgan_bn_relu* bn, const float* x, float* gx, float* partials, void* stream);
int srgan_conv2d_bwd_data_bnrelu_pair(const srgan_conv_desc* desc_a, const srgan_conv_desc* desc_b, const float* gy_a,
                                      const float* w_a, const srgan_bn_relu* bn_a, float* partials_a, const float* gy_b,
                                      const float* w_b, const srgan_bn_relu* bn_b, float* partials_b, const float* x, float* gx,
                                      void* stream);
/* The 3x3 / stride 1 / padding 1 cases of the three calls above with the operand's WEIGHT IMAGE next to w
 * (SRGAN_FEATURE_CONV3X3_WEIGHT_IMAGE): fp32, 16-byte aligned, srgan_conv3x3_image_floats(CI, CO) floats,
 *   image[(ci * 9 + tap) * CO_pad + o], CO_pad = CO rounded up to 64, ci up to CI rounded up to 8, zeros where o >= CO or ci >= CI,
 * with (CO, CI, tap) = (K, C, kh * 3 + kw) of w[K][C][3][3] for the forward ("forward" image) and (C, K, mirrored tap) for the
 * data gradient ("transposed" image): the elements the kernel otherwise gathers from w in every workgroup.  The image must hold
 * the current w (srgan_h_pack_conv3x3_image, or its job in srgan_h_pack_batched behind the optimizer update).  Same plans, tiles
 * and splits as the calls above and BIT-IDENTICAL results; other geometries: SRGAN_EUNSUPPORTED.  SRGAN_NO_CONV3_IMAGE=1 in the
 * environment (read once per process) makes them ignore the image. */
int64_t srgan_conv3x3_image_floats(int32_t CI, int32_t CO);
int srgan_conv2d_fwd_bnrelu_image(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* w,
                                  const float* image, const float* bias, float* y, void* stream);
int srgan_conv2d_bwd_data_bnrelu_image(const srgan_conv_desc* desc, const float* gy, const float* w, const float* image,
                                       const srgan_bn_relu* bn, const float* x, float* gx, float* g_gamma, float* g_beta,
                                       int accumulate, void* stream);
int srgan_conv2d_bwd_data_bnrelu_partials_image(const srgan_conv_desc* desc, const float* gy, const float* w, const float* image,
                                                const srgan_bn_relu* bn, const float* x, float* gx, float* partials,
                                                int accumulate, void* stream);

/* Grouped form of srgan_conv2d_bwd_weight_bnrelu: MANY independent weight gradients (all the 1x1, or all the 3x3,
 * convolutions of a dense block's backward: reference crowd/models.py:335-353 through loss.backward()) in ONE launch.
 * srgan_wgrad_group_plan fills one 128-byte table slot per problem on the host -- x / gy are ELEMENT OFFSETS from two base
 * pointers given at launch time, gw and the batch-norm vectors are absolute, the gradient is ACCUMULATED into gw -- and
 * returns the grid extent the problem needs and, in *ragged, the kernel variant the slot was planned for as a bit (3x3: 0 / 1 =
 * the ragged variant; 1x1: 1 = the LDS-staged 128 x 128 tiles, 2 = the register-streamed 64 x 64 tiles, 4 = their ragged
 * variant); the caller uploads the table once (it does not change between steps when the offsets are relative to per-step
 * buffers) and launches with the maxima of the grid extents and the OR of the variants over the group (a group whose slots
 * were planned for both 1x1 forms is served by one launch each).  All problems of a group share the plane size; group_size
 * (the number of problems that will be launched together) lets the plan give each problem fewer workgroups of its own, and
 * group_weights (the sum of CO x CI x taps over the group, 0 = not known) lets it share them out by work instead of in equal
 * parts (the staged 1x1 form: the same K range per worker whatever the problem's width).  bn == NULL plans the plain weight gradient
 * (x used as is; srgan_wgrad_group_run with fused_bn = 0): the double backward's gradients w.r.t. the scaled weights.
 * gw == NULL: the gradient goes to gw_base + gw_offset of the launch (a per-step buffer) instead of a fixed address.  sum_co_ci_taps / pixels / operand_elements only feed
 * the profile (logical FLOPs = 2 * sum_co_ci_taps * pixels; elements of x and gy read once).
 * Round 5, the ORDERED form: the K-slice workers of a problem no longer meet in gw through fp32 atomics -- each keeps its
 * partial tile in the stream's workspace and a second launch adds them in slice order (bit-identical from run to run).  The
 * caller lays the problems' partial regions out back to back: partial_offset = the sum of the *partial_floats the earlier
 * problems of the group returned, and srgan_wgrad_group_run gets the group's total (0, a total beyond the workspace, or no
 * workspace on the stream: fp32 atomics as before). */
int srgan_wgrad_group_plan(const srgan_conv_desc* desc, const srgan_bn_relu* bn, int64_t x_offset, int64_t gy_offset, float* gw,
                           int64_t gw_offset, int32_t group_size, int64_t group_weights, int64_t partial_offset, void* job,
                           int32_t* grid_x, int32_t* grid_y, int32_t* ragged, int64_t* partial_floats);
int srgan_wgrad_group_run(const void* jobs, int32_t count, int32_t kernel_size, int32_t grid_x, int32_t grid_y, int32_t ragged,
                          int32_t fused_bn, const float* x_base, const float* gy_base, float* gw_base, int64_t sum_co_ci_taps,
                          int64_t pixels, int64_t operand_elements, int64_t partial_floats, void* stream);

/* ---- strided GEMM  C[i*sci + j*scj] (=,+=) sum_k A[i*sai + k*sak] * B[k*sbk + j*sbj] + bias ----------------
 * C must be a dense M x N matrix (row- or column-major).  bias is indexed by row i, or by column j when
 * bias_on_columns != 0.  Replaces torch.nn.Linear forward/backward at reference coefficient/models.py:17-27,
 * 36-49,80-92 and age/vgg.py:33-41. */
int srgan_gemm_f32(int32_t M, int32_t N, int32_t K, const float* A, int64_t sai, int64_t sak, const float* B,
                   int64_t sbk, int64_t sbj, float* C, int64_t sci, int64_t scj, const float* bias,
                   int32_t bias_on_columns, int accumulate, int force_kernel, void* stream);
/* The same with the MFMA operand type chosen per call (compute_dtype = SRGAN_COMPUTE_*; srgan_gemm_f32 = fp32). */
int srgan_gemm(int32_t M, int32_t N, int32_t K, const float* A, int64_t sai, int64_t sak, const float* B,
               int64_t sbk, int64_t sbj, float* C, int64_t sci, int64_t scj, const float* bias,
               int32_t bias_on_columns, int accumulate, int force_kernel, int compute_dtype, void* stream);

/* ---- elementwise ------------------------------------------------------------------------------------------
 * Unary op codes: 0 copy, 1 neg, 2 abs, 3 sign, 4 sqrt, 5 exp, 6 log, 7 log1p, 8 square, 9 reciprocal, 10 tanh,
 * 11 relu, 12 step (x > 0), 13 affine (p0*x + p1), 14 pow (x^p0), 15 leaky_relu (slope p0), 16 sigmoid,
 * 17 softplus, 18 one_minus_square, 19 rsqrt, 20 acos, 21 clamp (to [p0, p1]; by comparisons, so a NaN stays a NaN as in
 * torch.clamp), 22 in_range (1 where p0 <= x <= p1, else 0 -- NaN included: the gradient mask of clamp, edges inclusive).
 * Binary op codes: 0 add, 1 sub, 2 mul, 3 div, 4 div_safe (0 where b == 0), 5 max,
 * 6 leaky_mask_mul (a where b > 0 else p0*a: the backward of leaky_relu / relu), 7 axpy (a + p0*b).
 * tanh is exactly +-1 from |x| = 9 on (1 - tanh(9) = 3.0e-8 is below the fp32 spacing 2^-24 under 1: at most 0.51 ulp off).
 * NaN rule: the ops that select with `x > 0` or take fmaxf -- relu, step, sign, leaky_relu, leaky_mask_mul (its mask b),
 * max, and srgan_row_max -- treat a NaN as "not positive" / drop it (relu, step, sign: NaN -> 0; leaky_relu: NaN -> p0 * NaN
 * = NaN; leaky_mask_mul: NaN mask -> p0 * a; max, row_max: the other operand), where torch propagates the NaN.  The same
 * `> 0` is the mask of the fused convolution epilogues, bit for bit; every other op follows IEEE arithmetic.
 * Replace torch elementwise call sites: leaky_relu/relu/tanh (reference coefficient/models.py:24-26;
 * age/models.py:47-51,70-73; crowd/models.py:339,343,780-784,1150,1154), the distance functions
 * (utility.py:201-243), logsumexp / BCE / CE pieces (utility.py:161-182, sgan.py:14-15). */
int srgan_ew_unary(int op, const float* x, float* y, int64_t n, float p0, float p1, void* stream);
int srgan_ew_binary(int op, const float* a, const float* b, float* y, int64_t n, float p0, void* stream);
int srgan_fill(float* y, int64_t n, float value, void* stream);

/* y[n,c,i] = ((x ? x[n,c,i] : 1) - mean[c]) * scale_a[c] * scale_b[c] + shift[c], i < HW; every vector optional.
 * Frozen (eval-mode) batch-norm in one pass (mean = running_mean, scale_a = 1/sqrt(running_var + eps),
 * scale_b = gamma, shift = beta: reference srgan.py:538-542 + crowd/models.py:338,342,367,1073,1091) and every
 * broadcast: with N = 1 a per-row scale (gradient-penalty norms), with HW = 1 a per-column one. */
int srgan_chan_affine(const float* x, const float* mean, const float* scale_a, const float* scale_b, const float* shift,
                      float* y, int32_t N, int32_t C, int64_t HW, void* stream);

/* As srgan_chan_affine, then optionally y = max(y, 0) (relu != 0) and y = 0 where mask[n,c,i] <= 0 (mask may be
 * NULL): frozen batch-norm + ReLU forward in one pass, and its input gradient g * [y > 0] * gamma / sigma
 * (reference crowd/models.py:338-339,342-343,367-368,1073-1074,1149-1150). */
int srgan_chan_affine_act(const float* x, const float* mean, const float* scale_a, const float* scale_b,
                          const float* shift, const float* mask, int relu, float* y, int32_t N, int32_t C, int64_t HW,
                          void* stream);
/* srgan_chan_affine_act on channel-slice views: image n of x / mask / y starts at n * its batch stride (0 = dense), and
 * accumulate != 0 adds into y.  Used by the concat-free dense block: batch-norm reads a slice of the block
 * buffer; its input gradient is accumulated into a slice of the block's gradient buffer. */
int srgan_chan_affine_act_strided(const float* x, const float* mean, const float* scale_a, const float* scale_b,
                                  const float* shift, const float* mask, int relu, float* y, int32_t N, int32_t C,
                                  int64_t HW, int64_t x_batch_stride, int64_t mask_batch_stride, int64_t y_batch_stride,
                                  int accumulate, void* stream);
/* Per-weight-element part of the DOUBLE backward of norm -> relu -> conv (gradient penalty, reference
 * srgan.py:360-375 through crowd/models.py:338-345), w and q shaped [CO][CI][taps], a = inv_std * gamma per input
 * channel: w_scaled = w * a (optional); when q (the weight gradient taken with the masked, unscaled tangent) is
 * given: w_grad += q * a and gamma_grad[ci] += inv_std[ci] * sum_{co,tap} w * q. */
int srgan_bn_conv_tangent_weights(const float* w, const float* q, const float* inv_std, const float* gamma,
                                  float* w_scaled, float* w_grad, float* gamma_grad, int32_t CO, int32_t CI, int32_t taps,
                                  void* stream);

/* The same for many convolutions in ONE launch (every layer of a dense block's double backward).  The `_job` call fills
 * one 64-byte table slot on the host: the parameters where they live, and `offset` (elements) of this convolution's
 * scaled weights / weight gradient q inside two per-step buffers; the caller uploads the table once.  `_grouped` with
 * scaled_base != NULL writes every w_scaled (start of the double backward), with q_base != NULL it applies the gradient
 * part (its end); max_inner = max CI * taps, max_co = max CO over the table. */
int srgan_bn_conv_tangent_weights_job(const float* w, const float* inv_std, const float* gamma, float* w_grad,
                                      float* gamma_grad, int64_t offset, int32_t CO, int32_t CI, int32_t taps, void* job);
int srgan_bn_conv_tangent_weights_grouped(const void* jobs, int32_t count, int32_t max_inner, int32_t max_co, float* scaled_base,
                                          const float* q_base, void* stream);

/* Whole backward of frozen batch-norm (+ReLU when relu != 0) in one pass over (g, x): the activation mask is
 * recomputed from x (y = fma(x, a, b), a = inv_std*gamma, b = beta - mean*a, exactly the forward's arithmetic);
 * gx (=,+=) g*[y>0]*a (gx may be NULL; g / x / gx may be channel-slice views, batch stride 0 = dense; unscaled != 0
 * drops the factor a: gx = g*[y>0], the masked tangent used by the double backward of the gradient penalty);
 * g_gamma[c] += inv_std[c] * sum g*[y>0]*(x - mean[c]) and g_beta[c] += sum g*[y>0] with fp32 atomics (both NULL =
 * frozen parameters).  Replaces the autograd backward of reference crowd/models.py:338-343 (norm+relu pairs). */
int srgan_bn_act_bwd(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                     const float* beta, int relu, float* gx, float* g_gamma, float* g_beta, int32_t N, int32_t C,
                     int64_t HW, int64_t g_batch_stride, int64_t x_batch_stride, int64_t gx_batch_stride,
                     int accumulate_gx, int unscaled, void* stream);

/* Training-mode batch normalisation (batch statistics) of an fp32 NCHW tensor, M = N * HW values per channel: the
 * norm layers of the DCGAN generators, which the reference never freezes (srgan.py:171, age/models.py:16-21).
 * _stats: ONE read of x -> mean[c], inv_std[c] = 1 / sqrt(biased variance + eps); the variance is summed from
 *   deviations about the mean ((count, mean, M2) partials merged by Chan's formula), and the channel's workgroups meet
 *   in the stream's workspace in a fixed order: bit-reproducible.  running_mean / running_var (each may be NULL)
 *   become (1 - momentum) * running + momentum * statistic, with the UNBIASED variance M2 / (M - 1) as
 *   torch.nn.BatchNorm2d; *num_batches_tracked (may be NULL) is incremented on the device.  2 <= M <= 2^24
 *   (the partial counts are carried as fp32; more values per channel: SRGAN_ERANGE).
 * _fwd: y = leaky((x - mean) * inv_std * gamma + beta, slope) in one pass (slope = 1: no activation).
 * _bwd_reduce: g' = g * (pre-activation > 0 ? 1 : slope), the mask recomputed from x with the forward's arithmetic;
 *   sums[c] = sum g', sums[C + c] = sum g' * xhat (xhat = (x - mean) * inv_std), in a fixed order; g_beta[c] += sums[c]
 *   and g_gamma[c] += sums[C + c] when given (each may be NULL).
 * _bwd_apply: gx = gamma * inv_std * (g' - sums[c] / M - xhat * sums[C + c] / M).
 * Nothing but x, mean and inv_std is kept between the passes. */
int srgan_batch_norm_train_stats(const float* x, float* mean, float* inv_std, float* running_mean, float* running_var,
                                 int64_t* num_batches_tracked, float momentum, float eps, int32_t N, int32_t C, int64_t HW,
                                 void* stream);
int srgan_batch_norm_train_fwd(const float* x, const float* mean, const float* inv_std, const float* gamma, const float* beta,
                               float slope, float* y, int32_t N, int32_t C, int64_t HW, void* stream);
int srgan_batch_norm_train_bwd_reduce(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                                      const float* beta, float slope, float* sums, float* g_gamma, float* g_beta, int32_t N,
                                      int32_t C, int64_t HW, void* stream);
int srgan_batch_norm_train_bwd_apply(const float* g, const float* x, const float* mean, const float* inv_std, const float* gamma,
                                     const float* beta, float slope, const float* sums, float* gx, int32_t N, int32_t C, int64_t HW,
                                     void* stream);

/* out[c] (=,+=) scale[c] * sum_{n,i} a[n,c,i] * ((b ? b[n,c,i] : 1) - mean[c])  (b, mean, scale optional).
 * Bias / batch-norm parameter gradients; with N = 1, C = batch it is the per-example dot product over C*H*W of
 * the gradient penalty (reference srgan.py:371,381); with HW = 1 the batch sum behind feature means
 * (srgan.py:442-443); with N = C = 1 a full sum. */
int srgan_chan_reduce(const float* a, const float* b, const float* mean, const float* scale, float* out, int32_t N,
                      int32_t C, int64_t HW, int accumulate, void* stream);
/* out[b] = max_f x[b,f] (logsumexp stabiliser, reference utility.py:179) and the one-hot of the nearest bin
 * (reference utility.py:141-144). */
int srgan_row_max(const float* x, float* out, int32_t B, int32_t F, void* stream);
int srgan_nearest_bin_onehot(const float* y, const float* bins, float* onehot, int32_t B, int32_t K, void* stream);

/* dst[n, dst_first + c, :] (=,+=) src[n, src_first + c, :], c < count: channel concat / slice
 * (reference crowd/models.py:353,1159-1165). */
int srgan_copy_channels(const float* src, int32_t src_channels, int32_t src_first, float* dst, int32_t dst_channels,
                        int32_t dst_first, int32_t count, int32_t N, int64_t HW, int accumulate, void* stream);

/* ---- pooling (planes = N*C) --------------------------------------------------------------------------------
 * reference crowd/models.py:371,1075,1151; age/vgg.py:76. */
/* The DenseNet stem's norm0 -> relu0 -> pool0 (reference crowd/models.py:1072-1076) as ONE pass each way: forward
 * y = maxpool(relu(batch_norm_eval(x))) with the arg-max of srgan_maxpool2d_fwd; backward gx = S * [bn(x) > 0] * inv_std *
 * gamma with S the pooled gradient gathered per input pixel, g_gamma / g_beta (both or neither) ADDED to.  The backward
 * exists for 3 / 2 / 1 windows on rows of whole float4s (`_supported`). */
int srgan_bn_relu_maxpool_fwd(const float* x, const float* mean, const float* inv_std, const float* gamma, const float* beta,
                              float* y, int32_t* argmax, int32_t N, int32_t C, int32_t H, int32_t W, int32_t k, int32_t s, int32_t p,
                              int32_t OH, int32_t OW, void* stream);
int srgan_bn_relu_maxpool_bwd_supported(int32_t N, int32_t C, int32_t H, int32_t W, int32_t k, int32_t s, int32_t p);
int srgan_bn_relu_maxpool_bwd(const float* gy, const int32_t* argmax, const float* x, const float* mean, const float* inv_std,
                              const float* gamma, const float* beta, float* gx, float* g_gamma, float* g_beta, int32_t N,
                              int32_t C, int32_t H, int32_t W, int32_t k, int32_t s, int32_t p, int32_t OH, int32_t OW,
                              void* stream);
/* avg_pool2d(relu(batch_norm_eval(x)), 2, 2) as ONE pass each way, for the DenseNet transitions evaluated as norm -> relu ->
 * pool -> conv (reference crowd/models.py:364-371 has conv -> pool; the 1x1 convolution and the average pooling commute, so
 * the convolution and its gradients run on a quarter of the pixels).  Forward: y[N, C, H/2, W/2]; backward: gx = 0.25 *
 * gy[h/2, w/2] * [bn(x) > 0] * inv_std * gamma, g_gamma / g_beta (both or neither) ADDED to.  Even H, W % 4 == 0
 * (`_supported`). */
int srgan_bn_relu_avgpool2_supported(int32_t N, int32_t C, int32_t H, int32_t W);
int srgan_bn_relu_avgpool2_fwd(const float* x, const float* mean, const float* inv_std, const float* gamma, const float* beta,
                               float* y, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);
int srgan_bn_relu_avgpool2_bwd(const float* gy, const float* x, const float* mean, const float* inv_std, const float* gamma,
                               const float* beta, float* gx, float* g_gamma, float* g_beta, int32_t N, int32_t C, int32_t H,
                               int32_t W, void* stream);
int srgan_maxpool2d_fwd(const float* x, float* y, int32_t* argmax, int32_t planes, int32_t H, int32_t W, int32_t k,
                        int32_t s, int32_t p, int32_t OH, int32_t OW, void* stream);
int srgan_maxpool2d_bwd(const float* g, const int32_t* argmax, float* gx, int32_t planes, int32_t H, int32_t W, int32_t k,
                        int32_t s, int32_t p, int32_t OH, int32_t OW, void* stream);   /* max-pool backward, gather form */
int srgan_pool_scatter(const float* g, const int32_t* argmax, float* out, int32_t planes, int64_t in_plane,
                       int64_t out_plane, void* stream);      /* out[argmax] += g (out is zero-filled first): backward of
                                                                 srgan_pool_gather */
int srgan_pool_gather(const float* src, const int32_t* argmax, float* out, int32_t planes, int64_t in_plane,
                      int64_t out_plane, void* stream);       /* max-pool double-backward */
int srgan_avgpool2d_fwd(const float* x, float* y, int32_t planes, int32_t H, int32_t W, int32_t k, int32_t s,
                        int32_t OH, int32_t OW, void* stream);
int srgan_avgpool2d_bwd(const float* g, float* gx, int32_t planes, int32_t H, int32_t W, int32_t k, int32_t s,
                        int32_t OH, int32_t OW, void* stream);

/* ---- fused pieces of the step ------------------------------------------------------------------------------
 * out = alpha[b]*u + (1 - alpha[b])*fake (reference srgan.py:365-366). */
int srgan_gp_interpolate(const float* unlabeled, const float* fake, const float* alpha, float* out, int32_t B,
                         int64_t F, void* stream);
/* The random tensors of an iteration drawn ON THE DEVICE (SRGAN_FEATURE_DEVICE_DRAWS): the two-Gaussian mixture z of the
 * discriminator step, alpha and the generator step's z (reference srgan.py:286-289, 364, 301; the reference draws them on
 * the host from NumPy's / torch's streams -- this stream is a different one, with the same distributions).
 *   out[i] = element (first + i) of draw `draw` of the iteration held in state, i in [0, n).
 *   state: device uint32[4] = {seed_lo, seed_hi, iteration, 0}, owned by the caller.
 * Element e is a pure function of (seed, iteration, draw, e): Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
 * constants 0x9E3779B9 / 0xBB67AE85) with key (seed_lo, seed_hi) and counter (block & 0xffffffff, block >> 32, draw,
 * iteration), block = e >> 2; the four output words w0..w3 belong to elements 4 * block + 0..3, element e owns w[e & 3].
 * A window [first, first + n) of a draw therefore holds the same bits whoever fills it: a data-parallel rank fills its rows
 * of the global tensor with first = rank * local_rows * columns.  first and n need not be multiples of 4.
 *   kind 0: U[0, 1) = float(w_own >> 8) * 2^-24 (exact).
 *   kind 1: N(0, 1) + (+/-)offset.  Box-Muller per word pair ((w0, w1) -> elements 0, 1; (w2, w3) -> elements 2, 3):
 *     u1 = 1 - float(w_even >> 8) * 2^-24 in (0, 1], u2 = float(w_odd >> 8) * 2^-24, r = sqrt(-2 ln u1); the even element
 *     is r cos(2 pi u2), the odd one r sin(2 pi u2) (precise logf / sqrtf / sincospif); then + offset when bit 0 of the
 *     element's OWN word is 1, - offset when it is 0 (offset == 0: nothing is added).  Bit 0 lies below the 24 bits the normal
 *     uses, so this is the equal-weight mixture of norm(-offset, 1) and norm(offset, 1).
 * Before any device work: NULL out / state, n < 0, first < 0 (or first + n beyond 2^63 - 1), kind outside {0, 1}, draw < 0,
 * a non-finite offset, n above max_tensor_elements: SRGAN_EINVAL.  n == 0 is a successful no-op.
 * srgan_random_advance: state[2] += 1 on the stream (one thread), so a HIP graph that captured the fills and the advance
 * replays as the next iteration each time. */
int srgan_random_fill(float* out, int64_t n, int64_t first, int32_t kind, float offset, int32_t draw, const uint32_t* state,
                      void* stream);
int srgan_random_advance(uint32_t* state, void* stream);
/* Inverted dropout whose mask is REGENERATED, never stored (SRGAN_FEATURE_DROPOUT; reference crowd/models.py:350-353, the
 * F.dropout on a dense layer's new features):
 *   y[r * y_row_stride + i] = keep(e) ? fl(x[r * x_row_stride + i] * scale) : +0.0f,  e = first + r * row_elems + i,
 * for r < rows and i < row_elems.  keep(e) is true exactly when element e of the kind 0 (uniform) draw `draw` that
 * srgan_random_fill defines for the iteration held in `state` -- same key, counter layout and word ownership -- is >= p.
 * scale = 1.0f / (1.0f - p), computed once in fp32 by the host launcher; the product is rounded once.  p == 0 is a copy;
 * p == 1 gives all zeros (the uniforms are < 1).  A dropped element is +0.0f whatever x holds (inf and NaN included).
 * Rows are contiguous runs of row_elems floats (one example's C x H x W); the two strides (in floats) let the call write
 * into, or read from, a channel slice of a wider NCHW tensor.  x == y is allowed when the strides are equal.  The operation is
 * linear with a fixed mask, so the same call is the forward, the backward (x = the gradient) and the double backward.
 * One thread per Philox block (4 elements); 16-byte loads and stores where first, the strides and the pointers allow, single
 * floats at ragged ends and in misaligned rows, with the same results.  No workspace, no atomics.
 * Draw ids: 0, 1, 2 are an iteration's three draws; the Python host gives every dropout call of a network's step a draw of
 * its own from that network's range -- SRGAN_DROPOUT_DRAWS_D / SRGAN_DROPOUT_DRAWS_DNN + the call's index in the step, each
 * range SRGAN_DROPOUT_DRAW_RANGE wide -- under a state of the network's own that is advanced once per iteration.
 * Before any device work: NULL x / y / state, negative rows / row_elems / first (or first + rows * row_elems beyond
 * 2^63 - 1), a stride smaller than row_elems, draw < 0, p outside [0, 1] or non-finite: SRGAN_EINVAL; rows * row_elems above
 * max_tensor_elements: SRGAN_ERANGE.  Zero elements is a successful no-op. */
#define SRGAN_DROPOUT_DRAWS_D 0x10000      /* the discriminator's dropout draws: [0x10000, 0x20000) */
#define SRGAN_DROPOUT_DRAWS_DNN 0x20000    /* the DNN baseline's: [0x20000, 0x30000) */
#define SRGAN_DROPOUT_DRAW_RANGE 0x10000
int srgan_dropout(const float* x, float* y, int64_t rows, int64_t row_elems, int64_t x_row_stride, int64_t y_row_stride,
                  int64_t first, float p, int32_t draw, const uint32_t* state, void* stream);
/* The correlation-matrix feature loss without its F x F matrices (SRGAN_FEATURE_FEATURE_LOSSES; reference srgan.py:511-535,
 * feature_covariance_loss).  base / other: features [B, F], fp32, row-major, contiguous.  Per side, with n = B:
 *   m_i = mean of column i, xm = x - m, s_i^2 = sum_b xm_bi^2 / (n - 1),
 *   C_ij = clamp(sum_b xm_bi xm_bj / ((n - 1) s_i s_j), -1, 1),          loss[0] = sum_{i != j} |Cb_ij - Co_ij|.
 * Evaluated as C = Z Z^T with z_i = xm_i / ||xm_i|| on the fp32 MFMA (v_mfma_f32_32x32x2_f32, K = batch); no entry of C is
 * ever stored.  THE DIAGONAL CONTRIBUTES EXACTLY 0: C_ii = 1 on both sides in exact arithmetic (the reference's fp32 diagonal
 * differs from that by at most an ulp per feature).  An entry whose unclamped value lies strictly outside [-1, 1] is clamped
 * and passes no gradient (on that side).  A feature with zero variance gives NaN for the loss and for every gradient element.
 * loss(x, x) is exactly 0.  No atomics and no meeting of workgroups inside a launch: sums are taken in a fixed order, two calls
 * on the same inputs give the same bits.  No host synchronisation, no allocation, no use of the stream's workspace.
 *   saved    [2][3][F] floats written by _fwd, read by _bwd: per side (0 base, 1 other) and feature the mean, 1 / ||xm_i|| and
 *            r_i = sum_{j != i} G_ij C_ij with G_ij = sign(Cb_ij - Co_ij) (negated on the other side), 0 where the side's
 *            entry was clamped
 *   scratch  srgan_feature_corrcoef_l1_scratch_bytes(B, F) bytes of the CALLER's, 16-byte aligned: the normalised, transposed,
 *            zero-padded copies Z [2][round_up(F, 128)][round_up(B, 32)] and the per-split partial sums.  _bwd reads the Z that
 *            _fwd left there, so the same buffer goes to both calls, untouched in between.
 * _bwd: grad_x = 2 g[0] / ||xm_i|| * ((G Z)_i - r_i z_i) for each requested side, [B, F]; grad_base or grad_other may be
 * NULL (the generator's loss needs `other` only; both NULL is a no-op); every element of a requested gradient is written.
 * It recomputes the Gram tiles (one more pass, once per side and per 128 examples).  First order only.
 * Capacity: 2 <= B <= 8192, 1 <= F <= 2^20, round_up(F, 128) * round_up(B, 32) <= 2^26 (512 MiB of Z); the scratch query
 * returns the bytes (> 0) or the status.  Before any device work: NULL base / other / loss / saved / scratch / g or a
 * misaligned scratch, B < 2, F < 1: SRGAN_EINVAL; a shape beyond the capacity: SRGAN_ERANGE with the shape in
 * srgan_last_error(). */
int64_t srgan_feature_corrcoef_l1_scratch_bytes(int32_t B, int32_t F);
int srgan_feature_corrcoef_l1_fwd(const float* base, const float* other, float* loss, float* saved, float* scratch, int32_t B,
                                  int32_t F, void* stream);
int srgan_feature_corrcoef_l1_bwd(const float* base, const float* other, const float* saved, const float* scratch, const float* g,
                                  float* grad_base, float* grad_other, int32_t B, int32_t F, void* stream);
/* rows[b] = sum_{hw} mean_c |maps[b,c,hw] - target[b,hw]| and its backward (reference crowd/srgan.py:252). */
int srgan_crowd_map_l1_fwd(const float* maps, const float* target, float* rows, int32_t B, int32_t Cm, int64_t HW,
                           void* stream);
int srgan_crowd_map_l1_bwd(const float* maps, const float* target, const float* g_rows, float* g_maps, int32_t B,
                           int32_t Cm, int64_t HW, void* stream);
/* Training-batch assembly of the crowd application on the device (replaces the reference's 4-worker NumPy patch
 * extractor, crowd/shanghai_tech_data.py:76-104 with crowd/data.py:41-128,370-453): example b = the P x P patch centred
 * on (ys[b], xs[b]) of scene b (images_u8[b]: uint8 RGB [H, W, 3]; labels[b] / maps[b]: float [H, W]; all device
 * pointers, the pointer tables and the int32 arrays live on the device too), mirrored left-right when flips[b] != 0,
 * image normalised to [-1, 1] and planar: out_images [B, 3, P, P], out_labels / out_maps [B, P, P] (labels / maps and
 * their outputs may be NULL).  Pixels outside the scene are 0 before normalisation (-1 after), 0 in label / map. */
int srgan_crowd_extract_patches(const void* const* images_u8, const float* const* labels, const float* const* maps,
                                const int32_t* heights, const int32_t* widths, const int32_t* ys, const int32_t* xs,
                                const int32_t* flips, int32_t B, int32_t P, float* out_images, float* out_labels,
                                float* out_maps, void* stream);
/* The same batch with the host taken out (SRGAN_FEATURE_CROWD_PATCH_DRAWS): the positions drawn on the device from the stream
 * of srgan_random_fill, and the cut driven by that table over per-SCENE tables that are uploaded once.  All pointers are device
 * pointers.
 * srgan_crowd_draw_patches: table int32[n][4], row i = {scene, y, x, flip_bit} of global example e = first + i.
 *   starts[S + 1]: the running count of valid patch centres; scene s owns starts[s + 1] - starts[s] =
 *     max(heights[s] - P + 1, 0) * max(widths[s] - P + 1, 0) of them; length = starts[S], 1 <= length < 2^63.
 *   state: the uint32[4] = {seed_lo, seed_hi, iteration, 0} of srgan_random_fill.
 *   Example e owns the WHOLE Philox block e of draw `draw` (counter (e & 0xffffffff, e >> 32, draw, iteration), words w0..w3):
 *     r = (uint64(w1) << 32) | w0;  index = floor(r * length / 2^64), the high half of the 128-bit product -- no rejection
 *     loop: a centre's probability deviates from 1 / length by less than 2^-64, i.e. the deviation from uniform is below
 *     length / 2^64 per centre, relative;
 *     scene = the largest s in [0, S) with starts[s] <= index (a scene without a centre is never chosen);
 *     local = index - starts[scene], columns = widths[scene] - P + 1;
 *     y = P / 2 + local / columns, x = P / 2 + local % columns;  flip_bit = flip ? (w2 >> 31) : 0;  w3 is unused.
 *   A window [first, first + n) holds the same rows whoever fills it: a data-parallel rank fills first = rank * local_batch.
 *   One thread per example; no LDS, no atomics, no workspace.  The consistency of starts / heights / widths is the caller's
 *   contract (checking it would need a synchronisation); the search is clamped to [0, S - 1], so the kernel never indexes
 *   outside the three tables whatever they hold.
 *   Before any device work: a NULL pointer, S < 1, P < 2 or odd, n < 0, first < 0 (or first + n beyond 2^63 - 1), draw < 0:
 *   SRGAN_EINVAL.  n == 0 is a successful no-op.
 * srgan_crowd_extract_patches_indexed: images_u8 / labels / maps / heights / widths have one entry per scene (length S);
 *   example b is the patch of scene table[b][0] centred on (table[b][1], table[b][2]), mirrored when table[b][3] != 0, with
 *   the pixel contract of srgan_crowd_extract_patches bit for bit (labels / maps and their outputs may be NULL).  A row whose
 *   scene is outside [0, S) yields an all-padding patch (-1 / 0 / 0) and reads no scene memory.  One wave per patch row, four
 *   rows per workgroup; 16-byte stores when P % 4 == 0 and the three outputs are 16-byte aligned, single floats otherwise,
 *   with the same results.  Before any device work: NULL images_u8 / heights / widths / table / out_images, S < 1, B < 1 or
 *   B > 65535, P < 1 or odd: SRGAN_EINVAL; B * 3 * P * P above max_tensor_elements: SRGAN_ERANGE. */
#define SRGAN_CROWD_PATCH_DRAW_LABELED 0x30000      /* the labeled loader's draw id: above the dropout ranges */
#define SRGAN_CROWD_PATCH_DRAW_UNLABELED 0x30001    /* the unlabeled loader's */
int srgan_crowd_draw_patches(const int64_t* starts, const int32_t* heights, const int32_t* widths, int32_t S, int32_t P,
                             int32_t flip, int64_t first, int32_t n, int32_t draw, const uint32_t* state, int32_t* table,
                             void* stream);
int srgan_crowd_extract_patches_indexed(const void* const* images_u8, const float* const* labels, const float* const* maps,
                                        const int32_t* heights, const int32_t* widths, int32_t S, const int32_t* table,
                                        int32_t B, int32_t P, float* out_images, float* out_labels, float* out_maps,
                                        void* stream);
/* The sums behind the crowd evaluation scalars (SRGAN_FEATURE_CROWD_EVALUATION; reference crowd/srgan.py:149-191: count ME /
 * MAE / MSE and kNN-map MAE / MSE) of one batch that lives on the device.  predicted_counts [B]; labels [B, HW], the head-count
 * label patches; predicted_maps [B, M, HW] and maps [B, HW], both or neither; all fp32, contiguous.  With L_b = the sum of
 * labels[b, :] and d_b = (double)predicted_counts[b] - L_b the call ADDS to the caller's eight doubles `sums`
 *   sums[0] += sum_b d_b      sums[1] += sum_b |d_b|      sums[2] += sum_b d_b * d_b      sums[3] += B
 * and, when the map pointers are given, with e = (double)predicted_maps[b, m, i] - (double)maps[b, i],
 *   sums[4] += sum |e|        sums[5] += sum e * e        sums[6] += B * M * HW
 * sums[7] is reserved and never touched.  Every accumulation is fp64; every square is rounded as a product before it is added
 * (no FMA contraction): each term is the one NumPy float64 arithmetic forms from the same fp32 inputs, only the order of the
 * additions differs.  Two launches on `stream`, nothing else: a partials kernel (256 threads per workgroup over (example,
 * 2048-element chunk of the plane); 16-byte loads where HW % 4 == 0 and labels / predicted_maps / maps are 16-byte aligned,
 * element loads otherwise) leaves three doubles per workgroup in `scratch`, and a one-workgroup kernel adds them in a fixed
 * order (16 lanes per example, lane s adding the example's slots s, s + 16, ... in that order; a butterfly over the 16; then
 * the examples' terms over the 256 threads in a fixed tree) and updates `sums`.
 * No atomics, no meeting of workgroups inside a launch, no workspace of the stream: the same inputs give the same bits.
 * `scratch`: srgan_crowd_evaluation_scratch_bytes(B, M, HW) bytes of the caller's, 8-byte aligned, fully overwritten before
 * it is read (it may hold anything).  The query returns the bytes (> 0) or the status.
 * Before any device work: NULL predicted_counts / labels / sums / scratch, exactly one of predicted_maps / maps, B < 0,
 * HW < 0, M < 1 with maps (M is ignored without), a misaligned sums / scratch: SRGAN_EINVAL; B * M * HW (B * HW without maps)
 * above max_tensor_elements, or more than 2^24 - 1 workgroups (B * ceil(HW / 2048): a launch holds fewer than 2^32 threads;
 * an evaluation batch at 512 x 512 / 16 is 2048): SRGAN_ERANGE, from the query too.  B == 0 or HW == 0: SRGAN_OK, `sums`
 * untouched.  The translation unit is compiled with FMA contraction off (`#pragma clang fp contract(off)`): the squares are
 * v_mul_f64 + v_add_f64 in the kernels' code. */
int srgan_crowd_evaluation_sums(const float* predicted_counts, const float* labels, const float* predicted_maps,
                                const float* maps, int32_t B, int32_t M, int64_t HW, double* sums, void* scratch,
                                void* stream);
int64_t srgan_crowd_evaluation_scratch_bytes(int32_t B, int32_t M, int64_t HW);
/* The sums behind the age and driving evaluation scalars (SRGAN_FEATURE_REGRESSION_EVALUATION; reference age/srgan.py:92-107,
 * driving/srgan.py:87-104: MAE / MSE, NMAE = MAE / label range) of one batch that lives on the device.  predictions: B rows,
 * row b starting at predictions[b * row_stride] (elements, row_stride >= K); labels [B]; all fp32.  The prediction p_b of a row:
 *   bins == NULL (then K == 1):  p_b = predictions[b * row_stride]
 *   bins != NULL (bins [K], K >= 1: the SGAN case, reference age/sgan.py:22-26): the row holds K class logits and
 *     p_b = bins[j], j the LOWEST index of the row's maximum -- utility.logits_to_bin_values, i.e. torch.max(dim=1)'s first
 *     maximal index; +0.0 and -0.0 compare equal, +-inf are ordinary values; a row that holds a NaN is outside the contract.
 * With d_b = (double)p_b - (double)labels[b] the call updates the caller's eight doubles `sums`
 *   sums[0] += sum_b d_b      sums[1] += sum_b |d_b|      sums[2] += sum_b d_b * d_b      sums[3] += B
 *   sums[4] = fmin(sums[4], min_b labels[b])              sums[5] = fmax(sums[5], max_b labels[b])
 * sums[6] and sums[7] are reserved and never touched.  An epoch's record starts as {0, 0, 0, 0, +inf, -inf, 0, 0}.  Every
 * accumulation is fp64; every square is rounded as a product before it is added (the translation unit is compiled with
 * `#pragma clang fp contract(off)`): each term is the one NumPy float64 arithmetic forms from the same fp32 inputs, only the
 * order of the additions differs.  One launch of one workgroup of 256 threads on `stream`, nothing else: thread t takes rows t,
 * t + 256, ... in that order, the wave's 64 sums meet in a butterfly and the four waves in wave order through LDS.  No atomics,
 * no scratch, no workspace of the stream: the same inputs give the same bits.
 * Before any device work: NULL predictions / labels / sums, B < 0, K < 1, K > 1 without bins, row_stride < K, a misaligned
 * sums: SRGAN_EINVAL; then K > 1024 or B * K > 2^22 (a limit of the one-workgroup design -- an evaluation batch is a few
 * thousand rows -- not a measured optimum): SRGAN_ERANGE.  B == 0: SRGAN_OK, `sums` untouched. */
int srgan_regression_evaluation_sums(const float* predictions, int64_t row_stride, int32_t K, const float* bins,
                                     const float* labels, int32_t B, double* sums, void* stream);

/* Training-batch assembly from a database of equally sized frames resident on the device (SRGAN_FEATURE_IMAGE_BATCHES):
 * the reference's AgeDataset / SteeringAngleDataset items (age/data.py:52-60, driving/data.py:44-51) collated by its
 * DataLoader, as one launch and no host-to-device copy.  store: count frames [C, h, w], planar and contiguous, values in the
 * 0..255 range; store_dtype 0 = uint8, 1 = float.  labels [count] float; order: int32 index list (an epoch's permutation);
 * all device pointers.  Example b of the batch is frame order[first + b] -- an entry outside [0, count) is clamped, it cannot
 * be checked here -- written to out_images [B, C, H, W] fp32 and out_labels [B] (labels and out_labels: both or neither).
 * (H, W) == (h, w): out = (float(v) / 127.5f) - 1.0f, an IEEE division and a separate subtraction: the bits of the
 * reference's to_normalized_range on a CPU tensor (utility.py:129-132).  Any other (H, W), larger or smaller, per axis: the
 * normalised frame resampled with the arithmetic of torch.nn.functional.interpolate(mode='bilinear', align_corners=False,
 * antialias=False) -- half-pixel centres, clamped edges.  A frame and the batch hold at most max_tensor_elements elements
 * each (SRGAN_EINVAL, like every other argument error); the store as a whole may be larger, frames are addressed in 64 bits. */
int srgan_image_batch_gather(const void* store, int store_dtype, int32_t count, int32_t C, int32_t h, int32_t w,
                             const float* labels, const int32_t* order, int64_t first, int32_t B, int32_t H, int32_t W,
                             float* out_images, float* out_labels, void* stream);
/* The epoch order of such a database drawn on the device (SRGAN_FEATURE_EPOCH_ORDER), so that a batch is a function of
 * (seed, step) and its launches take no argument that changes from step to step.  All pointers are device pointers.
 * The stream.  A loader with draw id `draw` under state = uint32[4] {seed_lo, seed_hi, iteration, 0} (srgan_random_fill's)
 * shuffles its n frames once per epoch.  With batches = n / B_global (integer division: the reference's drop_last) the
 * state's iteration word t -- the training step -- gives the epoch e = t / batches and the batch b = t % batches.  Frame i of
 * epoch e owns the 64-bit key
 *     key_i = (uint64(w1) << 32) | w0,   w0..w3 = the words of Philox block i of draw `draw` with the counter's iteration
 *     word set to e, NOT to the step: counter (i, 0, draw, e), key (seed_lo, seed_hi); w2 and w3 are unused;
 * order[p] is the frame at sorted position p of the keys in ascending order, a tie going to the lower frame index (a stable
 * argsort; NumPy: np.argsort(keys, kind='stable')).  Row r of the global batch of step t is frame order[b * B_global + r];
 * the n - batches * B_global frames at the end of an epoch's order are not used in that epoch.
 * srgan_epoch_order writes order int32[n] for the epoch of `state`.  One launch: a workgroup owns 256 frames and walks all n
 *   keys in LDS tiles that it computes itself; every thread counts the keys in front of its own and stores order[rank] = i.
 *   Every slot is written exactly once; no atomics, no workspace, no keys buffer; two calls give the same bits.  O(n^2)
 *   comparisons.  conditional == 1: every workgroup reads t and returns unless t % batches == 0, so a launch recorded in a HIP
 *   graph rebuilds the order exactly at the epoch starts and leaves it untouched otherwise; conditional == 0 always rebuilds
 *   (first use, a loader put at a step in the middle of an epoch).
 * srgan_argsort_u64 is the same ranking pass (the same kernel body) over n keys in memory: order = the stable argsort of
 *   keys.  64-bit Philox ties do not occur in practice; this is where the tie rule can be exercised.
 * srgan_epoch_batch_indices writes table[i] = order[(t % batches) * B_global + first_row + i] for i < rows, one thread per
 *   row: rows [first_row, first_row + rows) of the global batch of step t (a data-parallel rank: first_row = rank *
 *   local_batch).  srgan_image_batch_gather(..., order = table, first = 0, B = rows, ...) then cuts the batch and
 *   srgan_random_advance ends it: at most four launches, none with a step-dependent argument.
 * Before any device work: a NULL pointer, n < 1, batches < 1, draw < 0, conditional outside {0, 1}, B_global < 1,
 *   batches * B_global > n, rows < 0, first_row < 0, first_row + rows > B_global: SRGAN_EINVAL; then n above
 *   SRGAN_EPOCH_ORDER_MAX: SRGAN_ERANGE.  rows == 0 is a successful no-op.
 * SRGAN_EPOCH_ORDER_MAX is a capacity of the O(n^2) rebuild, not a tuned value (the reference's largest split is 50 000
 * frames; profiles/epoch_order.md has the rebuild's time at 2^20). */
#define SRGAN_EPOCH_ORDER_MAX (1 << 20)
#define SRGAN_IMAGE_BATCH_DRAW_LABELED 0x30002      /* the labeled loader's draw id: next to the crowd loaders' */
#define SRGAN_IMAGE_BATCH_DRAW_UNLABELED 0x30003    /* the unlabeled loader's */
int srgan_epoch_order(int32_t n, int32_t batches, int32_t conditional, int32_t draw, const uint32_t* state, int32_t* order,
                      void* stream);
int srgan_argsort_u64(const uint64_t* keys, int32_t n, int32_t* order, void* stream);
int srgan_epoch_batch_indices(const int32_t* order, int32_t n, int32_t B_global, int32_t batches, int32_t first_row,
                              int32_t rows, const uint32_t* state, int32_t* table, void* stream);

/* ---- full-image (sliding-window) inference of the crowd application on the device (SRGAN_FEATURE_CROWD_FULL_IMAGE) ----
 * The reference's predict_full_example (crowd/srgan.py:332-395) without its per-window NumPy work.
 * Windows first .. first + count - 1 of ONE resident scene (image_u8: uint8 RGB [H, W, 3]): window i is the P x P patch
 * centred on (ys[i / nx], xs[i % nx]) -- ys [ny] / xs [nx]: int32 arrays on the device, the centre lists of the reference's
 * ImageSlidingWindowDataset (crowd/data.py:521-560) -- normalised to [-1, 1] and planar, out_images [count, 3, P, P];
 * pixels outside the scene are 0 before normalisation (-1 after).  P even; first + count <= ny * nx; count <= 65535. */
int srgan_crowd_extract_windows(const void* image_u8, int32_t H, int32_t W, const int32_t* ys, int32_t ny,
                                const int32_t* xs, int32_t nx, int32_t first, int32_t count, int32_t P,
                                float* out_images, void* stream);
/* in [B, h, w] -> out [B, P, P], the float-mode bilinear resize the reference meant by scipy.misc.imresize(..., mode='F')
 * (crowd/srgan.py:364): half-pixel centres, clamped edges, values not rescaled (sums are NOT preserved) -- the arithmetic of
 * torch.nn.functional.interpolate(mode='bilinear', align_corners=False).  P >= h and P >= w (downscaling:
 * SRGAN_EUNSUPPORTED). */
int srgan_crowd_resize_bilinear(const float* in, int32_t B, int32_t h, int32_t w, int32_t P, float* out, void* stream);
/* The overlap average of the windows' predictions: out_density [H, W] = (sum over the windows covering a pixel, in window
 * order, of densities[i] at the pixel's place in window i) / (number of covering windows, 0 -> 1), bit-identical to the
 * reference's slice-add loop; *out_count = sum over the pixels of (sum of counts[i] / (P * P) over the same windows) / the
 * same number, reduced in a fixed order through the stream's workspace (same bits on every run; a stream without a
 * registered workspace gets SRGAN_EUNSUPPORTED when the image has more than 1024 pixels).  densities [ny * nx, P, P] may be
 * NULL (a network without a density: out_density is zero-filled, nothing is read); counts [ny * nx]; ys / xs as above;
 * P even.  All pointers are device pointers. */
int srgan_crowd_blend_windows(const float* densities, const float* counts, const int32_t* ys, int32_t ny, const int32_t* xs,
                              int32_t nx, int32_t H, int32_t W, int32_t P, float* out_density, float* out_count,
                              void* stream);

/* ---- image summaries on the device (SRGAN_FEATURE_IMAGE_SUMMARIES) --------------------------------------------------------
 * The pictures the reference writes at every summary step (age/srgan.py:73-90, driving/srgan.py:68-85,
 * crowd/srgan.py:119-145,193-245), which it builds on the host with torchvision.utils.make_grid and matplotlib after downloading
 * whole batches.  Both kernels are gathers: every output element is written exactly once, whatever `out` / `tiles` held before.
 *
 * srgan_image_grid: torchvision's make_grid of one contiguous batch.  images [N, C, H, W], C in {1, 3}; out [3, GH, GW] (one
 * channel is replicated).  N == 1: out is the image itself (GH = H, GW = W, no padding).  Otherwise xmaps = min(nrow, N),
 * ymaps = ceil(N / xmaps), GH = ymaps * (H + padding) + padding, GW = xmaps * (W + padding) + padding; image k sits at rows
 * (k / xmaps) * (H + padding) + padding ... and columns (k % xmaps) * (W + padding) + padding ...; everything else, the cells
 * after image N - 1 in the last row included, is pad_value (never normalised).  normalize != 0:
 * v = (min(max(x, low), high) - low) / max(high - low, 1e-5f) in fp32 with a correctly rounded division -- the rule of current
 * torchvision; releases old enough to take `range=` divided by (high - low + 1e-5) instead, at most 1e-5 relative away.
 * Before any device work: a NULL pointer, N < 1, C outside {1, 3}, H or W < 1, nrow < 1, padding < 0, or normalize with a
 * non-finite bound or high < low: SRGAN_EINVAL; out above max_tensor_elements: SRGAN_ERANGE. */
int srgan_image_grid(const float* images, int32_t N, int32_t C, int32_t H, int32_t W, int32_t nrow, int32_t padding,
                     float pad_value, int32_t normalize, float low, float high, float* out, void* stream);
/* srgan_density_heatmaps: the reference's convert_density_maps_to_heatmaps (crowd/srgan.py:193-217) for a whole batch and every
 * map head.  labels [B, h, w]; predicted [B, M, h, w]; lut [lut_entries, 3] RGB (matplotlib's inferno: 256 entries), all on the
 * device.  For each pair (b, m): vmin = min(min labels[b], min predicted[b, m]), vmax likewise, written to ranges[b, m, 0..1]
 * (ranges: [B, M, 2] floats).  A pixel of a map is first resized to P x P with exactly the arithmetic of
 * srgan_crowd_resize_bilinear (h == P and w == P: the identity, bit for bit); then t = (v - vmin) / (vmax - vmin) in fp32, t = 0
 * when vmax == vmin; the entry is (int)(t * lut_entries) truncated, lut_entries itself becomes lut_entries - 1, a negative t
 * gives entry 0 and anything above the last entry -- matplotlib's Normalize followed by Colormap.__call__ on a float32 array.
 * For example b the M + 1 planar RGB tiles [3, P, P] start at tiles + b * tile_stride (in floats; tile_stride >= (M + 1) * 3 *
 * P * P lets the caller leave a slot for the photograph in front of each row of tiles): first the label under the range of pair
 * (b, 0) -- the reference computes it for every m and keeps only that one -- then the M predictions, each under its own pair's
 * range.  Inputs are finite.  Two launches, no host round trip.  Argument errors (NULL, B / M / h / w / P / lut_entries < 1, a
 * short tile_stride): SRGAN_EINVAL; P < h or P < w: SRGAN_EUNSUPPORTED, as in srgan_crowd_resize_bilinear; a tensor above
 * max_tensor_elements or more than 65535 tiles: SRGAN_ERANGE. */
int srgan_density_heatmaps(const float* labels, const float* predicted, int32_t B, int32_t M, int32_t h, int32_t w, int32_t P,
                           const float* lut, int32_t lut_entries, float* tiles, int64_t tile_stride, float* ranges, void* stream);

/* ---- distribution summaries on the device (SRGAN_FEATURE_DISTRIBUTION_SUMMARIES) ----------------------------------------------
 * What the reference's coefficient application logs at a summary step beside its error scalars (coefficient/srgan.py:56-78,
 * coefficient/presentation.py:19-55): the 1-D Wasserstein distance between two sets of predictions and a frame of kernel-density
 * curves, which it computes on the host with scipy / seaborn / matplotlib after downloading every prediction.  All pointers are
 * device pointers; no call synchronises or reads anything back; no fp32 atomics; every sum that lanes or workgroups share is
 * finished in a fixed order, so a call repeats its bits; every output element is written exactly once, whatever it held before.
 * Inputs are finite (a NaN or an infinity in `u`, `v`, `samples` or `vertices` gives an unspecified, but in-bounds, result).
 *
 * srgan_wasserstein_1d: scipy.stats.wasserstein_distance(u, v) of unweighted samples u [n], v [m]; one float to `out`.  One
 * workgroup sorts the N = n + m values, each tagged with its origin, in LDS (a bitonic network over the next power of two,
 * padded with +inf), counts the values of u up to each sorted position (cu; cv = position + 1 - cu), and sums over the N - 1
 * gaps |cu * m - cv * n| * (x[k + 1] - x[k]) -- the CDF difference in integers, so equal values and their order cannot change
 * the result: their gap is 0 -- each thread over a contiguous run of gaps in order, the threads in a halving tree; then one
 * division by n * m.  SRGAN_WASSERSTEIN_MAX_VALUES is the largest power of two whose keys (4 bytes) and tags (1 byte) fit the
 * 160 KiB of LDS a workgroup may take together with the 8 KiB of scan and reduction scratch: 16384 values = 64 KiB + 16 KiB
 * (32768 values would fill the 160 KiB with keys and tags alone).  A NULL pointer, n < 1 or m < 1: SRGAN_EINVAL;
 * n + m > SRGAN_WASSERSTEIN_MAX_VALUES: SRGAN_EUNSUPPORTED. */
#define SRGAN_WASSERSTEIN_MAX_VALUES 16384
int srgan_wasserstein_1d(const float* u, int32_t n, const float* v, int32_t m, float* out, void* stream);
/* srgan_kde_curves: C Gaussian kernel-density curves, each as seaborn's kdeplot(data, bw=factor, cut=cut, gridsize=G) draws it
 * without statsmodels: scipy.stats.gaussian_kde(data, bw_method=factor) on linspace(min - cut * h, max + cut * h, G), h = factor *
 * std(data, ddof=1).  samples: the curves' values back to back, curve c = samples[offsets[c] .. offsets[c + 1]) (offsets: C + 1
 * int32, non-decreasing, offsets[0] >= 0); support, density [C, G]; stats [C, 4] = (count, min, max, h).  First launch, one
 * workgroup per curve: min, max and (count, mean, M2) in a fixed tree (Chan's merge), h = factor * sqrt(M2 / (count - 1)).
 * Second launch, one thread per (c, g): lo = min - cut * h, support[c, g] = lo + g * ((max + cut * h - lo) / (G - 1)) with every
 * operation rounded to fp32 on its own; density[c, g] = (sum_i exp(-0.5 * ((support[c, g] - x_i) * (1 / h))^2)) * (1 / (count * h *
 * sqrt(2 pi))), the samples staged through LDS and added in stored order.  A curve with fewer than 2 samples, or whose h is 0 or
 * not finite, is invalid: stats[c, 3] = 0 and its support and density rows are zeros, never NaN (min = max = 0 for an empty
 * curve).  A NULL pointer, C < 1, G < 2, factor <= 0 or cut < 0 (or either not finite): SRGAN_EINVAL; C * G above
 * max_tensor_elements or C > 65535: SRGAN_ERANGE.  The length of `samples` is on the device only: offsets[C] <=
 * max_tensor_elements is the caller's to keep. */
int srgan_kde_curves(const float* samples, const int32_t* offsets, int32_t C, int32_t G, float factor, float cut, float* support,
                     float* density, float* stats, void* stream);
/* srgan_curve_frame: a line chart out [3, H, W], planar RGB in [0, 1], one thread per pixel (a gather).  Data coordinates map to
 * pixel coordinates by px = (x - x_lo) / (x_hi - x_lo) * W - 0.5, py = (y_hi - y) / (y_hi - y_lo) * H - 0.5; pixel (row r, column
 * c) has its centre at (px, py) = (c, r).  The colour starts as background[3]; then the grid: one vertical line per x_ticks[n_x]
 * and one horizontal line per y_ticks[n_y] (data coordinates, device arrays; n_x / n_y may be 0, the array then NULL), one pixel
 * wide, in grid_colour[3]; then the C polylines in order, polyline k = vertices[offsets[k] .. offsets[k + 1]) (vertices [total, 2]
 * = (x, y) in data coordinates, offsets C + 1 int32) in colours[k, 0..2] at widths[k] pixels; fewer than 2 vertices: skipped.
 * Each line is composited as colour = colour * (1 - a) + line colour * a with the coverage a = clamp(0.5 + width / 2 - d, 0, 1),
 * d = the distance in pixels from the pixel's centre to the line (for a polyline the smallest over its segments, each taken in
 * coordinates relative to the segment's first vertex; a segment of length 0 is a point).  So a width <= -1 draws nothing.
 * Nothing outside the frame is special-cased: a curve above y_hi simply leaves it.  C may be 0 (vertices, offsets, colours,
 * widths then unused).  A NULL required pointer, H or W < 1, C, n_x or n_y < 0, a non-finite bound, x_hi <= x_lo or
 * y_hi <= y_lo: SRGAN_EINVAL; 3 * H * W above max_tensor_elements: SRGAN_ERANGE. */
int srgan_curve_frame(const float* vertices, const int32_t* offsets, int32_t C, const float* colours, const float* widths,
                      int32_t H, int32_t W, float x_lo, float x_hi, float y_lo, float y_hi, const float* background,
                      const float* grid_colour, const float* x_ticks, int32_t n_x, const float* y_ticks, int32_t n_y, float* out,
                      void* stream);

/* ---- histogram summaries on the device (SRGAN_FEATURE_SUMMARY_HISTOGRAM) -------------------------------------------------------
 * srgan_tensor_histogram: the record a summary writer logs for a tensor (the reference wrapper's add_histogram, utility.py:35-39),
 * of x [n] fp32 on the device, into out = device double[5 + (bins + 1) + bins]:
 *   out[0..4] = {min, max, sum, sum_squares, finite_count}     out[5 .. 5 + bins] = edges     out[6 + bins ..] = counts
 * Only FINITE elements count: NaN and +-inf are left out, and n - finite_count tells how many there were.  min and max are over
 * the finite elements, a zero minimum or maximum (of either sign) is reported as +0.0; sum and sum_squares are fp64 sums of the
 * fp32 values (each square formed in fp64, where it is exact), started from +0.0.  Edges, in fp64 without FMA contraction:
 * lo = min, hi = max, or lo = min - 0.5, hi = max + 0.5 when min == max (NumPy's rule); edge_i = lo + i * ((hi - lo) / bins) for
 * i < bins and edge_bins = hi exactly.  Element x belongs to the largest i <= bins - 1 with edge_i <= x, so x == hi goes to
 * bins - 1: np.histogram(x, bins=edges).  The bin is found by an estimate that is then corrected against the stored edges: the
 * result is the comparison's.  Counts are summed as integers (32-bit per workgroup in LDS, 64-bit across workgroups) and
 * converted at the end: exact above 2^24.  No finite element (n == 0 included): all of out is +0.0.
 * Two launches on `stream`: the moments (the workgroups' five fp64 values meet in the stream's workspace in a fixed order, see
 * srgan_split_is_ordered; no floating-point atomics, two calls give the same bits), then edges and counts.  16-byte loads over
 * the 16-byte aligned body of x, single floats for the at most 3 + 3 elements around it, with the same results.  A stream
 * without a registered workspace gets one workgroup per launch: the same record (the sums in another order), slowly.  Not for
 * use under stream capture.
 * Before any device work: NULL x with n > 0, NULL out, n < 0, bins outside [1, 1024], x not 4-byte or out not 8-byte aligned:
 * SRGAN_EINVAL; n above max_tensor_elements: SRGAN_ERANGE. */
int srgan_tensor_histogram(const float* x, int64_t n, int32_t bins, double* out, void* stream);

/* Offline ikNN label of a crowd scene (reference crowd/database_preprocessor.py:93-101,266-290: generate_knn_map +
 * 1 / (map + epsilon)): out[y, x] = 1 / (mean over the k nearest heads of the Euclidean distance from (y, x), each
 * clipped at upper_bound when upper_bound > 0, + epsilon).  heads_yx: M (y, x) pairs, float; k <= 8 and k = min(k, M) as in the reference. */
int srgan_crowd_iknn_map(const float* heads_yx, int32_t M, int32_t H, int32_t W, int32_t k, float epsilon, float upper_bound,
                         float* out, void* stream);
/* Gaussian density label before its final rescaling (reference generate_density_label + make_gaussian,
 * crowd/database_preprocessor.py:110-249), every variant: out[y, x] = sum over the heads' (and bodies') windowed Gaussians,
 * each normalised by body_parts x its unclipped window sum.
 *   perspective == NULL: sigma_h = beta * mean distance of head h to its <= 11 nearest heads including itself (the
 *     "density{beta}" labels of :82-91);
 *   perspective = device map [H][W]: sigma_h = 0.2 m * perspective[y_h, x_h]; flag 2 (ignore_tiny) drops heads with a
 *     perspective < 3.1 (they do not count); flag 1 (include_body) adds a second Gaussian 0.875 m below the head with sigma
 *     (0.2 m, 0.5 m) * perspective and halves both normalisers;
 *   flag 4: perspective_resizing = False (sigma = 8 pixels); flag 8: positions are (x, y) pairs (yx_order = False).
 * Window half-sizes int(2 sigma).  workspace: 64 * M bytes of device memory; after the call float 7 of record 2 * h is 1
 * when head h counts.  The caller multiplies by counted heads / sum(out) (force_full_image_count_normalize). */
int srgan_crowd_density_label(const float* heads, int32_t M, int32_t H, int32_t W, float beta, const float* perspective,
                              int32_t flags, void* workspace, float* out, void* stream);

/* Adam on a flat arena, torch.optim.Adam defaults and operation order (reference srgan.py:131-138,266,297,305);
 * `step` is the 1-based update count. */
int srgan_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int32_t step, void* stream);
/* The same update with the count kept on the device: `state` = 3 x 4 bytes {int32 updates so far, float, float} owned
 * by the caller (initialise the first word; the other two are scratch for the bias corrections).  Every call advances
 * the count by one ON THE STREAM, so a HIP graph that captured the call replays as the next update each time. */
int srgan_adam_step_counted(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int32_t* state, void* stream);

/* Gradient buckets on the wire in bf16 (data-parallel exchange of the comm-sensitive configurations; the
 * reference has no collectives: its gradients complete at srgan.py:264,295,304 and stay on one device): fp32 -> bf16
 * (round to nearest even) and back; both buffers 16-byte aligned.  The master gradients stay fp32. */
int srgan_pack_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);
int srgan_unpack_bf16(const uint16_t* src, float* dst, int64_t n, void* stream);

/* ---- collectives (RCCL over xGMI) -------------------------------------------------------------------------------
 * The reference has no collectives (one device: its batch means are `features.mean(0)`, srgan.py:442-443, and its
 * gradients complete on that device at srgan.py:264,295,304); the data-parallel path needs the SUM of the
 * ranks' feature sums in the forward pass (F floats: 80 for crowd) and the sum of the flat gradient arenas.  These are thin
 * wrappers: RCCL is resolved with dlopen("librccl.so.1") at first use -- the copy already mapped by the process if there
 * is one -- so the library has no link-time dependency on it.  A communicator belongs to the device that was current
 * when it was created; collectives are asynchronous on `stream`, in issue order; `dtype`: 0 = fp32, 1 = bf16 (the wire
 * format of srgan_pack_bf16).  A failing RCCL call returns 10000 + ncclResult_t with RCCL's message in srgan_last_error();
 * -2 when RCCL cannot be loaded. */
int srgan_comm_available(void);                               /* 1 when librccl could be resolved, else 0 (no error) */
int srgan_comm_unique_id(void* id128);                        /* ncclGetUniqueId: 128 bytes, made on rank 0 and handed to every rank by the caller */
int srgan_comm_init(void** comm, int32_t world_size, int32_t rank, const void* id128);   /* ncclCommInitRank on the current device */
int srgan_comm_world_size(void* comm, int32_t* world_size);
int srgan_comm_destroy(void* comm);
/* recv[i] = sum over ranks of send[i], i < count (send == recv: in place): gradient buckets and the tiny feature sums */
int srgan_all_reduce_sum(void* comm, const void* send, void* recv, int64_t count, int32_t dtype, void* stream);
/* the same sum as two halves over all links at once (point-to-point xGMI): rank r receives elements [r, r + 1) * recv_count
 * of the sum of send[0 .. world * recv_count); all_gather puts rank r's send_count elements at [r, r + 1) * send_count */
int srgan_reduce_scatter_sum(void* comm, const void* send, void* recv, int64_t recv_count, int32_t dtype, void* stream);
int srgan_all_gather(void* comm, const void* send, void* recv, int64_t send_count, int32_t dtype, void* stream);
/* ABI 1.1: buffer[0 .. count) of rank `root` to every rank, in place (ncclBroadcast): the initial weights, so that a caller whose
 * control plane is a host channel (TCP store, gloo) needs no second device transport */
int srgan_broadcast(void* comm, void* buffer, int64_t count, int32_t dtype, int32_t root, void* stream);

/* ---- 16-bit data path (ABI 1.1; BASELINE.json configs[1] "bf16" and configs[4] "fp16") ---------------------------------
 * "Blocked" tensors: logical [N, C, H, W] stored as [N][ceil(C / 8)][H][W][8] elements of bf16 (`dtype` 1) or fp16 (2); the 8
 * channels of a group at one pixel are one 16-byte slot = one MFMA operand fragment (sr-gan_amd/csrc/blocked16.h); channels
 * beyond C inside the last group hold zeros; an [N, F] matrix is the H = W = 1 case (row-major, row pitch ceil(F / 8) slots).
 * Activations, their gradients and a per-layer shadow of the weights live in this form; master weights, weight / bias
 * gradients (accumulated into), Adam and the losses stay fp32.  The reference has no analogue (it is fp32-only);
 * the call sites served are VGG-16's `conv3x3 -> ReLU`, `MaxPool2d(2, 2)` and `Linear -> ReLU` (age/vgg.py:33-41,70-84) and
 * the DCGAN stacks' `leaky_relu(conv)` (age/models.py:48-50,70-73).
 * epi (epilogue of a contraction): 0 = store; 1 = + bias (may be NULL), then leaky_relu with `slope` (0 = relu, 1 = identity);
 * 2 = multiply by the derivative of the activation that produced `ref` (1 where ref > 0, `slope` elsewhere; ref has the
 * output's shape): the gradient with respect to the PRE-activation tensor leaves the kernel, the un-masked one never exists.
 * Rounding: every 16-bit store is ONE round to nearest even of the fp32 value (ties to the even neighbour, beyond the largest
 * finite value to inf), fp32 subnormal inputs and 16-bit subnormal results included: nothing is flushed to zero, and
 * srgan_h_unpack is the exact conversion of all 65536 bit patterns.  srgan_h_add is one fp32 addition and one such rounding.
 * NaN and mask rule: "ref > 0" is decided per storage type.  The 16-bit forms (dtype 1 / 2) test the stored BITS -- sign bit
 * clear and not zero ((int16_t)bits > 0) -- in srgan_h_pack's mask, every contraction's epi 2, the blocked batch norm and
 * srgan_h_maxpool2_bwd's `masked` (on the pooled value): positive subnormals and +inf are positive, +-0 and everything with
 * the sign bit set are not, and a NaN counts as positive exactly when its sign bit is clear.  dtype 0 (fp32 slots) tests
 * `ref > 0.f` like the fp32 kernels above: a NaN of either sign is not positive.  The 2x2 max-pool takes the FIRST maximum in
 * scan order (0,0), (0,1), (1,0), (1,1) under `>`: torch's choice for every window without a NaN (+0 and -0 tie: the first
 * wins).  A NaN never beats the running maximum and is never beaten: a NaN at window position (0,0) is the result and the
 * arg-max, a NaN at one of the other three positions is skipped (torch propagates a NaN from every position). */
int srgan_h_pack(const float* x_nchw, void* out, const void* mask_ref, float slope, int32_t N, int32_t C, int64_t HW, int dtype,
                 void* stream);                                /* fp32 NCHW -> blocked (times mask(ref) when mask_ref != NULL) */
int srgan_h_unpack(const void* x, float* out_nchw, int32_t N, int32_t C, int64_t HW, int dtype, void* stream);
int srgan_h_add(const void* a, const void* b, void* out, int64_t slots, int dtype, void* stream);
int srgan_h_channel_sums(const void* x, float* out, int32_t N, int32_t C, int64_t HW, int dtype, void* stream);   /* out[c] += ... (bias gradient) */
/* mode 0: out = max_pool2d(x, 2, 2); mode 2: out = g (shape of x) gathered at the arg-max of x.  planes = N * groups. */
int srgan_h_maxpool2(const void* x, const void* g, void* out, int64_t planes, int32_t H, int32_t W, int mode, int dtype, void* stream);
/* gx (shape of x) = gp placed at the arg-max of x (first maximum in scan order: torch's rule without a NaN in the window, the
 * NaN rule above with one), zeros at the other three positions, times mask(pooled x, slope) if masked */
int srgan_h_maxpool2_bwd(const void* x, const void* gp, void* gx, int64_t planes, int32_t H, int32_t W, int masked, float slope,
                         int dtype, void* stream);
/* The 16-bit shadow of conv2d weights w[K][C][R][S] in operand slots; transposed = 1: the data-gradient operand (rows = C,
 * reduced over K, taps mirrored).  srgan_h_conv_weight_slots(rows, reduced, R, S) 16-byte slots. */
int64_t srgan_h_conv_weight_slots(int32_t rows, int32_t reduced, int32_t R, int32_t S);
int srgan_h_pack_conv_weights(const float* w, void* packed, int32_t K, int32_t C, int32_t R, int32_t S, int transposed, int dtype,
                              void* stream);
/* out[N, C_out, H, W] = epi(conv2d 3x3 / stride 1 / pad 1 of x[N, C_in, H, W]) with a packed operand of `rows` rows. */
int srgan_h_conv3x3(const void* x, const void* packed, const float* bias, const void* ref, float slope, int epi, void* out,
                    int32_t N, int32_t C_in, int32_t C_out, int32_t rows, int32_t H, int32_t W, int dtype, void* stream);
/* gw[C_out][C_in][3][3] (fp32) += weight gradient from x[N, C_in, H, W] and gy[N, C_out, H, W] (fixed summation order) */
int srgan_h_conv3x3_wgrad(const void* x, const void* gy, float* gw, int32_t N, int32_t C_in, int32_t C_out, int32_t H, int32_t W,
                          int dtype, void* stream);
/* out16[rows][cols] = src[map(r, row_plane) * row_stride + map(c, col_plane) * col_stride] (0 outside rows_real x cols_real);
 * map(i, P) = NCHW-flattened index of element i of a flattened blocked tensor with P pixels per channel (P <= 1: i). */
int srgan_h_pack_matrix(const float* src, void* out, int64_t rows, int64_t cols, int64_t rows_real, int64_t cols_real,
                        int64_t row_stride, int64_t col_stride, int32_t row_plane, int32_t col_plane, int dtype, void* stream);
/* out[N][out_cols] = epi(B[N][K] * A[M][K]^T): torch.nn.functional.linear (age/vgg.py:33-41) and its data gradient */
int srgan_h_gemm(const void* a, const void* b, const float* bias, const void* ref, float slope, int epi, void* out, int32_t M,
                 int32_t N, int32_t K, int32_t out_cols, int32_t bias_entries, int dtype, void* stream);
/* gw element (m, k) at gw[map(m, row_plane) * ldw_m + map(k, col_plane) * ldw_k] += sum_n S[n][m] * X[n][k] */
int srgan_h_linear_wgrad(const void* s, const void* x, float* gw, int32_t N, int32_t M, int32_t K, int64_t M_real, int64_t K_real,
                         int64_t ldw_m, int64_t ldw_k, int32_t row_plane, int32_t col_plane, int dtype, void* stream);

/* 4x4 / stride 2 / pad 1 pair (the DCGAN stacks, reference age/models.py:37-51,61-73).  A weight tensor [A][B][4][4] in torch's
 * layout -- conv2d weights [K][C][4][4]: A = K, B = C; conv_transpose2d weights [Cin][Cout][4][4]: A = Cin, B = Cout -- always
 * has A = the channels of the tensor on the SMALL (H/2 x W/2) plane.  direction 0 "down" (big -> small plane, rows = A): conv2d's
 * forward, conv_transpose2d's data gradient; direction 1 "up" (small -> big plane, rows = B, the four output parity classes):
 * conv_transpose2d's forward, conv2d's data gradient.  epi as srgan_h_conv3x3.  This family (and srgan_h_pack / _unpack / _add /
 * _channel_sums) also takes `dtype` 0: fp32 tensors in the same blocked layout with FOUR channels per 16-byte slot
 * ([N][ceil(C / 4)][H][W][4]), v_mfma_f32_32x32x2_f32 -- the exact form (the fp32 gradient-penalty chain of configs[4], the
 * crowd generator, reference crowd/models.py:132-146). */
int64_t srgan_h_k4s2_weight_slots(int32_t A, int32_t B, int direction, int dtype);
int srgan_h_pack_k4s2_weights(const float* w, void* packed, int32_t A, int32_t B, int direction, int dtype, void* stream);
/* The batched form of the two weight packers above: every convolution shadow of a network re-rounded by ONE launch behind its
 * optimizer update.  The caller keeps a device array of jobs, srgan_h_pack_job_bytes() each; a job function takes the arguments
 * of its single-layer call, writes the job(s) at `jobs` (HOST memory; the "up" direction of the 4x4 family writes four) with
 * workgroups from `first_block` on and returns the number of workgroups they take (< 0: error); srgan_h_pack_batched launches
 * `count` jobs of `blocks` workgroups in total from the device copy of the array. */
int32_t srgan_h_pack_job_bytes(void);
int64_t srgan_h_pack_job_conv_weights(void* jobs, int64_t first_block, const float* w, void* packed, int32_t K, int32_t C, int32_t R,
                                      int32_t S, int transposed, int dtype);
int64_t srgan_h_pack_job_k4s2_weights(void* jobs, int64_t first_block, const float* w, void* packed, int32_t A, int32_t B,
                                      int direction, int dtype, int32_t* jobs_written);
/* The matrix shadows and the bias rows as jobs of the same launch (SRGAN_FEATURE_BATCHED_SHADOWS): srgan_h_pack_job_matrix
 * takes the arguments of srgan_h_pack_matrix (every extent and stride below 2^31) and writes one job; srgan_h_pack_job_bias_rows
 * writes the fp32 rows[(g * plane + p) * 8 + j] = bias[8 g + j] (0 from `channels` on; ceil(channels / 8) * plane * 8 floats) of a
 * seed transposed convolution (a linear map onto [channels][plane]). */
int64_t srgan_h_pack_job_matrix(void* jobs, int64_t first_block, const float* src, void* out, int64_t rows, int64_t cols,
                                int64_t rows_real, int64_t cols_real, int64_t row_stride, int64_t col_stride, int32_t row_plane,
                                int32_t col_plane, int dtype);
int64_t srgan_h_pack_job_bias_rows(void* jobs, int64_t first_block, const float* bias, float* rows, int32_t channels, int32_t plane);
/* The fp32 weight images of a 3x3 convolution w[K][C][3][3] (SRGAN_FEATURE_CONV3X3_WEIGHT_IMAGE; layout above): transposed 0
 * writes the forward image (srgan_conv3x3_image_floats(C, K) floats), 1 the data gradient's (srgan_conv3x3_image_floats(K, C)),
 * padding zeros included; `image` 16-byte aligned.  The job form is one more job kind of srgan_h_pack_batched. */
int srgan_h_pack_conv3x3_image(const float* w, float* image, int32_t K, int32_t C, int transposed, void* stream);
int64_t srgan_h_pack_job_conv3x3_image(void* jobs, int64_t first_block, const float* w, float* image, int32_t K, int32_t C,
                                       int transposed);
int srgan_h_pack_batched(const void* jobs_device, int32_t count, int64_t blocks, void* stream);
int srgan_h_conv4x4s2(const void* x, const void* packed, const float* bias, const void* ref, float slope, int epi, void* out,
                      int32_t N, int32_t C_in, int32_t rows, int32_t H, int32_t W, int dtype, void* stream);
int srgan_h_conv_transpose4x4s2(const void* x, const void* packed, const float* bias, const void* ref, float slope, int epi,
                                void* out, int32_t N, int32_t C_in, int32_t rows, int32_t h, int32_t w, int dtype, void* stream);
/* gw (fp32 [A][B][4][4]) += weight gradient from `small` [N, A, H/2, W/2] and `big` [N, B, H, W] (small_is_rows must be 1) */
int srgan_h_k4s2_wgrad(const void* big, const void* small, float* gw, int32_t N, int32_t C_big, int32_t C_small, int32_t H, int32_t W,
                       int small_is_rows, int dtype, void* stream);

/* Training-mode batch normalisation (batch statistics) of a BLOCKED tensor (SRGAN_FEATURE_BLOCKED_BATCH_NORM): logical
 * shape [N, C, HW], dtype 0 (fp32, 4 channels per slot) / 1 (bf16) / 2 (fp16, 8 per slot), M = N * HW values per channel --
 * the norm layers of a DCGAN generator that stays on the blocked data path.  mean / inv_std / gamma / beta / sums and the
 * running buffers are fp32 [C] ([2][C] for sums); all arithmetic is fp32 on the stored elements converted exactly, and y / gx
 * are rounded to nearest even once.  Channels beyond C in the last group are written as zeros.
 * _stats: as srgan_batch_norm_train_stats -- ONE read of x, (count, mean, M2) partials merged by Chan's formula, the
 *   workgroups of a channel group meeting in the stream's workspace in a fixed order (bit-reproducible; without a workspace
 *   one workgroup per group); running_mean / running_var / num_batches_tracked (each may be NULL) updated on the device
 *   with the unbiased variance and `momentum`.
 * _fwd: y = leaky((x - mean) * inv_std * gamma + beta, slope) (slope = 1: no activation); eval mode passes the running
 *   mean and its inverse standard deviation.
 * _bwd_reduce: `s` is the PRE-MASKED gradient (already multiplied by the activation's derivative, the convention of the
 *   blocked path): sums[c] = sum s, sums[C + c] = sum s * xhat (xhat = (x - mean) * inv_std), in a fixed order;
 *   g_beta[c] += sums[c] and g_gamma[c] += sums[C + c] when given (each may be NULL).
 * _bwd_apply: gx = gamma * inv_std * (s - sums[c] / M - xhat * sums[C + c] / M), times (ref > 0 ? 1 : slope) when `ref`
 *   (the blocked tensor whose sign pattern masks x; may be NULL) is given.
 * All four: unknown dtype, a NULL required pointer or M < 2: SRGAN_EINVAL; M > 2^24: SRGAN_ERANGE (before any device
 * work).  Nothing but x, mean and inv_std is kept between the passes. */
int srgan_h_batch_norm_stats(const void* x, float* mean, float* inv_std, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, float momentum, float eps, int32_t N, int32_t C, int64_t HW,
                             int32_t dtype, void* stream);
int srgan_h_batch_norm_fwd(const void* x, const float* mean, const float* inv_std, const float* gamma, const float* beta,
                           float slope, void* y, int32_t N, int32_t C, int64_t HW, int32_t dtype, void* stream);
int srgan_h_batch_norm_bwd_reduce(const void* s, const void* x, const float* mean, const float* inv_std, float* sums,
                                  float* g_gamma, float* g_beta, int32_t N, int32_t C, int64_t HW, int32_t dtype, void* stream);
int srgan_h_batch_norm_bwd_apply(const void* s, const void* x, const float* mean, const float* inv_std, const float* gamma,
                                 const float* sums, const void* ref, float slope, void* gx, int32_t N, int32_t C, int64_t HW,
                                 int32_t dtype, void* stream);
/* The backward of a norm with GIVEN statistics -- the frozen norm layers of the DCGAN discriminators, y = (x - mean) * inv_std *
 * gamma + beta, whose forward is srgan_h_batch_norm_fwd with the running statistics -- on BLOCKED tensors
 * (SRGAN_FEATURE_BLOCKED_FROZEN_NORM): a per-channel affine map, so ONE pass reads `s` once (and `x`, `ref` once when needed)
 * and writes gx once:
 *   gx = s * gamma[c] * inv_std[c], times (ref > 0 ? 1 : slope) when `ref` is given;
 *   g_gamma[c] += inv_std[c] * sum_{n,i} s * (x - mean[c]);     g_beta[c] += sum_{n,i} s.
 * Each of gx, g_gamma, g_beta may be NULL (not all three); mean may be NULL (= zero); x is needed only with g_gamma.  `s` is
 * used as it arrives (PRE-MASKED by the layer's own activation, as everywhere on the blocked path); `ref` / `slope` are the
 * mask of the tensor x itself, as in srgan_h_batch_norm_bwd_apply.  The same call is the recorded backward (gx alone) and the
 * double backward (s = the incoming cotangent, x = the first sweep's gradient, mean = NULL: gx and g_gamma in one pass).
 * fp32 arithmetic on the stored elements, gx rounded to nearest even once, channels beyond C in the last group written as
 * zeros; the per-channel sums of several workgroups meet in the stream's workspace in a fixed order (bit-reproducible; without
 * a workspace one workgroup per channel group).  Before any device work: unknown dtype, NULL s / inv_std / gamma, all three
 * outputs NULL, or g_gamma without x: SRGAN_EINVAL; more than max_tensor_elements (N * C * HW): SRGAN_ERANGE.  M = N * HW = 1
 * is legal (nothing is divided by a count). */
int srgan_h_frozen_norm_bwd(const void* s, const void* x, const float* mean, const float* inv_std, const float* gamma,
                            const void* ref, float slope, void* gx, float* g_gamma, float* g_beta, int32_t N, int32_t C, int64_t HW,
                            int32_t dtype, void* stream);

/* ---- measurement ---------------------------------------------------------------------------------------------
 * Between begin and end every contraction launch (conv / gemm passes) is bracketed by a pair of HIP events on
 * its launch stream; end() synchronises and returns the summed kernel time, the summed logical 2*M*N*K, the
 * part of it executed by the MFMA kernel, and the launch count (bench.py's roofline leg). */
int srgan_profile_begin(void);
int srgan_profile_end(double* kernel_ms, double* flops, double* mfma_flops, int64_t* launches);
/* Algorithmic HBM bytes of the bracketed launches: every operand / result element once, 4 B each (a 3x3 tap or a
 * stride class does not count an input element twice): the figure bench.py's roofline.algorithmic_bytes_per_step
 * reports next to the PMC traffic. */
int srgan_profile_bytes(double* algorithmic_bytes_total);
/* The part of the bracketed launches that ran with bf16 / fp16 MFMA operands: logical FLOPs and summed kernel time (the
 * mixed-precision bench lines price it against the 2.5 PFLOP/s dense bf16 / fp16 peak, the rest against 157.3 TFLOP/s). */
int srgan_profile_mixed(double* flops, double* kernel_ms);
/* Per-shape text report of the last profiled region ("M N K kind bm bn split akf bkf count ms bytes" per line; kind:
 * 0 gg_direct, 1 gg_mfma, 2 conv3x3_lds, 3 pointwise, 4 conv3x3_wgrad, 5 gg_rows, 6 pointwise_wgrad, (7 unused,)
 * 8 pointwise_ksplit, 9 gg_dot, 10 stem7x7_fwd, 11 stem7x7_wgrad, 12 stem7x7_bwd_data, 13 pointwise_ring, 14 hconv3x3,
 * 15 hwgrad3x3, 16 hgemm, 17 hlinear_wgrad, 18 hconv4x4s2, 19 hwgrad4x4s2, 20 bn_stats, 21 bn_fwd, 22 bn_bwd_reduce,
 * 23 bn_bwd_apply, 24 h_frozen_norm_bwd; for kind 2, akf = 1 marks a launch that staged its weights from the weight image);
 * returns the bytes needed. */
int64_t srgan_profile_report(char* buffer, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* SRGAN_HIP_H */
