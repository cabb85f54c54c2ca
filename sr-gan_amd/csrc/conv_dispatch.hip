// conv_dispatch.hip -- the convolution C ABI: which kernel a convolution pass takes (the routing predicates) and the entry
// points that apply them, in the order that is the behaviour.  Host code only: the kernels live with their launchers
// (conv3x3.hip, pointwise*.hip, conv3x3_wgrad.hip, stem7x7.hip, and gather_gemm_kernels.hip for everything else).
#include "common.h"
#include "split_finish.h"
#include "gather_gemm.h"
#include "conv_plan.h"
#include "launchers.h"
#include <vector>

using namespace srgan;

// 1x1 / stride 1 / unpadded: the register-streamed pointwise kernel (any plane size: an image's last 32-pixel group may
// be ragged; planes of fewer than 32 pixels stay on the generic kernel).
static bool use_pointwise(const ConvGeom& g, int out_channels, int force) {
  const int in_channels = out_channels == g.K ? g.C : g.K;     // forward: C -> K; data gradient: K -> C
  const bool plane_ok = g.H * g.W >= 32;       // (geom_ok: H, W >= 1)
  return force == 0 && pointwise(g) && plane_ok && out_channels >= 8 && in_channels % 2 == 0;
}

// 3x3 / stride 1 / pad 1 with enough width to fill most of a 16-pixel tile row (two image rows share a 32-pixel MFMA
// column block): the LDS-halo kernel.
static bool use_conv3x3(const ConvGeom& g, int out_channels, int force) {
  return force == 0 && g.R == 3 && g.S == 3 && g.sh == 1 && g.sw == 1 && g.ph == 1 && g.pw == 1 &&
         g.W >= CONV3_MIN_WIDTH && out_channels >= 8;
}

// Mixed precision also takes the 4 x 4 planes (whole images side by side in a tile: conv3x3_mixed_small_kernel) and
// fewer than 8 output channels -- the gradient with respect to a 3-channel image, which the penalty chain of the VGG / DCGAN
// discriminators asks for (reference srgan.py:366-370): 29 of a 32-row tile's rows are padding there, and the generic
// kernel's gather still made it six times slower (5.9 TF/s on [3 x 524 288] x 576).
static bool use_conv3x3_mixed(const ConvGeom& g, int out_channels) {
  if (use_conv3x3(g, out_channels, 0)) return true;
  const bool geometry = g.R == 3 && g.S == 3 && g.sh == 1 && g.sw == 1 && g.ph == 1 && g.pw == 1;
  if (!geometry) return false;
  return (g.H == 4 && g.W == 4 && out_channels >= 8) || (g.W >= CONV3_MIN_WIDTH && out_channels >= 1);
}

// Weight gradient of a 3x3 / stride 1 / pad 1 convolution with at least one wave's worth of input channels: the
// LDS-patch kernel of conv3x3_wgrad.hip.
// `aligned_only`: widths that are a multiple of 4 with 16-byte aligned rows (the float4 staging; the mixed-precision
// variants have no other); otherwise the kernel's ragged variant also takes the 14- and 7-wide planes of 224 x 224.
static bool wgrad3x3_geometry(const ConvGeom& g, int min_width = 7, bool aligned_only = false) {
  const bool aligned = g.W % 4 == 0 && g.x_bs % 4 == 0 && g.y_bs % 4 == 0;
  if (!aligned && aligned_only) return false;
  return g.R == 3 && g.S == 3 && g.sh == 1 && g.sw == 1 && g.ph == 1 && g.pw == 1 && g.W >= min_width && g.C >= 32;
}

static bool use_wgrad3x3(const ConvGeom& g, int force) { return force == 0 && wgrad3x3_geometry(g); }

static bool pointwise_wgrad_geometry(const ConvGeom& g) {
  return pointwise(g) && g.H * g.W >= 32 && g.C >= 16 && g.K >= 16;
}

// Weight gradient of a 1x1 / stride 1 convolution: the register-streamed kernel of pointwise_wgrad.hip (whole 32-pixel
// chunks with 16-byte aligned rows, or its ragged variant).
static bool use_pointwise_wgrad(const ConvGeom& g, int force) {
  return force == 0 && pointwise_wgrad_enabled() && pointwise_wgrad_geometry(g);
}

// ------------------------------------------------------------------------------------------- C ABI
extern "C" {

static bool dtype_ok(int dtype) { return dtype >= 0 && dtype <= 2; }

static bool to_geom(const srgan_conv_desc* d, ConvGeom& g) {
  if (d == nullptr) return false;
  g.N = d->N; g.C = d->C; g.H = d->H; g.W = d->W; g.K = d->K; g.R = d->R; g.S = d->S;
  g.sh = d->stride_h; g.sw = d->stride_w; g.ph = d->pad_h; g.pw = d->pad_w; g.OH = d->OH; g.OW = d->OW;
  g.x_bs = d->x_batch_stride; g.y_bs = d->y_batch_stride;
  return geom_ok(g);
}

// Descriptor -> geometry with the two failure classes kept apart: a malformed descriptor (-1) and one whose tensors pass
// the 2^31-element limit of the 32-bit offsets (-3, with the extent in the message so that the caller can split the batch).
#define SRGAN_GEOM(desc, g, what)                                                                        \
  do {                                                                                                   \
    SRGAN_REQUIRE(to_geom(desc, g), SRGAN_EINVAL, what " geometry");                                     \
    if (geom_largest_extent(g) >= ((int64_t)1 << 31)) {                                                  \
      set_error(what ": a tensor of %lld elements (batch %d) exceeds the 2^31 - 1 element limit",       \
                (long long)geom_largest_extent(g), (int)g.N);                                            \
      return SRGAN_ERANGE;                                                                               \
    }                                                                                                    \
  } while (0)

int srgan_conv2d_fwd(const srgan_conv_desc* desc, const float* x, const float* w, const float* bias, float* y,
                     int force_kernel, void* stream) {
  ConvGeom g;
  SRGAN_GEOM(desc, g, "srgan_conv2d_fwd");
  SRGAN_REQUIRE(x && w && y, SRGAN_EINVAL, "srgan_conv2d_fwd pointers");
  const int dtype = desc->compute_dtype;
  SRGAN_REQUIRE(dtype_ok(dtype), SRGAN_EINVAL, "srgan_conv2d_fwd compute_dtype");
  if (dtype && force_kernel == 0 && use_conv3x3_mixed(g, g.K))     // mixed precision: the LDS-halo 3x3 kernel, or
    return conv3x3_run(x, g.x_bs, conv3_forward_taps(w, g.C), bias, y, g.y_bs, g.N, g.C, g.K, g.H, g.W, 0, (hipStream_t)stream,
                       nullptr, nullptr, dtype);
  if (dtype) force_kernel = 2;                                      // the generic MFMA kernel for every other geometry
  if (use_pointwise(g, g.K, force_kernel) && ((uintptr_t)w & 15) == 0 &&
      pointwise_ksplit_wanted(g.N, g.C, g.K, g.H * g.W, false))
    return pointwise_ksplit_run(x, g.x_bs, w, bias, y, g.y_bs, g.N, g.C, g.K, g.H * g.W, 0, (hipStream_t)stream, nullptr);
  if (use_pointwise(g, g.K, force_kernel))
    return pointwise_run(x, g.x_bs, w, g.C, 1, bias, y, g.y_bs, g.N, g.C, g.K, g.H * g.W, 0, (hipStream_t)stream);
  if (use_conv3x3(g, g.K, force_kernel))
    return conv3x3_run(x, g.x_bs, conv3_forward_taps(w, g.C), bias, y, g.y_bs, g.N, g.C, g.K, g.H, g.W, 0, (hipStream_t)stream);
  if (force_kernel == 0 && dtype == 0 && bias == nullptr &&
      stem7x7_geometry(g.C, g.K, g.R, g.S, g.sh, g.sw, g.ph, g.pw))
    return stem7x7_fwd_run(x, g.x_bs, w, y, g.y_bs, g.N, g.H, g.W, g.K, g.OH, g.OW, (hipStream_t)stream);
  std::vector<GatherGemm> plans{plan_conv_fwd(g, x, w, bias, y)};
  plans[0].precision = dtype;
  // (y may be a strided-batch view -- a channel slice of a wider buffer: one row per image)
  return gg_run_group(plans, y, g.y_bs, (int64_t)g.K * g.OH * g.OW, g.N, 0, force_kernel, (hipStream_t)stream);
}

int srgan_conv2d_bwd_data(const srgan_conv_desc* desc, const float* gy, const float* w, const float* bias,
                          float* gx, int accumulate, int force_kernel, void* stream) {
  ConvGeom g;
  SRGAN_GEOM(desc, g, "srgan_conv2d_bwd_data");
  SRGAN_REQUIRE(gy && w && gx, SRGAN_EINVAL, "srgan_conv2d_bwd_data pointers");
  SRGAN_REQUIRE(g.x_bs == (int64_t)g.C * g.H * g.W, SRGAN_EUNSUPPORTED, "srgan_conv2d_bwd_data dense gx");
  const int dtype = desc->compute_dtype;
  SRGAN_REQUIRE(dtype_ok(dtype), SRGAN_EINVAL, "srgan_conv2d_bwd_data compute_dtype");
  if (dtype && force_kernel == 0 && use_conv3x3_mixed(g, g.C))
    return conv3x3_run(gy, g.y_bs, conv3_flipped_taps(w, g.C), bias, gx, g.x_bs, g.N, g.K, g.C, g.H, g.W, accumulate,
                       (hipStream_t)stream, nullptr, nullptr, dtype);
  if (force_kernel == 0 && dtype == 0 && bias == nullptr && !accumulate &&
      stem7x7_geometry(g.C, g.K, g.R, g.S, g.sh, g.sw, g.ph, g.pw) && (g.W & 1) == 0 && (((uintptr_t)gx) & 7) == 0)
    return stem7x7_bwd_data_run(gy, g.y_bs, w, gx, g.x_bs, g.N, g.H, g.W, g.K, g.OH, g.OW, (hipStream_t)stream);
  // k4 / s2 / p1 (the DCGAN generators' transposed convolutions, reference crowd/models.py:132-136, age/models.py:37-41,
  // as forward passes; the discriminators' strided convolutions as data gradients): output pixel (2q + a, 2r + b) only
  // meets the 2x2 taps kh = 3 + a - 2i, kw = 3 + b - 2j of the input pixels (q - 1 + i, r - 1 + j), i in {a, a + 1},
  // j in {b, b + 1} -- four 2x2 sub-windows of the LDS-halo 3x3 kernel with strided stores, instead of four gathered
  // GEMMs on the generic kernel (50 TF/s).
  if (force_kernel == 0 && g.R == 4 && g.S == 4 && g.sh == 2 && g.sw == 2 && g.ph == 1 &&
      g.pw == 1 && g.H == 2 * g.OH && g.W == 2 * g.OW && g.OW >= 8 && (g.C >= 8 || dtype) && !accumulate) {   // (mixed: also the 3-channel image gradient)
    // small problems split the input channels over the grid and add with atomics: the output is zeroed once for all classes
    // (only when the split adds with atomics: with a workspace the slices meet in a fixed order and the sums are stored)
    const bool split = conv3x3_splits(g.N, g.K, g.C, g.OH, g.OW, dtype) > 1 && !srgan_split_is_ordered(stream);
    if (split) if (const int status = zero_floats(gx, (int64_t)g.N * g.x_bs, (hipStream_t)stream)) return status;
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        Conv3Placement placement;
        const Conv3Weights taps = conv3_k4s2_class(w, g.C, a, b, g.H, g.W, &placement);
        const int status = conv3x3_run(gy, g.y_bs, taps, bias, gx, g.x_bs, g.N, g.K, g.C, g.OH, g.OW, split ? 2 : 0,
                                       (hipStream_t)stream, nullptr, nullptr, dtype, &placement);
        if (status != SRGAN_OK) return status;
      }
    return SRGAN_OK;
  }
  if (dtype) force_kernel = 2;
  if (use_pointwise(g, g.C, force_kernel))   // the data gradient of a 1x1 convolution is the 1x1 convolution with W^T
    return pointwise_run(gy, g.y_bs, w, 1, g.C, bias, gx, g.x_bs, g.N, g.K, g.C, g.H * g.W, accumulate,
                         (hipStream_t)stream);
  if (use_conv3x3(g, g.C, force_kernel))     // the data gradient is the same convolution with flipped taps
    return conv3x3_run(gy, g.y_bs, conv3_flipped_taps(w, g.C), bias, gx, g.x_bs, g.N, g.K, g.C, g.H, g.W, accumulate,
                       (hipStream_t)stream);
  std::vector<GatherGemm> plans = plan_conv_bwd_data(g, gy, w, bias, gx);
  for (GatherGemm& plan : plans) plan.precision = dtype;
  return gg_run_group(plans, gx, g.x_bs, g.x_bs, g.N, accumulate, force_kernel, (hipStream_t)stream);
}

int srgan_conv2d_bwd_weight(const srgan_conv_desc* desc, const float* x, const float* gy, float* gw,
                            int accumulate, int force_kernel, void* stream) {
  ConvGeom g;
  SRGAN_GEOM(desc, g, "srgan_conv2d_bwd_weight");
  SRGAN_REQUIRE(x && gy && gw, SRGAN_EINVAL, "srgan_conv2d_bwd_weight pointers");
  const int dtype = desc->compute_dtype;
  SRGAN_REQUIRE(dtype_ok(dtype), SRGAN_EINVAL, "srgan_conv2d_bwd_weight compute_dtype");
  // (mixed precision also takes 8-wide planes on the 16-wide tile: half of the columns are dead, but the alternative is
  // the gather-bound generic kernel)
  if (dtype && force_kernel == 0 && wgrad3x3_geometry(g, 8, true) &&
      (((uintptr_t)x | (uintptr_t)gy) & 15) == 0)
    return conv3x3_wgrad_run(x, g.x_bs, gy, g.y_bs, gw, g.N, g.C, g.K, g.H, g.W, accumulate, (hipStream_t)stream, nullptr,
                             dtype);
  if (dtype) force_kernel = 2;
  if (use_pointwise_wgrad(g, force_kernel))
    return pointwise_wgrad_run(x, g.x_bs, gy, g.y_bs, gw, g.N, g.C, g.K, g.H * g.W, accumulate, (hipStream_t)stream);
  if (force_kernel == 0 && dtype == 0 && stem7x7_geometry(g.C, g.K, g.R, g.S, g.sh, g.sw, g.ph, g.pw))
    return stem7x7_wgrad_run(x, g.x_bs, gy, g.y_bs, gw, g.N, g.H, g.W, g.K, g.OH, g.OW, accumulate, (hipStream_t)stream);
  if (use_wgrad3x3(g, force_kernel))
    return conv3x3_wgrad_run(x, g.x_bs, gy, g.y_bs, gw, g.N, g.C, g.K, g.H, g.W, accumulate, (hipStream_t)stream);
  std::vector<GatherGemm> plans{plan_conv_bwd_weight(g, x, gy, gw)};
  plans[0].precision = dtype;
  const int64_t weights = (int64_t)g.K * g.C * g.R * g.S;
  return gg_run_group(plans, gw, weights, weights, 1, accumulate, force_kernel, (hipStream_t)stream);
}

// ---- convolutions whose input is relu(batch_norm_eval(x)) evaluated on the fly (DenseNet norm -> relu -> conv)
static bool bn_ok(const srgan_bn_relu* bn) { return bn && bn->mean && bn->inv_std && bn->gamma && bn->beta; }

int srgan_conv2d_bnrelu_supported(const srgan_conv_desc* desc, int pass) {
  ConvGeom g;
  if (desc && desc->compute_dtype != 0) return 0;       // the fused forms are fp32 kernels
  if (!to_geom(desc, g) || geom_largest_extent(g) >= ((int64_t)1 << 31)) return 0;
  if (pass == 0) {
    if (pointwise(g)) return use_pointwise(g, g.K, 0) ? 1 : 0;
    return (use_conv3x3(g, g.K, 0) && g.C <= 512) ? 1 : 0;
  }
  if (pass == 1) {
    // the epilogue's per-workgroup parameter sums must fit the caller's workspace (<= 1/32 of the gradient tensor's bytes)
    if ((size_t)g.N * g.H * g.W * g.C / 8 > workspace_capacity()) return 0;
    if (pointwise(g)) return use_pointwise(g, g.C, 0) ? 1 : 0;
    return (use_conv3x3(g, g.C, 0) && conv3x3_epilogue_supported(g.N, g.K, g.C, g.H, g.W)) ? 1 : 0;
  }
  if (pass == 2) {
    if (pointwise(g)) return pointwise_wgrad_geometry(g) ? 1 : 0;
    return wgrad3x3_geometry(g) ? 1 : 0;
  }
  return 0;
}

// y_state: 0 = y holds anything (stored over), 2 = y is already zero where the convolution writes (a kernel that splits
// K over the grid then skips its own zero-fill launch; see srgan_conv2d_fwd_bnrelu_splits).
static int fwd_bnrelu(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* w, const float* bias,
                      float* y, int y_state, int* plan_only_split, void* stream, const float* image = nullptr) {
  ConvGeom g;
  SRGAN_GEOM(desc, g, "srgan_conv2d_fwd_bnrelu");
  SRGAN_REQUIRE(plan_only_split || (x && w && y && bn_ok(bn)), SRGAN_EINVAL, "srgan_conv2d_fwd_bnrelu pointers");
  SRGAN_REQUIRE(srgan_conv2d_bnrelu_supported(desc, 0), SRGAN_EUNSUPPORTED, "srgan_conv2d_fwd_bnrelu geometry support");
  const BnVectors coefficients = bn_vectors(bn);
  SRGAN_REQUIRE(image == nullptr || !pointwise(g), SRGAN_EUNSUPPORTED, "srgan_conv2d_fwd_bnrelu_image: 3x3 convolutions");
  if (pointwise(g) && (plan_only_split || ((uintptr_t)w & 15) == 0) &&
      pointwise_ksplit_wanted(g.N, g.C, g.K, g.H * g.W, true)) {
    if (plan_only_split) { *plan_only_split = 1; return SRGAN_OK; }
    return pointwise_ksplit_run(x, g.x_bs, w, bias, y, g.y_bs, g.N, g.C, g.K, g.H * g.W, 0, (hipStream_t)stream,
                                coefficients.v);
  }
  if (pointwise(g))
    return pointwise_run(x, g.x_bs, w, g.C, 1, bias, y, g.y_bs, g.N, g.C, g.K, g.H * g.W, y_state, (hipStream_t)stream,
                         coefficients.v, nullptr, plan_only_split);
  if (plan_only_split) { *plan_only_split = conv3x3_splits(g.N, g.C, g.K, g.H, g.W); return SRGAN_OK; }
  return conv3x3_run(x, g.x_bs, conv3_forward_taps(w, g.C, image), bias, y, g.y_bs, g.N, g.C, g.K, g.H, g.W, y_state,
                     (hipStream_t)stream, coefficients.v);
}

int srgan_conv2d_fwd_bnrelu_image(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* w,
                                  const float* image, const float* bias, float* y, void* stream) {
  SRGAN_REQUIRE(image != nullptr, SRGAN_EINVAL, "srgan_conv2d_fwd_bnrelu_image: the weight image");
  return fwd_bnrelu(desc, x, bn, w, bias, y, 0, nullptr, stream, image);
}

int srgan_conv2d_fwd_bnrelu(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* w,
                            const float* bias, float* y, void* stream) {
  return fwd_bnrelu(desc, x, bn, w, bias, y, 0, nullptr, stream);
}

int srgan_conv2d_fwd_bnrelu_into_zeros(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* w,
                                       const float* bias, float* y, void* stream) {
  return fwd_bnrelu(desc, x, bn, w, bias, y, 2, nullptr, stream);
}

int srgan_conv2d_fwd_bnrelu_splits(const srgan_conv_desc* desc) {
  int split = 0;
  return fwd_bnrelu(desc, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &split, nullptr) == SRGAN_OK ? split : -1;
}

static int bwd_data_bnrelu(const srgan_conv_desc* desc, const float* gy, const float* w, const srgan_bn_relu* bn, const float* x,
                          float* gx, float* g_gamma, float* g_beta, float* partials, int accumulate, void* stream,
                          const float* image = nullptr) {
  ConvGeom g;
  SRGAN_GEOM(desc, g, "srgan_conv2d_bwd_data_bnrelu");
  SRGAN_REQUIRE(gy && w && x && gx && bn_ok(bn), SRGAN_EINVAL, "srgan_conv2d_bwd_data_bnrelu pointers");
  SRGAN_REQUIRE((g_gamma == nullptr) == (g_beta == nullptr), SRGAN_EINVAL,
                "srgan_conv2d_bwd_data_bnrelu parameter gradients (both or neither)");
  SRGAN_REQUIRE(srgan_conv2d_bnrelu_supported(desc, 1), SRGAN_EUNSUPPORTED,
                "srgan_conv2d_bwd_data_bnrelu geometry support");
  const BnBackwardEpilogue epilogue = bn_backward_epilogue(bn, x, g.x_bs, g_gamma, g_beta, partials);
  SRGAN_REQUIRE(image == nullptr || !pointwise(g), SRGAN_EUNSUPPORTED, "srgan_conv2d_bwd_data_bnrelu_image: 3x3 convolutions");
  if (pointwise(g))
    return pointwise_run(gy, g.y_bs, w, 1, g.C, nullptr, gx, g.x_bs, g.N, g.K, g.C, g.H * g.W, accumulate,
                         (hipStream_t)stream, nullptr, &epilogue);
  SRGAN_REQUIRE(!accumulate, SRGAN_EUNSUPPORTED, "srgan_conv2d_bwd_data_bnrelu 3x3: gx is stored, not accumulated");
  return conv3x3_run(gy, g.y_bs, conv3_flipped_taps(w, g.C, image), nullptr, gx, g.x_bs, g.N, g.K, g.C, g.H, g.W, 0,
                     (hipStream_t)stream, nullptr, &epilogue);
}

int srgan_conv2d_bwd_data_bnrelu_image(const srgan_conv_desc* desc, const float* gy, const float* w, const float* image,
                                       const srgan_bn_relu* bn, const float* x, float* gx, float* g_gamma, float* g_beta,
                                       int accumulate, void* stream) {
  SRGAN_REQUIRE(image != nullptr, SRGAN_EINVAL, "srgan_conv2d_bwd_data_bnrelu_image: the weight image");
  return bwd_data_bnrelu(desc, gy, w, bn, x, gx, g_gamma, g_beta, nullptr, accumulate, stream, image);
}

int srgan_conv2d_bwd_data_bnrelu_partials_image(const srgan_conv_desc* desc, const float* gy, const float* w, const float* image,
                                                const srgan_bn_relu* bn, const float* x, float* gx, float* partials,
                                                int accumulate, void* stream) {
  SRGAN_REQUIRE(partials != nullptr && image != nullptr, SRGAN_EINVAL,
                "srgan_conv2d_bwd_data_bnrelu_partials_image: the partial-sum region and the weight image");
  return bwd_data_bnrelu(desc, gy, w, bn, x, gx, nullptr, nullptr, partials, accumulate, stream, image);
}

int srgan_conv2d_bwd_data_bnrelu(const srgan_conv_desc* desc, const float* gy, const float* w, const srgan_bn_relu* bn,
                                 const float* x, float* gx, float* g_gamma, float* g_beta, int accumulate, void* stream) {
  return bwd_data_bnrelu(desc, gy, w, bn, x, gx, g_gamma, g_beta, nullptr, accumulate, stream);
}

int64_t srgan_conv2d_bwd_data_bnrelu_tiles(const srgan_conv_desc* desc) {
  ConvGeom g;
  if (!to_geom(desc, g) || !srgan_conv2d_bnrelu_supported(desc, 1)) return -1;
  return pointwise(g) ? pointwise_epilogue_tiles(g.N, g.H * g.W) : conv3x3_epilogue_tiles(g.N, g.K, g.C, g.H, g.W);
}

int srgan_conv2d_bwd_data_bnrelu_partials(const srgan_conv_desc* desc, const float* gy, const float* w, const srgan_bn_relu* bn,
                                          const float* x, float* gx, float* partials, int accumulate, void* stream) {
  SRGAN_REQUIRE(partials != nullptr, SRGAN_EINVAL, "srgan_conv2d_bwd_data_bnrelu_partials: the partial-sum region");
  return bwd_data_bnrelu(desc, gy, w, bn, x, gx, nullptr, nullptr, partials, accumulate, stream);
}

// ---- the 1x1 data gradients of two consecutive dense layers A (C rows) and B (C - 32 rows) with one pass over B's rows
static bool pair_geometry(const srgan_conv_desc* desc_a, const srgan_conv_desc* desc_b, ConvGeom& a, ConvGeom& b) {
  if (!srgan_conv2d_bnrelu_supported(desc_a, 1) || !srgan_conv2d_bnrelu_supported(desc_b, 1)) return false;
  if (!to_geom(desc_a, a) || !to_geom(desc_b, b) || !pointwise(a) || !pointwise(b)) return false;
  return a.N == b.N && a.H == b.H && a.W == b.W && a.K == b.K && a.x_bs == b.x_bs && a.y_bs == b.y_bs;
}

int srgan_conv2d_bwd_data_bnrelu_pair_supported(const srgan_conv_desc* desc_a, const srgan_conv_desc* desc_b) {
  ConvGeom a, b;
  if (!pair_geometry(desc_a, desc_b, a, b)) return 0;
  return pointwise_ring_pair_eligible(nullptr, nullptr, a.y_bs, nullptr, nullptr, nullptr, a.x_bs, nullptr, a.x_bs, a.N, a.K, a.C,
                                      b.C, a.H * a.W) ? 1 : 0;
}

int srgan_conv2d_bwd_data_bnrelu_strip(const srgan_conv_desc* desc_a, const srgan_conv_desc* desc_b, const float* gy, const float* w,
                                       const srgan_bn_relu* bn, const float* x, float* gx, float* partials, void* stream) {
  ConvGeom a, b;
  SRGAN_REQUIRE(gy && w && x && gx && bn_ok(bn), SRGAN_EINVAL, "srgan_conv2d_bwd_data_bnrelu_strip pointers");
  SRGAN_REQUIRE(pair_geometry(desc_a, desc_b, a, b) &&
                pointwise_ring_pair_eligible(gy, gy, a.y_bs, w, w, x, a.x_bs, gx, a.x_bs, a.N, a.K, a.C, b.C, a.H * a.W),
                SRGAN_EUNSUPPORTED, "srgan_conv2d_bwd_data_bnrelu_strip: not a pair (srgan_conv2d_bwd_data_bnrelu_pair_supported)");
  const BnBackwardEpilogue epilogue = bn_backward_epilogue(bn, x, a.x_bs, nullptr, nullptr, partials);
  return pointwise_ring_strip_run(gy, a.y_bs, w, gx, a.x_bs, a.N, a.K, a.C, b.C, a.H * a.W, epilogue, (hipStream_t)stream);
}

int srgan_conv2d_bwd_data_bnrelu_pair(const srgan_conv_desc* desc_a, const srgan_conv_desc* desc_b, const float* gy_a,
                                      const float* w_a, const srgan_bn_relu* bn_a, float* partials_a, const float* gy_b,
                                      const float* w_b, const srgan_bn_relu* bn_b, float* partials_b, const float* x, float* gx,
                                      void* stream) {
  ConvGeom a, b;
  SRGAN_REQUIRE(gy_a && w_a && gy_b && w_b && x && gx && bn_ok(bn_a) && bn_ok(bn_b), SRGAN_EINVAL,
                "srgan_conv2d_bwd_data_bnrelu_pair pointers");
  SRGAN_REQUIRE((partials_a == nullptr) == (partials_b == nullptr), SRGAN_EINVAL,
                "srgan_conv2d_bwd_data_bnrelu_pair partial-sum regions (both or neither)");
  SRGAN_REQUIRE(pair_geometry(desc_a, desc_b, a, b) &&
                pointwise_ring_pair_eligible(gy_a, gy_b, a.y_bs, w_a, w_b, x, a.x_bs, gx, a.x_bs, a.N, a.K, a.C, b.C, a.H * a.W),
                SRGAN_EUNSUPPORTED, "srgan_conv2d_bwd_data_bnrelu_pair: not a pair (srgan_conv2d_bwd_data_bnrelu_pair_supported)");
  const BnBackwardEpilogue epilogue_a = bn_backward_epilogue(bn_a, x, a.x_bs, nullptr, nullptr, partials_a);
  const BnBackwardEpilogue epilogue_b = bn_backward_epilogue(bn_b, x, a.x_bs, nullptr, nullptr, partials_b);
  return pointwise_ring_pair_run(gy_a, w_a, a.C, epilogue_a, gy_b, w_b, b.C, epilogue_b, a.y_bs, gx, a.x_bs, a.N, a.K, a.H * a.W,
                                 (hipStream_t)stream);
}

int srgan_bn_partial_reduce_batched(const srgan_bn_reduce_job* jobs_device, int32_t count, int32_t max_channels, int32_t max_tiles,
                                    const float* scratch, void* stream) {
  SRGAN_REQUIRE(jobs_device && scratch && count > 0 && max_channels > 0 && max_tiles > 0, SRGAN_EINVAL,
                "srgan_bn_partial_reduce_batched arguments");
  SRGAN_REQUIRE(count <= 65535, SRGAN_ERANGE, "srgan_bn_partial_reduce_batched job count");
  return bn_partial_reduce_batched_run(jobs_device, count, max_channels, max_tiles, scratch, (hipStream_t)stream);
}

int srgan_conv2d_bwd_weight_bnrelu(const srgan_conv_desc* desc, const float* x, const srgan_bn_relu* bn, const float* gy,
                                   float* gw, int accumulate, void* stream) {
  ConvGeom g;
  SRGAN_GEOM(desc, g, "srgan_conv2d_bwd_weight_bnrelu");
  SRGAN_REQUIRE(x && gy && gw && bn_ok(bn), SRGAN_EINVAL, "srgan_conv2d_bwd_weight_bnrelu pointers");
  SRGAN_REQUIRE(srgan_conv2d_bnrelu_supported(desc, 2), SRGAN_EUNSUPPORTED,
                "srgan_conv2d_bwd_weight_bnrelu geometry support");
  const BnVectors coefficients = bn_vectors(bn);
  if (pointwise(g))
    return pointwise_wgrad_run(x, g.x_bs, gy, g.y_bs, gw, g.N, g.C, g.K, g.H * g.W, accumulate, (hipStream_t)stream,
                               coefficients.v);
  return conv3x3_wgrad_run(x, g.x_bs, gy, g.y_bs, gw, g.N, g.C, g.K, g.H, g.W, accumulate, (hipStream_t)stream,
                           coefficients.v);
}

// ---- grouped weight gradients: all the norm -> relu -> conv weight gradients of a dense block's backward in two launches
int srgan_wgrad_group_plan(const srgan_conv_desc* desc, const srgan_bn_relu* bn, int64_t x_offset, int64_t gy_offset, float* gw,
                           int64_t gw_offset, int32_t group_size, int64_t group_weights, int64_t partial_offset, void* job, int32_t* grid_x,
                           int32_t* grid_y, int32_t* ragged, int64_t* partial_floats) {
  ConvGeom g;
  SRGAN_GEOM(desc, g, "srgan_wgrad_group_plan");
  SRGAN_REQUIRE(job && grid_x && grid_y && ragged && partial_floats && (bn == nullptr || bn_ok(bn)) && x_offset >= 0 &&
                gy_offset >= 0 && gw_offset >= 0 && partial_offset >= 0 && group_size >= 1 && group_weights >= 0, SRGAN_EINVAL,
                "srgan_wgrad_group_plan arguments");
  SRGAN_REQUIRE(srgan_conv2d_bnrelu_supported(desc, 2), SRGAN_EUNSUPPORTED, "srgan_wgrad_group_plan geometry support");
  const BnVectors coefficients = bn_vectors(bn);
  const float* const* fused = bn ? coefficients.v : nullptr;
  if (pointwise(g))
    return pointwise_wgrad_group_plan(x_offset, g.x_bs, gy_offset, g.y_bs, gw, gw_offset, g.N, g.C, g.K, g.H * g.W, fused,
                                      group_size, group_weights, partial_offset, job, grid_x, grid_y, ragged, partial_floats);
  return conv3x3_wgrad_group_plan(x_offset, g.x_bs, gy_offset, g.y_bs, gw, gw_offset, g.N, g.C, g.K, g.H, g.W, fused, group_size,
                                  partial_offset, job, grid_x, grid_y, ragged, partial_floats);
}

int srgan_wgrad_group_run(const void* jobs, int32_t count, int32_t kernel_size, int32_t grid_x, int32_t grid_y, int32_t ragged,
                          int32_t fused_bn, const float* x_base, const float* gy_base, float* gw_base, int64_t sum_co_ci_taps,
                          int64_t pixels, int64_t operand_elements, int64_t partial_floats, void* stream) {
  SRGAN_REQUIRE(jobs && x_base && gy_base && count >= 1 && grid_x >= 1 && grid_y >= 1 && (kernel_size == 1 || kernel_size == 3) &&
                partial_floats >= 0, SRGAN_EINVAL, "srgan_wgrad_group_run arguments");
  if (kernel_size == 1)
    return pointwise_wgrad_group_run(jobs, count, grid_x, grid_y, ragged, fused_bn, x_base, gy_base, gw_base, sum_co_ci_taps,
                                     pixels, operand_elements, partial_floats, (hipStream_t)stream);
  return conv3x3_wgrad_group_run(jobs, count, grid_x, grid_y, ragged, x_base, gy_base, gw_base, sum_co_ci_taps, pixels,
                                 operand_elements, partial_floats, (hipStream_t)stream);
}

}  // extern "C"
