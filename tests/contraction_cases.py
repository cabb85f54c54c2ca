"""The convolution shapes of the contraction-kernel tests, shared by test_ops_gpu.py (fp32 against torch, 1e-3) and
test_exact_contractions_gpu.py (exact operands, bit for bit), with the kernels each shape exists to reach.

``reach`` lists the kinds of include/srgan_hip.h's profile report (srgan_profile_report) that the shape's passes, planned
with force = 0, must launch; ``split`` marks a shape that is there for a K-split combine (a report line of a declared kind
with split > 1).  The exact test asserts both per case, so a planner threshold that moves a shape onto another kernel fails
the case instead of quietly dropping the specialised kernel's only test.
"""
from collections import namedtuple

# kind numbers of srgan_profile_report (include/srgan_hip.h, bench.py's shape-report header)
KINDS = {0: 'gg_direct', 1: 'gg_mfma', 2: 'conv3x3_lds', 3: 'pointwise', 4: 'conv3x3_wgrad', 5: 'gg_rows', 6: 'pointwise_wgrad',
         8: 'pointwise_ksplit', 9: 'gg_dot', 10: 'stem7x7_fwd', 11: 'stem7x7_wgrad', 12: 'stem7x7_bwd_data', 13: 'pointwise_ring'}
FP32_KINDS = frozenset(KINDS)
# (no kind 7: the number is unused)
KINDS16 = {14: 'hconv3x3', 15: 'hwgrad3x3', 16: 'hgemm', 17: 'hlinear_wgrad', 18: 'hconv4x4s2', 19: 'hwgrad4x4s2'}

# Exact operands (test_exact_contractions_gpu.py): integers x, gy in [-X, X], weights in [-W, W], biases in [-B, B]; prefills
# of the accumulate forms are integers in [-PREFILL, PREFILL].  Every partial sum then stays below 2^24: fp32 adds exactly in
# any order.
X, W, B, PREFILL = 3, 2, 4, 64
EXACT_LIMIT = 2 ** 24

Case = namedtuple('Case', 'shape reach split')


def case(n, c, h, w, k, r, s, stride, pad, reach=(), split=False):
    return Case((n, c, h, w, k, r, s, stride, pad), frozenset(reach), split)


def output_plane(shape):
    n, c, h, w, k, r, s, stride, pad = shape
    return (h + 2 * pad[0] - r) // stride[0] + 1, (w + 2 * pad[1] - s) // stride[1] + 1


def worst_partial_sums(shape):
    """Largest magnitude any partial sum of the case's passes can reach on the exact operands (forward + bias, data gradient +
    bias, weight gradient; each onto a prefill): the bound behind the bit-exact assertions."""
    n, c, h, w, k, r, s, stride, pad = shape
    oh, ow = output_plane(shape)
    forward = X * W * c * r * s + B
    data = W * X * k * r * s + B
    weight = X * X * n * oh * ow
    return max(forward, data, weight) + PREFILL


DIRECT_LIMIT = 3e8        # force = 1 (the direct kernel) is a cross-check for shapes below n * c * h * w * k * r * s


def direct_is_cheap(shape):
    n, c, h, w, k, r, s, _, _ = shape
    return n * c * h * w * k * r * s <= DIRECT_LIMIT


CONV_CASES = [
    # N, C, H, W, K, R, S, stride, pad
    case(2, 3, 9, 8, 5, 3, 3, (1, 1), (1, 1), reach={1}),
    case(2, 4, 7, 7, 6, 1, 1, (1, 1), (0, 0), reach={1}),
    case(2, 3, 12, 10, 4, 4, 4, (2, 2), (1, 1), reach={1}),
    case(1, 3, 15, 13, 4, 7, 7, (2, 2), (3, 3), reach={1}),
    case(2, 2, 8, 8, 3, 2, 2, (2, 2), (0, 0), reach={1}),
    case(3, 5, 4, 6, 7, 4, 6, (1, 1), (0, 0), reach={1}),
    case(1, 2, 10, 10, 3, 3, 3, (3, 3), (1, 1), reach={0, 1}),
    # DenseNet / DCGAN / VGG tile-boundary shapes (multi-tile, split-K, all MFMA tile configs)
    case(4, 256, 28, 28, 128, 1, 1, (1, 1), (0, 0), reach={3}),
    case(4, 128, 28, 28, 32, 3, 3, (1, 1), (1, 1), reach={2, 4}),
    case(3, 200, 7, 7, 128, 1, 1, (1, 1), (0, 0), reach={3}),
    case(2, 3, 64, 64, 64, 7, 7, (2, 2), (3, 3), reach={10, 11, 12}),
    case(2, 64, 32, 32, 128, 4, 4, (2, 2), (1, 1), reach={2}),
    case(2, 64, 20, 20, 64, 3, 3, (1, 1), (1, 1), reach={2, 4}),
    case(2, 48, 8, 8, 1, 8, 8, (8, 8), (0, 0), reach={0}),          # map head in conv form (K = 1 -> direct kernel)
    case(2, 32, 16, 16, 20, 16, 16, (1, 1), (0, 0), reach={0, 1}),  # "linear" conv with a long reduction
    case(5, 70, 9, 9, 40, 3, 3, (1, 1), (1, 1), reach={2, 4}),      # ragged in every dimension
    # pointwise shapes eligible for 16-byte staging (all extents multiples of 4) and near-misses
    case(2, 64, 16, 16, 96, 1, 1, (1, 1), (0, 0), reach={3}),
    case(2, 160, 32, 32, 128, 1, 1, (1, 1), (0, 0), reach={3}),
    case(1, 36, 8, 12, 20, 1, 1, (1, 1), (0, 0), reach={3}),
    case(2, 64, 16, 18, 32, 1, 1, (1, 1), (0, 0), reach={3}),
    case(3, 896, 16, 16, 448, 1, 1, (1, 1), (0, 0), reach={3, 8}),
    # data gradient with <= 128 output channels: the resident-weight kernel, remainder tiles of 96 / 64 rows
    case(2, 224, 16, 16, 128, 1, 1, (1, 1), (0, 0), reach={3}),
    # few pixels, many input channels: the forward takes the kernel that splits K over the waves of a workgroup
    case(2, 288, 16, 16, 100, 1, 1, (1, 1), (0, 0), reach={3, 8}),
    case(4, 1024, 8, 8, 136, 1, 1, (1, 1), (0, 0), reach={3, 8}),
    case(2, 192, 8, 32, 64, 1, 1, (1, 1), (0, 0), reach={3}),
    # many input channels on planes that are no multiple of 32 pixels (the 14 x 14 and 7 x 7 planes of the reference's 224 x 224
    # patches): the streaming kernel with ragged pixel groups and a K split finished in a fixed order
    case(16, 256, 14, 14, 128, 1, 1, (1, 1), (0, 0), reach={3}, split=True),
    case(4, 1024, 7, 7, 128, 1, 1, (1, 1), (0, 0), reach={3}, split=True),
    case(3, 512, 14, 14, 136, 1, 1, (1, 1), (0, 0), reach={3}, split=True),
    case(1, 320, 6, 6, 40, 1, 1, (1, 1), (0, 0), reach={3}, split=True),
    # 3x3 / s1 / p1 shapes for the LDS-halo kernel (force = 0): all three channel-tile widths, ragged tiles,
    # fewer input channels than one chunk, split over input-channel chunks
    case(2, 128, 32, 32, 32, 3, 3, (1, 1), (1, 1), reach={2, 4}, split=True),
    case(1, 3, 40, 48, 64, 3, 3, (1, 1), (1, 1), reach={2}),
    case(2, 32, 16, 64, 130, 3, 3, (1, 1), (1, 1), reach={2, 4}, split=True),
    case(2, 24, 33, 35, 16, 3, 3, (1, 1), (1, 1), reach={2}),
    case(16, 128, 64, 64, 32, 3, 3, (1, 1), (1, 1), reach={2, 4}),
    case(2, 128, 16, 16, 32, 3, 3, (1, 1), (1, 1), reach={2, 4}),   # 16-wide images: two image rows per 32-lane column block
    case(3, 40, 13, 16, 24, 3, 3, (1, 1), (1, 1), reach={2, 4}),
    # 14-wide planes of the 224-pixel configuration: two dead columns per tile
    case(2, 128, 14, 14, 32, 3, 3, (1, 1), (1, 1), reach={2, 4}),
    case(2, 32, 14, 13, 128, 3, 3, (1, 1), (1, 1), reach={2, 4}),
    case(3, 128, 7, 7, 32, 3, 3, (1, 1), (1, 1), reach={2, 4}),
    case(3, 200, 20, 24, 40, 3, 3, (1, 1), (1, 1), reach={2, 4}, split=True), # LDS-patch weight gradient: ragged channel chunks and tiles
    case(4, 3, 96, 96, 16, 7, 7, (2, 2), (3, 3), reach={5, 10, 11, 12}), # stem: the 3-row image gradient takes the few-rows kernel
    case(2, 5, 72, 72, 7, 3, 3, (1, 1), (1, 1), reach={5}),         # 5 and 7 rows (MR = 8) in the few-rows kernel
    case(8, 2, 256, 128, 3, 2, 2, (2, 2), (0, 0), reach={5, 9}, split=True), # weight gradient 3 x 8 over K = 65536 pixels: lanes-along-K
    # k4 / s2 / p1 at the DCGAN pair's own shapes (reference age/models.py:61-65 on 64 x 192 driving frames and 128 x 128
    # faces, crowd/models.py:132-136 backwards): three input channels, rectangular and ragged planes, 24- to 512-row outputs,
    # K splits with the ordered finish
    case(3, 3, 64, 192, 64, 4, 4, (2, 2), (1, 1), reach={5}, split=True),
    case(2, 64, 32, 96, 128, 4, 4, (2, 2), (1, 1), reach={2}, split=True),
    case(2, 128, 16, 48, 256, 4, 4, (2, 2), (1, 1), reach={2}, split=True),
    case(2, 256, 16, 24, 512, 4, 4, (2, 2), (1, 1), reach={2}, split=True),
    case(5, 20, 36, 44, 24, 4, 4, (2, 2), (1, 1), reach={2}),
    case(1, 64, 128, 128, 32, 4, 4, (2, 2), (1, 1), reach={2}, split=True),
    # the LDS-DMA 1x1 kernel (pointwise_ring.hip; whole 128-row tiles, >= 192 workgroups): 128- and 64-pixel tiles, weights
    # k-contiguous (forward) and m-contiguous (data gradient), several row tiles, remainder rows of 32 / 96 on the old kernel
    case(16, 128, 64, 64, 128, 1, 1, (1, 1), (0, 0), reach={3, 13}),
    case(16, 256, 32, 32, 128, 1, 1, (1, 1), (0, 0), reach={3, 13}),
    case(4, 160, 64, 64, 288, 1, 1, (1, 1), (0, 0), reach={3, 13}),
    case(6, 96, 64, 64, 224, 1, 1, (1, 1), (0, 0), reach={3, 13}),
    case(24, 128, 24, 12, 128, 1, 1, (1, 1), (0, 0), reach={3, 13}), # planes of 9 x 32 pixels: the 32-pixel tile, both layouts
    # the map modules' 2x2 / s2 convolutions (reference crowd/models.py:131-133) at their own channel counts: tiny weight
    # gradients from 10^4 - 10^5 pixels (many K slices, ordered finish), rectangular planes, an odd input height
    case(3, 8, 128, 128, 16, 2, 2, (2, 2), (0, 0), reach={1}, split=True),
    case(2, 16, 64, 128, 32, 2, 2, (2, 2), (0, 0), reach={1}, split=True),
    case(2, 1, 64, 64, 8, 2, 2, (2, 2), (0, 0), reach={1}, split=True),
    case(2, 5, 67, 64, 20, 2, 2, (2, 2), (0, 0), reach={1}, split=True),
    case(1, 3, 4, 64, 7, 2, 2, (2, 2), (0, 0), reach={1}),
]

# srgan_gemm at test_linear_and_mm's shapes (batch, in, out): the five products of a linear layer's passes
GEMM_CASES = [
    Case((7, 11, 5), frozenset({1}), False),
    Case((256, 50, 10), frozenset({1}), False),
    Case((64, 300, 130), frozenset({1}), False),
    Case((2, 25088 // 8, 512), frozenset({1}), False),
    Case((130, 64, 1), frozenset({0, 1}), False),
    Case((16, 65536, 20), frozenset({1}), True),        # tiny output, long K: split-K through the partial-sum workspace
]

# conv_transpose2d at test_conv_transpose's shapes: (in channels, out channels, kernel, stride, pad, input size, batch)
CONVT_CASES = [(6, 4, 4, 2, 1, 5, 2), (32, 48, 3, 1, 0, 1, 3), (40, 1, 4, 4, 0, 6, 2), (64, 3, 4, 2, 1, 16, 2), (256, 64, 2, 1, 0, 1, 4),
               (64, 3, 4, 2, 1, 64, 2)]

# The fused batch-norm convolutions at the shapes of test_ops_gpu.py's test_fused_batch_norm_convolutions (forward, weight
# gradient) and test_fused_batch_norm_backward_in_the_data_gradient: (n, c, channels of the wider buffer, h, w, k, r)
BN_FORWARD_CASES = [(2, 48, 80, 16, 16, 32, 1), (3, 160, 160, 8, 32, 128, 1), (2, 320, 352, 16, 16, 96, 1), (1, 512, 512, 8, 8, 40, 1),
                    (2, 32, 32, 16, 16, 8, 3), (2, 128, 128, 32, 32, 32, 3), (1, 70, 96, 20, 24, 40, 3),
                    (3, 160, 200, 28, 28, 128, 1), (2, 200, 264, 14, 14, 128, 1), (5, 96, 131, 7, 7, 128, 1),
                    (16, 64, 64, 7, 7, 40, 1), (2, 34, 41, 9, 7, 20, 1), (2, 128, 128, 14, 14, 32, 3), (3, 128, 128, 7, 7, 32, 3),
                    (2, 40, 57, 7, 9, 33, 3), (2, 128, 128, 28, 28, 32, 3), (16, 1024, 1056, 14, 14, 128, 1),
                    (16, 896, 928, 7, 7, 128, 1), (3, 512, 640, 14, 14, 128, 1), (16, 256, 320, 32, 32, 128, 1),
                    (16, 64, 64, 64, 64, 128, 1), (4, 160, 192, 64, 64, 256, 1)]
BN_DATA_CASES = [(2, 48, 80, 16, 16, 32, 1), (3, 160, 160, 8, 32, 128, 1), (2, 192, 224, 32, 32, 128, 1), (1, 512, 512, 8, 8, 40, 1),
                 (4, 96, 256, 64, 64, 128, 1), (2, 300, 300, 16, 16, 128, 1), (4, 128, 128, 32, 32, 32, 3),
                 (16, 128, 128, 16, 16, 32, 3), (2, 128, 128, 64, 64, 32, 3), (3, 40, 40, 20, 24, 16, 3),
                 (16, 128, 128, 64, 64, 32, 3), (3, 160, 200, 28, 28, 128, 1), (2, 200, 264, 14, 14, 128, 1),
                 (5, 96, 131, 7, 7, 128, 1), (16, 64, 64, 7, 7, 128, 1), (2, 34, 41, 9, 7, 20, 1), (2, 128, 128, 14, 14, 32, 3),
                 (3, 128, 128, 7, 7, 32, 3), (16, 256, 320, 32, 32, 128, 1), (8, 416, 512, 32, 32, 128, 1),
                 (8, 224, 256, 64, 64, 128, 1)]
# srgan_wgrad_group_plan / _run at test_grouped_weight_gradients_gpu.py's shapes: (plane, shares by work)
GROUPED_WGRAD_CASES = [((32, 32), True), ((32, 32), False), ((16, 8), True), ((14, 14), True)]

# The fused batch-norm weight gradients (srgan_conv2d_bwd_weight_bnrelu, srgan_wgrad_group_run) by kernel size: kind 6 is only
# reached through them (srgan_conv2d_bwd_weight takes the register-streamed 1x1 kernel only when SRGAN_PW_WGRAD is set)
FUSED_WGRAD_REACH = {1: frozenset({6}), 3: frozenset({4})}
GROUPED_WGRAD_REACH = frozenset({6})

# Kinds no shape of the table can reach, with the reason (the table test accepts these as uncovered, nothing else).
UNREACHABLE = {}

# The 16-bit kernels (blocked16*.hip) and the shape lists of test_blocked16_gpu.py that reach each of them.
REACH16 = {14: 'CONVS (srgan_h_conv3x3: forward and data gradient)', 15: 'CONVS (weight gradient)',
           16: 'LINEARS (srgan_h_gemm)', 17: 'LINEARS (srgan_h_linear_wgrad)', 18: 'K4S2 (forward, both data gradients)',
           19: 'K4S2 (weight gradients)'}
