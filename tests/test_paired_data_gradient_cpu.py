"""srgan_conv2d_bwd_data_bnrelu_pair_supported on the host (no GPU): which two consecutive dense layers A (C rows) and
B (C - 32 rows) may apply their 1x1 data gradients as strip + pair (include/srgan_hip.h).  Everything it refuses takes the
per-layer launches."""
import pytest


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    return _lib


def desc(lib, n, c, h, w, k=128, x_bs=None, y_bs=0, dtype=0):
    total = 512
    return lib.ConvDesc(n, c, h, w, k, 1, 1, 1, 1, 0, 0, h, w, total * h * w if x_bs is None else x_bs, y_bs, dtype)


def supported(lib, a, b):
    return lib.library().srgan_conv2d_bwd_data_bnrelu_pair_supported(a, b)


def test_pairs_of_the_crowd_blocks_are_supported(lib):
    for n, plane, rows_a in [(16, 32, 224), (16, 32, 192), (16, 32, 512), (16, 64, 160), (16, 128, 256), (64, 16, 1024)]:
        assert supported(lib, desc(lib, n, rows_a, plane, plane), desc(lib, n, rows_a - 32, plane, plane)) == 1, (n, plane, rows_a)


def test_fewer_than_128_common_rows(lib):
    assert supported(lib, desc(lib, 16, 128, 64, 64), desc(lib, 16, 96, 64, 64)) == 0
    assert supported(lib, desc(lib, 16, 96, 64, 64), desc(lib, 16, 64, 64, 64)) == 0
    assert supported(lib, desc(lib, 16, 160, 64, 64), desc(lib, 16, 128, 64, 64)) == 1


def test_planes_that_are_no_multiple_of_128_pixels(lib):
    for h, w in [(8, 8), (28, 28), (14, 14), (24, 12), (8, 24)]:
        assert supported(lib, desc(lib, 128, 224, h, w), desc(lib, 128, 192, h, w)) == 0, (h, w)
    assert supported(lib, desc(lib, 128, 224, 8, 16), desc(lib, 128, 192, 8, 16)) == 1


def test_mismatched_strides(lib):
    plane = 32 * 32
    a = desc(lib, 16, 224, 32, 32, x_bs=256 * plane)
    assert supported(lib, a, desc(lib, 16, 192, 32, 32, x_bs=256 * plane)) == 1
    assert supported(lib, a, desc(lib, 16, 192, 32, 32, x_bs=288 * plane)) == 0          # another buffer
    assert supported(lib, a, desc(lib, 16, 192, 32, 32, x_bs=256 * plane, y_bs=160 * plane)) == 0      # another gradient layout
    odd = 256 * plane + 2                                                                  # rows not 16-byte aligned
    assert supported(lib, desc(lib, 16, 224, 32, 32, x_bs=odd), desc(lib, 16, 192, 32, 32, x_bs=odd)) == 0


def test_layers_that_are_not_consecutive_or_not_alike(lib):
    a = desc(lib, 16, 224, 32, 32)
    assert supported(lib, a, desc(lib, 16, 160, 32, 32)) == 0            # 64 rows apart
    assert supported(lib, a, desc(lib, 16, 224, 32, 32)) == 0
    assert supported(lib, desc(lib, 16, 192, 32, 32), a) == 0            # the order is (l + 1, l)
    assert supported(lib, a, desc(lib, 8, 192, 32, 32)) == 0
    assert supported(lib, a, desc(lib, 16, 192, 16, 64)) == 0
    assert supported(lib, desc(lib, 16, 224, 32, 32, k=64), desc(lib, 16, 192, 32, 32, k=64)) == 0     # four K stages per layer
    assert supported(lib, desc(lib, 16, 224, 32, 32, k=256), desc(lib, 16, 192, 32, 32, k=256)) == 0
    assert supported(lib, desc(lib, 16, 224, 32, 32, dtype=1), desc(lib, 16, 192, 32, 32, dtype=1)) == 0   # fp32 kernels
    assert supported(lib, None, None) == 0


def test_launches_too_small_to_gain(lib):
    """Fewer than 16 384 pixels: the launch-bound strip costs more than the pair saves (the 16 x 16 planes of the last crowd
    block at batch 16 and 48)."""
    for n, plane in [(16, 16), (48, 16), (63, 16), (8, 32)]:
        assert supported(lib, desc(lib, n, 1024, plane, plane), desc(lib, n, 992, plane, plane)) == 0, (n, plane)
    assert supported(lib, desc(lib, 64, 1024, 16, 16), desc(lib, 64, 992, 16, 16)) == 1


def test_a_layer_the_lds_dma_kernel_refuses_by_itself(lib):
    """The per-layer launches then run on pointwise_kernel, whose sums have another order: no pair.  16 images of 32 x 32
    pixels and one 128-row tile are 128 workgroups, fewer than the LDS-DMA kernel takes."""
    assert supported(lib, desc(lib, 16, 160, 32, 32), desc(lib, 16, 128, 32, 32)) == 0
    assert supported(lib, desc(lib, 32, 160, 32, 32), desc(lib, 32, 128, 32, 32)) == 1
