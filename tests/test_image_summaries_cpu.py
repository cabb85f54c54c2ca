"""Image summaries without a device: the tests' NumPy restatement of the two contracts (image_summaries_reference.py) against
hand-written answers (``make_grid``: torchvision is not installed where the fixtures are generated) and against the reference's
own heatmaps (golden g17), the inferno table of the product against matplotlib's, and the argument errors of the two entry
points, which are reported before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import image_summaries_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
PTR = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its argument checks first


@pytest.fixture(scope='module')
def g17():
    return np.load(os.path.join(HERE, 'golden', 'g17_image_summaries.npz'))


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    _lib.library()
    return _lib


# ---- the restated grid ------------------------------------------------------------------------------------------------------
def numbered_images(n, channels, height, width):
    """Image k holds 100 * k + 10 * channel + (its pixel's index in the plane) / 100: every element names its place."""
    k, c, y, x = np.meshgrid(np.arange(n), np.arange(channels), np.arange(height), np.arange(width), indexing='ij')
    return (100 * k + 10 * c + (y * width + x) / 100.0).astype(np.float32)


def test_the_grid_of_five_images_three_wide():
    images = numbered_images(5, 3, 2, 3)
    grid = R.make_grid(images, nrow=3, padding=2, pad_value=-7.0)
    assert grid.shape == (3, 10, 17) == R.grid_shape(5, 2, 3, 3, 2)
    corners = {0: (2, 2), 1: (2, 7), 2: (2, 12), 3: (6, 2), 4: (6, 7)}             # (row, column) of every image's first pixel
    covered = np.zeros(grid.shape[1:], dtype=bool)
    for k, (top, left) in corners.items():
        assert np.array_equal(grid[:, top:top + 2, left:left + 3], images[k]), k
        assert grid[1, top, left] == np.float32(100 * k + 10)
        assert grid[2, top + 1, left + 2] == np.float32(100 * k + 20 + 0.05)
        covered[top:top + 2, left:left + 3] = True
    assert covered.sum() == 5 * 6
    assert (grid[:, ~covered] == np.float32(-7.0)).all()                           # every other element is padding
    assert (grid[:, 6:8, 12:15] == np.float32(-7.0)).all()                         # the empty sixth slot in particular
    assert (grid[:, :2] == -7).all() and (grid[:, :, :2] == -7).all() and (grid[:, 8:] == -7).all() and (grid[:, :, 15:] == -7).all()


def test_one_image_is_returned_without_padding():
    images = numbered_images(1, 3, 2, 3)
    assert np.array_equal(R.make_grid(images, nrow=3, padding=2, pad_value=9.0), images[0])
    assert R.grid_shape(1, 2, 3, 3, 2) == (3, 2, 3)
    single = numbered_images(1, 1, 4, 5)
    assert np.array_equal(R.make_grid(single, normalize=True, value_range=(0, 4)), np.repeat(R.normalise(single, 0, 4)[0], 3, axis=0))


def test_one_channel_is_replicated():
    images = numbered_images(4, 1, 3, 2)
    grid = R.make_grid(images, nrow=2, padding=1)
    assert grid.shape == (3, 9, 7)
    assert np.array_equal(grid[0], grid[1]) and np.array_equal(grid[0], grid[2])
    assert np.array_equal(grid[2, 5:8, 4:6], images[3, 0])


def test_fewer_images_than_a_row_make_a_narrower_grid():
    assert R.make_grid(numbered_images(2, 3, 5, 7), nrow=5, padding=2).shape == (3, 9, 20)
    assert R.make_grid(numbered_images(9, 3, 5, 7), nrow=3, padding=0).shape == (3, 15, 21)


@pytest.mark.parametrize('low, high, values, expected', [
    (0, 1, [-0.5, 0.0, 0.25, 1.0, 3.0], [0.0, 0.0, 0.25, 1.0, 1.0]),
    (-1, 1, [-2.0, -1.0, -0.5, 0.0, 1.0, 1.5], [0.0, 0.0, 0.25, 0.5, 1.0, 1.0]),
    (0, 255, [-1.0, 0.0, 51.0, 127.5, 255.0, 300.0], [0.0, 0.0, 0.2, 0.5, 1.0, 1.0])])
def test_clamp_and_scale(low, high, values, expected):
    images = np.array(values, dtype=np.float32).reshape(1, 1, 1, -1)
    got = R.make_grid(images, normalize=True, value_range=(low, high))
    assert np.array_equal(got[0, 0], np.array(expected, dtype=np.float32))         # 0.2 = fl(51 / 255): one rounded division
    padded = R.make_grid(np.repeat(images, 2, axis=0), normalize=True, value_range=(low, high), padding=1, pad_value=300.0)
    assert padded[0, 0, 0] == np.float32(300.0)                                    # the pad value is not normalised


def test_an_empty_range_divides_by_the_floor():
    images = np.array([1.0, 2.0, 3.0], dtype=np.float32).reshape(1, 1, 1, 3)
    assert np.array_equal(R.make_grid(images, normalize=True, value_range=(2, 2))[0, 0], np.zeros(3, dtype=np.float32))


# ---- the restated heatmap against the reference -----------------------------------------------------------------------------
def test_matplotlib_known_answers_of_the_entry_rule():
    """to_rgba of [[0, 1], [2, 4]] with clim (0, 4) returns entries 0, 64, 128 and 255; clim (1, 1) returns entry 0."""
    values = np.array([[0, 1], [2, 4]], dtype=np.float32)
    assert R.entries_of(R.scaled_positions(values, 0, 4, 256), 256).tolist() == [[0, 64], [128, 255]]
    assert R.entries_of(R.scaled_positions(values, 1, 1, 256), 256).tolist() == [[0, 0], [0, 0]]
    assert R.entries_of(np.array([-0.5, -1e-9, 255.999, 256.0, 300.0], dtype=np.float32), 256).tolist() == [0, 0, 255, 255, 255]


@pytest.mark.parametrize('name', ['random', 'constant', 'heads'])
def test_the_restated_heatmap_against_the_reference(g17, name):
    table, size = g17['inferno'], int(g17['size'])
    label, predicted = g17[f'{name}/label'], g17[f'{name}/predicted']
    tiles, ranges, entries, scaled = R.density_heatmaps(label[None], predicted[None, None], size, table)
    assert tiles.shape == (1, 2, 3, size, size) and tiles.dtype == np.float32
    assert ranges[0, 0].tolist() == [min(label.min(), predicted.min()), max(label.max(), predicted.max())]
    recorded = R.entries_from_colours(g17[f'{name}/heatmaps'], table)
    R.check_entries(entries[0], recorded, scaled[0], name)
    same = entries[0] == recorded
    assert np.array_equal(tiles[0].transpose(0, 2, 3, 1)[same], g17[f'{name}/heatmaps'].transpose(0, 2, 3, 1)[same])
    if name == 'constant':
        assert (recorded == 0).all() and (entries == 0).all()
    if name == 'random':
        assert R.near_an_integer(scaled).reshape(2, -1).mean(axis=1).max() <= 0.01      # the rule's cap holds for the reference alone


def test_the_inferno_table_is_matplotlibs(g17):
    import srgan_amd  # noqa: F401
    from srgan_amd import image_summaries
    assert image_summaries.INFERNO.dtype == np.float32 and image_summaries.INFERNO.shape == (256, 3)
    assert np.array_equal(image_summaries.INFERNO, g17['inferno'])


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_and_advertised(lib):
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_IMAGE_SUMMARIES\s+0x800u', header)
    for name in ('srgan_image_grid', 'srgan_density_heatmaps'):
        assert name in lib.SIGNATURES and getattr(lib.library(), name)
    assert lib.capabilities().features & 0x800
    assert lib.library().srgan_version() == 110


def test_image_grid_argument_errors_are_reported_before_any_device_work(lib):
    grid = lib.library().srgan_image_grid

    def call(images=PTR, n=5, c=3, h=2, w=3, nrow=3, padding=2, pad_value=0.0, normalize=0, low=0.0, high=1.0, out=PTR):
        return grid(images, n, c, h, w, nrow, padding, pad_value, normalize, low, high, out, None)
    assert call(images=None) == lib.EINVAL and call(out=None) == lib.EINVAL
    assert call(n=0) == lib.EINVAL
    assert call(c=2) == lib.EINVAL and call(c=4) == lib.EINVAL and call(c=0) == lib.EINVAL
    assert call(h=0) == lib.EINVAL and call(w=0) == lib.EINVAL
    assert call(nrow=0) == lib.EINVAL
    assert call(padding=-1) == lib.EINVAL
    assert call(normalize=1, low=float('nan')) == lib.EINVAL
    assert call(normalize=1, high=float('inf')) == lib.EINVAL
    assert call(normalize=1, low=1.0, high=0.0) == lib.EINVAL
    assert b'srgan_image_grid' in lib.library().srgan_last_error()
    # 3 * GH * GW above max_tensor_elements = 2^31 - 1 (formed without overflow), with and without a grid
    assert lib.capabilities().max_tensor_elements == 2 ** 31 - 1
    assert call(n=9, h=20000, w=20000) == lib.ERANGE
    assert call(n=1, h=2 ** 15, w=2 ** 15) == lib.ERANGE
    assert call(n=2 ** 31 - 1, h=2 ** 31 - 1, w=2 ** 31 - 1, nrow=2 ** 31 - 1, padding=2 ** 31 - 1) == lib.ERANGE


def test_density_heatmaps_argument_errors_are_reported_before_any_device_work(lib):
    heatmaps = lib.library().srgan_density_heatmaps

    def call(labels=PTR, predicted=PTR, b=2, m=3, h=8, w=8, p=8, lut=PTR, entries=256, tiles=PTR, stride=None, ranges=PTR):
        stride = (m + 1) * 3 * p * p if stride is None else stride
        return heatmaps(labels, predicted, b, m, h, w, p, lut, entries, tiles, stride, ranges, None)
    for name in ('labels', 'predicted', 'lut', 'tiles', 'ranges'):
        assert call(**{name: None}) == lib.EINVAL, name
    for name in ('b', 'm', 'h', 'w', 'entries'):
        assert call(**{name: 0}) == lib.EINVAL, name
    assert call(p=0, stride=1) == lib.EINVAL
    assert call(stride=4 * 3 * 64 - 1) == lib.EINVAL                               # shorter than the M + 1 tiles of an example
    assert call(h=9) == lib.EUNSUPPORTED and call(w=9) == lib.EUNSUPPORTED         # downscaling, as in the resize entry point
    assert b'srgan_density_heatmaps' in lib.library().srgan_last_error()
    assert call(b=2, stride=2 ** 31) == lib.ERANGE
    assert call(b=20000, m=3) == lib.ERANGE                                        # more than 65535 tiles
    assert call(p=2 ** 15, h=8, w=8) == lib.ERANGE


# ---- the Python surface, as far as it goes without a device -----------------------------------------------------------------
def test_make_grid_refuses_what_is_not_implemented():
    import torch
    import srgan_amd  # noqa: F401
    from srgan_amd import image_summaries
    images = torch.zeros(2, 3, 4, 4)
    with pytest.raises(NotImplementedError):
        image_summaries.make_grid(images, scale_each=True)
    with pytest.raises(NotImplementedError):
        image_summaries.make_grid(images, normalize=True)                          # without a range: the batch extrema


def test_the_writer_keeps_the_latest_image_per_tag():
    import srgan_amd  # noqa: F401
    from srgan_amd.utility import SummaryWriter
    writer = SummaryWriter()
    assert writer.images == {}
    writer.step = 4
    writer.add_image('Real', np.zeros((3, 2, 2)))
    writer.add_image('Real', np.ones((3, 2, 2), dtype=np.float64), global_step=6)
    step, image = writer.images['Real']
    assert step == 6 and image.dtype == np.float32 and image.shape == (3, 2, 2) and (image == 1).all()
    assert list(writer.images) == ['Real'] and writer.scalars == {}
