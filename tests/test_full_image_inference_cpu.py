"""Full-image crowd inference on the device, the parts that can be checked without one: the three entry points are
exported / bound (tests/test_abi_cpu.py compares header, exports and ctypes table) and refuse bad arguments before any
device work, the window table ``DeviceSlidingWindows`` uploads is ``ImageSlidingWindowDataset``'s, and the index rule of
the gather kernel (restated in NumPy below) reproduces the host slice-add loop of ``predict_full_example`` bit for bit."""
import numpy as np
import pytest

# (H, W, P, step): the three g9 shapes (larger than / equal to / smaller than a patch) and a ShanghaiTech part B scene
GEOMETRIES = [(100, 150, 64, 24), (64, 64, 64, 24), (40, 90, 64, 24), (768, 1024, 224, 128)]
FEATURE_CROWD_FULL_IMAGE = 0x20
PTR = 0x10000          # a stand-in for a device address (never dereferenced: the calls below fail before any launch)


def host_blend(densities, counts, centres, height, width, patch_size):
    """The accumulation of ``CrowdExperiment.predict_full_example`` (reference crowd/srgan.py:366-394) on given per-window
    predictions: ``centres[i] = (y, x)``.  Returns (density[H, W], the per-pixel count terms[H, W]) in float32."""
    half = patch_size // 2
    sum_density = np.zeros((height, width), dtype=np.float32)
    sum_count = np.zeros((height, width), dtype=np.float32)
    hits = np.zeros((height, width), dtype=np.int32)
    for (y, x), density, count in zip(centres, densities, counts):
        count_array = np.full(density.shape, count / density.size, dtype=np.float32)
        y_start = half - y if y - half < 0 else 0
        y_end = y + half - height if y + half > height else 0
        x_start = half - x if x - half < 0 else 0
        x_end = x + half - width if x + half > width else 0
        target = (slice(y - half + y_start, y + half - y_end), slice(x - half + x_start, x + half - x_end))
        source = (slice(y_start, density.shape[0] - y_end), slice(x_start, density.shape[1] - x_end))
        sum_density[target] += density[source]
        sum_count[target] += count_array[source]
        hits[target] += 1
    hits[hits == 0] = 1
    return sum_density / hits.astype(np.float32), sum_count / hits.astype(np.float32)


def gather_emulation(densities, counts, ys, xs, height, width, patch_size):
    """The index arithmetic of ``crowd_blend_windows_kernel`` for every pixel at once: windows in index order (y-major,
    then x), window (iy, ix) covers the pixel iff 0 <= py - (ys[iy] - P/2) < P and the same in x; fp32 sums from 0."""
    half = patch_size // 2
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing='ij')
    density_sum = np.zeros((height, width), dtype=np.float32)
    count_sum = np.zeros((height, width), dtype=np.float32)
    hits = np.zeros((height, width), dtype=np.int32)
    patch_pixels = np.float32(patch_size * patch_size)
    for iy in range(len(ys)):
        dy = py - (int(ys[iy]) - half)
        for ix in range(len(xs)):
            dx = px - (int(xs[ix]) - half)
            covered = (dy >= 0) & (dy < patch_size) & (dx >= 0) & (dx < patch_size)
            window = iy * len(xs) + ix
            density_sum[covered] += densities[window][dy[covered], dx[covered]]
            count_sum[covered] += np.float32(counts[window]) / patch_pixels
            hits[covered] += 1
    covering = np.where(hits > 0, hits, 1).astype(np.float32)
    return density_sum / covering, count_sum / covering


def sliding_windows(height, width, patch_size, step, batch_size=4, seed=0):
    from srgan_amd.crowd.data import CrowdExample, DeviceSlidingWindows, ImageSlidingWindowDataset
    image = np.random.RandomState(seed).randint(0, 256, size=(height, width, 3)).astype(np.uint8)
    example = CrowdExample(image=image, label=np.zeros((height, width), dtype=np.float32))
    return DeviceSlidingWindows(example, batch_size, patch_size, step), ImageSlidingWindowDataset(example, patch_size, step)


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    return _lib


def test_the_entry_points_are_bound_and_advertised(lib):
    for name in ('srgan_crowd_extract_windows', 'srgan_crowd_resize_bilinear', 'srgan_crowd_blend_windows'):
        assert name in lib.SIGNATURES and getattr(lib.library(), name) is not None
    assert lib.capabilities().features & FEATURE_CROWD_FULL_IMAGE
    assert lib.library().srgan_version() == 110


def test_bad_arguments_are_refused_before_any_device_work(lib):
    library = lib.library()
    extract = library.srgan_crowd_extract_windows
    good = [PTR, 100, 150, PTR, 3, PTR, 5, 0, 4, 64, PTR, None]
    for position, bad in ((0, None), (3, None), (5, None), (10, None),          # NULL pointers
                          (1, 0), (2, -1), (4, 0), (6, 0), (7, -1), (8, 0), (9, 0),     # non-positive sizes
                          (9, 63),                                                # odd P
                          (7, 12)):                                               # windows 12 .. 15 of 15
        arguments = list(good)
        arguments[position] = bad
        assert extract(*arguments) == lib.EINVAL, ('extract', position, bad)
    assert extract(PTR, 100, 150, PTR, 300, PTR, 300, 0, 70000, 64, PTR, None) == lib.ERANGE

    resize = library.srgan_crowd_resize_bilinear
    good = [PTR, 4, 16, 16, 64, PTR, None]
    for position, bad in ((0, None), (5, None), (1, 0), (2, 0), (3, -4), (4, 0)):
        arguments = list(good)
        arguments[position] = bad
        assert resize(*arguments) == lib.EINVAL, ('resize', position, bad)
    assert resize(PTR, 4, 64, 16, 32, PTR, None) == lib.EUNSUPPORTED            # downscaling
    assert b'downscaling' in library.srgan_last_error()
    assert resize(PTR, 1 << 20, 16, 16, 64, PTR, None) == lib.ERANGE

    blend = library.srgan_crowd_blend_windows
    good = [PTR, PTR, PTR, 3, PTR, 5, 100, 150, 64, PTR, PTR, None]
    for position, bad in ((1, None), (2, None), (4, None), (9, None), (10, None),
                          (3, 0), (5, -1), (6, 0), (7, 0), (8, 0), (8, 63)):
        arguments = list(good)
        arguments[position] = bad
        assert blend(*arguments) == lib.EINVAL, ('blend', position, bad)
    assert blend(PTR, PTR, PTR, 300, PTR, 300, 100, 150, 224, PTR, PTR, None) == lib.ERANGE


@pytest.mark.parametrize('height,width,patch_size,step', GEOMETRIES)
def test_the_uploaded_window_table_is_the_datasets(height, width, patch_size, step):
    import srgan_amd  # noqa: F401
    windows, dataset = sliding_windows(height, width, patch_size, step)
    assert windows.ys.dtype == windows.xs.dtype == np.int32
    assert windows.ys.tolist() == dataset.y_positions and windows.xs.tolist() == dataset.x_positions
    assert len(windows) == len(dataset) == len(windows.ys) * len(windows.xs)
    for index in range(len(dataset)):
        y_index, x_index = np.unravel_index(index, dataset.positions_shape)
        assert windows.centre(index) == (dataset.y_positions[y_index], dataset.x_positions[x_index])
    if (height, width) == (768, 1024):
        assert (len(windows.ys), len(windows.xs)) == (6, 8)
    if (height, width) == (40, 90):
        assert windows.ys.tolist() == [8] and windows.xs.tolist() == [32, 56, 58]
    assert windows.scene is None                  # nothing was uploaded: the table is host data until the first batch


def test_an_odd_patch_size_is_refused():
    import srgan_amd  # noqa: F401
    with pytest.raises(ValueError):
        sliding_windows(100, 150, 63, 24)


@pytest.mark.parametrize('height,width,patch_size,step', GEOMETRIES)
def test_the_gather_rule_equals_the_host_slice_add_loop(height, width, patch_size, step):
    import srgan_amd  # noqa: F401
    windows, _ = sliding_windows(height, width, patch_size, step)
    generator = np.random.RandomState(height + width)
    densities = (generator.rand(len(windows), patch_size, patch_size).astype(np.float32) - 0.3) * 3
    counts = (generator.rand(len(windows)).astype(np.float32) - 0.2) * 50
    centres = [windows.centre(index) for index in range(len(windows))]
    density, terms = host_blend(densities, counts, centres, height, width, patch_size)
    gathered_density, gathered_terms = gather_emulation(densities, counts, windows.ys, windows.xs, height, width, patch_size)
    assert density.dtype == gathered_density.dtype == np.float32
    np.testing.assert_array_equal(gathered_density.view(np.uint32), density.view(np.uint32))
    np.testing.assert_array_equal(gathered_terms.view(np.uint32), terms.view(np.uint32))
