"""Distribution summaries without a device: the tests' NumPy restatement of the three contracts
(distribution_summaries_reference.py) against ``scipy.stats.wasserstein_distance`` and ``gaussian_kde`` on random inputs and on
the arrays the reference's own summary step produced (golden g18), the frame restatement against hand-written answers, the
module's constants (the step polyline of the real density, the pseudo-inverse of the cubic fit, the palette), and the argument
errors of the three entry points, which are reported before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.stats import gaussian_kde, uniform, wasserstein_distance

import distribution_summaries_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
PTR = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its argument checks first
FRAME_SETS = ('fake_coefficients', 'unlabeled_predictions', 'gan_validation', 'gan_train', 'dnn_validation', 'dnn_train')


@pytest.fixture(scope='module')
def g18():
    return np.load(os.path.join(HERE, 'golden', 'g18_coefficient_distributions.npz'))


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    _lib.library()
    return _lib


@pytest.fixture(scope='module')
def module():
    import srgan_amd  # noqa: F401
    from srgan_amd import distribution_summaries
    return distribution_summaries


# ---- the restatement against scipy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, m', [(1, 1), (3, 5), (37, 100), (64, 64), (1000, 1000)])
def test_the_restated_wasserstein_distance_is_scipys(n, m):
    generator = np.random.RandomState(n * 1000 + m)
    u, v = generator.normal(0.3, 0.8, size=n), generator.uniform(-2, 2, size=m)
    assert abs(R.wasserstein(u, v) - wasserstein_distance(u, v)) <= 1e-12
    tied_u, tied_v = np.round(u * 4) / 4, np.round(v * 4) / 4                      # heavy ties, and ties across the sets
    assert abs(R.wasserstein(tied_u, tied_v) - wasserstein_distance(tied_u, tied_v)) <= 1e-12
    assert abs(float(R.wasserstein32(u, v)) - wasserstein_distance(u, v)) <= 1e-5


def test_the_restated_wasserstein_distance_on_the_references_arrays(g18):
    """The reference logged scipy's distance between D's predictions on its generated examples and the unlabeled labels."""
    import torch
    weights = {key[len('weights/D/'):]: g18[key] for key in g18.files if key.startswith('weights/D/')}
    hidden = g18['fake_examples']
    for layer in (1, 2, 3):
        hidden = torch.nn.functional.leaky_relu(torch.from_numpy(hidden @ weights[f'linear{layer}.weight'].T +
                                                                 weights[f'linear{layer}.bias'])).numpy()
    predicted = (hidden @ weights['linear4.weight'].T + weights['linear4.bias'])[:, 0]
    assert abs(R.wasserstein(predicted, g18['unlabeled_labels']) - float(g18['wasserstein'])) <= 1e-5      # fp32 forward passes
    assert abs(R.wasserstein(predicted, g18['unlabeled_labels']) - wasserstein_distance(predicted, g18['unlabeled_labels'])) <= 1e-12


def scipy_curve(x, gridsize, factor=0.1, cut=3):
    x = np.asarray(x, dtype=np.float64)
    h = factor * x.std(ddof=1)
    support = np.linspace(x.min() - cut * h, x.max() + cut * h, gridsize)
    return support, gaussian_kde(x, bw_method=factor)(support), h


def test_the_restated_curves_are_scipys():
    generator = np.random.RandomState(5)
    sets = [generator.normal(0.3, 0.8, size=size) for size in (2, 7, 64, 257)]
    sets.insert(2, np.array([1.25]))                                                # cannot be fitted: one sample
    sets.insert(3, np.full(9, -0.5))                                                # cannot be fitted: no spread
    for gridsize in (2, 100):
        support, density, stats = R.kde_curves(sets, gridsize)
        for c, x in enumerate(sets):
            assert stats[c, 0] == len(x) and stats[c, 1] == x.min() and stats[c, 2] == x.max()
            if c in (2, 3):
                assert stats[c, 3] == 0 and not support[c].any() and not density[c].any()
                continue
            expected_support, expected_density, h = scipy_curve(x, gridsize)
            assert abs(stats[c, 3] - h) <= 1e-12 * h
            assert np.abs(support[c] - expected_support).max() <= 1e-12
            assert np.abs(density[c] - expected_density).max() <= 1e-12 * expected_density.max()
    assert np.isfinite(R.kde_curves([np.array([])], 5)[2]).all()


def test_the_restated_curves_on_the_references_arrays(g18):
    support, density, _ = R.kde_curves([g18[name] for name in FRAME_SETS], 100)
    for c, name in enumerate(FRAME_SETS):
        assert np.abs(support[c] - g18[f'kde/{name}/support']).max() <= 1e-12
        assert np.abs(density[c] - g18[f'kde/{name}/density']).max() <= 1e-12 * g18[f'kde/{name}/density'].max()
    single = R.kde_curves([g18[name] for name in FRAME_SETS], 100, dtype=np.float32)
    assert single[1].dtype == np.float32
    for c, name in enumerate(FRAME_SETS):
        assert np.abs(single[1][c] - g18[f'kde/{name}/density']).max() <= 1e-4 * g18[f'kde/{name}/density'].max()


# ---- the module's constants ----------------------------------------------------------------------------------------------------
def test_the_step_polyline_is_the_real_label_density(module):
    from srgan_amd.utility import MixtureModel
    x = np.arange(-4, 4, 0.001)
    x = x[np.abs(np.abs(x)[:, None] - np.array([1.0, 2.0])).min(axis=1) > 1e-6]     # away from the four jumps
    polyline = module.REAL_DENSITY.astype(np.float64)
    assert polyline.shape == (10, 2) and (np.diff(polyline[:, 0]) >= 0).all()
    segment = np.searchsorted(polyline[:, 0], x, side='right') - 1
    assert (polyline[segment, 1] == polyline[segment + 1, 1]).all()                 # flat between the jumps
    assert np.array_equal(polyline[segment, 1], MixtureModel([uniform(-2, 1), uniform(1, 1)]).pdf(x))


def test_the_pseudo_inverse_is_polyfit(module, g18):
    fake = g18['fake_examples'].astype(np.float64)
    fitted = np.transpose(np.polyfit(np.linspace(-1, 1, num=10), np.transpose(fake[:, :10]), 3))        # presentation.py:24
    assert module.POLYFIT_PSEUDO_INVERSE.shape == (4, 10) and module.POLYFIT_PSEUDO_INVERSE.dtype == np.float32
    assert np.abs(fake[:, :10] @ module.POLYFIT_PSEUDO_INVERSE.astype(np.float64).T - fitted).max() <= 1e-6
    assert np.abs(fitted[0, :] - g18['fake_coefficients']).max() <= 1e-12          # the four samples of the "fake" curve


def test_the_palette_is_seaborns_deep(module):
    from matplotlib.colors import to_rgb
    deep = ['#4C72B0', '#DD8452', '#55A868', '#C44E52', '#8172B3', '#937860', '#DA8BC3', '#8C8C8C', '#CCB974', '#64B5CD']
    assert module.DEEP_PALETTE.dtype == np.float32 and module.DEEP_PALETTE.shape == (10, 3)
    assert np.abs(module.DEEP_PALETTE - np.array([to_rgb(colour) for colour in deep])).max() <= 1e-7
    assert np.abs(module.DARKGRID_BACKGROUND - np.array(to_rgb('#EAEAF2'))).max() <= 1e-7
    assert np.abs(module.DARKGRID_BACKGROUND - np.array([0.918, 0.918, 0.949])).max() <= 5e-4
    assert module.CURVE_PALETTE_INDEXES == (0, 4, 1, 2, 2, 3, 3)
    widths = module.curve_pixel_widths(640)
    assert np.allclose(widths[[4, 6]] * 3, widths[[3, 5]]) and abs(widths[1] - 1.5 * 100 / 72) <= 1e-6
    assert module.X_TICKS.tolist() == list(range(-4, 5)) and np.allclose(module.Y_TICKS, [0, 0.2, 0.4, 0.6, 0.8, 1.0])
    assert module.WASSERSTEIN_MAX_VALUES == 16384


# ---- the restated frame against hand-written answers ---------------------------------------------------------------------------
GREY, RED, BLUE = (0.25, 0.25, 0.25), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)


def small_frame(widths, **ticks):
    """8 x 8 over x, y in [0, 8]: px = x - 0.5, py = 7.5 - y.  A horizontal segment on row 2 from column 1 to column 6, then a
    vertical one on column 3 from row 0 to row 6."""
    vertices = [(1.5, 5.5), (6.5, 5.5), (3.5, 7.5), (3.5, 1.5)]
    return R.curve_frame(vertices, [0, 2, 4], [RED, BLUE], widths, 8, 8, (0, 8), (0, 8), GREY, (1.0, 1.0, 1.0), **ticks)


def test_a_frame_with_one_horizontal_and_one_vertical_segment():
    frame = small_frame([1.0, 1.0])
    expected = np.broadcast_to(np.array(GREY)[:, None, None], (3, 8, 8)).copy()
    expected[:, 2, 1:7] = np.array(RED)[:, None]
    expected[:, 0:7, 3] = np.array(BLUE)[:, None]                                   # drawn second: over the red at (2, 3)
    assert np.abs(frame - expected).max() <= 1e-15
    wide = small_frame([2.0, -1.0])                                                 # coverage 1.5 - d; the second draws nothing
    assert np.abs(wide[:, 2, 1:7] - np.array(RED)[:, None]).max() <= 1e-15
    half = 0.5 * np.array(GREY) + 0.5 * np.array(RED)
    for row, column in ((1, 1), (3, 6), (2, 0), (2, 7)):                            # one pixel away: half covered
        assert np.abs(wide[:, row, column] - half).max() <= 1e-15
    corner = 1.5 - 2 ** 0.5                                                         # diagonal neighbours of the two ends
    assert np.abs(wide[:, 1, 0] - ((1 - corner) * np.array(GREY) + corner * np.array(RED))).max() <= 1e-15
    assert np.abs(wide[:, 4, 3] - np.array(GREY)).max() <= 1e-15 and np.abs(wide[:, 0, 3] - np.array(GREY)).max() <= 1e-15


def test_a_frame_with_grid_lines_and_skipped_polylines():
    frame = R.curve_frame([(1.0, 1.0)], [0, 1], [RED], [1.0], 8, 8, (0, 8), (0, 8), GREY, (1.0, 1.0, 1.0),
                          x_ticks=[2.5, 5.0], y_ticks=[0.5])                        # one vertex: nothing drawn
    expected = np.broadcast_to(np.array(GREY)[:, None, None], (3, 8, 8)).copy()
    expected[:, :, 2] = 1.0                                                         # x = 2.5 is the centre of column 2
    expected[:, :, 4:6] = 0.5 * 0.25 + 0.5                                          # x = 5 lies between columns 4 and 5
    expected[:, 7, :] = 1.0                                                         # y = 0.5 is the centre of the bottom row
    assert np.abs(frame - expected).max() <= 1e-15


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_and_advertised(lib):
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_DISTRIBUTION_SUMMARIES\s+0x1000u', header)
    capacity = int(re.search(r'#define\s+SRGAN_WASSERSTEIN_MAX_VALUES\s+(\d+)', header).group(1))
    assert capacity >= 8192 and capacity & (capacity - 1) == 0
    for name in ('srgan_wasserstein_1d', 'srgan_kde_curves', 'srgan_curve_frame'):
        assert name in lib.SIGNATURES and getattr(lib.library(), name)
    assert lib.capabilities().features & 0x1000
    assert lib.library().srgan_version() == 110


def test_wasserstein_argument_errors_are_reported_before_any_device_work(lib, module):
    distance = lib.library().srgan_wasserstein_1d

    def call(u=PTR, n=3, v=PTR, m=5, out=PTR):
        return distance(u, n, v, m, out, None)
    for name in ('u', 'v', 'out'):
        assert call(**{name: None}) == lib.EINVAL, name
    assert call(n=0) == lib.EINVAL and call(m=0) == lib.EINVAL and call(n=-1) == lib.EINVAL
    assert b'srgan_wasserstein_1d' in lib.library().srgan_last_error()
    capacity = module.WASSERSTEIN_MAX_VALUES
    assert call(n=capacity, m=1) == lib.EUNSUPPORTED and call(n=1, m=capacity) == lib.EUNSUPPORTED
    assert call(n=2 ** 31 - 1, m=2 ** 31 - 1) == lib.EUNSUPPORTED                   # n + m formed without overflow
    assert b'srgan_wasserstein_1d' in lib.library().srgan_last_error()


def test_kde_curves_argument_errors_are_reported_before_any_device_work(lib):
    curves = lib.library().srgan_kde_curves

    def call(samples=PTR, offsets=PTR, c=3, g=100, factor=0.1, cut=3.0, support=PTR, density=PTR, stats=PTR):
        return curves(samples, offsets, c, g, factor, cut, support, density, stats, None)
    for name in ('samples', 'offsets', 'support', 'density', 'stats'):
        assert call(**{name: None}) == lib.EINVAL, name
    assert call(c=0) == lib.EINVAL
    assert call(g=1) == lib.EINVAL
    assert call(factor=0.0) == lib.EINVAL and call(factor=-0.1) == lib.EINVAL and call(factor=float('nan')) == lib.EINVAL
    assert call(cut=-1.0) == lib.EINVAL and call(cut=float('inf')) == lib.EINVAL
    assert b'srgan_kde_curves' in lib.library().srgan_last_error()
    assert call(c=65535, g=2 ** 16) == lib.ERANGE                                   # C * G above max_tensor_elements
    assert call(c=65536, g=2) == lib.ERANGE
    assert b'srgan_kde_curves' in lib.library().srgan_last_error()


def test_curve_frame_argument_errors_are_reported_before_any_device_work(lib):
    frame = lib.library().srgan_curve_frame

    def call(vertices=PTR, offsets=PTR, c=2, colours=PTR, widths=PTR, h=8, w=8, x_lo=0.0, x_hi=1.0, y_lo=0.0, y_hi=1.0,
             background=PTR, grid_colour=PTR, x_ticks=PTR, n_x=2, y_ticks=PTR, n_y=2, out=PTR):
        return frame(vertices, offsets, c, colours, widths, h, w, x_lo, x_hi, y_lo, y_hi, background, grid_colour, x_ticks, n_x,
                     y_ticks, n_y, out, None)
    for name in ('vertices', 'offsets', 'colours', 'widths', 'background', 'grid_colour', 'x_ticks', 'y_ticks', 'out'):
        assert call(**{name: None}) == lib.EINVAL, name
    assert call(h=0) == lib.EINVAL and call(w=0) == lib.EINVAL and call(c=-1) == lib.EINVAL and call(n_x=-1) == lib.EINVAL
    assert call(x_lo=1.0, x_hi=1.0) == lib.EINVAL and call(x_lo=2.0, x_hi=1.0) == lib.EINVAL
    assert call(y_lo=1.0, y_hi=1.0) == lib.EINVAL and call(y_hi=float('nan')) == lib.EINVAL
    assert b'srgan_curve_frame' in lib.library().srgan_last_error()
    assert call(h=2 ** 15, w=2 ** 15) == lib.ERANGE
    assert b'srgan_curve_frame' in lib.library().srgan_last_error()


# ---- the Python surface, as far as it goes without a device --------------------------------------------------------------------
def test_host_tensors_are_refused(lib, module):
    import torch
    with pytest.raises(lib.HipLibraryError, match='device tensors'):
        module.wasserstein_distance(torch.zeros(3), torch.zeros(4))
    with pytest.raises(lib.HipLibraryError, match='device tensors'):
        module.kde_curves([torch.zeros(3)])
    with pytest.raises(ValueError):
        module.kde_curves([])


def test_the_switch_is_off_by_default():
    import srgan_amd  # noqa: F401
    from srgan_amd.settings import Settings
    assert not hasattr(Settings(), 'distribution_summaries')
