"""Distribution summaries built on the device: what the coefficient application logs about distributions at a summary step
(reference coefficient/srgan.py:56-78, coefficient/presentation.py:19-55).  The reference downloads every prediction and calls
``scipy.stats.wasserstein_distance``, seaborn's ``kdeplot`` and matplotlib on the host; here the predictions already sit in HBM
and three entry points (csrc/distribution_summaries.hip: ``srgan_wasserstein_1d``, ``srgan_kde_curves``, ``srgan_curve_frame``)
compute the distance, the kernel-density curves and the picture there.  Only the finished scalar and the finished picture are
downloaded, by the summary writer.  The figure's text (the legend, the "Step: N" label) is not drawn: DESIGN.md section 9."""
import numpy as np
import torch

from . import _lib, functional as F
from .tape import Var

WASSERSTEIN_MAX_VALUES = 16384      # SRGAN_WASSERSTEIN_MAX_VALUES of include/srgan_hip.h


def _tensor(value):
    return value.data if isinstance(value, Var) else value


def _device_floats(value):
    value = _tensor(value).detach()
    if not value.is_cuda:
        raise _lib.HipLibraryError('distribution summaries need device tensors (there is no CPU fallback)')
    return value.float().contiguous()


_constants = {}      # (device index, name, key) -> a small constant tensor on that device, uploaded once


def _constant(device, name, key, make):
    """``make()`` (a NumPy array) on ``device``, uploaded at first use: offsets for a set of sizes, colour tables, ticks."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    if (index, name, key) not in _constants:
        _constants[(index, name, key)] = torch.from_numpy(np.ascontiguousarray(make())).to(torch.device('cuda', index))
    return _constants[(index, name, key)]


def offsets_table(device, sizes):
    """Device int32 ``[len(sizes) + 1]``: where each of the back-to-back arrays of ``sizes`` elements starts, and the end."""
    sizes = tuple(int(size) for size in sizes)
    return _constant(device, 'offsets', sizes, lambda: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))


def wasserstein_distance(u, v):
    """``scipy.stats.wasserstein_distance(u, v)`` of two device tensors (any shape; every element is a sample) as a 0-d device
    tensor: one launch of ``srgan_wasserstein_1d``, one workgroup; at most ``WASSERSTEIN_MAX_VALUES`` samples together."""
    u, v = _device_floats(u).reshape(-1), _device_floats(v).reshape(-1)
    out = F._empty((), u)
    F._call('srgan_wasserstein_1d', u.data_ptr(), u.numel(), v.data_ptr(), v.numel(), out.data_ptr(), F._stream())
    return out


def kde_curves(samples, gridsize=100, bw=0.1, cut=3):
    """The curves seaborn's ``kdeplot(x, bw=bw, cut=cut, gridsize=gridsize)`` draws for each device tensor of ``samples`` (a
    list), in one ``srgan_kde_curves`` call: ``(support, density, stats)``, ``[C, gridsize]`` twice and ``[C, 4]`` = (count, min,
    max, bandwidth h).  A curve that cannot be fitted (fewer than 2 samples, no spread) has h = 0 and zero rows."""
    parts = [_device_floats(part).reshape(-1) for part in samples]
    if not parts:
        raise ValueError('kde_curves takes at least one tensor of samples')
    together = parts[0] if len(parts) == 1 else torch.cat(parts)
    offsets = offsets_table(together.device, [part.numel() for part in parts])
    count, gridsize = len(parts), int(gridsize)
    support, density = F._empty((count, gridsize), together), F._empty((count, gridsize), together)
    stats = F._empty((count, 4), together)
    F._call('srgan_kde_curves', together.data_ptr() if together.numel() else stats.data_ptr(), offsets.data_ptr(), count, gridsize,
            float(bw), float(cut), support.data_ptr(), density.data_ptr(), stats.data_ptr(), F._stream())
    return support, density, stats


def curve_frame(vertices, offsets, colours, widths, height, width, x_limits, y_limits, background, grid_colour, x_ticks=None,
                y_ticks=None):
    """A line chart ``[3, height, width]`` in [0, 1], one ``srgan_curve_frame`` launch: polyline ``k`` is ``vertices[offsets[k] :
    offsets[k + 1]]`` (``[total, 2]`` of (x, y) in data coordinates; ``offsets`` device int32) in ``colours[k]`` at ``widths[k]``
    pixels, over ``background`` with one-pixel grid lines in ``grid_colour`` at the ticks.  Every tensor is a device tensor."""
    vertices, colours, widths = _device_floats(vertices), _device_floats(colours), _device_floats(widths)
    background, grid_colour = _device_floats(background), _device_floats(grid_colour)
    if not offsets.is_cuda or offsets.dtype != torch.int32:
        raise _lib.HipLibraryError('curve_frame takes its offsets as a device int32 tensor')
    curves = offsets.numel() - 1
    if vertices.dim() != 2 or vertices.shape[1] != 2 or colours.shape != (curves, 3) or widths.shape != (curves,):
        raise ValueError(f'curve_frame takes vertices [total, 2], colours [C, 3] and widths [C] for C + 1 offsets, not '
                         f'{tuple(vertices.shape)}, {tuple(colours.shape)}, {tuple(widths.shape)} and {offsets.numel()} offsets')
    if background.numel() != 3 or grid_colour.numel() != 3:
        raise ValueError('curve_frame takes RGB triples as background and grid colour')
    x_ticks = None if x_ticks is None else _device_floats(x_ticks)
    y_ticks = None if y_ticks is None else _device_floats(y_ticks)
    out = F._empty((3, int(height), int(width)), vertices)
    F._call('srgan_curve_frame', vertices.data_ptr(), offsets.data_ptr(), curves, colours.data_ptr(), widths.data_ptr(),
            int(height), int(width), float(x_limits[0]), float(x_limits[1]), float(y_limits[0]), float(y_limits[1]),
            background.data_ptr(), grid_colour.data_ptr(), None if x_ticks is None else x_ticks.data_ptr(),
            0 if x_ticks is None else x_ticks.numel(), None if y_ticks is None else y_ticks.data_ptr(),
            0 if y_ticks is None else y_ticks.numel(), out.data_ptr(), F._stream())
    return out


# seaborn's default palette "deep" (ten colours, #4C72B0 ...) and the axes face colour of its "darkgrid" style (#EAEAF2) under
# white grid lines: what ``sns.set()`` / ``sns.set_style('darkgrid')`` give the reference's figure.
DEEP_PALETTE = (np.array([(0x4C, 0x72, 0xB0), (0xDD, 0x84, 0x52), (0x55, 0xA8, 0x68), (0xC4, 0x4E, 0x52), (0x81, 0x72, 0xB3),
                          (0x93, 0x78, 0x60), (0xDA, 0x8B, 0xC3), (0x8C, 0x8C, 0x8C), (0xCC, 0xB9, 0x74), (0x64, 0xB5, 0xCD)],
                         dtype=np.float32) / np.float32(255))
DARKGRID_BACKGROUND = np.array([0xEA, 0xEA, 0xF2], dtype=np.float32) / np.float32(255)
GRID_COLOUR = np.ones(3, dtype=np.float32)

X_LIMITS, Y_LIMITS = (-4.0, 4.0), (0.0, 1.0)
X_TICKS = np.arange(-4, 5, dtype=np.float32)
Y_TICKS = np.arange(6, dtype=np.float32) * np.float32(0.2)
# The real label density, MixtureModel([uniform(-2, 1), uniform(1, 1)]).pdf: 0.5 on [-2, -1] and on [1, 2], 0 elsewhere -- the
# reference samples it every 0.001; the same steps as ten vertices.
REAL_DENSITY = np.array([(-4, 0), (-2, 0), (-2, 0.5), (-1, 0.5), (-1, 0), (1, 0), (1, 0.5), (2, 0.5), (2, 0), (4, 0)],
                        dtype=np.float32)
# presentation.py:30-46 in drawing order: the real density, then the fake / unlabeled / GAN validation / GAN train / DNN
# validation / DNN train curves.  Line widths in points; the reference's figure is 6.4 inches wide.
CURVE_PALETTE_INDEXES = (0, 4, 1, 2, 2, 3, 3)
CURVE_POINT_WIDTHS = (1.5, 1.5, 1.5, 1.5, 0.5, 1.5, 0.5)
KDE_GRIDSIZE, KDE_BANDWIDTH, KDE_CUT = 100, 0.1, 3      # kdeplot's gridsize and cut defaults, the reference's bw
# polyfit(linspace(-1, 1, 10), y, 3) as a product: y [10] -> the four coefficients, highest power first.
POLYFIT_PSEUDO_INVERSE = np.linalg.pinv(np.vander(np.linspace(-1, 1, num=10), 4)).astype(np.float32)


def curve_pixel_widths(width):
    """The curves' line widths in pixels of a frame ``width`` wide: points at width / 6.4 dots per inch."""
    return np.array(CURVE_POINT_WIDTHS, dtype=np.float32) * np.float32(width / 6.4 / 72)


def fake_coefficients(fake_examples):
    """The samples of the reference's "Fake Data Distribution" curve, ``fake_a3[0, :]`` of presentation.py:24,33: the four
    coefficients of the cubic fitted to the first ten numbers of the FIRST generated example -- ``np.transpose(np.polyfit(...))``
    is [examples, 4], so ``[0, :]`` is one example's fit and not the cubic coefficient of every example.  Kept as it is written.
    The fit is a product with the fixed 4 x 10 pseudo-inverse of the Vandermonde matrix, through the linear kernel."""
    fake_examples = _device_floats(fake_examples)
    observations = fake_examples[:1, :10].contiguous()
    weight = _constant(fake_examples.device, 'polyfit', (), lambda: POLYFIT_PSEUDO_INVERSE)
    return F.linear(F.constant(observations), F.constant(weight)).data.reshape(-1)


def distribution_frame(fake_coefficients, unlabeled, gan_validation, gan_train, dnn_validation, dnn_train, height=480, width=640):
    """The reference's ``generate_display_frame`` picture as a device tensor ``[3, height, width]``: x in [-4, 4], y in [0, 1],
    seaborn's darkgrid background with white grid lines at the integer x and at every 0.2 in y, the real label density as a
    step polyline in palette colour 0, then the kernel-density curves (bw 0.1) of the six sample sets in the reference's order
    and colours -- palette 4, 1, 2, 2, 3, 3 -- the two train curves at a third of the others' width.  A set whose curve cannot be
    fitted is left out, as the reference leaves it out.  One ``srgan_kde_curves`` and one ``srgan_curve_frame`` call."""
    sets = [_device_floats(part).reshape(-1) for part in (fake_coefficients, unlabeled, gan_validation, gan_train, dnn_validation,
                                                         dnn_train)]
    device = sets[0].device
    support, density, stats = kde_curves(sets, KDE_GRIDSIZE, KDE_BANDWIDTH, KDE_CUT)
    real = _constant(device, 'real density', (), lambda: REAL_DENSITY)
    vertices = torch.cat([real, torch.stack([support, density], dim=2).reshape(-1, 2)])
    offsets = offsets_table(device, [REAL_DENSITY.shape[0]] + [KDE_GRIDSIZE] * len(sets))
    colours = _constant(device, 'curve colours', (), lambda: DEEP_PALETTE[list(CURVE_PALETTE_INDEXES)])
    widths = _constant(device, 'curve widths', (int(width),), lambda: curve_pixel_widths(width)).clone()
    # an unfitted curve (h = 0: rows of zeros) gets the width -1, at which the frame kernel's coverage is 0 everywhere
    widths[1:] = torch.where(stats[:, 3] > 0, widths[1:], torch.full_like(widths[1:], -1.0))
    return curve_frame(vertices, offsets, colours, widths, height, width, X_LIMITS, Y_LIMITS,
                       _constant(device, 'background', (), lambda: DARKGRID_BACKGROUND),
                       _constant(device, 'grid colour', (), lambda: GRID_COLOUR),
                       _constant(device, 'x ticks', (), lambda: X_TICKS), _constant(device, 'y ticks', (), lambda: Y_TICKS))
