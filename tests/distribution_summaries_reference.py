"""NumPy restatement of the three distribution-summary contracts of include/srgan_hip.h (``srgan_wasserstein_1d``,
``srgan_kde_curves``, ``srgan_curve_frame``) and of ``distribution_summaries.distribution_frame``: float64 throughout, plus
float32 variants of the Wasserstein sum and of the KDE that round where the kernels round.  test_distribution_summaries_cpu.py
pins the float64 forms against scipy (``wasserstein_distance``, ``gaussian_kde``) and hand-written frames; the GPU tests take
their bounds from the float32 forms' own distance to scipy."""
import numpy as np

THREADS = 1024      # the workgroup of srgan_wasserstein_1d


# ---- Wasserstein ---------------------------------------------------------------------------------------------------------------
def _sorted_with_counts(u, v):
    u, v = np.asarray(u).reshape(-1), np.asarray(v).reshape(-1)
    values = np.concatenate([u, v])
    order = np.argsort(values, kind='stable')
    tags = np.concatenate([np.ones(len(u), dtype=np.int64), np.zeros(len(v), dtype=np.int64)])[order]
    cu = np.cumsum(tags)[:-1]                                  # values of u among the sorted positions 0 .. k
    cv = np.arange(1, len(values)) - cu
    return values[order], np.abs(cu * len(v) - cv * len(u))    # a gap of 0 between equal values: their order cannot matter


def wasserstein(u, v):
    """sum over the gaps of |cu * m - cv * n| * (x[k + 1] - x[k]) / (n * m) in float64."""
    values, weights = _sorted_with_counts(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
    return float((weights * np.diff(values)).sum() / (np.size(u) * np.size(v)))


def wasserstein32(u, v):
    """The kernel's float32 arithmetic and summation tree: P = the power of two >= n + m, thread t of 1024 adds the gaps
    [t * E, (t + 1) * E), E = max(P / 1024, 1), in order; the 1024 partial sums meet in a halving tree; one division."""
    values, weights = _sorted_with_counts(np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32))
    terms = weights.astype(np.float32) * (values[1:] - values[:-1])
    padded = 2
    while padded < len(values):
        padded *= 2
    per_thread = max(padded // THREADS, 1)
    table = np.zeros(THREADS * per_thread, dtype=np.float32)
    table[:len(terms)] = terms
    table = table.reshape(THREADS, per_thread)
    partial = np.zeros(THREADS, dtype=np.float32)
    for column in range(per_thread):
        partial = partial + table[:, column]
    stride = THREADS // 2
    while stride:
        partial = partial[:stride] + partial[stride:2 * stride]
        stride //= 2
    return np.float32(partial[0] / np.float32(np.size(u) * np.size(v)))


# ---- kernel-density curves -----------------------------------------------------------------------------------------------------
def kde_curves(sample_sets, gridsize=100, factor=0.1, cut=3, dtype=np.float64):
    """(support [C, G], density [C, G], stats [C, 4] = (count, min, max, h)) as srgan_kde_curves defines them; ``dtype=float32``
    rounds every operation of the evaluation to float32 in the kernel's order (the statistics come from NumPy's float32
    reductions: the kernel's tree is another, equally fixed one)."""
    real = np.dtype(dtype).type
    count = len(sample_sets)
    support, density = np.zeros((count, gridsize), dtype=dtype), np.zeros((count, gridsize), dtype=dtype)
    stats = np.zeros((count, 4), dtype=dtype)
    for c, samples in enumerate(sample_sets):
        x = np.asarray(samples, dtype=dtype).reshape(-1)
        n = len(x)
        stats[c, 0] = n
        if n == 0:
            continue
        stats[c, 1], stats[c, 2] = x.min(), x.max()
        if n < 2:
            continue
        h = real(factor) * np.sqrt(((x - x.mean()) ** 2).sum() / real(n - 1))
        if not (np.isfinite(h) and h > 0):
            continue
        stats[c, 3] = h
        reach = real(cut) * h
        lo = stats[c, 1] - reach
        step = ((stats[c, 2] + reach) - lo) / real(gridsize - 1)
        s = lo + np.arange(gridsize).astype(dtype) * step
        inverse_h = real(1) / h
        total = np.zeros(gridsize, dtype=dtype)
        for value in x:                                        # the samples in stored order
            z = (s - value) * inverse_h
            total = total + np.exp((real(-0.5) * z) * z)
        support[c] = s
        density[c] = total * (real(1) / ((real(n) * h) * real(2.5066282746310002)))
    return support, density, stats


# ---- the frame -----------------------------------------------------------------------------------------------------------------
def _composite(colour, line, coverage):
    a = np.clip(coverage, 0.0, 1.0)[..., None]
    return colour * (1 - a) + np.asarray(line, dtype=np.float64) * a


def curve_frame(vertices, offsets, colours, widths, height, width, x_limits, y_limits, background, grid_colour, x_ticks=(),
                y_ticks=()):
    """out [3, H, W] in float64 as srgan_curve_frame defines it."""
    vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    (x_lo, x_hi), (y_lo, y_hi) = x_limits, y_limits

    def to_px(x):
        return (np.asarray(x, dtype=np.float64) - x_lo) / (x_hi - x_lo) * width - 0.5

    def to_py(y):
        return (y_hi - np.asarray(y, dtype=np.float64)) / (y_hi - y_lo) * height - 0.5
    cy, cx = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing='ij')
    colour = np.broadcast_to(np.asarray(background, dtype=np.float64), (height, width, 3)).copy()
    for tick in x_ticks:
        colour = _composite(colour, grid_colour, 1 - np.abs(to_px(tick) - cx))
    for tick in y_ticks:
        colour = _composite(colour, grid_colour, 1 - np.abs(to_py(tick) - cy))
    for k in range(len(offsets) - 1):
        begin, end = int(offsets[k]), int(offsets[k + 1])
        if end - begin < 2:
            continue
        px, py = to_px(vertices[begin:end, 0]), to_py(vertices[begin:end, 1])
        nearest = np.full((height, width), np.inf)
        for j in range(end - begin - 1):
            dx, dy = px[j + 1] - px[j], py[j + 1] - py[j]
            qx, qy = cx - px[j], cy - py[j]
            length2 = dx * dx + dy * dy
            along = np.clip((qx * dx + qy * dy) / length2, 0, 1) if length2 > 0 else 0.0
            nearest = np.minimum(nearest, (qx - along * dx) ** 2 + (qy - along * dy) ** 2)
        colour = _composite(colour, colours[k], 0.5 + 0.5 * float(widths[k]) - np.sqrt(nearest))
    return np.ascontiguousarray(colour.transpose(2, 0, 1))


def distribution_frame(module, sample_sets, height=480, width=640):
    """``distribution_summaries.distribution_frame`` from the module's documented constants: the step polyline of the real
    density, then the fitted curves of the six sets; an unfitted set is left out."""
    support, density, stats = kde_curves(sample_sets, module.KDE_GRIDSIZE, module.KDE_BANDWIDTH, module.KDE_CUT)
    pieces, offsets = [np.asarray(module.REAL_DENSITY, dtype=np.float64)], [0, len(module.REAL_DENSITY)]
    for c in range(len(sample_sets)):
        pieces.append(np.stack([support[c], density[c]], axis=1))
        offsets.append(offsets[-1] + support.shape[1])
    widths = module.curve_pixel_widths(width).astype(np.float64)
    widths[1:][stats[:, 3] == 0] = -1.0
    return curve_frame(np.concatenate(pieces), offsets, module.DEEP_PALETTE[list(module.CURVE_PALETTE_INDEXES)], widths, height,
                       width, module.X_LIMITS, module.Y_LIMITS, module.DARKGRID_BACKGROUND, module.GRID_COLOUR, module.X_TICKS,
                       module.Y_TICKS)
