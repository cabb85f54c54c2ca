"""NumPy fp32 restatement of the two image-summary contracts of include/srgan_hip.h (``srgan_image_grid``,
``srgan_density_heatmaps``), for the tests.  It does not import the product.

``make_grid`` restates torchvision.utils.make_grid (which is not installed where the fixtures are generated, so it is pinned by
hand-written answers in test_image_summaries_cpu.py); ``density_heatmaps`` restates the reference's
``convert_density_maps_to_heatmaps`` -- matplotlib's Normalize and Colormap.__call__ on a float32 array -- and is pinned against
the reference's own output in tests/golden/g17_image_summaries.npz."""
import numpy as np

F32 = np.float32


def grid_shape(n, height, width, nrow, padding):
    if n == 1:
        return 3, height, width
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    return 3, ymaps * (height + padding) + padding, xmaps * (width + padding) + padding


def normalise(images, low, high):
    """(min(max(x, low), high) - low) / max(high - low, 1e-5), every step rounded to fp32."""
    low, high = F32(low), F32(high)
    clamped = np.minimum(np.maximum(np.asarray(images, dtype=F32), low), high)
    return ((clamped - low) / np.maximum(high - low, F32(1e-5))).astype(F32)


def make_grid(images, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0):
    """images [N, C, H, W], C in {1, 3} -> [3, GH, GW] float32."""
    images = np.asarray(images, dtype=F32)
    n, channels, height, width = images.shape
    assert channels in (1, 3)
    if channels == 1:
        images = np.repeat(images, 3, axis=1)
    if normalize:
        images = normalise(images, *value_range)
    if n == 1:
        return images[0].copy()
    xmaps = min(nrow, n)
    grid = np.full(grid_shape(n, height, width, nrow, padding), F32(pad_value), dtype=F32)
    for k in range(n):
        top = (k // xmaps) * (height + padding) + padding
        left = (k % xmaps) * (width + padding) + padding
        grid[:, top:top + height, left:left + width] = images[k]
    return grid


def scaled_positions(values, vmin, vmax, entries):
    """t * entries in fp32 (t = 0 where the range is empty): the number whose truncation is the table entry."""
    values = np.asarray(values, dtype=F32)
    vmin, vmax = F32(vmin), F32(vmax)
    if vmax == vmin:
        return np.zeros(values.shape, dtype=F32)
    return (((values - vmin) / (vmax - vmin)).astype(F32) * F32(entries)).astype(F32)


def entries_of(scaled, entries):
    scaled = np.asarray(scaled, dtype=F32)
    truncated = np.clip(scaled, 0, entries).astype(np.int64)          # (in range before the cast; truncation toward zero)
    return np.where(scaled < 0, 0, np.where(scaled >= entries, entries - 1, truncated))


def identity_resize(plane, size):
    assert plane.shape == (size, size), 'only the equal-size case is restated without torch'
    return np.asarray(plane, dtype=F32)


def torch_resize(plane, size):
    """torch.nn.functional.interpolate(mode='bilinear', align_corners=False) on the CPU: the arithmetic the resize entry
    point is defined by."""
    import torch
    source = torch.from_numpy(np.ascontiguousarray(plane, dtype=F32))[None, None]
    return torch.nn.functional.interpolate(source, size=(size, size), mode='bilinear', align_corners=False)[0, 0].numpy()


def density_heatmaps(labels, predicted, size, lut, resize=identity_resize):
    """labels [B, h, w], predicted [B, M, h, w], lut [entries, 3] -> (tiles [B, M + 1, 3, size, size], ranges [B, M, 2],
    entries [B, M + 1, size, size], scaled [B, M + 1, size, size]): per example the label under the range of pair (b, 0), then
    every prediction under its own pair's range."""
    labels, predicted, lut = np.asarray(labels, dtype=F32), np.asarray(predicted, dtype=F32), np.asarray(lut, dtype=F32)
    batch, heads = predicted.shape[:2]
    count = lut.shape[0]
    ranges = np.empty((batch, heads, 2), dtype=F32)
    indices = np.empty((batch, heads + 1, size, size), dtype=np.int64)
    scaled = np.empty((batch, heads + 1, size, size), dtype=F32)
    for b in range(batch):
        for m in range(heads):
            ranges[b, m] = (min(labels[b].min(), predicted[b, m].min()), max(labels[b].max(), predicted[b, m].max()))
            scaled[b, m + 1] = scaled_positions(resize(predicted[b, m], size), ranges[b, m, 0], ranges[b, m, 1], count)
        scaled[b, 0] = scaled_positions(resize(labels[b], size), ranges[b, 0, 0], ranges[b, 0, 1], count)
    indices[:] = entries_of(scaled, count)
    tiles = np.ascontiguousarray(lut[indices].transpose(0, 1, 4, 2, 3))
    return tiles, ranges, indices, scaled


def entries_from_colours(tiles, lut):
    """The table entry of every pixel of planar RGB tiles [..., 3, P, P] whose colours are rows of ``lut`` (rows are unique)."""
    lut = np.asarray(lut, dtype=F32)
    table = {tuple(row): index for index, row in enumerate(lut.tolist())}
    assert len(table) == len(lut)
    pixels = np.moveaxis(np.asarray(tiles, dtype=F32), -3, -1)
    flat = pixels.reshape(-1, 3).tolist()
    return np.array([table[tuple(colour)] for colour in flat], dtype=np.int64).reshape(pixels.shape[:-1])


def near_an_integer(scaled, margin=1e-3):
    """Pixels whose t * entries lies within ``margin`` of an integer: where one rounding may move the entry by one."""
    scaled = np.asarray(scaled, dtype=np.float64)
    return np.abs(scaled - np.rint(scaled)) <= margin


def check_entries(got, expected, scaled, what=''):
    """The rule of the heatmap tests: entries are equal except where t * entries is within 1e-3 of an integer; there they may
    differ by one entry, and such pixels are at most 1 % of a tile."""
    got, expected = np.asarray(got), np.asarray(expected)
    assert got.shape == expected.shape, (what, got.shape, expected.shape)
    different = got != expected
    close = near_an_integer(scaled)
    assert not (different & ~close).any(), (what, 'an entry differs away from an integer boundary')
    assert (np.abs(got - expected) <= 1).all(), (what, 'an entry differs by more than one')
    tiles = different.reshape(-1, got.shape[-2] * got.shape[-1])
    assert (tiles.sum(axis=1) <= 0.01 * tiles.shape[1]).all(), (what, 'more than 1 % of a tile differs')
