"""The tests' own reference of the crowd loader's device draws: ``srgan_crowd_draw_patches`` (include/srgan_hip.h) written
out in NumPy and Python integers -- the Philox words from device_draws_reference.py, the 128-bit product in ``int`` -- and a
NumPy restatement of ``srgan_crowd_extract_patches_indexed`` on the host transforms of ``srgan_amd.crowd.data``
(``extract_padded_patch`` / ``negative_one_to_one``) with the rule for a scene outside the table.  Shared by
test_crowd_patch_draws_cpu.py and test_crowd_patch_draws_gpu.py; no tests of its own."""
import numpy as np

from device_draws_reference import block_words

LABELED_DRAW, UNLABELED_DRAW = 0x30000, 0x30001
INT_MIN = -2 ** 31


def scene_starts(shapes, patch_size):
    """``starts[S + 1]`` (Python ints): the running count of valid patch centres of scenes ``(H, W)``."""
    starts = [0]
    for height, width in shapes:
        starts.append(starts[-1] + max(height - patch_size + 1, 0) * max(width - patch_size + 1, 0))
    return starts


def row_from_words(words, starts, widths, patch_size, flip):
    """``(scene, y, x, flip_bit)`` of one example from its block's four words."""
    scenes, length = len(starts) - 1, int(starts[-1])
    r = (int(words[1]) << 32) | int(words[0])
    index = (r * length) >> 64
    scene = int(np.searchsorted(np.asarray(starts[:scenes], dtype=np.int64), index, side='right')) - 1
    scene = min(max(scene, 0), scenes - 1)
    local, columns = index - int(starts[scene]), int(widths[scene]) - patch_size + 1
    half = patch_size // 2
    return scene, half + local // columns, half + local % columns, (int(words[2]) >> 31) if flip else 0


def draw_table(starts, widths, patch_size, flip, first, n, draw, seed, iteration):
    """int64 ``[n, 4]``: rows ``first .. first + n - 1`` of the draw's table.  Example ``e`` owns the whole block ``e``: element
    ``4 * e`` of the ``srgan_random_fill`` stream's word layout."""
    table = np.empty((n, 4), dtype=np.int64)
    if n:
        words, skip = block_words(seed, iteration, draw, 4 * int(first), 4 * n)
        assert skip == 0 and words.shape == (n, 4)
        for i in range(n):
            table[i] = row_from_words(words[i], starts, widths, patch_size, flip)
    return table


def sorted_search(starts, index):
    """The scene of ``index`` by a plain loop: the largest ``s`` with ``starts[s] <= index``."""
    return max(s for s in range(len(starts) - 1) if starts[s] <= index)


def indexed_patches(images, labels, maps, table, patch_size):
    """``(image f32[B, 3, P, P], label f32[B, P, P], map f32[B, P, P])`` of table rows ``(scene, y, x, flip)`` over scenes
    ``images[s]`` u8 ``[H, W, 3]``, ``labels[s]`` / ``maps[s]`` f32 ``[H, W]`` (``labels`` / ``maps`` may be None: zeros then).
    A scene outside ``[0, S)``: image -1, label and map 0."""
    from srgan_amd.crowd.data import extract_padded_patch, negative_one_to_one
    count = len(table)
    out_image = np.empty((count, 3, patch_size, patch_size), dtype=np.float32)
    out_label = np.zeros((count, patch_size, patch_size), dtype=np.float32)
    out_map = np.zeros((count, patch_size, patch_size), dtype=np.float32)
    for b, (scene, y, x, flip) in enumerate(np.asarray(table).tolist()):
        if not 0 <= scene < len(images):
            out_image[b] = -1.0
            continue
        planes = [images[scene]]
        planes.append(labels[scene][:, :, None] if labels is not None else None)
        planes.append(maps[scene][:, :, None] if maps is not None else None)
        cut = [None if plane is None else padded_patch(plane, y, x, patch_size, extract_padded_patch) for plane in planes]
        if flip:
            cut = [None if patch is None else patch[:, ::-1] for patch in cut]
        out_image[b] = negative_one_to_one(cut[0]).transpose((2, 0, 1))
        if cut[1] is not None:
            out_label[b] = cut[1][:, :, 0]
        if cut[2] is not None:
            out_map[b] = cut[2][:, :, 0]
    return out_image, out_label, out_map


def padded_patch(plane, y, x, patch_size, extract):
    """``extract_padded_patch`` for ANY centre: the host transform pads a centre that lies inside the scene; a centre whose
    patch misses the scene altogether (or starts beyond it) is cut from a canvas of zeros, which is what padding means."""
    half = patch_size // 2
    height, width = plane.shape[0], plane.shape[1]
    if 0 <= y <= height and 0 <= x <= width:
        return extract(plane, y, x, patch_size)
    canvas = np.zeros((patch_size, patch_size, plane.shape[2]), dtype=plane.dtype)
    for row in range(patch_size):
        for col in range(patch_size):
            sy, sx = y - half + row, x - half + col
            if 0 <= sy < height and 0 <= sx < width:
                canvas[row, col] = plane[sy, sx]
    return canvas
