"""The crowd loader's device draws, the parts that need no GPU: the reference of ``srgan_crowd_draw_patches``
(crowd_patch_draws_reference.py) on hand-made scene tables and on tables whose length needs more than 32 bits, the validity of
every drawn centre, the uniformity of the centres and the fairness of the coin the reference produces, the data-parallel
windows, the binding and the argument checks of the two entry points (made before any device work), the loader's unchanged
host mode and the experiment's switch."""
import os
import re

import numpy as np
import pytest
import torch
from scipy.stats import chi2

from crowd_patch_draws_reference import (LABELED_DRAW, UNLABELED_DRAW, draw_table, row_from_words, scene_starts,
                                         sorted_search)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 16        # a non-NULL, 16-byte aligned "pointer" for calls that must fail before touching memory
CPU = torch.device('cpu')

# P = 4: smaller than a patch (no centre) | equal to a patch (one centre) | odd width | odd height and width | no centre again
HAND_SHAPES = [(3, 9), (4, 4), (5, 7), (9, 6), (8, 3)]
HAND_PATCH = 4


def words_for_index(index, length, flip_word=0):
    """Block words whose 64-bit word is the smallest ``r`` with ``floor(r * length / 2^64) == index``."""
    r = -((-index << 64) // length)
    assert (r * length) >> 64 == index and (r == 0 or ((r - 1) * length) >> 64 == index - 1)
    return [r & 0xffffffff, r >> 32, flip_word, 0xdeadbeef]


# ---- the reference on hand-made tables ------------------------------------------------------------------------------------
def test_hand_made_tables():
    starts = scene_starts(HAND_SHAPES, HAND_PATCH)
    assert starts == [0, 0, 1, 1 + 2 * 4, 9 + 6 * 3, 27]
    widths = [shape[1] for shape in HAND_SHAPES]
    seen = []
    for index in range(starts[-1]):                          # every centre is reached, in order, and lies inside its scene
        scene, y, x, flip = row_from_words(words_for_index(index, starts[-1]), starts, widths, HAND_PATCH, True)
        assert scene == sorted_search(starts, index) and scene in (1, 2, 3) and flip == 0
        height, width = HAND_SHAPES[scene]
        assert 2 <= y <= height - 2 and 2 <= x <= width - 2
        seen.append((scene, y, x))
    assert seen[0] == (1, 2, 2)                                                          # the scene equal to a patch
    assert seen[1:9] == [(2, y, x) for y in (2, 3) for x in (2, 3, 4, 5)]                # row-major over the odd width
    assert seen[9:] == [(3, y, x) for y in range(2, 8) for x in (2, 3, 4)]
    assert len(set(seen)) == 27
    # the same centre rule as the host's draw_example
    from srgan_amd.crowd.data import draw_example

    class Fixed:
        def __init__(self, value):
            self.value = value

        def randint(self, bound):
            return self.value if bound != 2 else 1
    for index in range(starts[-1]):
        assert draw_example(Fixed(index), starts[-1], starts[:-1], HAND_SHAPES, HAND_PATCH, True) == seen[index] + (1,)
    # the coin is bit 31 of w2, and only with flip
    assert row_from_words([5, 5, 0x80000000, 0], starts, widths, HAND_PATCH, True)[3] == 1
    assert row_from_words([5, 5, 0x7fffffff, 0], starts, widths, HAND_PATCH, True)[3] == 0
    assert row_from_words([5, 5, 0xffffffff, 0], starts, widths, HAND_PATCH, False)[3] == 0


def test_length_one():
    starts = scene_starts([(2, 2), (6, 6)], 6)
    assert starts == [0, 0, 1]
    table = draw_table(starts, [2, 6], 6, True, 0, 64, LABELED_DRAW, seed=9, iteration=3)
    assert np.array_equal(table[:, :3], np.tile([1, 3, 3], (64, 1))) and set(table[:, 3]) == {0, 1}


def test_every_drawn_centre_is_valid():
    """``index < length`` for the largest word, ``index == 0`` for the smallest, whatever the length."""
    for length in (1, 2, 27, 2 ** 32 - 1, 2 ** 32, 3 * 70000 ** 2, 2 ** 63 - 1):
        assert ((2 ** 64 - 1) * length) >> 64 == length - 1
        top = row_from_words([0xffffffff, 0xffffffff, 0, 0], [0, length], [length + 3], 4, False)
        assert top == (0, 2, 2 + length - 1, 0)
        assert row_from_words([0, 0, 0, 0], [0, length], [length + 3], 4, False) == (0, 2, 2, 0)


# ---- lengths beyond 2^32 --------------------------------------------------------------------------------------------------
BIG_PATCH = 224
BIG_SHAPES = [(70000 + 223, 70001 + 223), (69999 + 223, 70000 + 223), (70002 + 223, 69998 + 223)]


def test_fake_tables_whose_length_needs_the_high_word():
    starts = scene_starts(BIG_SHAPES, BIG_PATCH)
    assert starts[1] > 2 ** 32 and starts[-1] > 3 * 2 ** 32
    widths = [shape[1] for shape in BIG_SHAPES]
    table = draw_table(starts, widths, BIG_PATCH, True, 0, 512, UNLABELED_DRAW, seed=(7 << 32) | 11, iteration=2 ** 31 + 5)
    assert sorted(set(table[:, 0])) == [0, 1, 2]
    indexes = []
    for scene, y, x, flip in table.tolist():
        height, width = BIG_SHAPES[scene]
        assert 112 <= y <= height - 112 and 112 <= x <= width - 112 and flip in (0, 1)
        indexes.append(starts[scene] + (y - 112) * (width - 223) + (x - 112))
    assert max(indexes) > 2 ** 33 and min(indexes) < 2 ** 32                 # both halves of the product matter
    # r's low word alone moves the index by less than one centre here, its high word decides
    low = row_from_words([0xffffffff, 0, 0, 0], starts, widths, BIG_PATCH, False)
    high = row_from_words([0, 0x80000000, 0, 0], starts, widths, BIG_PATCH, False)
    assert low == (0, 112, 112 + 3, 0)                                       # floor((2^32 - 1) * length / 2^64) == 3
    assert ((2 ** 32 - 1) * starts[-1]) >> 64 == 3
    half = starts[-1] // 2
    scene = sorted_search(starts, half)
    assert high[0] == scene == 1 and starts[1] + (high[1] - 112) * 70000 + (high[2] - 112) == half


# ---- the distribution the reference produces ------------------------------------------------------------------------------
UNIFORM_SHAPES = [(10, 20), (3, 3), (13, 11), (9, 30)]               # P = 6: 5 * 15 + 0 + 8 * 6 + 4 * 25 = 223 centres
UNIFORM_PAIRS = [(1, 0), (2 ** 40 + 12345, 7), (0xfeedfacecafebeef, 2 ** 31 + 3), (77, 2 ** 32 - 1)]    # (seed, iteration)


@pytest.fixture(scope='module')
def uniform_tables():
    starts = scene_starts(UNIFORM_SHAPES, 6)
    assert starts[-1] == 223
    widths = [shape[1] for shape in UNIFORM_SHAPES]
    return starts, widths, [draw_table(starts, widths, 6, True, 0, 2 ** 16, LABELED_DRAW, seed, iteration)
                            for seed, iteration in UNIFORM_PAIRS]


def test_the_centres_are_uniform(uniform_tables):
    """Chi-square of 2^16 centres over the 223 cells (222 degrees of freedom, about 294 expected per cell)."""
    starts, widths, tables = uniform_tables
    for (seed, iteration), table in zip(UNIFORM_PAIRS, tables):
        index = np.array([starts[s] + (y - 3) * (widths[s] - 5) + (x - 3) for s, y, x, _ in table.tolist()])
        counts = np.bincount(index, minlength=223)
        assert counts.shape == (223,) and counts.min() > 0
        expected = 2 ** 16 / 223
        statistic = float(((counts - expected) ** 2).sum() / expected)
        p = float(chi2.sf(statistic, 222))
        print('seed %#x iteration %d: chi-square %.2f p %.4f' % (seed, iteration, statistic, p))
        assert p > 1e-3, (seed, iteration, statistic, p)
        assert 1 not in set(table[:, 0])                                    # the scene smaller than a patch


def test_the_coin_is_fair_and_independent_of_the_centre(uniform_tables):
    """Chi-square with one degree of freedom on the coin, and on the coin against the half of the centres."""
    starts, widths, tables = uniform_tables
    for (seed, iteration), table in zip(UNIFORM_PAIRS, tables):
        heads = int(table[:, 3].sum())
        n = len(table)
        statistic = (heads - n / 2) ** 2 / (n / 2) + ((n - heads) - n / 2) ** 2 / (n / 2)
        p = float(chi2.sf(statistic, 1))
        print('seed %#x iteration %d: heads %d of %d, p %.4f' % (seed, iteration, heads, n, p))
        assert p > 1e-3 and set(table[:, 3]) == {0, 1}
        first_scene = table[:, 0] == 0
        cells = np.array([[np.sum(first_scene & (table[:, 3] == c)), np.sum(~first_scene & (table[:, 3] == c))] for c in (0, 1)],
                         dtype=np.float64)
        fitted = cells.sum(1, keepdims=True) * cells.sum(0, keepdims=True) / n
        assert float(chi2.sf(((cells - fitted) ** 2 / fitted).sum(), 1)) > 1e-3
    unflipped = draw_table(starts, widths, 6, False, 0, 256, LABELED_DRAW, *UNIFORM_PAIRS[0])
    assert not unflipped[:, 3].any() and np.array_equal(unflipped[:, :3], tables[0][:256, :3])


def test_draws_differ_with_the_key_the_iteration_and_the_draw_id(uniform_tables):
    starts, widths, tables = uniform_tables
    seed, iteration = UNIFORM_PAIRS[1]
    base = tables[1][:64]
    assert not np.array_equal(base, draw_table(starts, widths, 6, True, 0, 64, UNLABELED_DRAW, seed, iteration))
    assert not np.array_equal(base, draw_table(starts, widths, 6, True, 0, 64, LABELED_DRAW, seed, iteration + 1))
    assert not np.array_equal(base, draw_table(starts, widths, 6, True, 0, 64, LABELED_DRAW, seed ^ (1 << 32), iteration))
    assert np.array_equal(base, draw_table(starts, widths, 6, True, 0, 64, LABELED_DRAW, seed, iteration))


@pytest.mark.parametrize('world_size', [2, 3])
def test_the_ranks_windows_tile_the_global_table(world_size):
    starts = scene_starts(HAND_SHAPES, HAND_PATCH)
    widths = [shape[1] for shape in HAND_SHAPES]
    batch = 12
    whole = draw_table(starts, widths, HAND_PATCH, True, 0, batch, LABELED_DRAW, seed=5, iteration=8)
    local = batch // world_size
    parts = [draw_table(starts, widths, HAND_PATCH, True, rank * local, local, LABELED_DRAW, seed=5, iteration=8)
             for rank in range(world_size)]
    assert np.array_equal(np.concatenate(parts), whole)
    far = 2 ** 32 - 2                                                   # a window across the 32-bit word of the block index
    across = draw_table(starts, widths, HAND_PATCH, True, far, 5, LABELED_DRAW, seed=5, iteration=8)
    for offset in range(5):
        assert np.array_equal(across[offset:offset + 1],
                              draw_table(starts, widths, HAND_PATCH, True, far + offset, 1, LABELED_DRAW, seed=5, iteration=8))
    assert draw_table(starts, widths, HAND_PATCH, True, 3, 0, LABELED_DRAW, seed=5, iteration=8).shape == (0, 4)


# ---- the entry points -----------------------------------------------------------------------------------------------------
def test_the_library_advertises_and_binds_the_entry_points():
    from srgan_amd import _lib
    from srgan_amd.crowd import data
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_CROWD_PATCH_DRAWS\s+0x80000u', header)
    assert re.search(r'#define\s+SRGAN_CROWD_PATCH_DRAW_LABELED\s+0x30000\b', header)
    assert re.search(r'#define\s+SRGAN_CROWD_PATCH_DRAW_UNLABELED\s+0x30001\b', header)
    assert (data.CROWD_DRAW_LABELED, data.CROWD_DRAW_UNLABELED) == (LABELED_DRAW, UNLABELED_DRAW) == (0x30000, 0x30001)
    assert _lib.capabilities().features & 0x80000
    assert _lib.library().srgan_version() == 110
    assert {'srgan_crowd_draw_patches', 'srgan_crowd_extract_patches_indexed'} <= set(_lib.SIGNATURES)
    assert 'srgan_crowd_draw_patches' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def draw_call(lib, **changes):
    a = dict(dict(starts=PTR, heights=PTR, widths=PTR, S=3, P=8, flip=1, first=0, n=4, draw=LABELED_DRAW, state=PTR, table=PTR),
             **changes)
    return lib.library().srgan_crowd_draw_patches(a['starts'], a['heights'], a['widths'], a['S'], a['P'], a['flip'], a['first'],
                                                  a['n'], a['draw'], a['state'], a['table'], None)


def indexed_call(lib, **changes):
    a = dict(dict(images=PTR, labels=PTR, maps=PTR, heights=PTR, widths=PTR, S=3, table=PTR, B=2, P=8, out_images=PTR,
                  out_labels=PTR, out_maps=PTR), **changes)
    return lib.library().srgan_crowd_extract_patches_indexed(a['images'], a['labels'], a['maps'], a['heights'], a['widths'],
                                                             a['S'], a['table'], a['B'], a['P'], a['out_images'],
                                                             a['out_labels'], a['out_maps'], None)


def test_argument_errors_are_reported_before_any_device_work():
    from srgan_amd import _lib
    for name in ('starts', 'heights', 'widths', 'state', 'table'):
        assert draw_call(_lib, **{name: None}) == _lib.EINVAL, name
        assert _lib.library().srgan_last_error()
    assert draw_call(_lib, S=0) == _lib.EINVAL and draw_call(_lib, S=-1) == _lib.EINVAL
    for patch in (0, 1, 7, -2):
        assert draw_call(_lib, P=patch) == _lib.EINVAL, patch
    assert draw_call(_lib, n=-1) == _lib.EINVAL and draw_call(_lib, draw=-1) == _lib.EINVAL
    assert draw_call(_lib, first=-1) == _lib.EINVAL
    assert draw_call(_lib, first=2 ** 63 - 4, n=4) == _lib.EINVAL           # first + n passes 2^63 - 1
    # zero rows: a successful no-op (nothing is launched, the fake pointers are never used), also at the far end
    assert draw_call(_lib, n=0) == 0 and draw_call(_lib, n=0, first=2 ** 63 - 1) == 0
    assert draw_call(_lib, n=0, table=None) == _lib.EINVAL                  # the checks come first

    for name in ('images', 'heights', 'widths', 'table', 'out_images'):
        assert indexed_call(_lib, **{name: None}) == _lib.EINVAL, name
    assert indexed_call(_lib, S=0) == _lib.EINVAL
    assert indexed_call(_lib, B=0) == _lib.EINVAL and indexed_call(_lib, B=-1) == _lib.EINVAL
    assert indexed_call(_lib, B=65536, P=2) == _lib.EINVAL
    for patch in (0, 7, -2):
        assert indexed_call(_lib, P=patch) == _lib.EINVAL, patch
    assert indexed_call(_lib, B=65535, P=106) == _lib.ERANGE                # 65535 * 3 * 106^2 = 2.2e9 elements
    assert b'2^31' in _lib.library().srgan_last_error()
    assert indexed_call(_lib, B=1, P=26756) == _lib.ERANGE                  # 3 * 26756^2 = 2^31 + 1.1e5
    assert indexed_call(_lib, B=65535, P=2 ** 31 - 2) == _lib.ERANGE        # no 64-bit overflow


# ---- the loader -----------------------------------------------------------------------------------------------------------
SHAPES = [(80, 100), (88, 100), (96, 128)]


def scenes():
    from srgan_amd.crowd.data import CrowdExample
    return [CrowdExample(image=np.zeros(shape + (3,), dtype=np.uint8), label=np.zeros(shape, dtype=np.float32),
                         map_=np.zeros(shape, dtype=np.float32)) for shape in SHAPES]


def test_host_mode_is_the_parents_rule_and_creates_no_device_state():
    from srgan_amd.crowd.data import DeviceCrowdPatchLoader, draw_example
    for flip in (True, False):
        loader = DeviceCrowdPatchLoader(scenes(), 6, 64, seed=3, device=CPU, flip=flip)
        explicit = DeviceCrowdPatchLoader(scenes(), 6, 64, seed=3, device=CPU, flip=flip, draws='host')
        generator = np.random.RandomState(3)
        starts = scene_starts(SHAPES, 64)
        for _ in range(3):
            expected = [draw_example(generator, starts[-1], starts[:-1], SHAPES, 64, flip) for _ in range(6)]
            assert loader.draw_positions() == expected == explicit.draw_positions()
        for host in (loader, explicit):
            assert host.draw_mode == 'host' and host.state is None and host.last_table is None and host.scene_pointers is None
            with pytest.raises(ValueError):
                host.start_at(0)
    with pytest.raises(ValueError):
        DeviceCrowdPatchLoader(scenes(), 6, 64, seed=3, device=CPU, draws='gpu')


def test_device_mode_uploads_the_scene_table_once():
    from srgan_amd.crowd.data import DeviceCrowdPatchLoader
    loader = DeviceCrowdPatchLoader(scenes(), 6, 64, seed=2 ** 40 + 1, device=CPU, draws='device', draw_id=UNLABELED_DRAW)
    assert loader.draw_mode == 'device' and loader.draw_id == UNLABELED_DRAW and loader.state is None
    assert loader.scene_starts.dtype == torch.int64 and loader.scene_starts.tolist() == scene_starts(SHAPES, 64)
    assert loader.scene_heights.dtype == loader.scene_widths.dtype == torch.int32
    assert loader.scene_heights.tolist() == [80, 88, 96] and loader.scene_widths.tolist() == [100, 100, 128]
    assert loader.scene_pointers.dtype == torch.int64 and tuple(loader.scene_pointers.shape) == (3, 3)
    for row, tensors in enumerate((loader.images, loader.labels, loader.maps)):
        assert loader.scene_pointers[row].tolist() == [tensor.data_ptr() for tensor in tensors]
    pointers = loader.scene_pointers
    assert loader.upload_scene_table().scene_pointers is pointers            # once
    assert loader.local_batch_size == 6
    with pytest.raises(ValueError):
        DeviceCrowdPatchLoader(scenes(), 6, 63, device=CPU, draws='device')


def test_the_experiment_declares_the_switch():
    from srgan_amd import settings, srgan
    from srgan_amd.crowd.srgan import CrowdExperiment
    assert srgan.Experiment.crowd_patch_draws == 'host'
    experiment = CrowdExperiment(settings.Settings())
    assert experiment.crowd_patch_draws == 'host' and 'crowd_patch_draws' not in vars(experiment)      # a class attribute
    names = {row[0] for row in settings.EXTENSIONS}
    assert 'crowd_patch_draws' not in names and not hasattr(settings.Settings(), 'crowd_patch_draws')
    labeled, unlabeled = experiment.patch_loader_arguments()
    assert labeled == dict(seed=experiment.settings.labeled_dataset_seed) and unlabeled == dict(seed=100)
    experiment.crowd_patch_draws = 'device'
    experiment.settings.device_random_seed = 2 ** 35 + 9
    labeled, unlabeled = experiment.patch_loader_arguments()
    assert labeled == dict(seed=2 ** 35 + 9, draws='device', draw_id=0x30000)
    assert unlabeled == dict(seed=2 ** 35 + 9, draws='device', draw_id=0x30001)
    experiment.crowd_patch_draws = 'gpu'
    with pytest.raises(ValueError, match='crowd_patch_draws'):
        experiment.patch_loader_arguments()
