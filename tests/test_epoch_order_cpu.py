"""The epoch order of the resident image loaders' device draws, without a GPU: the reference stream of
epoch_order_reference.py (permutations, epochs and draw ids, data-parallel windows, the drop-last tail, uniformity), the
public header's constants, and ``ResidentImageLoader``'s arguments in both modes."""
import os
import re

import numpy as np
import pytest
import torch

from device_draws_reference import philox4x32_10
from epoch_order_reference import (EPOCH_ORDER_MAX, LABELED_DRAW, UNLABELED_DRAW, batch_table, epoch_and_batch, epoch_keys,
                                   epoch_order, stable_argsort)

SEED = 2 ** 40 + 17
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('n', [1, 2, 3, 255, 256, 257, 1000, 50000])
def test_every_order_is_a_permutation(n):
    for seed, epoch, draw in ((0, 0, LABELED_DRAW), (SEED, 3, UNLABELED_DRAW)):
        order = epoch_order(seed, epoch, draw, n)
        assert order.shape == (n,) and np.array_equal(np.sort(order), np.arange(n))
        keys = epoch_keys(seed, epoch, draw, n)
        assert np.all(np.diff(keys[order].astype(object)) >= 0)          # ascending keys


def test_epochs_and_draw_ids_differ():
    base = epoch_order(SEED, 0, LABELED_DRAW, 1000).tolist()
    assert base != epoch_order(SEED, 1, LABELED_DRAW, 1000).tolist()
    assert base != epoch_order(SEED, 0, UNLABELED_DRAW, 1000).tolist()
    assert base != epoch_order(SEED + 1, 0, LABELED_DRAW, 1000).tolist()
    assert base != epoch_order(SEED + 2 ** 32, 0, LABELED_DRAW, 1000).tolist()          # the seed's high half counts
    assert base == epoch_order(SEED, 0, LABELED_DRAW, 1000).tolist()
    # a frame's key does not depend on n: the first keys of a longer database are those of a shorter one
    assert np.array_equal(epoch_keys(SEED, 2, LABELED_DRAW, 1000)[:10], epoch_keys(SEED, 2, LABELED_DRAW, 10))


def test_the_tie_rule_of_the_reference_is_the_stable_one():
    assert stable_argsort([5, 5, 5, 5]).tolist() == [0, 1, 2, 3]
    assert stable_argsort([7, 3, 7, 3, 1]).tolist() == [4, 1, 3, 0, 2]
    assert stable_argsort([2 ** 32, 1, 2 ** 63, 2 ** 32 - 1]).tolist() == [1, 3, 0, 2]  # the high word decides first


def test_steps_map_to_epochs_and_batches():
    assert epoch_and_batch(0, 10, 4) == (0, 0, 2)
    assert epoch_and_batch(1, 10, 4) == (0, 1, 2)
    assert epoch_and_batch(2, 10, 4) == (1, 0, 2)
    assert epoch_and_batch(5, 12, 4) == (1, 2, 3)
    assert epoch_and_batch(7, 4, 4) == (7, 0, 1)
    with pytest.raises(AssertionError):
        epoch_and_batch(0, 3, 4)


def test_the_data_parallel_windows_tile_the_global_table():
    n, batch = 23, 6
    for step in (0, 2, 3, 7):
        whole = batch_table(SEED, step, LABELED_DRAW, n, batch)
        assert len(whole) == batch and len(set(whole)) == batch
        for world_size in (2, 3):
            local = batch // world_size
            parts = [batch_table(SEED, step, LABELED_DRAW, n, batch, rank * local, local) for rank in range(world_size)]
            assert [frame for part in parts for frame in part] == whole
    assert batch_table(SEED, 0, LABELED_DRAW, n, batch, 1, 4) == batch_table(SEED, 0, LABELED_DRAW, n, batch)[1:5]
    assert batch_table(SEED, 0, LABELED_DRAW, n, batch, 6, 0) == []


def test_the_drop_last_tail_never_appears_in_a_table():
    for n, batch, draw in ((10, 4, LABELED_DRAW), (12, 4, UNLABELED_DRAW), (23, 6, LABELED_DRAW)):
        batches = n // batch
        for epoch in range(3):
            order = epoch_order(SEED, epoch, draw, n).tolist()
            seen = []
            for step in range(epoch * batches, (epoch + 1) * batches):
                seen += batch_table(SEED, step, draw, n, batch)
            assert seen == order[:batches * batch]
            assert not set(seen) & set(order[batches * batch:]) and len(set(seen)) == batches * batch


@pytest.mark.parametrize('draw', [LABELED_DRAW, UNLABELED_DRAW])
@pytest.mark.parametrize('n', [16, 64])
def test_positions_and_frames_are_independent_over_many_epochs(n, draw):
    """Chi-square of the position x frame counts over 4096 epochs at seed 0: every frame should visit every position equally
    often.  (n - 1)^2 degrees of freedom; the cap is the mean plus six standard deviations of that distribution.  A cap on the
    reference itself: the kernel has to equal the reference exactly (test_epoch_order_gpu.py)."""
    epochs = 4096
    counter = np.zeros((epochs, n, 4), dtype=np.uint64)
    counter[:, :, 0] = np.arange(n, dtype=np.uint64)[None, :]
    counter[:, :, 2] = draw
    counter[:, :, 3] = np.arange(epochs, dtype=np.uint64)[:, None]
    words = philox4x32_10(counter, np.array([0, 0], dtype=np.uint64))
    keys = (words[..., 1].astype(np.uint64) << np.uint64(32)) | words[..., 0].astype(np.uint64)
    assert np.array_equal(keys[5], epoch_keys(0, 5, draw, n))             # the vectorised keys are the reference's
    orders = np.argsort(keys, axis=1, kind='stable')
    counts = np.zeros((n, n), dtype=np.int64)
    np.add.at(counts, (np.broadcast_to(np.arange(n), orders.shape), orders), 1)
    expected = epochs / n
    chi_square = float(((counts - expected) ** 2 / expected).sum())
    dof = (n - 1) ** 2
    cap = dof + 6 * np.sqrt(2 * dof)
    print(f'n = {n}, draw {draw:#x}: chi-square {chi_square:.1f}, dof {dof}, cap {cap:.1f}')
    assert chi_square < cap


def test_the_header_reserves_the_constants():
    with open(os.path.join(ROOT, 'include', 'srgan_hip.h')) as handle:
        header = handle.read()
    assert re.search(r'#define\s+SRGAN_FEATURE_EPOCH_ORDER\s+0x100000u', header)
    assert re.search(r'#define\s+SRGAN_IMAGE_BATCH_DRAW_LABELED\s+0x30002\b', header)
    assert re.search(r'#define\s+SRGAN_IMAGE_BATCH_DRAW_UNLABELED\s+0x30003\b', header)
    assert re.search(r'#define\s+SRGAN_EPOCH_ORDER_MAX\s+\(1 << 20\)', header)
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib, data
    assert (data.IMAGE_DRAW_LABELED, data.IMAGE_DRAW_UNLABELED) == (LABELED_DRAW, UNLABELED_DRAW) == (0x30002, 0x30003)
    assert data.EPOCH_ORDER_MAX == EPOCH_ORDER_MAX == 2 ** 20
    for name in ('srgan_epoch_order', 'srgan_argsort_u64', 'srgan_epoch_batch_indices'):
        assert name in _lib.SIGNATURES
    assert _lib.capabilities().features & 0x100000
    assert _lib.library().srgan_version() == 110


def dataset(count, seed=1):
    import srgan_amd  # noqa: F401
    from srgan_amd.data import ResidentImageDataset
    generator = np.random.RandomState(seed)
    return ResidentImageDataset(generator.randint(0, 256, size=(count, 3, 4, 4)).astype(np.uint8),
                                generator.rand(count).astype(np.float32))


class Ranks:
    def __init__(self, world_size, rank):
        self.world_size, self.rank = world_size, rank

    def local_batch(self, batch_size):
        if batch_size % self.world_size:
            raise ValueError('the global batch does not divide over the ranks')
        return batch_size // self.world_size


def test_the_loaders_arguments():
    from srgan_amd.data import ResidentImageLoader
    frames = dataset(10)
    with pytest.raises(ValueError):
        ResidentImageLoader(frames, 4, draws='gpu')
    with pytest.raises(ValueError):
        ResidentImageLoader(frames, 4, draws='device', shuffle=False)
    with pytest.raises(ValueError):
        ResidentImageLoader(frames, 11, draws='device')                   # not one full batch
    with pytest.raises(ValueError):
        ResidentImageLoader(frames, 4, draws='device', draw_id=-1)
    with pytest.raises(ValueError):
        ResidentImageLoader(frames, 4, draws='device', draw_id=2 ** 31)
    with pytest.raises(ValueError):
        ResidentImageLoader(frames, 4, draws='device', dp=Ranks(3, 0))
    loader = ResidentImageLoader(frames, 4, seed=2 ** 64 + 5, draws='device', draw_id=UNLABELED_DRAW, dp=Ranks(2, 1))
    assert (loader.draw_mode, loader.draw_id, loader.local_batch, len(loader)) == ('device', UNLABELED_DRAW, 2, 2)
    assert loader.generator is None and loader.state is None and loader.order is None and loader.last_table is None
    assert loader.batch_shapes() == ((2, 3, 4, 4), (2,))
    assert ResidentImageLoader(frames, 4, image_size=(6, 8), draws='device').batch_shapes() == ((4, 3, 6, 8), (4,))
    assert ResidentImageLoader(frames, 4, draws='device').draw_id == LABELED_DRAW
    with pytest.raises(ValueError):
        loader.epoch_order()                                              # the host list belongs to the host mode


def test_host_mode_is_the_default_and_keeps_its_generator():
    from srgan_amd.data import ResidentImageLoader
    frames = dataset(10)
    for loader in (ResidentImageLoader(frames, 4, seed=9), ResidentImageLoader(frames, 4, seed=9, draws='host')):
        assert loader.draw_mode == 'host' and loader.state is None and loader.order is None
        generator = torch.Generator().manual_seed(9)                      # the parent's loader: this generator, this call
        for _ in range(2):
            assert torch.equal(loader.epoch_order(), torch.randperm(10, generator=generator).to(torch.int32))
        for call in (lambda: loader.start_at(0), loader.device_batch, loader.prepare_capture):
            with pytest.raises(ValueError):
                call()
    unshuffled = ResidentImageLoader(frames, 4, shuffle=False)
    assert unshuffled.epoch_order().tolist() == list(range(10))


def test_the_experiments_switches_default_to_today():
    import srgan_amd  # noqa: F401
    from srgan_amd.srgan import Experiment
    assert Experiment.image_batch_draws == 'host' and Experiment.capture_loaders is False
