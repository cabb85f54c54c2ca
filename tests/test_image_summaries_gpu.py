"""Image summaries on the MI355X (settings.image_summaries; csrc/image_summaries.hip): ``srgan_image_grid`` and
``srgan_density_heatmaps`` against the tests' NumPy restatement (image_summaries_reference.py, pinned on the CPU against
hand-written answers and the reference's own heatmaps), the composed map comparison, and the summaries of tiny age and crowd
experiments -- tags, shapes, G's samples recomputed from the same device draw, and that switching the pictures on leaves the
training bits alone.

Outputs are pre-filled with NaN and sit between NaN guards at a start that is not 16-byte aligned: both kernels are gathers
that write every element exactly once and nothing else."""
import datetime
import os

import numpy as np
import pytest
import torch

import image_summaries_reference as R
from test_steps_gpu import finish_setup

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 5                                   # floats of NaN on either side of an output (an odd count: an unaligned start)


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    _lib.library()
    return _lib


@pytest.fixture(scope='module')
def table():
    from srgan_amd import image_summaries
    return image_summaries.INFERNO


def guarded(count):
    return torch.full((count + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')


def unguard(buffer, shape):
    host = buffer.cpu().numpy()
    count = int(np.prod(shape))
    assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + count:]).all(), 'a write outside the output'
    return host[GUARD:GUARD + count].reshape(shape)


# ---- the grid kernel --------------------------------------------------------------------------------------------------------
def device_grid(lib, images, nrow, padding, pad_value, normalize, low, high):
    n, channels, height, width = images.shape
    shape = R.grid_shape(n, height, width, nrow, padding)
    buffer = guarded(int(np.prod(shape)))
    source = torch.from_numpy(images).cuda()
    lib.check(lib.library().srgan_image_grid(source.data_ptr(), n, channels, height, width, nrow, padding, pad_value,
                                             int(normalize), low, high, buffer.data_ptr() + 4 * GUARD, lib.stream_handle()),
              'srgan_image_grid')
    return unguard(buffer, shape)


@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('height, width', [(5, 7), (33, 17)])
def test_the_grid_kernel_is_bit_for_bit_the_restatement(lib, height, width, normalize):
    generator = np.random.RandomState(height * 100 + width)
    cases = 0
    for n in (1, 2, 5, 9):
        for nrow in (3, 5):
            for channels in (1, 3):
                for padding in (0, 2):
                    images = generator.uniform(-1.5, 1.5, size=(n, channels, height, width)).astype(np.float32)   # outside [-1, 1]
                    got = device_grid(lib, images, nrow, padding, 0.25, normalize, -1.0, 1.0)
                    expected = R.make_grid(images, nrow, padding, normalize, (-1.0, 1.0), 0.25)
                    assert got.shape == expected.shape
                    assert np.array_equal(got.view(np.uint32), expected.view(np.uint32)), (n, nrow, channels, padding)
                    cases += 1
    assert cases == 32


@pytest.mark.parametrize('low, high', [(0.0, 1.0), (0.0, 255.0)])
def test_the_grid_kernel_over_the_other_ranges(lib, low, high):
    generator = np.random.RandomState(3)
    images = generator.uniform(low - 0.3 * (high - low), high + 0.3 * (high - low), size=(5, 3, 33, 17)).astype(np.float32)
    got = device_grid(lib, images, 3, 2, 0.0, True, low, high)
    assert np.array_equal(got.view(np.uint32), R.make_grid(images, 3, 2, True, (low, high), 0.0).view(np.uint32))


def test_make_grid_takes_lists_single_images_and_vars(lib):
    from srgan_amd import image_summaries, functional as F
    generator = np.random.RandomState(4)
    images = generator.uniform(0, 1, size=(4, 3, 6, 5)).astype(np.float32)
    device = torch.from_numpy(images).cuda()
    expected = R.make_grid(images, 8, 2, False, None, 0.0)
    assert np.array_equal(image_summaries.make_grid(device).cpu().numpy(), expected)
    assert np.array_equal(image_summaries.make_grid([image for image in device]).cpu().numpy(), expected)
    assert np.array_equal(image_summaries.make_grid(F.constant(device)).cpu().numpy(), expected)
    assert np.array_equal(image_summaries.make_grid(device[0]).cpu().numpy(), images[0])
    plane = image_summaries.make_grid(device[0, 0], normalize=True, range=(0.25, 0.75)).cpu().numpy()
    assert np.array_equal(plane, R.make_grid(images[:1, :1], normalize=True, value_range=(0.25, 0.75)))
    with pytest.raises(lib.HipLibraryError):
        image_summaries.make_grid(torch.from_numpy(images))                        # a host tensor: there is no CPU fallback


# ---- the heatmap kernel -----------------------------------------------------------------------------------------------------
def device_heatmaps(lib, table, labels, predicted, size, front_slot=False):
    """The raw entry point into a guarded, NaN-filled buffer; ``front_slot``: every example's tiles start one tile into a row
    of ``M + 2`` tiles, as ``map_comparison_image`` asks.  Returns (tiles [B, M + 1, 3, P, P], ranges, the front slots)."""
    batch, heads = predicted.shape[:2]
    tile = 3 * size * size
    slots = heads + 1 + int(front_slot)
    buffer, ranges = guarded(batch * slots * tile), guarded(batch * heads * 2)
    device_labels, device_predicted, lut = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
                                            for a in (labels, predicted, table))
    first = buffer.data_ptr() + 4 * (GUARD + int(front_slot) * tile)
    lib.check(lib.library().srgan_density_heatmaps(device_labels.data_ptr(), device_predicted.data_ptr(), batch, heads,
                                                   labels.shape[1], labels.shape[2], size, lut.data_ptr(), table.shape[0], first,
                                                   slots * tile, ranges.data_ptr() + 4 * GUARD, lib.stream_handle()),
              'srgan_density_heatmaps')
    rows = unguard(buffer, (batch, slots, 3, size, size))
    return rows[:, int(front_slot):], unguard(ranges, (batch, heads, 2)), rows[:, :int(front_slot)]


def dyadic_maps(generator, batch, heads, size):
    """k / 64 in [0, 4] with 0 and 4 planted in every label: every pair's range is (0, 4) and every division is exact."""
    labels = generator.randint(0, 257, size=(batch, size, size)).astype(np.float32) / 64
    predicted = generator.randint(0, 257, size=(batch, heads, size, size)).astype(np.float32) / 64
    labels[:, 0, 1], labels[:, size - 1, size - 2] = 0.0, 4.0
    return labels, predicted


@pytest.mark.parametrize('size', [8, 31, 70])          # 70 x 70: more than one pass of a 1024-thread reduction
def test_dyadic_maps_give_exactly_the_restated_entries(lib, table, size):
    labels, predicted = dyadic_maps(np.random.RandomState(size), 2, 3, size)
    tiles, ranges, _ = device_heatmaps(lib, table, labels, predicted, size)
    expected_tiles, expected_ranges, entries, _ = R.density_heatmaps(labels, predicted, size, table)
    assert np.array_equal(ranges, expected_ranges) and (ranges == np.array([0.0, 4.0], dtype=np.float32)).all()
    assert np.array_equal(R.entries_from_colours(tiles, table), entries)
    assert np.array_equal(tiles, expected_tiles)
    assert entries.min() == 0 and entries.max() == 255


def test_ranges_are_per_pair(lib, table):
    generator = np.random.RandomState(9)
    labels = generator.uniform(1.0, 2.0, size=(2, 31, 31)).astype(np.float32)
    predicted = generator.uniform(0.0, 3.0, size=(2, 3, 31, 31)).astype(np.float32) * np.array([1, 2, 0.5], dtype=np.float32)[None, :, None, None]
    predicted[1, 2] = 1.5                                                           # inside the label's range: the label sets it
    _, ranges, _ = device_heatmaps(lib, table, labels, predicted, 31)
    _, expected, _, _ = R.density_heatmaps(labels, predicted, 31, table)
    assert np.array_equal(ranges, expected)
    assert ranges[1, 2].tolist() == [labels[1].min(), labels[1].max()]


def test_a_constant_pair_gives_entry_zero_everywhere(lib, table):
    labels = np.full((1, 31, 31), 0.75, dtype=np.float32)
    tiles, ranges, _ = device_heatmaps(lib, table, labels, labels[:, None].copy(), 31)
    assert (ranges == np.float32(0.75)).all()
    assert (R.entries_from_colours(tiles, table) == 0).all()


def test_random_maps_under_the_one_entry_rule(lib, table):
    generator = np.random.RandomState(21)
    labels = generator.uniform(0.05, 3.0, size=(2, 31, 31)).astype(np.float32)
    predicted = generator.uniform(-0.5, 4.0, size=(2, 3, 31, 31)).astype(np.float32)
    tiles, ranges, _ = device_heatmaps(lib, table, labels, predicted, 31)
    _, expected_ranges, entries, scaled = R.density_heatmaps(labels, predicted, 31, table)
    assert np.array_equal(ranges, expected_ranges)
    got = R.entries_from_colours(tiles, table)
    print(f'[image summaries] random maps: {int((got != entries).sum())} of {got.size} entries differ from the restatement')
    R.check_entries(got, entries, scaled, 'random maps')


def test_resized_maps_against_torch_interpolate(lib, table):
    generator = np.random.RandomState(6)
    labels = generator.uniform(0.0, 2.0, size=(2, 6, 6)).astype(np.float32)
    predicted = generator.uniform(0.0, 3.0, size=(2, 3, 6, 6)).astype(np.float32)
    tiles, ranges, _ = device_heatmaps(lib, table, labels, predicted, 12)
    _, expected_ranges, entries, _ = R.density_heatmaps(labels, predicted, 12, table, resize=R.torch_resize)
    assert np.array_equal(ranges, expected_ranges)                                  # the ranges come from the maps before the resize
    got = R.entries_from_colours(tiles, table)
    print(f'[image summaries] 6 x 6 -> 12 x 12: {int((got != entries).sum())} of {got.size} entries differ from the restatement')
    assert np.abs(got - entries).max() <= 1


def test_the_tile_stride_leaves_a_front_slot_untouched(lib, table):
    labels, predicted = dyadic_maps(np.random.RandomState(2), 3, 2, 8)
    dense, _, _ = device_heatmaps(lib, table, labels, predicted, 8)
    strided, _, front = device_heatmaps(lib, table, labels, predicted, 8, front_slot=True)
    assert front.shape == (3, 1, 3, 8, 8) and np.isnan(front).all()
    assert np.array_equal(strided, dense)


def test_the_reference_heatmaps_through_density_heatmaps(lib, table):
    from srgan_amd import image_summaries
    g17 = np.load(os.path.join(HERE, 'golden', 'g17_image_summaries.npz'))
    size = int(g17['size'])
    names = ('random', 'constant', 'heads')
    labels = np.stack([g17[f'{name}/label'] for name in names])
    predicted = np.stack([g17[f'{name}/predicted'] for name in names])[:, None]
    tiles, ranges = image_summaries.density_heatmaps(torch.from_numpy(labels).cuda(), torch.from_numpy(predicted).cuda(), size)
    assert tuple(tiles.shape) == (3, 2, 3, size, size) and tuple(ranges.shape) == (3, 1, 2)
    _, expected_ranges, _, scaled = R.density_heatmaps(labels, predicted, size, table)
    assert np.array_equal(ranges.cpu().numpy(), expected_ranges)
    got = R.entries_from_colours(tiles.cpu().numpy(), table)
    recorded = np.stack([R.entries_from_colours(g17[f'{name}/heatmaps'], table) for name in names])
    R.check_entries(got, recorded, scaled, 'g17')


def test_the_map_comparison_image_is_the_host_composition(lib, table):
    from srgan_amd import image_summaries
    generator = np.random.RandomState(12)
    size, heads, count = 16, 3, 3
    images = generator.uniform(-1, 1, size=(4, 3, size, size)).astype(np.float32)
    images[0, 0, 0, :2] = (-1.0, 1.0)
    maps, predicted = dyadic_maps(generator, 4, heads, size)
    got = image_summaries.map_comparison_image(torch.from_numpy(images).cuda(), torch.from_numpy(maps).cuda(),
                                               torch.from_numpy(predicted).cuda()).cpu().numpy()
    assert got.shape == (3, 56, 92)
    heatmaps, _, _, _ = R.density_heatmaps(maps[:count], predicted[:count], size, table)
    rows = np.concatenate([((images[:count] + np.float32(1)) / np.float32(2))[:, None], heatmaps], axis=1)
    expected = R.make_grid(rows.reshape(count * (2 + heads), 3, size, size), 2 + heads, 2, True, (0.0, 1.0), 0.0)
    assert np.array_equal(got.view(np.uint32), expected.view(np.uint32))


# ---- the experiments --------------------------------------------------------------------------------------------------------
SEED = 2 ** 33 + 5


def age_experiment(batch, **overrides):
    """AgeExperiment with the tiny DCGAN (32 x 32, conv_dim 8) on its synthetic loaders, summary period 1."""
    from srgan_amd.age.srgan import AgeExperiment
    from srgan_amd.age.models import Generator, Discriminator
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all

    class TinyAge(AgeExperiment):
        image_size = 32

        def model_setup(self):
            self.G, self.D, self.DNN = Generator(image_size=32, conv_dim=8), Discriminator(32, 8), Discriminator(32, 8)

    settings = Settings()
    for key, value in dict(batch_size=batch, mean_offset=0.5, steps_to_run=10 ** 9, summary_step_period=1,
                           device_random_seed=SEED, **overrides).items():
        setattr(settings, key, value)
    experiment = TinyAge(settings)
    seed_all(0)
    experiment.dataset_setup()
    experiment.model_setup()
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    finish_setup(experiment)
    return experiment


def summary_step(experiment, step):
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.step = step
    experiment.end_of_step(step, experiment.gan_summary_writer, datetime.datetime.now())
    torch.cuda.synchronize()


@pytest.mark.parametrize('batch, shape', [(9, (3, 104, 104)), (4, (3, 70, 104))])
def test_age_writes_its_three_grids(lib, batch, shape):
    from srgan_amd import image_summaries, functional as F
    from srgan_amd.tape import no_grad
    from srgan_amd.utility import to_image_range
    experiment = age_experiment(batch, image_summaries=True)
    summary_step(experiment, 7)
    images = experiment.gan_summary_writer.images
    assert sorted(images) == ['Fake/Offset', 'Fake/Standard', 'Real'] and experiment.dnn_summary_writer.images == {}
    for tag, (step, image) in images.items():
        assert step == 7 and image.shape == shape and image.dtype == np.float32, tag
        assert np.isfinite(image).all() and image.min() >= 0.0 and image.max() <= 1.0, tag
    # Real: the first batch of the train loader, in order
    first = next(iter(experiment.train_dataset_loader))[0]
    expected = image_summaries.make_grid(to_image_range(first[:9]), nrow=3, normalize=True, range=(0, 255)).cpu().numpy()
    assert np.array_equal(images['Real'][1], expected)
    assert np.abs(images['Real'][1][:, 2:34, 2:34] - (first[0].cpu().numpy() + 1) / 2).max() <= 1e-6
    # Fake/Standard: G on draw 8 of the state {seed, step}, recomputed here
    words = np.array([SEED & 0xffffffff, SEED >> 32, 7, 0], dtype=np.uint32)
    state = torch.from_numpy(words.view(np.int32)).cuda()
    experiment.eval_mode()
    with no_grad():
        fake = experiment.G(F.random_fill((min(9, batch), experiment.G.input_size), 1, 0.0, 8, state)).data
    experiment.train_mode()
    recomputed = image_summaries.make_grid(to_image_range(fake), nrow=3, normalize=True, range=(0, 255)).cpu().numpy()
    assert np.array_equal(images['Fake/Standard'][1], recomputed)
    assert not np.array_equal(images['Fake/Offset'][1], images['Fake/Standard'][1])         # mean_offset = 0.5
    # the next summary step draws again
    summary_step(experiment, 8)
    assert experiment.gan_summary_writer.images['Fake/Standard'][0] == 8
    assert not np.array_equal(experiment.gan_summary_writer.images['Fake/Standard'][1], recomputed)
    assert np.array_equal(experiment.gan_summary_writer.images['Real'][1], expected)


def test_the_pictures_are_off_by_default(lib):
    experiment = age_experiment(4)
    assert not hasattr(experiment.settings, 'image_summaries') and not experiment.image_summaries_on()
    summary_step(experiment, 0)
    assert experiment.gan_summary_writer.images == {} and experiment.dnn_summary_writer.images == {}
    assert '1 Validation Error/MAE' in experiment.gan_summary_writer.scalars                # the scalars still are written


def train_three_iterations(**overrides):
    from srgan_amd.utility import seed_all
    experiment = age_experiment(4, **overrides)
    seed_all(5)                                                                             # the host streams of the draws
    labeled = experiment.infinite_iter(experiment.train_dataset_loader)
    unlabeled = experiment.infinite_iter(experiment.unlabeled_dataset_loader)
    for step in range(3):
        examples, labels = next(labeled)
        experiment.training_iteration(examples, labels, next(unlabeled)[0], step)
        experiment.end_of_step(step, experiment.gan_summary_writer, datetime.datetime.now())
    torch.cuda.synchronize()
    return experiment


def test_the_pictures_do_not_perturb_training(lib):
    """Three iterations with host draws, a summary step after each: the arenas carry the same bits with the pictures on and
    off -- nothing of theirs draws from a host stream or advances a loader."""
    without, with_pictures = train_three_iterations(), train_three_iterations(image_summaries=True)
    assert without.gan_summary_writer.images == {} and len(with_pictures.gan_summary_writer.images) == 3
    assert with_pictures.gan_summary_writer.images['Fake/Standard'][0] == 2
    for name in ('D', 'G', 'DNN'):
        a, b = getattr(without, name)._srgan_arena.data, getattr(with_pictures, name)._srgan_arena.data
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert without.gan_summary_writer.scalars == with_pictures.gan_summary_writer.scalars


def crowd_items(seed, count=3, size=64):
    generator = np.random.RandomState(seed)
    return [(generator.uniform(-1, 1, size=(3, size, size)).astype(np.float32),
             (generator.uniform(size=(size, size)) < 0.002).astype(np.float32),
             generator.uniform(0, 1, size=(size, size)).astype(np.float32)) for _ in range(count)]


def test_crowd_writes_map_comparisons_and_samples(lib):
    from srgan_amd.crowd.srgan import CrowdExperiment
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all
    size = 64
    settings = Settings()
    for key, value in dict(batch_size=4, image_patch_size=size, mean_offset=0.5, steps_to_run=10 ** 9, image_summaries=True).items():
        setattr(settings, key, value)
    experiment = CrowdExperiment(settings)                         # KnnDenseNetCat(image_size=64) twice and the DCGAN generator
    seed_all(0)
    experiment.model_setup()
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    finish_setup(experiment)
    experiment.train_dataset, experiment.validation_dataset = crowd_items(1), crowd_items(2)
    summary_step(experiment, 3)
    gan, dnn = experiment.gan_summary_writer.images, experiment.dnn_summary_writer.images
    assert sorted(gan) == ['Fake/Offset', 'Fake/Standard', 'Real', 'Validation'] and sorted(dnn) == ['Real', 'Validation']
    for images in (gan, dnn):
        for tag in ('Real', 'Validation'):
            step, image = images[tag]
            assert step == 3 and image.shape == (3, 200, 332), tag                          # 3 rows of 2 + 3 tiles of 64 + 2
            assert np.isfinite(image).all() and image.min() >= 0.0 and image.max() <= 1.0, tag
    for tag in ('Fake/Standard', 'Fake/Offset'):
        assert gan[tag][1].shape == (3, 134, 200) and np.isfinite(gan[tag][1]).all()        # 4 samples, three wide
        assert gan[tag][1].min() >= 0.0 and gan[tag][1].max() <= 1.0
    assert not np.array_equal(gan['Fake/Standard'][1], gan['Fake/Offset'][1])
    # the photograph of each row, and that Validation shows the validation items (the reference shows the train items twice)
    for tag, items in (('Real', experiment.train_dataset), ('Validation', experiment.validation_dataset)):
        for row, item in enumerate(items):
            top = 2 + row * 66
            for images in (gan, dnn):
                assert np.array_equal(images[tag][1][:, top:top + 64, 2:66], (item[0] + np.float32(1)) / np.float32(2)), (tag, row)
    # the map label's tile is the same on both writers only when the pair (label, first head) has the same range: the
    # photograph's is always; D and the DNN start from different weights, so their predicted tiles differ
    assert not np.array_equal(gan['Real'][1], dnn['Real'][1])
    assert '1 Validation Error/MAE' in experiment.gan_summary_writer.scalars
