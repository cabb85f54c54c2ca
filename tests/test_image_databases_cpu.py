"""The resident image datasets of the age and driving applications on the CPU (no GPU, no launch): the readers of the
reference's on-disk layouts reproduce its three-way split and its items bit for bit (tests/golden/g15_image_databases.npz,
recorded from the unmodified reference by tests/golden/make_image_database_goldens.py), the loader's epoch schedule, its
data-parallel slices, and the ABI of the one entry point behind it."""
import math
import re

import numpy as np
import pytest
import torch

from image_database_fixture import PARTS, golden, settings_for, write_age_database, write_driving_database
from test_abi_cpu import header_code, header_prototypes


@pytest.fixture(scope='module')
def fixture():
    return golden()


@pytest.fixture(scope='module')
def databases(fixture, tmp_path_factory):
    root = tmp_path_factory.mktemp('image_databases')
    return {'driving': write_driving_database(fixture, root / 'driving'), 'age': write_age_database(fixture, root / 'age')}


def read(application, directory, settings):
    import srgan_amd  # noqa: F401
    if application == 'driving':
        from srgan_amd.driving.data import driving_datasets
        return driving_datasets(directory, settings)
    from srgan_amd.age.data import age_datasets
    return age_datasets(directory, settings)


@pytest.mark.parametrize('tag', ['A', 'B'])
@pytest.mark.parametrize('application', ['driving', 'age'])
def test_the_readers_reproduce_the_reference_split_and_items(fixture, databases, application, tag):
    settings = settings_for(fixture, tag)
    numpy_state, torch_state = np.random.get_state(), torch.get_rng_state()
    datasets = read(application, databases[application], settings)
    for part, dataset in zip(PARTS, datasets):
        prefix = f'{application}/{tag}/{part}'
        assert [str(name) for name in dataset.names] == [str(name) for name in fixture[prefix + '/names']], prefix
        assert dataset.labels.dtype == np.float32 and np.array_equal(dataset.labels, fixture[prefix + '/labels']), prefix
        assert len(dataset) == len(fixture[prefix + '/items']) >= settings.batch_size
        assert dataset.images.dtype == (np.float32 if application == 'driving' else np.uint8)
        for index in range(len(dataset)):
            image, label = dataset[index]
            assert image.dtype == torch.float32 and label.dtype == torch.float32 and label.shape == ()
            assert np.array_equal(image.numpy(), fixture[prefix + '/items'][index]), (prefix, index)       # bit for bit
            assert float(label) == float(fixture[prefix + '/item_labels'][index])
    # building the datasets leaves the process-wide generators alone (upstream seeds them)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), numpy_state))
    assert torch.equal(torch.get_rng_state(), torch_state)


def test_setting_b_runs_the_repeat_branch(fixture):
    """The labeled slice (5) is shorter than the batch (8): each element twice, in place -- a a b b, not a b a b."""
    names = [str(name) for name in fixture['driving/B/train/names']]
    assert len(names) == 10 and names[0::2] == names[1::2] and len(set(names)) == 5


def test_a_float_store_keeps_the_fractions_and_an_integer_store_is_uint8():
    import srgan_amd  # noqa: F401
    from srgan_amd.data import ResidentImageDataset
    frames = np.arange(2 * 3 * 2 * 2, dtype=np.float64).reshape(2, 3, 2, 2) + 0.375
    dataset = ResidentImageDataset(list(frames), [1, 2], names=['a', 'b'])
    assert dataset.images.dtype == np.float32 and np.array_equal(dataset.images, frames.astype(np.float32))
    assert list(dataset.names) == ['a', 'b'] and len(dataset) == 2
    expected = (torch.tensor(frames[1].astype(np.float32)) / 127.5) - 1
    assert torch.equal(dataset[1][0], expected)
    assert ResidentImageDataset(frames.astype(np.int64), [1, 2]).images.dtype == np.uint8


class RecordingLoader:
    """A ResidentImageLoader whose upload and launch are replaced by records of what they were asked for."""

    def __new__(cls, *args, **kwargs):
        from srgan_amd.data import ResidentImageLoader

        class Recording(ResidentImageLoader):
            def to_device(self, order):
                self.uploads.append(order.clone())
                return order

            def gather(self, order, first, count):
                self.launches.append((first, count))
                return order[first:first + count].clone(), None

        loader = Recording(*args, **kwargs)
        loader.uploads, loader.launches = [], []
        return loader


class StubDataset:
    frame_shape = (3, 8, 8)

    def __init__(self, count):
        self.count = count

    def __len__(self):
        return self.count


class World:
    def __init__(self, world_size, rank):
        self.world_size, self.rank = world_size, rank

    def local_batch(self, global_batch):
        if global_batch % self.world_size:
            raise ValueError(f'global batch {global_batch} is not divisible by {self.world_size} ranks')
        return global_batch // self.world_size


def test_an_epoch_is_a_fresh_permutation_cut_into_whole_batches():
    import srgan_amd  # noqa: F401
    numpy_state, torch_state = np.random.get_state(), torch.get_rng_state()
    loader = RecordingLoader(StubDataset(23), 4, seed=7)
    first_epoch = [batch for batch, _ in loader]
    assert len(first_epoch) == len(loader) == 23 // 4 and loader.launches == [(4 * i, 4) for i in range(5)]
    assert len(loader.uploads) == 1 and loader.uploads[0].dtype == torch.int32            # one upload per epoch
    assert sorted(loader.uploads[0].tolist()) == list(range(23))
    seen = torch.cat(first_epoch).tolist()
    assert len(seen) == 20 and len(set(seen)) == 20                                        # no index twice within it
    second_epoch = [batch for batch, _ in loader]
    assert len(loader.uploads) == 2 and loader.uploads[0].tolist() != loader.uploads[1].tolist()
    assert sorted(loader.uploads[1].tolist()) == list(range(23)) and len(second_epoch) == 5
    # the same seed gives the same epochs; another seed another order
    twin = RecordingLoader(StubDataset(23), 4, seed=7)
    assert [batch.tolist() for batch, _ in twin] == [batch.tolist() for batch in first_epoch]
    assert [batch.tolist() for batch, _ in twin] == [batch.tolist() for batch in second_epoch]
    other = RecordingLoader(StubDataset(23), 4, seed=8)
    assert [batch.tolist() for batch, _ in other] != [batch.tolist() for batch in first_epoch]
    # the permutations come from a private generator
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), numpy_state))
    assert torch.equal(torch.get_rng_state(), torch_state)


def test_an_unshuffled_loader_walks_the_stored_order():
    loader = RecordingLoader(StubDataset(10), 4, shuffle=False)
    assert [batch.tolist() for batch, _ in loader] == [[0, 1, 2, 3], [4, 5, 6, 7]]


@pytest.mark.parametrize('world', [2, 4])
def test_the_ranks_slices_tile_the_global_batch_in_rank_order(world):
    single = [batch.tolist() for batch, _ in RecordingLoader(StubDataset(23), 8, seed=5)]
    ranks = [RecordingLoader(StubDataset(23), 8, seed=5, dp=World(world, rank)) for rank in range(world)]
    per_rank = [[batch.tolist() for batch, _ in loader] for loader in ranks]
    local = 8 // world
    for rank, loader in enumerate(ranks):
        assert loader.launches == [(8 * i + rank * local, local) for i in range(23 // 8)]
    for step, whole in enumerate(single):
        assert sum((per_rank[rank][step] for rank in range(world)), []) == whole


def test_a_batch_that_does_not_divide_over_the_ranks_raises():
    with pytest.raises(ValueError, match='not divisible'):
        RecordingLoader(StubDataset(23), 6, dp=World(4, 0))


def test_a_dataset_smaller_than_one_batch_cannot_be_iterated():
    with pytest.raises(ValueError, match='do not fill one batch'):
        next(iter(RecordingLoader(StubDataset(3), 4)))


@pytest.mark.parametrize('count, batch', [(23, 4), (8, 4), (3, 4)])
def test_in_order_keeps_the_short_last_batch(count, batch):
    loader = RecordingLoader(StubDataset(count), batch, seed=1, dp=World(2, 1))            # not sharded
    batches = [indexes.tolist() for indexes, _ in loader.in_order()]
    assert len(batches) == math.ceil(count / batch)
    assert sum(batches, []) == list(range(count)) and all(len(b) == batch for b in batches[:-1])
    assert [indexes.tolist() for indexes, _ in loader.in_order()] == batches and len(loader.uploads) == 1


def test_image_size_defaults_to_the_stored_size():
    assert RecordingLoader(StubDataset(8), 4).image_size == (8, 8)
    assert RecordingLoader(StubDataset(8), 4, image_size=16).image_size == (16, 16)
    assert RecordingLoader(StubDataset(8), 4, image_size=(4, 12)).image_size == (4, 12)


def test_the_experiments_choose_the_database_by_environment_variable(fixture, databases, monkeypatch):
    """dataset_setup with the variable set builds the three loaders and the two evaluation datasets from the reader (no
    device is touched before the first batch); without it the loaders stay synthetic (those need a device: not built here)."""
    import srgan_amd  # noqa: F401
    from srgan_amd.data import ResidentImageLoader
    from srgan_amd.driving.srgan import DrivingExperiment
    from srgan_amd.age.srgan import AgeExperiment
    from srgan_amd.settings import Settings
    for experiment_class, application, size in ((DrivingExperiment, 'driving', (4, 12)), (AgeExperiment, 'age', 16)):
        monkeypatch.setenv(experiment_class.DATABASE_ENV, databases[application])
        settings = Settings()
        for name, value in vars(settings_for(fixture, 'A')).items():
            setattr(settings, name, value)
        experiment = experiment_class(settings)
        experiment.image_size = size
        experiment.dataset_setup()
        loaders = (experiment.train_dataset_loader, experiment.unlabeled_dataset_loader, experiment.validation_dataset_loader)
        assert all(isinstance(loader, ResidentImageLoader) for loader in loaders)
        assert [len(loader.dataset) for loader in loaders] == [5, 6, 4]
        assert all(loader.image_size == ((size, size) if isinstance(size, int) else size) for loader in loaders)
        assert experiment.train_dataset is loaders[0].dataset and experiment.validation_dataset is loaders[2].dataset
        assert [str(n) for n in experiment.validation_dataset.names] == [str(n) for n in fixture[f'{application}/A/validation/names']]
        assert loaders[0].shuffle and loaders[1].shuffle and not loaders[2].shuffle


def test_the_entry_point_is_declared_bound_and_advertised():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    prototypes = header_prototypes()
    c_return, c_arguments = prototypes['srgan_image_batch_gather']
    argtypes, restype = _lib.SIGNATURES['srgan_image_batch_gather']
    assert c_return == 'int' and len(c_arguments) == len(argtypes) == 15
    assert c_arguments[8] == 'int64_t' and c_arguments[1] == 'int' and c_arguments[0] == 'const void*'
    assert re.search(r'#define\s+SRGAN_FEATURE_IMAGE_BATCHES\s+0x40u', open(header_code.__globals__['HEADER']).read())
    assert _lib.capabilities().features & 0x40
    assert _lib.library().srgan_version() == 110                      # additive: the version stays
    assert getattr(_lib.library(), 'srgan_image_batch_gather') is not None


def test_argument_errors_are_reported_before_any_device_work():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    gather = _lib.library().srgan_image_batch_gather
    good = dict(store=16, dtype=0, count=5, C=3, h=8, w=8, labels=16, order=16, first=0, B=4, H=8, W=8, out=16, out_labels=16)

    def call(**changes):
        a = dict(good, **changes)
        return gather(a['store'], a['dtype'], a['count'], a['C'], a['h'], a['w'], a['labels'], a['order'], a['first'], a['B'],
                      a['H'], a['W'], a['out'], a['out_labels'], None)
    for changes in (dict(store=None), dict(B=0), dict(dtype=7), dict(order=None), dict(out=None), dict(first=-1),
                    dict(count=0), dict(labels=None), dict(out_labels=None), dict(H=0),
                    dict(B=2 ** 20, H=2 ** 10, W=2 ** 10), dict(C=2 ** 11, h=2 ** 10, w=2 ** 10)):
        assert call(**changes) == _lib.EINVAL, changes
        assert b'srgan_image_batch_gather' in _lib.library().srgan_last_error()
