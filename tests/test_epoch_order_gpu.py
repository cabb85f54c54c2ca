"""The resident image loaders' epoch order drawn on the device: ``srgan_epoch_order`` / ``srgan_argsort_u64`` /
``srgan_epoch_batch_indices`` bit for bit against epoch_order_reference.py, their argument errors, the chain replayed from a
HIP graph, ``ResidentImageLoader(draws='device')``, and tiny age / driving / crowd experiments with ``image_batch_draws`` and
``capture_loaders``."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from epoch_order_reference import LABELED_DRAW, UNLABELED_DRAW, batch_table, epoch_order, stable_argsort
from image_database_fixture import write_age_database, write_driving_database

pytestmark = pytest.mark.gpu

SEEDS = (0x1234, 2 ** 40 + 17)                       # the second one has a high half
EINVAL, ERANGE = -1, -3


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def device_state(seed, iteration):
    words = np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff, iteration & 0xffffffff, 0], dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)).cuda()


def minus_ones(count):
    return torch.full((count,), -1, dtype=torch.int32, device='cuda')


def build_order(lib, n, batches, conditional, draw, state, order=None, guard=8):
    """One ``srgan_epoch_order`` call into a -1-filled buffer with ``guard`` extra slots; returns the whole buffer."""
    order = minus_ones(n + guard) if order is None else order
    lib.check(lib.library().srgan_epoch_order(n, batches, conditional, draw, state.data_ptr(), order.data_ptr(),
                                              lib.stream_handle()), 'srgan_epoch_order')
    torch.cuda.synchronize()
    return order


# ---- the kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 255, 256, 257, 513, 1000, 4097, 65537])
def test_the_order_equals_the_reference(lib, n):
    batches = max(n // 4, 1)
    for seed, draw, epoch in ((SEEDS[0], LABELED_DRAW, 0), (SEEDS[1], UNLABELED_DRAW, 3)):
        step = epoch * batches + (1 if batches > 1 else 0)           # (unconditional: any step of the epoch rebuilds)
        order = build_order(lib, n, batches, 0, draw, device_state(seed, step)).cpu().numpy()
        assert np.array_equal(order[:n], epoch_order(seed, epoch, draw, n)), (seed, epoch)
        assert np.all(order[n:] == -1)
        if n == 1000:                                                # two calls give the same bits
            again = build_order(lib, n, batches, 0, draw, device_state(seed, step)).cpu().numpy()
            assert np.array_equal(order, again)


def test_the_conditional_rebuild_happens_at_epoch_starts_only(lib):
    n, batches, seed = 300, 3, SEEDS[1]
    for step in range(8):
        order = build_order(lib, n, batches, 1, LABELED_DRAW, device_state(seed, step)).cpu().numpy()
        if step % batches:
            assert np.all(order == -1), step
        else:
            assert np.array_equal(order[:n], epoch_order(seed, step // batches, LABELED_DRAW, n)), step
            assert np.all(order[n:] == -1)
    # an order in place survives the steps in the middle of its epoch
    state = device_state(seed, 3)
    order = build_order(lib, n, batches, 1, LABELED_DRAW, state)
    kept = order.clone()
    for step in (4, 5):
        build_order(lib, n, batches, 1, LABELED_DRAW, device_state(seed, step), order=order)
        assert torch.equal(order, kept)
    build_order(lib, n, batches, 1, LABELED_DRAW, device_state(seed, 6), order=order)
    assert not torch.equal(order, kept)


def argsort(lib, keys, guard=8):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    device_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    order = minus_ones(len(keys) + guard)
    lib.check(lib.library().srgan_argsort_u64(device_keys.data_ptr(), len(keys), order.data_ptr(), lib.stream_handle()),
              'srgan_argsort_u64')
    torch.cuda.synchronize()
    order = order.cpu().numpy()
    assert np.all(order[len(keys):] == -1)
    return order[:len(keys)]


def test_the_argsort_breaks_ties_by_index(lib):
    generator = np.random.RandomState(3)

    def random_keys(count):
        return (generator.randint(0, 2 ** 32, size=count).astype(np.uint64) << np.uint64(32)) | \
            generator.randint(0, 2 ** 32, size=count).astype(np.uint64)

    cases = {'all equal': np.full(513, 2 ** 63 + 5, dtype=np.uint64),
             'all equal, the largest key': np.full(513, 2 ** 64 - 1, dtype=np.uint64),
             'all zero': np.zeros(257, dtype=np.uint64)}
    pairs = random_keys(4500)                     # LDS tiles of 2048 keys, workgroups of 256 frames
    for a, b in ((2047, 2048), (255, 256), (100, 3000), (4095, 4096), (2048, 4499), (0, 4200), (2300, 2301)):
        pairs[b] = pairs[a]
    pairs[1000:1010] = pairs[3500]                # a run of equal keys in front of their twin's tile
    cases['pairwise equal across tiles'] = pairs
    cases['every key twice'] = np.concatenate([pairs[:2100], pairs[:2100]])
    high = generator.randint(0, 2 ** 32, size=700).astype(np.uint64) << np.uint64(32) | np.uint64(0xdeadbeef)
    cases['high words only'] = high
    cases['low words only'] = np.uint64(7 << 32) | generator.randint(0, 2 ** 32, size=700).astype(np.uint64)
    cases['bit 63 and bit 31'] = np.array([2 ** 63, 2 ** 31, 2 ** 63 - 1, 2 ** 32, 2 ** 31 - 1, 0, 2 ** 64 - 1, 2 ** 63],
                                          dtype=np.uint64)
    for name, keys in cases.items():
        assert np.array_equal(argsort(lib, keys), stable_argsort(keys)), name


WINDOWS = [(0, 6), (1, 4), (5, 1), (3, 3), (0, 1), (6, 0), (2, 0)]


def test_the_batch_indices(lib):
    n, batch, batches, seed = 23, 6, 3, SEEDS[1]
    for step in range(7):                                            # two epochs and the first step of a third
        epoch = step // batches
        order = torch.from_numpy(epoch_order(seed, epoch, LABELED_DRAW, n).astype(np.int32)).cuda()
        for first_row, rows in WINDOWS:
            table = minus_ones(rows + 4)
            lib.check(lib.library().srgan_epoch_batch_indices(order.data_ptr(), n, batch, batches, first_row, rows,
                                                              device_state(seed, step).data_ptr(), table.data_ptr(),
                                                              lib.stream_handle()), 'srgan_epoch_batch_indices')
            torch.cuda.synchronize()
            table = table.cpu().tolist()
            assert table[:rows] == batch_table(seed, step, LABELED_DRAW, n, batch, first_row, rows), (step, first_row, rows)
            assert table[rows:] == [-1] * 4
    # more rows than one workgroup
    n, batch = 2000, 700
    order = torch.from_numpy(epoch_order(seed, 1, UNLABELED_DRAW, n).astype(np.int32)).cuda()
    table = minus_ones(600)
    lib.check(lib.library().srgan_epoch_batch_indices(order.data_ptr(), n, batch, 2, 50, 600, device_state(seed, 3).data_ptr(),
                                                      table.data_ptr(), lib.stream_handle()), 'srgan_epoch_batch_indices')
    torch.cuda.synchronize()
    assert table.cpu().tolist() == batch_table(seed, 3, UNLABELED_DRAW, n, batch, 50, 600)


def test_argument_errors_launch_nothing(lib):
    library, stream = lib.library(), lib.stream_handle()
    state = device_state(SEEDS[0], 0)
    order, table = minus_ones(64), minus_ones(16)
    keys = torch.zeros(64, dtype=torch.int64, device='cuda')
    big = 2 ** 20 + 1

    def epoch(n=10, batches=2, conditional=0, draw=LABELED_DRAW, state_=state.data_ptr(), order_=order.data_ptr()):
        return library.srgan_epoch_order(n, batches, conditional, draw, state_, order_, stream)

    def sort(keys_=keys.data_ptr(), n=10, order_=order.data_ptr()):
        return library.srgan_argsort_u64(keys_, n, order_, stream)

    def indices(order_=order.data_ptr(), n=10, batch=4, batches=2, first_row=0, rows=4, state_=state.data_ptr(),
                table_=table.data_ptr()):
        return library.srgan_epoch_batch_indices(order_, n, batch, batches, first_row, rows, state_, table_, stream)

    invalid = [epoch(state_=None), epoch(order_=None), epoch(n=0), epoch(n=-5), epoch(batches=0), epoch(batches=-1),
               epoch(draw=-1), epoch(conditional=2),
               sort(keys_=None), sort(order_=None), sort(n=0), sort(n=-1),
               indices(order_=None), indices(state_=None), indices(table_=None), indices(n=0), indices(batches=0),
               indices(batch=0), indices(batches=3), indices(batch=6), indices(rows=-1), indices(first_row=-1),
               indices(first_row=1, rows=4), indices(first_row=5, rows=0), indices(first_row=2 ** 31 - 1, rows=2 ** 31 - 1)]
    assert invalid == [EINVAL] * len(invalid)
    assert b'requirement' in library.srgan_last_error()
    too_large = [epoch(n=big), sort(n=big), indices(n=big)]
    assert too_large == [ERANGE] * 3
    assert epoch(n=big, batches=0) == EINVAL                          # an invalid argument is reported first
    torch.cuda.synchronize()
    assert bool((order == -1).all()) and bool((table == -1).all())
    assert indices(rows=0) == 0 and indices(first_row=4, rows=0) == 0  # an empty window succeeds
    torch.cuda.synchronize()
    assert bool((table == -1).all())
    with pytest.raises(lib.HipLibraryError) as error:
        lib.check(epoch(n=0), 'srgan_epoch_order')
    assert error.value.status == EINVAL


# ---- the chain in a HIP graph ---------------------------------------------------------------------------------------------
def frames_and_labels(count, seed=7, size=4):
    generator = np.random.RandomState(seed)
    return (generator.randint(0, 256, size=(count, 3, size, size)).astype(np.uint8),
            generator.uniform(10, 90, size=count).astype(np.float32))


class Chain:
    """Conditional rebuild, slice, gather, advance on raw entry points over one state and one order."""

    def __init__(self, lib, n, batch, seed, draw):
        self.lib, self.n, self.batch, self.batches, self.draw = lib, n, batch, n // batch, draw
        frames, labels = frames_and_labels(n)
        self.store, self.labels = torch.from_numpy(frames).cuda(), torch.from_numpy(labels).cuda()
        self.state, self.order = device_state(seed, 0), minus_ones(n)
        self.table = minus_ones(batch)
        self.images = torch.full((batch, 3, 4, 4), float('nan'), device='cuda')
        self.out_labels = torch.full((batch,), float('nan'), device='cuda')

    def gather(self, table, images, out_labels, stream):
        self.lib.check(self.lib.library().srgan_image_batch_gather(
            self.store.data_ptr(), 0, self.n, 3, 4, 4, self.labels.data_ptr(), table.data_ptr(), 0, self.batch, 4, 4,
            images.data_ptr(), out_labels.data_ptr(), stream), 'srgan_image_batch_gather')

    def enqueue(self):
        lib, library, stream = self.lib, self.lib.library(), self.lib.stream_handle()
        lib.check(library.srgan_epoch_order(self.n, self.batches, 1, self.draw, self.state.data_ptr(), self.order.data_ptr(),
                                            stream), 'srgan_epoch_order')
        lib.check(library.srgan_epoch_batch_indices(self.order.data_ptr(), self.n, self.batch, self.batches, 0, self.batch,
                                                    self.state.data_ptr(), self.table.data_ptr(), stream),
                  'srgan_epoch_batch_indices')
        self.gather(self.table, self.images, self.out_labels, stream)
        lib.check(library.srgan_random_advance(self.state.data_ptr(), stream), 'srgan_random_advance')

    def outputs(self):
        torch.cuda.synchronize()
        return self.table.clone(), self.images.clone(), self.out_labels.clone(), self.order.clone()


def test_the_chain_replays_from_a_captured_graph(lib):
    n, batch, seed = 10, 4, SEEDS[1]
    iterations = 2 * (n // batch) + 1
    eager = Chain(lib, n, batch, seed, UNLABELED_DRAW)
    expected = []
    for _ in range(iterations):
        eager.enqueue()
        expected.append(eager.outputs())
    chain = Chain(lib, n, batch, seed, UNLABELED_DRAW)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                                   # (the kernels were loaded by the eager chain)
    with torch.cuda.graph(graph):
        chain.enqueue()
    torch.cuda.synchronize()
    assert chain.state.cpu().tolist()[2] == 0 and bool((chain.order == -1).all())      # capturing ran nothing
    for step in range(iterations):
        chain.table.fill_(-1)
        chain.images.fill_(float('nan'))
        chain.out_labels.fill_(float('nan'))
        graph.replay()
        got = chain.outputs()
        for a, b in zip(got, expected[step]):
            assert torch.equal(a, b), step
        reference = batch_table(seed, step, UNLABELED_DRAW, n, batch)
        assert got[0].cpu().tolist() == reference
        assert got[3].cpu().tolist() == epoch_order(seed, step // (n // batch), UNLABELED_DRAW, n).tolist()
        images = torch.full_like(chain.images, float('nan'))
        labels = torch.full_like(chain.out_labels, float('nan'))
        chain.gather(torch.tensor(reference, dtype=torch.int32).cuda(), images, labels, lib.stream_handle())
        torch.cuda.synchronize()
        assert torch.equal(got[1], images) and torch.equal(got[2], labels)
    assert chain.state.cpu().tolist()[2] == iterations


# ---- the loader -----------------------------------------------------------------------------------------------------------
class Ranks:
    """What the loader asks of a data-parallel context."""

    def __init__(self, world_size, rank):
        self.world_size, self.rank = world_size, rank

    def local_batch(self, batch_size):
        assert batch_size % self.world_size == 0
        return batch_size // self.world_size


def device_loader(count=23, batch_size=4, draw_id=LABELED_DRAW, seed=SEEDS[1], **arguments):
    from srgan_amd.data import ResidentImageDataset, ResidentImageLoader
    frames, labels = frames_and_labels(count)
    return ResidentImageLoader(ResidentImageDataset(frames, labels), batch_size, seed=seed, draws='device', draw_id=draw_id,
                               **arguments)


def test_the_loader_in_device_mode(lib):
    loader = device_loader()
    dataset, batches = loader.dataset, len(loader)
    assert batches == 5 and loader.state is None
    for epoch in range(2):
        seen = []
        for number, (images, labels) in enumerate(loader):
            step = epoch * batches + number
            table = loader.last_table.cpu().tolist()
            assert table == batch_table(SEEDS[1], step, LABELED_DRAW, 23, 4)
            assert tuple(images.shape) == (4, 3, 4, 4) and tuple(labels.shape) == (4,)
            for position, index in enumerate(table):
                image, label = dataset[index]
                assert torch.equal(images[position].cpu(), image) and float(labels[position]) == float(label)
            seen += table
            assert loader.state.cpu().numpy().view(np.uint32).tolist() == [17, 2 ** 8, step + 1, 0]
        assert len(seen) == len(set(seen)) == batches * 4             # one epoch: 20 distinct frames of the 23
        assert loader.order.cpu().tolist() == epoch_order(SEEDS[1], epoch, LABELED_DRAW, 23).tolist()
    assert loader.generator is None
    other = device_loader(draw_id=UNLABELED_DRAW)
    next(iter(other))
    assert other.last_table.cpu().tolist() == batch_table(SEEDS[1], 0, UNLABELED_DRAW, 23, 4)
    # in_order() is the stored order, as in host mode
    walked = torch.cat([images for images, _ in loader.in_order()]).cpu()
    assert torch.equal(walked, torch.stack([dataset[index][0] for index in range(23)]))
    # data-parallel ranks take their rows of the global batch
    whole = device_loader(batch_size=6)
    whole.start_at(4)
    global_images, global_labels = whole.device_batch()
    for world_size in (2, 3):
        local = 6 // world_size
        for rank in range(world_size):
            ranked = device_loader(batch_size=6, dp=Ranks(world_size, rank))
            ranked.start_at(4)
            images, labels = ranked.device_batch()
            assert torch.equal(ranked.last_table, whole.last_table[rank * local:(rank + 1) * local])
            assert torch.equal(images, global_images[rank * local:(rank + 1) * local])
            assert torch.equal(labels, global_labels[rank * local:(rank + 1) * local])
            assert torch.equal(ranked.order, whole.order)


def test_a_loader_started_at_a_step_reproduces_that_step(lib):
    first = device_loader(count=10)
    batches = [tuple(tensor.clone() for tensor in first.device_batch()) + (first.last_table.clone(),) for _ in range(6)]
    for step in (0, 1, 3, 4, 5):                                     # 1, 3, 5: the middle of an epoch of two batches
        resumed = device_loader(count=10)
        resumed.start_at(step)
        for later in range(step, 6):
            got = resumed.device_batch() + (resumed.last_table,)
            assert all(torch.equal(a, b) for a, b in zip(got, batches[later])), (step, later)
    assert not torch.equal(batches[0][2], batches[2][2])
    # the same loader put back
    first.start_at(1)
    assert torch.equal(first.device_batch()[0], batches[1][0])


def test_the_loaders_batch_replays_from_a_graph_captured_in_the_middle_of_an_epoch(lib):
    eager = device_loader(count=10)
    eager.start_at(1)
    expected = [tuple(tensor.clone() for tensor in eager.device_batch()) + (eager.last_table.clone(),) for _ in range(5)]
    loader = device_loader(count=10)
    loader.start_at(1)
    loader.prepare_capture()                                         # the order of epoch 0 is built here, not in the graph
    state, order = loader.state, loader.order
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = loader.device_batch()
    table = loader.last_table
    assert loader.state is state and loader.order is order and loader.state.cpu().tolist()[2] == 1
    for iteration in range(5):
        for tensor in captured:
            tensor.fill_(float('nan'))
        table.fill_(-1)
        graph.replay()
        loader.replayed()
        torch.cuda.synchronize()
        got = captured + (table,)
        assert all(torch.equal(a, b) for a, b in zip(got, expected[iteration])), iteration
    assert loader.state.cpu().tolist()[2] == 6
    # the host's count followed the replays: the next eager batch is step 6, an epoch start that the host rebuilds
    assert torch.equal(loader.device_batch()[0], eager.device_batch()[0])
    assert loader.last_table.cpu().tolist() == batch_table(SEEDS[1], 6, LABELED_DRAW, 10, 4)


# ---- the experiments ------------------------------------------------------------------------------------------------------
EXPERIMENT_SEED = 2 ** 36 + 21
FP16 = dict(compute_dtype='f16', storage_dtype='f16', gradient_penalty_dtype='f32', loss_scale=256.0)


@pytest.fixture(scope='module')
def databases(tmp_path_factory):
    """26 frames of 8 x 8 each: 10 labeled, 12 unlabeled and 4 validation frames, so that six steps of batch 4 cross the epoch
    boundaries of both loaders (two and three batches per epoch)."""
    generator = np.random.RandomState(12)
    count = 26
    age_names = np.array(['face_%02d.png' % index for index in range(count)])
    ages = generator.randint(10, 90, size=count).astype(np.float64)
    content = {'driving/names': np.array(['%d.jpg' % (100 + index) for index in range(count)]),
               'driving/angles': generator.uniform(-1, 1, size=count),
               'driving/frames': generator.uniform(0, 255, size=(count, 3, 8, 8)),
               'age/names': age_names, 'age/images': generator.randint(0, 256, size=(count, 8, 8, 3)).astype(np.uint8),
               'age/meta_json': json.dumps([[str(name), float(age), 'x'] for name, age in zip(age_names, ages)])}
    root = tmp_path_factory.mktemp('epoch_order_databases')
    return {'driving': write_driving_database(content, root / 'driving'), 'age': write_age_database(content, root / 'age')}


def image_experiment(kind, databases, monkeypatch, steps, attributes=(), load_from=None, **overrides):
    """An age (DCGAN networks) or driving experiment at 16 x 16 over the tiny database, ready for ``training_loop``."""
    import srgan_amd.age.srgan as age
    from srgan_amd.driving.srgan import DrivingExperiment
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all
    base, variable = {'age': (age.AgeExperiment, 'SRGAN_AGE_DATABASE'),
                      'driving': (DrivingExperiment, 'SRGAN_DRIVING_DATABASE')}[kind]

    class Small(base):
        def validation_summaries(self, step):
            pass

    monkeypatch.setattr(age, 'model_architecture', 'dcgan')
    monkeypatch.setenv(variable, databases[kind])
    settings = Settings()
    values = dict(labeled_dataset_size=10, validation_dataset_size=4, unlabeled_dataset_size=12, batch_size=4,
                  labeled_dataset_seed=3, matching_loss_multiplier=1e2, contrasting_loss_multiplier=1e1,
                  gradient_penalty_multiplier=1e2, steps_to_run=steps, device_random_draws=True,
                  device_random_seed=EXPERIMENT_SEED, save_step_period=0)
    for key, value in dict(values, **overrides).items():
        setattr(settings, key, value)
    if load_from is not None:
        settings.load_model_path, settings.continue_existing_experiments = load_from, True
    experiment = Small(settings)
    experiment.image_size = 16
    for key, value in dict(attributes).items():
        setattr(experiment, key, value)
    seed_all(0)
    experiment.dataset_setup()
    experiment.model_setup()
    quiet_writers(experiment)
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    experiment.load_models()
    experiment.train_mode()
    seed_all(5)                                                      # the host streams a host-mode run draws from
    return experiment


def quiet_writers(experiment):
    from srgan_amd.utility import SummaryWriter
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.summary_period = 10 ** 9                              # step 0 is the one summary step


def count_on_device(experiment):
    for optimizer in (experiment.d_optimizer, experiment.g_optimizer, experiment.dnn_optimizer):
        optimizer.count_on_device()                                  # the Adam entry point a capture needs, for both runs
    return experiment


def trained(experiment):
    """``training_loop`` to the end; the weight arenas and the Adam moments."""
    experiment.training_loop()
    torch.cuda.synchronize()
    tensors = {}
    for network, optimizer in experiment.CHECKPOINT_PARTS:
        tensors[network] = getattr(experiment, network)._srgan_arena.data.clone()
        tensors[optimizer + '.exp_avg'] = getattr(experiment, optimizer).exp_avg.clone()
        tensors[optimizer + '.exp_avg_sq'] = getattr(experiment, optimizer).exp_avg_sq.clone()
    assert all(bool(torch.isfinite(tensor).all()) for tensor in tensors.values())
    return tensors


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name], b[name]), (name, float((a[name] - b[name]).abs().max()))


def assert_loaders_at(experiment, step, sizes=(10, 12)):
    """Both loaders drew on the device; their states stand at ``step`` and their last tables are those of ``step - 1``."""
    for loader, draw, n in zip((experiment.train_dataset_loader, experiment.unlabeled_dataset_loader),
                               (LABELED_DRAW, UNLABELED_DRAW), sizes):
        assert (loader.draw_mode, loader.draw_id, loader.seed, len(loader.dataset)) == ('device', draw, EXPERIMENT_SEED, n)
        assert loader.state.cpu().tolist()[2] == step
        assert loader.last_table.cpu().tolist() == batch_table(EXPERIMENT_SEED, step - 1, draw, n, 4)


DEVICE = {'image_batch_draws': 'device'}


def test_an_age_run_continued_from_a_checkpoint_repeats_the_uninterrupted_run(lib, databases, monkeypatch, tmp_path):
    six = image_experiment('age', databases, monkeypatch, 6, DEVICE)
    whole = trained(six)
    assert_loaders_at(six, 6)
    three = image_experiment('age', databases, monkeypatch, 3, DEVICE)
    half = trained(three)
    assert_loaders_at(three, 3)
    assert not torch.equal(half['D'], whole['D'])
    three.trial_directory = str(tmp_path)
    three.save_models(step=2)
    resumed = image_experiment('age', databases, monkeypatch, 6, DEVICE, load_from=str(tmp_path))
    assert resumed.starting_step == 3
    result = trained(resumed)
    assert_loaders_at(resumed, 6)
    assert_same_bits(result, whole)


CAPTURED = dict(step_graph=True, step_graph_warmup=1)


def assert_loaders_were_captured(experiment, steps):
    captured = experiment._captured_iteration
    # step 0 is the summary step and the one warm-up iteration; every later step is a replay that copied no input
    assert (captured.eager_iterations, captured.replays, captured.input_copies) == (1, steps - 1, 0)
    assert all(record['inputs'] == [] and record['batches'] is not None for record in captured.records.values())


def test_an_age_run_with_captured_loaders_equals_the_eager_run(lib, databases, monkeypatch):
    eager = count_on_device(image_experiment('age', databases, monkeypatch, 6, DEVICE))
    expected = trained(eager)
    assert eager._captured_iteration is None
    replayed = count_on_device(image_experiment('age', databases, monkeypatch, 6, dict(DEVICE, capture_loaders=True),
                                                **CAPTURED))
    result = trained(replayed)
    assert_loaders_were_captured(replayed, 6)
    assert_loaders_at(replayed, 6)
    assert replayed.train_dataset_loader._step == replayed.unlabeled_dataset_loader._step == 6
    assert_same_bits(result, expected)
    # without capture_loaders the same run copies its three input tensors in front of every replay, as before
    copied = count_on_device(image_experiment('age', databases, monkeypatch, 6, DEVICE, **CAPTURED))
    assert copied.captured_loaders() is None
    result = trained(copied)
    captured = copied._captured_iteration
    assert (captured.eager_iterations, captured.replays, captured.input_copies) == (1, 5, 15)
    assert_same_bits(result, expected)


def test_a_driving_run_on_fp16_storage_with_captured_loaders_equals_the_eager_run(lib, databases, monkeypatch):
    eager = count_on_device(image_experiment('driving', databases, monkeypatch, 6, DEVICE, **FP16))
    expected = trained(eager)
    replayed = count_on_device(image_experiment('driving', databases, monkeypatch, 6, dict(DEVICE, capture_loaders=True),
                                                **dict(FP16, **CAPTURED)))
    result = trained(replayed)
    assert_loaders_were_captured(replayed, 6)
    assert_loaders_at(replayed, 6)
    assert_same_bits(result, expected)


def test_a_crowd_run_with_captured_loaders_equals_the_eager_run(lib, monkeypatch, tmp_path):
    from test_crowd_patch_draws_gpu import small_experiment, write_database
    write_database(str(tmp_path / 'shanghai'), 'shanghai')

    def run(**overrides):
        experiment = small_experiment(monkeypatch, tmp_path, draws='device', steps=4, **overrides)     # two labeled scenes
        quiet_writers(experiment)
        return count_on_device(experiment)

    eager = run()
    expected = trained(eager)
    replayed = run(**CAPTURED)
    replayed.capture_loaders = True
    result = trained(replayed)
    assert_loaders_were_captured(replayed, 4)
    for loader in (replayed.train_dataset_loader, replayed.unlabeled_dataset_loader):
        assert loader.state.cpu().tolist()[2] == 4
    assert torch.equal(replayed.train_dataset_loader.last_table, eager.train_dataset_loader.last_table)
    assert_same_bits(result, expected)


def test_capture_loaders_needs_loaders_in_device_mode(lib, databases, monkeypatch):
    experiment = image_experiment('age', databases, monkeypatch, 2, {'capture_loaders': True}, **CAPTURED)
    assert experiment.train_dataset_loader.draw_mode == 'host'
    before = experiment.D._srgan_arena.data.clone()
    with pytest.raises(ValueError):
        experiment.training_loop()
    torch.cuda.synchronize()
    assert torch.equal(experiment.D._srgan_arena.data, before)        # raised before the first step
    with pytest.raises(ValueError):
        image_experiment('age', databases, monkeypatch, 2, {'image_batch_draws': 'gpu'})
    # without step_graph the switch asks for nothing
    experiment = image_experiment('age', databases, monkeypatch, 1, {'capture_loaders': True})
    assert experiment.captured_loaders() is None


def test_the_defaults_train_the_bits_of_the_loop_without_the_feature(lib, databases, monkeypatch):
    """Host mode through ``training_loop`` against the same iterations driven by hand from the loaders' own iterators (the
    loop as it was before the switches existed); the loaders are the host generators' and nothing of the device mode exists."""
    untouched = image_experiment('age', databases, monkeypatch, 3, device_random_draws=False)
    assert 'image_batch_draws' not in vars(untouched) and 'capture_loaders' not in vars(untouched)
    assert untouched.image_batch_draws == 'host' and untouched.capture_loaders is False and untouched.captured_loaders() is None
    for loader, seed in ((untouched.train_dataset_loader, 3), (untouched.unlabeled_dataset_loader, 100)):
        assert loader.draw_mode == 'host' and loader.state is None and loader.order is None
        peek = torch.Generator()
        peek.set_state(loader.generator.get_state())
        assert torch.equal(torch.randperm(len(loader.dataset), generator=peek),
                           torch.randperm(len(loader.dataset), generator=torch.Generator().manual_seed(seed)))
    first = trained(untouched)
    assert untouched.train_dataset_loader.state is None and untouched.train_dataset_loader.last_table is None
    by_hand = image_experiment('age', databases, monkeypatch, 3, {'image_batch_draws': 'host'}, device_random_draws=False)
    labeled = by_hand.infinite_iter(by_hand.train_dataset_loader)
    unlabeled = by_hand.infinite_iter(by_hand.unlabeled_dataset_loader)
    for step in range(3):
        by_hand.adjust_learning_rate(step)
        examples, labels = by_hand.unpack_labeled(next(labeled))
        by_hand.dnn_training_step(examples, labels, step)
        by_hand.gan_training_step(examples, labels, next(unlabeled)[0], step)
    torch.cuda.synchronize()
    for network, _ in by_hand.CHECKPOINT_PARTS:
        assert torch.equal(getattr(by_hand, network)._srgan_arena.data, first[network]), network
