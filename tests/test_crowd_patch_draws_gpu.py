"""The crowd loader's device draws on the GPU: ``srgan_crowd_draw_patches`` exactly against the reference
(crowd_patch_draws_reference.py) on hand-made scene tables and on tables whose length needs more than 32 bits, its keys and
windows; ``srgan_crowd_extract_patches_indexed`` bit for bit against ``srgan_crowd_extract_patches`` and exactly against the
NumPy restatement on both store widths; the loader's device mode, its resume, the three launches of a batch replayed from a
captured graph, the evaluation set over a device table; and the crowd experiment with the switch on and off.  Every output is
NaN-filled (int: -2^31) beforehand so that an unwritten element shows."""
import os

import numpy as np
import pytest
import torch

from crowd_patch_draws_reference import (INT_MIN, LABELED_DRAW, UNLABELED_DRAW, draw_table, indexed_patches, scene_starts)
from test_crowd_patch_draws_cpu import BIG_PATCH, BIG_SHAPES, HAND_PATCH, HAND_SHAPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def device_state(seed, iteration):
    words = np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff, iteration & 0xffffffff, 0], dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)).cuda()


class SceneTables:
    """``starts`` / ``heights`` / ``widths`` of scenes ``(H, W)`` on the device -- no scene memory: the draw needs none."""

    def __init__(self, shapes, patch_size):
        self.shapes, self.patch_size = shapes, patch_size
        self.starts = scene_starts(shapes, patch_size)
        self.widths = [shape[1] for shape in shapes]
        self.device_starts = torch.tensor(self.starts, dtype=torch.int64).cuda()
        self.device_heights = torch.tensor([shape[0] for shape in shapes], dtype=torch.int32).cuda()
        self.device_widths = torch.tensor(self.widths, dtype=torch.int32).cuda()

    def draw(self, lib, flip, first, n, draw, seed, iteration):
        """Rows ``[first, first + n)`` drawn into the middle of a table of ``n + 2`` rows of -2^31; the guard rows must stay."""
        table = torch.full((n + 2, 4), INT_MIN, dtype=torch.int32, device='cuda')
        state = device_state(seed, iteration)
        lib.check(lib.library().srgan_crowd_draw_patches(
            self.device_starts.data_ptr(), self.device_heights.data_ptr(), self.device_widths.data_ptr(), len(self.shapes),
            self.patch_size, int(flip), first, n, draw, state.data_ptr(), table[1:].data_ptr(), stream()),
            'srgan_crowd_draw_patches')
        torch.cuda.synchronize()
        assert state.cpu().numpy().view(np.uint32).tolist() == [seed & 0xffffffff, (seed >> 32) & 0xffffffff,
                                                                  iteration & 0xffffffff, 0]          # read only
        out = table.cpu().numpy().astype(np.int64)
        assert (out[0] == INT_MIN).all() and (out[-1] == INT_MIN).all()
        return out[1:-1]

    def expected(self, flip, first, n, draw, seed, iteration):
        return draw_table(self.starts, self.widths, self.patch_size, flip, first, n, draw, seed, iteration)


@pytest.fixture(scope='module')
def tables():
    return {'hand': SceneTables(HAND_SHAPES, HAND_PATCH), 'big': SceneTables(BIG_SHAPES, BIG_PATCH),
            'one': SceneTables([(2, 2), (6, 6)], 6)}


# ---- the draw kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', [0, 3, 2 ** 32 - 2])
@pytest.mark.parametrize('name', ['hand', 'big', 'one'])
def test_the_draw_kernel_against_the_reference(lib, tables, name, first):
    scene_tables = tables[name]
    seed, iteration = 2 ** 40 + 3, 123456
    for n in (1, 5, 64, 257):
        got = scene_tables.draw(lib, True, first, n, LABELED_DRAW, seed, iteration)
        expected = scene_tables.expected(True, first, n, LABELED_DRAW, seed, iteration)
        assert np.array_equal(got, expected), (name, first, n, got[:4], expected[:4])
    unflipped = scene_tables.draw(lib, False, first, 64, LABELED_DRAW, seed, iteration)
    assert np.array_equal(unflipped, scene_tables.expected(False, first, 64, LABELED_DRAW, seed, iteration))
    assert not unflipped[:, 3].any()
    if name == 'big':
        assert sorted(set(got[:, 0])) == [0, 1, 2]
    if name == 'hand':
        assert set(got[:, 0]) == {1, 2, 3}                                  # the scenes without a centre are never drawn
    assert scene_tables.draw(lib, True, first, 0, LABELED_DRAW, seed, iteration).shape == (0, 4)        # n == 0: untouched


def test_the_draw_kernels_keys_and_windows(lib, tables):
    scene_tables = tables['big']
    seen = []
    for seed in ((1 << 32) | 5, (2 << 32) | 5):                           # the high words differ
        for iteration in (2 ** 31 + 1, 2 ** 32 - 1):
            for draw in (LABELED_DRAW, UNLABELED_DRAW):
                whole = scene_tables.draw(lib, True, 0, 96, draw, seed, iteration)
                assert np.array_equal(whole, scene_tables.expected(True, 0, 96, draw, seed, iteration)), (seed, iteration, draw)
                seen.append(whole.tobytes())
    assert len(set(seen)) == 8
    seed, iteration = (2 << 32) | 5, 2 ** 31 + 1
    whole = scene_tables.draw(lib, True, 0, 96, LABELED_DRAW, seed, iteration)
    for world_size in (2, 3):
        local = 96 // world_size
        for rank in range(world_size):
            window = scene_tables.draw(lib, True, rank * local, local, LABELED_DRAW, seed, iteration)
            assert np.array_equal(window, whole[rank * local:(rank + 1) * local]), (world_size, rank)
    assert np.array_equal(scene_tables.draw(lib, True, 37, 5, LABELED_DRAW, seed, iteration), whole[37:42])


# ---- the indexed extraction -----------------------------------------------------------------------------------------------
def patch_scenes(patch_size, seed=11):
    """Scenes smaller than, equal to and larger than a patch, with odd widths; uint8 images, labels and maps on a dyadic grid."""
    from srgan_amd.crowd.data import CrowdExample
    generator = np.random.RandomState(seed)
    shapes = [(patch_size - 1, patch_size + 1), (patch_size, patch_size), (patch_size + 3, 2 * patch_size + 1),
              (2 * patch_size + 1, patch_size + 5)]
    return [CrowdExample(image=generator.randint(0, 256, size=shape + (3,)).astype(np.uint8),
                         label=(generator.randint(0, 17, size=shape) / 8).astype(np.float32),
                         map_=(generator.randint(-32, 33, size=shape) / 16).astype(np.float32)) for shape in shapes]


def case_rows(scenes, with_outside=True):
    """Per scene the centres (0, 0), (H - 1, W - 1) and one inside, each with and without flip; then scenes -1 and S."""
    rows = []
    for index, scene in enumerate(scenes):
        height, width = scene.image.shape[:2]
        for y, x in ((0, 0), (height - 1, width - 1), (height // 2, width // 2 + 1)):
            rows += [(index, y, x, 0), (index, y, x, 1)]
    if with_outside:
        rows += [(-1, 2, 2, 0), (len(scenes), 1, 3, 1)]
    return rows


def guarded(shape, offset):
    """A NaN-filled output of ``shape`` that starts ``offset`` floats into its allocation, with 64 guard floats behind it."""
    count = int(np.prod(shape))
    flat = torch.full((offset + count + 64,), float('nan'), dtype=torch.float32, device='cuda')
    return flat, flat[offset:offset + count].view(shape)


def indexed(lib, loader, rows, offset=0, with_labels=True, with_maps=True):
    """One ``srgan_crowd_extract_patches_indexed`` call over ``loader``'s scene tables; checks the guards."""
    size, count = loader.patch_size, len(rows)
    loader.upload_scene_table()
    table = torch.tensor(rows, dtype=torch.int32).cuda()
    flats, outs = zip(*(guarded(shape, offset) for shape in ((count, 3, size, size), (count, size, size), (count, size, size))))
    pointers = loader.scene_pointers
    lib.check(lib.library().srgan_crowd_extract_patches_indexed(
        pointers[0].data_ptr(), pointers[1].data_ptr() if with_labels else None, pointers[2].data_ptr() if with_maps else None,
        loader.scene_heights.data_ptr(), loader.scene_widths.data_ptr(), len(loader.shapes), table.data_ptr(), count, size,
        outs[0].data_ptr(), outs[1].data_ptr() if with_labels else None, outs[2].data_ptr() if with_maps else None, stream()),
        'srgan_crowd_extract_patches_indexed')
    torch.cuda.synchronize()
    for flat, out, written in zip(flats, outs, (True, with_labels, with_maps)):
        assert torch.isnan(flat[:offset]).all() and torch.isnan(flat[offset + out.numel():]).all()      # nothing around it
        assert bool(torch.isnan(out).any()) != written and (written or bool(torch.isnan(out).all()))
    return tuple(out.cpu().numpy() for out in outs)


@pytest.mark.parametrize('offset', [0, 1])                       # an output base off the 16-byte grid takes single floats
@pytest.mark.parametrize('patch_size', [4, 6, 8])                # 6: single floats; 4 and 8: 16-byte runs
def test_the_indexed_extraction(lib, patch_size, offset):
    from srgan_amd.crowd.data import DeviceCrowdPatchLoader
    scenes = patch_scenes(patch_size)
    loader = DeviceCrowdPatchLoader(scenes, 4, patch_size, seed=0)
    rows = case_rows(scenes)
    got = indexed(lib, loader, rows, offset=offset)
    arrays = [[scene.image for scene in scenes], [scene.label for scene in scenes], [scene.map for scene in scenes]]
    expected = indexed_patches(*arrays, rows, patch_size)
    for name, a, b in zip(('image', 'label', 'map'), got, expected):
        assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:4])
    # the rows outside the scene table: all padding
    assert (got[0][-2:] == -1.0).all() and not got[1][-2:].any() and not got[2][-2:].any()
    # the parent's entry point on the same draws, bit for bit
    old = [part.cpu().numpy() for part in loader.batch_for(rows[:-2])]
    for name, a, b in zip(('image', 'label', 'map'), got, old):
        assert a[:-2].tobytes() == b.tobytes(), name
    # the loader's own call
    through = [part.cpu().numpy() for part in loader.batch_for_table(torch.tensor(rows, dtype=torch.int32).cuda())]
    for a, b in zip(got, through):
        assert a.tobytes() == b.tobytes()
    # NULL labels / maps
    image_only = indexed(lib, loader, rows, offset=offset, with_labels=False, with_maps=False)
    assert image_only[0].tobytes() == got[0].tobytes()
    no_map = indexed(lib, loader, rows, offset=offset, with_maps=False)
    assert no_map[0].tobytes() == got[0].tobytes() and no_map[1].tobytes() == got[1].tobytes()
    no_label = indexed(lib, loader, rows, offset=offset, with_labels=False)
    assert no_label[2].tobytes() == got[2].tobytes()


def test_the_indexed_extraction_over_several_workgroup_rows(lib):
    """P = 12 is three workgroups of four rows; P = 10 leaves the last workgroup two idle waves; B beyond one."""
    from srgan_amd.crowd.data import DeviceCrowdPatchLoader
    for patch_size in (10, 12):
        scenes = patch_scenes(patch_size, seed=patch_size)
        loader = DeviceCrowdPatchLoader(scenes, 4, patch_size, seed=0)
        rows = case_rows(scenes)
        got = indexed(lib, loader, rows)
        expected = indexed_patches([s.image for s in scenes], [s.label for s in scenes], [s.map for s in scenes], rows, patch_size)
        for a, b in zip(got, expected):
            assert a.tobytes() == b.tobytes(), patch_size


# ---- the loader -----------------------------------------------------------------------------------------------------------
LOADER_SHAPES = [(70, 90), (20, 200), (64, 64), (100, 81)]           # P = 64: the second scene has no centre
LOADER_SEED = 2 ** 40 + 17


def loader_scenes():
    from srgan_amd.crowd.data import CrowdExample
    generator = np.random.RandomState(5)
    return [CrowdExample(image=generator.randint(0, 256, size=shape + (3,)).astype(np.uint8),
                         label=(generator.rand(*shape) < 0.01).astype(np.float32),
                         map_=generator.rand(*shape).astype(np.float32)) for shape in LOADER_SHAPES]


def device_loader(batch_size=6, draw_id=LABELED_DRAW, dp=None, **arguments):
    from srgan_amd.crowd.data import DeviceCrowdPatchLoader
    return DeviceCrowdPatchLoader(loader_scenes(), batch_size, 64, seed=LOADER_SEED, draws='device', draw_id=draw_id, dp=dp,
                                  **arguments)


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


class Ranks:
    """What the loader asks of a data-parallel context."""

    def __init__(self, world_size, rank):
        self.world_size, self.rank = world_size, rank

    def local_batch(self, batch_size):
        assert batch_size % self.world_size == 0
        return batch_size // self.world_size


def test_the_loader_in_device_mode(lib):
    loader = device_loader()
    assert loader.state is None and loader.last_table is None
    starts, widths = scene_starts(LOADER_SHAPES, 64), [shape[1] for shape in LOADER_SHAPES]
    batches = iter(loader)
    for iteration in range(4):
        batch = next(batches)
        table = loader.last_table
        assert table.dtype == torch.int32 and tuple(table.shape) == (6, 4)
        rows = table.cpu().tolist()
        assert rows == draw_table(starts, widths, 64, True, 0, 6, LABELED_DRAW, LOADER_SEED, iteration).tolist()
        assert same_bits(batch, loader.batch_for([tuple(row) for row in rows])), iteration
        assert tuple(batch[0].shape) == (6, 3, 64, 64) and tuple(batch[1].shape) == tuple(batch[2].shape) == (6, 64, 64)
        assert loader.state.cpu().numpy().view(np.uint32).tolist() == [17, 2 ** 8, iteration + 1, 0]
        for scene, y, x, flip in rows:
            height, width = LOADER_SHAPES[scene]
            assert scene != 1 and 32 <= y <= height - 32 and 32 <= x <= width - 32 and flip in (0, 1)
    assert loader.generator is None                                     # no host stream in device mode
    with pytest.raises(ValueError):
        loader.draw_positions()
    # the other loader's draw id and an unflipped loader
    other = device_loader(draw_id=UNLABELED_DRAW)
    next(iter(other))
    assert other.last_table.cpu().tolist() == draw_table(starts, widths, 64, True, 0, 6, UNLABELED_DRAW, LOADER_SEED, 0).tolist()
    unflipped = device_loader(flip=False)
    next(iter(unflipped))
    assert unflipped.last_table.cpu().tolist() == draw_table(starts, widths, 64, False, 0, 6, LABELED_DRAW, LOADER_SEED, 0).tolist()
    # data-parallel ranks draw their own rows of the global table only
    whole = device_loader()
    global_batch = next(iter(whole))
    for world_size in (2, 3):
        local = 6 // world_size
        for rank in range(world_size):
            ranked = device_loader(dp=Ranks(world_size, rank))
            part = next(iter(ranked))
            assert tuple(ranked.last_table.shape) == (local, 4)
            assert torch.equal(ranked.last_table, whole.last_table[rank * local:(rank + 1) * local])
            assert same_bits(part, [tensor[rank * local:(rank + 1) * local] for tensor in global_batch])


def test_a_loader_started_at_a_step_reproduces_the_later_batches(lib):
    first = iter(device_loader())
    batches = [next(first) for _ in range(4)]
    resumed = device_loader()
    resumed.start_at(2)
    second = iter(resumed)
    assert same_bits(next(second), batches[2]) and same_bits(next(second), batches[3])
    assert not same_bits(batches[0], batches[2])
    again = device_loader()
    again.start_at(0)
    assert same_bits(next(iter(again)), batches[0])


def test_the_batch_replays_from_a_captured_graph(lib):
    """Draw, cut and advance recorded once on one stream: three replays are the next three iterations' batches."""
    eager = device_loader()
    eager.start_at(1)
    expected = []
    for _ in range(3):
        batch = next(iter(eager))
        expected.append(([tensor.clone() for tensor in batch], eager.last_table.clone()))
    loader = device_loader()
    loader.start_at(1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                                      # (the kernels were loaded by the eager batches)
    with torch.cuda.graph(graph):
        captured = loader.device_batch()
    table = loader.last_table
    assert loader.state.cpu().tolist()[2] == 1                           # capturing ran nothing
    for iteration in range(3):
        for tensor in captured + (table,):
            tensor.fill_(float('nan') if tensor.is_floating_point() else INT_MIN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(table, expected[iteration][1]), iteration
        assert same_bits(captured, expected[iteration][0]), iteration
    assert loader.state.cpu().tolist()[2] == 4


def test_the_evaluation_set_over_a_device_table(lib):
    from srgan_amd.crowd.data import DeviceCrowdPatchLoader, ResidentCrowdEvaluationSet
    host_loader = DeviceCrowdPatchLoader(loader_scenes(), 50, 64, seed=3)
    loader = device_loader(batch_size=50)
    loader.start_at(5)
    state = loader.state.cpu().tolist()
    host_set = ResidentCrowdEvaluationSet(host_loader, 50, 64, seed=3, flip=True)
    device_set = ResidentCrowdEvaluationSet(loader, 50, 64, seed=3, flip=True)
    assert host_set.table is None and device_set.draws == host_set.draws
    assert device_set.table.dtype == torch.int32 and device_set.table.cpu().tolist() == [list(draw) for draw in host_set.draws]
    device_batches, host_batches = list(device_set.device_batches()), list(host_set.device_batches())
    assert len(device_batches) == len(host_batches) == 3
    for a, b in zip(device_batches, host_batches):
        assert same_bits(a, b)
    for index in (0, 77, 149, -1):
        assert same_bits(device_set[index], host_set[index]), index
    with pytest.raises(IndexError):
        device_set[150]
    assert loader.state.cpu().tolist() == state and loader.last_table is None          # the loader's stream has not moved
    own = ResidentCrowdEvaluationSet(loader_scenes(), 50, 64, seed=101, flip=False, draws='device')   # scenes uploaded here
    own_host = ResidentCrowdEvaluationSet(loader_scenes(), 50, 64, seed=101, flip=False)
    assert own.table is not None and own_host.table is None
    assert same_bits(next(own.device_batches()), next(own_host.device_batches()))


# ---- the experiment -------------------------------------------------------------------------------------------------------
EXPERIMENT_SEED = 2 ** 36 + 21
LOSSES = ('dnn_loss', 'labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss')


def write_database(directory, layout, train=5, test=1, seed=4):
    """Scenes of about 80 x 100 in the ShanghaiTech layout (``part_A/<split>_data``) or the UCF-QNRF one (``<Split>``)."""
    generator = np.random.RandomState(seed)
    for split, count in (('train', train), ('test', test)):
        folder = os.path.join(directory, 'part_A', split + '_data') if layout == 'shanghai' else \
            os.path.join(directory, split.capitalize())
        for index in range(count):
            shape = (80 + 4 * index, 100 + index)
            arrays = {'images': generator.randint(0, 256, size=shape + (3,)).astype(np.uint8),
                      'labels': (generator.rand(*shape) < 0.004).astype(np.float32),
                      'i1nn_maps': generator.rand(*shape).astype(np.float32)}
            for kind, array in arrays.items():
                os.makedirs(os.path.join(folder, kind), exist_ok=True)
                np.save(os.path.join(folder, kind, 'IMG_%d.npy' % index), array)


@pytest.fixture(scope='module')
def databases(tmp_path_factory):
    root = tmp_path_factory.mktemp('crowd_patch_draw_databases')
    for layout in ('shanghai', 'ucf'):
        write_database(str(root / layout), layout)
    return root


def small_experiment(monkeypatch, databases, layout='shanghai', draws=None, steps=2, load_from=None, **overrides):
    """A crowd experiment over the tiny database with small networks, ready for ``training_loop``; ``draws``: the value
    ``crowd_patch_draws`` is set to (None: the attribute is left alone)."""
    from srgan_amd.crowd.models import DCGenerator, KnnDenseNetCat
    from srgan_amd.crowd.srgan import CrowdExperiment
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all

    class Small(CrowdExperiment):
        def model_setup(self):
            arguments = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16, bn_size=2, image_size=64)
            self.G = DCGenerator(image_size=64, conv_dim=16)
            self.D, self.DNN = KnnDenseNetCat(**arguments), KnnDenseNetCat(**arguments)

        def validation_summaries(self, step):
            pass

    monkeypatch.setenv('SRGAN_CROWD_DATABASE', str(databases / layout))
    if layout == 'shanghai':
        monkeypatch.setenv('SRGAN_CROWD_DATABASE_PART', 'part_A')
    else:
        monkeypatch.delenv('SRGAN_CROWD_DATABASE_PART', raising=False)
    settings = Settings()
    values = dict(batch_size=4, image_patch_size=64, labeled_dataset_size=2, unlabeled_dataset_size=3,
                  map_directory_name='i1nn_maps', matching_loss_multiplier=1e3, contrasting_loss_multiplier=1e2,
                  gradient_penalty_multiplier=1e2, map_multiplier=1e-3, steps_to_run=steps, device_random_draws=True,
                  device_random_seed=EXPERIMENT_SEED, save_step_period=0)
    for key, value in dict(values, **overrides).items():
        setattr(settings, key, value)
    if load_from is not None:
        settings.load_model_path, settings.continue_existing_experiments = load_from, True
    experiment = Small(settings)
    if draws is not None:
        experiment.crowd_patch_draws = draws
    experiment.dataset_setup()
    seed_all(0)
    experiment.model_setup()
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    experiment.load_models()
    experiment.train_mode()
    return experiment


def trained(experiment):
    """``training_loop`` to the end; the last step's losses and the three weight arenas."""
    experiment.training_loop()
    torch.cuda.synchronize()
    losses = {name: float(value.item()) for name, value in experiment.last_losses.items() if value is not None and name in LOSSES}
    assert losses and all(np.isfinite(value) for value in losses.values()), losses
    weights = {name: getattr(experiment, name)._srgan_arena.data.clone() for name in ('D', 'DNN', 'G')}
    return losses, weights


def assert_same_run(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for name in ('D', 'DNN', 'G'):
        assert torch.equal(a[1][name], b[1][name]), (name, float((a[1][name] - b[1][name]).abs().max()))
        assert float(a[1][name].double().sum()) == float(b[1][name].double().sum())


def test_host_mode_leaves_the_experiment_unchanged(lib, databases, monkeypatch):
    from srgan_amd.crowd.data import draw_example
    untouched = small_experiment(monkeypatch, databases)
    assert 'crowd_patch_draws' not in vars(untouched) and untouched.crowd_patch_draws == 'host'
    for loader, seed in ((untouched.train_dataset_loader, untouched.settings.labeled_dataset_seed),
                         (untouched.unlabeled_dataset_loader, 100)):
        assert loader.draw_mode == 'host' and loader.state is None and loader.scene_pointers is None
        generator = np.random.RandomState(seed)                      # the parent's loader: this generator, this rule
        peek = np.random.RandomState(seed)
        peek.set_state(loader.generator.get_state())
        assert [draw_example(peek, loader.length, loader.start_indexes, loader.shapes, 64, True) for _ in range(4)] == \
            [draw_example(generator, loader.length, loader.start_indexes, loader.shapes, 64, True) for _ in range(4)]
    first = trained(untouched)
    assert untouched.train_dataset_loader.state is None and untouched.train_dataset_loader.last_table is None
    explicit = small_experiment(monkeypatch, databases, draws='host')
    assert explicit.train_dataset_loader.draw_mode == 'host'
    assert_same_run(first, trained(explicit))


@pytest.fixture(scope='module')
def device_runs(lib, databases, tmp_path_factory):
    """Device mode: four iterations in one run | two iterations and a checkpoint of step 1."""
    monkeypatch = pytest.MonkeyPatch()
    try:
        four = small_experiment(monkeypatch, databases, draws='device', steps=4)
        for loader, draw_id in ((four.train_dataset_loader, 0x30000), (four.unlabeled_dataset_loader, 0x30001)):
            assert loader.draw_mode == 'device' and loader.draw_id == draw_id and loader.seed == EXPERIMENT_SEED
        whole = trained(four)
        assert four.train_dataset_loader.state.cpu().tolist()[2] == 4 and four.unlabeled_dataset_loader.state.cpu().tolist()[2] == 4
        two = small_experiment(monkeypatch, databases, draws='device', steps=2)
        half = trained(two)
        two.trial_directory = str(tmp_path_factory.mktemp('crowd_patch_draw_trial'))
        two.save_models(step=1)
        return whole, half, two.trial_directory, four.train_dataset_loader.last_table.cpu().tolist()
    finally:
        monkeypatch.undo()


def test_device_mode_runs_are_bit_identical(device_runs, databases, monkeypatch):
    again = small_experiment(monkeypatch, databases, draws='device', steps=2)
    assert_same_run(device_runs[1], trained(again))
    host = small_experiment(monkeypatch, databases, steps=2)
    assert trained(host)[0] != device_runs[1][0]                        # other patches than the host generator's


def test_a_continued_run_cuts_what_the_uninterrupted_run_cuts(device_runs, databases, monkeypatch):
    whole, _, trial_directory, last_rows = device_runs
    resumed = small_experiment(monkeypatch, databases, draws='device', steps=4, load_from=trial_directory)
    assert resumed.starting_step == 2
    result = trained(resumed)
    assert resumed.train_dataset_loader.state.cpu().tolist()[2] == 4
    assert resumed.train_dataset_loader.last_table.cpu().tolist() == last_rows
    for name in ('D', 'DNN', 'G'):
        assert torch.equal(result[1][name], whole[1][name]), (name, float((result[1][name] - whole[1][name]).abs().max()))
    assert result[0] == whole[0]


def test_the_ucf_qnrf_branch_in_device_mode(lib, databases, monkeypatch):
    experiment = small_experiment(monkeypatch, databases, layout='ucf', draws='device', steps=1, crowd_dataset='UCF QNRF',
                                  unlabeled_dataset_size=None)
    labeled, unlabeled = experiment.train_dataset_loader, experiment.unlabeled_dataset_loader
    assert (labeled.draw_mode, labeled.draw_id, unlabeled.draw_mode, unlabeled.draw_id) == ('device', 0x30000, 'device', 0x30001)
    assert len(labeled.shapes) == 2 and len(unlabeled.shapes) == 3 and not set(labeled.shapes) & set(unlabeled.shapes)
    trained(experiment)
    for loader, draw in ((labeled, 0x30000), (unlabeled, 0x30001)):
        widths = [shape[1] for shape in loader.shapes]
        assert loader.last_table.cpu().tolist() == draw_table(scene_starts(loader.shapes, 64), widths, 64, True, 0, 4, draw,
                                                              EXPERIMENT_SEED, 0).tolist()
        assert loader.state.cpu().tolist()[2] == 1
