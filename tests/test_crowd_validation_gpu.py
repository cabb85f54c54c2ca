"""Crowd validation from the resident database on the GPU: ``srgan_crowd_evaluation_sums`` bit for bit against the NumPy
restatement on inputs whose sums are exact in fp64 (every path of the launcher: element and 16-byte loads, misaligned bases,
several chunks with a ragged last one, more examples and more chunks than the finish kernel takes per pass), within the summation-order bound
on normal inputs, its argument errors; and the experiment: the
evaluation sets cut on the device, the six scalars per network and set against the untouched host ``evaluation_epoch`` on the
very same patches, the map comparisons, the UCF-QNRF branch, and training bits that do not move with the setting."""
import os

import numpy as np
import pytest
import torch

from crowd_validation_reference import TAGS, contraction_cases, evaluation_sums, order_bounds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def device_sums(lib, counts, labels, predicted=None, maps=None, sums=None, offset=0):
    """One call on uploaded copies; ``scratch`` is NaN beforehand; ``sums``: a device tensor to add to (default: new zeros).
    ``offset``: floats by which the labels / maps / predicted maps are shifted off their 16-byte aligned allocations."""
    def upload(array):
        if array is None:
            return None
        flat = torch.zeros(array.size + offset, dtype=torch.float32, device='cuda')
        flat[offset:].copy_(torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32).reshape(-1)))
        return flat[offset:]
    batch, plane = labels.shape[0], int(np.prod(labels.shape[1:]))
    channels = predicted.shape[1] if predicted is not None else 0
    tensors = [upload(counts), upload(labels), upload(predicted), upload(maps)]
    if sums is None:
        sums = torch.zeros(8, dtype=torch.float64, device='cuda')
    needed = lib.library().srgan_crowd_evaluation_scratch_bytes(batch, channels, plane)
    assert needed > 0 and needed % 8 == 0
    scratch = torch.full((needed // 8,), float('nan'), dtype=torch.float64, device='cuda')
    pointer = lambda tensor: None if tensor is None else tensor.data_ptr()
    lib.check(lib.library().srgan_crowd_evaluation_sums(
        pointer(tensors[0]), pointer(tensors[1]), pointer(tensors[2]), pointer(tensors[3]), batch, channels, plane,
        sums.data_ptr(), scratch.data_ptr(), lib.stream_handle()), 'srgan_crowd_evaluation_sums')
    torch.cuda.synchronize()
    return sums


def exact_batch(generator, batch, channels, size):
    """Inputs whose every term and partial sum is a multiple of 2^-6 far below 2^53: any order of additions is exact."""
    labels = generator.choice(np.array([0.0, 1.0, 0.5], dtype=np.float32), size=(batch, size * size))
    counts = generator.randint(-40, 41, size=batch).astype(np.float32)
    maps = (generator.randint(-32, 33, size=(batch, size * size)) / 8).astype(np.float32)
    predicted = (generator.randint(-32, 33, size=(batch, channels, size * size)) / 8).astype(np.float32)
    return counts, labels, predicted, maps


# (B, M, P): smallest case | odd plane, element loads | misaligned example bases | HW % 4 == 0 | several chunks, ragged last
# | more examples than one row of a folded grid, and than the finish kernel's 16 teams | many passes of the finish kernel's
# loop over the examples | more chunks (17) than a team of the finish kernel has lanes
EXACT_SHAPES = [(1, 1, 1), (1, 3, 5), (3, 3, 5), (2, 1, 6), (2, 3, 72), (17, 3, 8), (300, 1, 2), (2, 1, 184)]


@pytest.mark.parametrize('with_maps', [True, False])
@pytest.mark.parametrize('batch,channels,size', EXACT_SHAPES)
def test_the_sums_are_exact_on_exact_inputs(lib, batch, channels, size, with_maps):
    generator = np.random.RandomState(1000 * batch + 10 * size + channels)
    first, second = exact_batch(generator, batch, channels, size), exact_batch(generator, batch, channels, size)
    take = lambda inputs: inputs if with_maps else inputs[:2]
    preloaded = np.array([1.5, -2.0, 3.25, 4.0, 5.5, 6.0, 7.0, 8.25])
    sums = torch.from_numpy(preloaded.copy()).cuda()
    after_first = device_sums(lib, *take(first), sums=sums).cpu().numpy()
    expected_first = evaluation_sums(*take(first), sums=preloaded)
    assert np.array_equal(after_first, expected_first), (after_first, expected_first)
    after_second = device_sums(lib, *take(second), sums=sums).cpu().numpy()          # a second batch accumulates
    expected_second = evaluation_sums(*take(second), sums=expected_first)
    assert np.array_equal(after_second, expected_second), (after_second, expected_second)
    assert after_second[7] == 8.25 and after_second[3] == 4.0 + 2 * batch
    if with_maps:
        assert after_second[6] == 7.0 + 2 * batch * channels * size * size
    else:
        assert after_second[4:7].tolist() == [5.5, 6.0, 7.0]
    # mixed, as an evaluation epoch calls it: maps with the first batch only
    mixed = device_sums(lib, *take(second), sums=device_sums(lib, *first)).cpu().numpy()
    assert np.array_equal(mixed, evaluation_sums(*take(second), sums=evaluation_sums(*first)))


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_bases_off_the_16_byte_grid_take_the_element_loads(lib, offset):
    """HW % 4 == 0 but the tensors start ``offset`` floats into their allocation."""
    inputs = exact_batch(np.random.RandomState(offset), 2, 3, 52)                    # 2704 elements: two chunks
    assert np.array_equal(device_sums(lib, *inputs, offset=offset).cpu().numpy(), evaluation_sums(*inputs))


@pytest.mark.parametrize('plane', [1, 4])             # element loads | 16-byte loads
def test_the_squares_are_rounded_before_they_are_added(lib, plane):
    """Errors with 30 significant bits, whose squares are inexact in fp64: ``fl(fl(e1 * e1) + fl(e2 * e2))``, NumPy's value,
    is one unit in the last place away from what a fused multiply-add leaves -- in the map sum (partials kernel) and in the
    count sum (finish kernel); every other addition of the batch is exact, so the bits must equal the restatement's."""
    for inputs, unfused, fused in contraction_cases(4, plane):
        got = device_sums(lib, *inputs).cpu().numpy()
        print('sums[2] %r sums[5] %r rounded squares %r fused %r' % (got[2], got[5], unfused, fused))
        assert got[2] == unfused != fused and got[5] == unfused
        assert np.array_equal(got, evaluation_sums(*inputs))


def test_normal_inputs_within_the_summation_order_bound(lib):
    generator = np.random.RandomState(7)
    batch, channels, size = 5, 3, 37
    counts = generator.standard_normal(batch).astype(np.float32)
    labels = generator.standard_normal((batch, size * size)).astype(np.float32)
    maps = generator.standard_normal((batch, size * size)).astype(np.float32)
    predicted = generator.standard_normal((batch, channels, size * size)).astype(np.float32)
    got = device_sums(lib, counts, labels, predicted, maps).cpu().numpy()
    expected, bounds = evaluation_sums(counts, labels, predicted, maps), order_bounds(counts, labels, predicted, maps)
    for index in range(8):
        print('sums[%d] device %.17g restatement %.17g |difference| %.3g bound %.3g' % (
            index, got[index], expected[index], abs(got[index] - expected[index]), bounds[index]))
    for index in range(8):
        assert abs(got[index] - expected[index]) <= bounds[index], index
    assert got[3] == batch and got[6] == batch * channels * size * size and got[7] == 0.0
    again = device_sums(lib, counts, labels, predicted, maps).cpu().numpy()
    assert again.tobytes() == got.tobytes()                                        # the same bits on every run


def test_argument_errors_leave_the_sums_untouched(lib):
    counts, labels, predicted, maps = (torch.ones(shape, dtype=torch.float32, device='cuda')
                                       for shape in ((2,), (2, 25), (2, 3, 25), (2, 25)))
    preloaded = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    sums = torch.tensor(preloaded, dtype=torch.float64, device='cuda')
    scratch = torch.zeros(64, dtype=torch.float64, device='cuda')
    good = dict(counts=counts.data_ptr(), labels=labels.data_ptr(), predicted=predicted.data_ptr(), maps=maps.data_ptr(), B=2,
                M=3, HW=25, sums=sums.data_ptr(), scratch=scratch.data_ptr())

    def call(**changes):
        a = dict(good, **changes)
        return lib.library().srgan_crowd_evaluation_sums(a['counts'], a['labels'], a['predicted'], a['maps'], a['B'], a['M'],
                                                         a['HW'], a['sums'], a['scratch'], lib.stream_handle())
    for name in ('counts', 'labels', 'sums', 'scratch'):
        assert call(**{name: None}) == lib.EINVAL, name
    assert call(predicted=None) == lib.EINVAL and call(maps=None) == lib.EINVAL        # exactly one map pointer
    assert call(B=-1) == lib.EINVAL and call(HW=-1) == lib.EINVAL and call(M=0) == lib.EINVAL
    limit = lib.capabilities().max_tensor_elements
    assert call(B=1, M=1, HW=limit + 1) == lib.ERANGE and call(B=2 ** 10, M=2 ** 10, HW=2 ** 11) == lib.ERANGE
    assert call(B=0) == 0 and call(HW=0) == 0                                           # nothing to add: untouched
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == preloaded
    assert call() == 0                                                                  # ... and the good call does add
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [1.0 + 2 * (1 - 25), 2.0 + 48, 3.0 + 2 * 576, 6.0, 5.0, 6.0, 7.0 + 150, 8.0]


# ---- the experiment -------------------------------------------------------------------------------------------------------
def write_database(directory, layout, train=3, test=2, seed=4):
    """Scenes of about 80 x 100 in the ShanghaiTech layout (``part_A/<split>_data``) or the UCF-QNRF one (``<Split>``); the
    test scenes are 104 wide, the train scenes 100, and every scene has its own height."""
    generator = np.random.RandomState(seed)
    for split, count, width in (('train', train, 100), ('test', test, 104)):
        folder = os.path.join(directory, 'part_A', split + '_data') if layout == 'shanghai' else \
            os.path.join(directory, split.capitalize())
        for index in range(count):
            shape = (80 + 4 * index, width)
            arrays = {'images': generator.randint(0, 256, size=shape + (3,)).astype(np.uint8),
                      'labels': (generator.rand(*shape) < 0.004).astype(np.float32),
                      'i1nn_maps': generator.rand(*shape).astype(np.float32)}
            for kind, array in arrays.items():
                os.makedirs(os.path.join(folder, kind), exist_ok=True)
                np.save(os.path.join(folder, kind, 'IMG_%d.npy' % index), array)


def crowd_experiment(monkeypatch, directory, layout, **overrides):
    from srgan_amd.settings import Settings
    from srgan_amd.crowd.srgan import CrowdExperiment
    from srgan_amd.utility import SummaryWriter, seed_all
    monkeypatch.setenv('SRGAN_CROWD_DATABASE', str(directory))
    if layout == 'shanghai':
        monkeypatch.setenv('SRGAN_CROWD_DATABASE_PART', 'part_A')
    else:
        monkeypatch.delenv('SRGAN_CROWD_DATABASE_PART', raising=False)
    settings = Settings()
    values = dict(batch_size=50, image_patch_size=64, test_sliding_window_size=32, labeled_dataset_size=2,
                  unlabeled_dataset_size=3, test_summary_size=None, matching_loss_multiplier=1e3,
                  contrasting_loss_multiplier=1e2, gradient_penalty_multiplier=1e2, map_multiplier=1e-3)
    for key, value in dict(values, **overrides).items():
        setattr(settings, key, value)
    experiment = CrowdExperiment(settings)
    experiment.dataset_setup()
    seed_all(0)
    experiment.model_setup()
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    experiment.train_mode()
    return experiment


def last_scalars(writer):
    return {tag: values[-1][1] for tag, values in writer.scalars.items()}


def check_against_the_host_epoch(experiment):
    """Every ``1 Validation Error/*`` / ``2 Train Error/*`` scalar of both writers against the host ``evaluation_epoch`` fed
    the very same patches (downloaded through ``__getitem__``): rtol 2e-9 (n * 2^-53 at n = 2^24, above any n here); for ME,
    whose terms cancel, 2e-9 of the MAE instead."""
    from srgan_amd.utility import SummaryWriter
    host_sets = {}
    for name in ('train_dataset', 'validation_dataset'):
        dataset = getattr(experiment, name)
        assert len(dataset) == 150 and len(list(dataset.device_batches())) == 3
        host_sets[name] = [tuple(part.cpu() for part in dataset[index]) for index in range(len(dataset))]
        assert tuple(host_sets[name][0][0].shape) == (3, 64, 64) and tuple(host_sets[name][0][2].shape) == (64, 64)
    compared = 0
    dnn_mae = None
    for network, writer in ((experiment.DNN, experiment.dnn_summary_writer), (experiment.D, experiment.gan_summary_writer)):
        logged = last_scalars(writer)
        for summary_name, name in (('2 Train Error', 'train_dataset'), ('1 Validation Error', 'validation_dataset')):
            host_writer = SummaryWriter()
            comparison = dnn_mae if (network is experiment.D and summary_name == '1 Validation Error') else None
            mae = experiment.evaluation_epoch(experiment.settings, network, host_sets[name], host_writer, summary_name,
                                              comparison_value=comparison, shuffle=False)
            if network is experiment.DNN and summary_name == '1 Validation Error':
                dnn_mae = mae
            host = last_scalars(host_writer)
            assert list(host_writer.scalars) == [tag for tag in writer.scalars if tag.startswith(summary_name)]   # same order
            for tag, value in host.items():
                tolerance = 2e-9 * (host[summary_name + '/MAE'] if tag.endswith('/ME') else abs(value))
                print('%s device %.17g host %.17g' % (tag, logged[tag], value))
                assert abs(logged[tag] - value) <= tolerance, (tag, logged[tag], value)
                compared += 1
    assert compared == 4 * 5 + 1


def test_validation_summaries_from_the_resident_database(lib, tmp_path, monkeypatch):
    write_database(str(tmp_path), 'shanghai')
    experiment = crowd_experiment(monkeypatch, tmp_path, 'shanghai', crowd_validation='device', image_summaries=True)
    assert experiment.train_dataset.scenes is experiment.train_dataset_loader                # no second upload
    assert [shape[1] for shape in experiment.validation_dataset.scenes.shapes] == [104, 104]  # the test split
    assert all(flip == 0 for *_, flip in experiment.validation_dataset.draws)
    experiment.eval_mode()
    experiment.validation_summaries(0)
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        for summary_name in ('1 Validation Error', '2 Train Error'):
            for tag in TAGS:
                assert np.isfinite(last_scalars(writer)['%s/%s' % (summary_name, tag)]), (summary_name, tag)
    assert np.isfinite(last_scalars(experiment.gan_summary_writer)['1 Validation Error/Ratio MAE GAN DNN'])
    assert '1 Validation Error/Ratio MAE GAN DNN' not in experiment.dnn_summary_writer.scalars
    assert '0 Test Error/MAE count' in experiment.gan_summary_writer.scalars                 # the full-image summaries stay
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        for tag in ('Real', 'Validation'):
            assert writer.images[tag][1].shape == (3, 200, 332) and np.isfinite(writer.images[tag][1]).all(), tag
    check_against_the_host_epoch(experiment)


def test_without_the_setting_nothing_is_attached(lib, tmp_path, monkeypatch):
    write_database(str(tmp_path), 'shanghai')
    experiment = crowd_experiment(monkeypatch, tmp_path, 'shanghai', batch_size=2)
    assert getattr(experiment, 'train_dataset', None) is None and getattr(experiment, 'validation_dataset', None) is None
    experiment.eval_mode()
    experiment.validation_summaries(0)
    tags = list(experiment.gan_summary_writer.scalars) + list(experiment.dnn_summary_writer.scalars)
    assert tags and all(tag.startswith('0 Test Error/') for tag in tags)


def test_ucf_qnrf_branch(lib, tmp_path, monkeypatch):
    from srgan_amd.crowd.data import CrowdDataset
    write_database(str(tmp_path), 'ucf', train=4)
    experiment = crowd_experiment(monkeypatch, tmp_path, 'ucf', crowd_validation='device', crowd_dataset='UCF QNRF',
                                  labeled_dataset_size=2, unlabeled_dataset_size=None)
    labeled, unlabeled = experiment.train_dataset_loader.shapes, experiment.unlabeled_dataset_loader.shapes
    assert len(labeled) == len(unlabeled) == 2 and not set(labeled) & set(unlabeled)         # every scene has its own height
    assert sorted(labeled + unlabeled) == [(80 + 4 * index, 100) for index in range(4)]
    assert sorted(experiment.validation_dataset.scenes.shapes) == [(80, 104), (84, 104)]      # read from Test
    x, heads, knn = next(iter(experiment.train_dataset_loader))
    u = next(iter(experiment.unlabeled_dataset_loader))[0]
    experiment.gan_training_step(x, (heads, knn), u, 0)
    assert np.isfinite(last_scalars(experiment.gan_summary_writer)['Discriminator/Labeled Loss'])
    experiment.eval_mode()
    experiment.validation_summaries(0)
    assert np.isfinite(last_scalars(experiment.gan_summary_writer)['1 Validation Error/Ratio MAE GAN DNN'])
    assert np.isfinite(last_scalars(experiment.gan_summary_writer)['0 Test Error/MAE count'])     # dataset_class reads Test
    check_against_the_host_epoch(experiment)
    # the enum member selects the branch as the string does, with or without crowd_validation
    by_member = crowd_experiment(monkeypatch, tmp_path, 'ucf', crowd_dataset=CrowdDataset.ucf_qnrf, labeled_dataset_size=2,
                                 unlabeled_dataset_size=None, batch_size=2)
    assert by_member.train_dataset_loader.shapes == labeled and by_member.unlabeled_dataset_loader.shapes == unlabeled
    assert getattr(by_member, 'train_dataset', None) is None


def train_two_iterations(monkeypatch, directory, **overrides):
    from srgan_amd.utility import seed_all
    experiment = crowd_experiment(monkeypatch, directory, 'shanghai', **overrides)
    seed_all(5)                                                     # the host streams of the iteration's draws
    labeled, unlabeled = iter(experiment.train_dataset_loader), iter(experiment.unlabeled_dataset_loader)
    for step in range(2):
        x, heads, knn = next(labeled)
        u = next(unlabeled)[0]
        experiment.dnn_training_step(x, (heads, knn), step)
        experiment.gan_training_step(x, (heads, knn), u, step)
        if step == 0:
            experiment.eval_mode()
            experiment.validation_summaries(step)
            experiment.train_mode()
    torch.cuda.synchronize()
    return experiment


def test_the_evaluation_does_not_perturb_training(lib, tmp_path, monkeypatch):
    write_database(str(tmp_path), 'shanghai')
    without = train_two_iterations(monkeypatch, tmp_path)
    with_validation = train_two_iterations(monkeypatch, tmp_path, crowd_validation='device')
    assert '1 Validation Error/MAE' in with_validation.gan_summary_writer.scalars
    assert '1 Validation Error/MAE' not in without.gan_summary_writer.scalars
    for name in ('D', 'G', 'DNN'):
        a, b = getattr(without, name)._srgan_arena.data, getattr(with_validation, name)._srgan_arena.data
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
