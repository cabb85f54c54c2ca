"""``srgan_image_batch_gather`` and the loader / experiments on top of it, on the device: the copy case bit for bit
against the reference's ``to_normalized_range`` on a CPU fp32 tensor, the resize case against
``torch.nn.functional.interpolate`` of the normalised CPU tensor, argument errors, one epoch of ``ResidentImageLoader``
against ``dataset[i]``, and the driving / age experiments trained and evaluated on the tiny databases of
tests/golden/g15_image_databases.npz."""
import numpy as np
import pytest
import torch

from image_database_fixture import golden, settings_for, write_age_database, write_driving_database
from test_steps_gpu import finish_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope='module')
def fixture():
    return golden()


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def normalised(frames):
    """The reference's item arithmetic on the CPU (utility.py:129-132 after ``.astype(np.float32)``)."""
    return (torch.from_numpy(np.asarray(frames)).float() / 127.5) - 1


def gather(lib, frames, order, first, count, size=None, labels=None, out_examples=None):
    """One launch; the outputs are pre-filled with NaN and may be larger than the batch (``out_examples``)."""
    frames = np.ascontiguousarray(frames)
    assert frames.dtype in (np.uint8, np.float32)
    channels, height, width = frames.shape[1:]
    out_height, out_width = size or (height, width)
    store = torch.from_numpy(frames).cuda()
    device_order = torch.tensor(order, dtype=torch.int32).cuda()
    out = torch.full((out_examples or count, channels, out_height, out_width), float('nan'), device='cuda')
    device_labels = out_labels = None
    if labels is not None:
        device_labels = torch.from_numpy(np.asarray(labels, dtype=np.float32)).cuda()
        out_labels = torch.full((out_examples or count,), float('nan'), device='cuda')
    lib.check(lib.library().srgan_image_batch_gather(
        store.data_ptr(), 0 if frames.dtype == np.uint8 else 1, len(frames), channels, height, width,
        None if labels is None else device_labels.data_ptr(), device_order.data_ptr(), first, count, out_height, out_width,
        out.data_ptr(), None if labels is None else out_labels.data_ptr(), lib.stream_handle()), 'srgan_image_batch_gather')
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if labels is None else out_labels.cpu().numpy()


def test_copy_of_a_uint8_store_is_the_reference_normalisation_bit_for_bit(lib):
    frames = (np.arange(5 * 3 * 6 * 10) % 256).astype(np.uint8).reshape(5, 3, 6, 10)        # every byte value, 3.5 times
    assert len(np.unique(frames)) == 256
    labels = np.linspace(-3.25, 91.5, 5).astype(np.float32)
    order, first, count = [4, 0, 0, 3, 1, 2, 4], 1, 5
    images, out_labels = gather(lib, frames, order, first, count, labels=labels, out_examples=7)
    chosen = order[first:first + count]
    np.testing.assert_array_equal(bits(images[:count]), bits(normalised(frames[chosen]).numpy()))
    np.testing.assert_array_equal(bits(out_labels[:count]), bits(labels[chosen]))
    assert np.isnan(images[count:]).all() and np.isnan(out_labels[count:]).all()            # the tail is untouched
    # without labels, and an index outside [0, count) is clamped instead of read
    images, none = gather(lib, frames, [-7, 99, 2], 0, 3)
    assert none is None
    np.testing.assert_array_equal(bits(images), bits(normalised(frames[[0, 4, 2]]).numpy()))


@pytest.mark.parametrize('shape', [(4, 3, 5, 7), (3, 1, 4, 64), (2, 3, 3, 9), (3, 1, 2, 3)])
def test_copy_of_a_float_store_is_bit_for_bit(lib, shape):
    """Width 7 / 9 / 3: the last run of every row is short and rows start at any element; [1, 4, 64]: whole 16-byte runs."""
    generator = np.random.RandomState(shape[3])
    frames = (generator.rand(*shape) * 255).astype(np.float32)
    labels = generator.randn(shape[0]).astype(np.float32)
    order = list(generator.permutation(shape[0])) + [0]
    images, out_labels = gather(lib, frames, order, 1, shape[0], labels=labels, out_examples=shape[0] + 1)
    chosen = order[1:]
    np.testing.assert_array_equal(bits(images[:-1]), bits(normalised(frames[chosen]).numpy()))
    np.testing.assert_array_equal(bits(out_labels[:-1]), bits(labels[chosen]))
    assert np.isnan(images[-1]).all() and np.isnan(out_labels[-1])


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('stored, size', [((8, 8), (16, 16)), ((8, 8), (4, 12)), ((5, 7), (9, 6)), ((16, 16), (14, 14)),
                                          ((6, 10), (6, 10))])
def test_resize_equals_torch_interpolate_of_the_normalised_frames(lib, stored, size, dtype):
    """Bound: 4 ulp of the largest input magnitude, the rule of test_resize_bilinear_equals_torch_cpu -- the four taps are
    exact inputs, the two horizontal blends and the vertical one round once per product and sum."""
    generator = np.random.RandomState(stored[0] * 100 + size[1])
    frames = generator.rand(6, 3, *stored) * 255
    frames = frames.astype(np.float32) if dtype is np.float32 else np.round(frames).astype(np.uint8)
    order = [5, 1, 1, 0, 3]
    got, _ = gather(lib, frames, order, 0, len(order), size=size)
    source = normalised(frames[order])
    expected = torch.nn.functional.interpolate(source, size=size, mode='bilinear', align_corners=False,
                                               antialias=False).numpy()
    ulp = float(np.spacing(np.abs(source.numpy()).max()))            # one ulp of the largest input magnitude
    error = float(np.abs(got - expected).max())
    print(f'{dtype.__name__} {stored} -> {size}: max |difference| {error:.3e} = {error / ulp:.2f} ulp of the largest input; '
          f'{(got == expected).mean():.3f} of the outputs exact')
    assert got.shape == expected.shape and error <= 4 * ulp
    if stored == size:
        np.testing.assert_array_equal(bits(got), bits(source.numpy()))                      # the identity: the copy case


def test_argument_errors_launch_nothing(lib):
    library = lib.library()
    out = torch.full((4, 3, 8, 8), float('nan'), device='cuda')
    store = torch.zeros((5, 3, 8, 8), dtype=torch.uint8, device='cuda')
    order = torch.zeros(4, dtype=torch.int32, device='cuda')

    def call(store_pointer, dtype, count):
        return library.srgan_image_batch_gather(store_pointer, dtype, 5, 3, 8, 8, None, order.data_ptr(), 0, count, 8, 8,
                                                out.data_ptr(), None, lib.stream_handle())
    for arguments in ((None, 0, 4), (store.data_ptr(), 0, 0), (store.data_ptr(), 7, 4)):
        assert call(*arguments) == lib.EINVAL, arguments
        assert b'srgan_image_batch_gather' in library.srgan_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(store.data_ptr(), 0, 4) == 0
    torch.cuda.synchronize()
    assert bool((out == -1).all())


@pytest.fixture(scope='module')
def databases(fixture, tmp_path_factory):
    root = tmp_path_factory.mktemp('image_databases')
    return {'driving': write_driving_database(fixture, root / 'driving'), 'age': write_age_database(fixture, root / 'age')}


def test_one_epoch_of_the_loader_is_the_dataset_in_the_permutations_order(lib, fixture, databases):
    from srgan_amd.data import ResidentImageDataset, ResidentImageLoader
    from srgan_amd.driving.data import driving_datasets
    datasets = list(driving_datasets(databases['driving'], settings_for(fixture, 'A')))
    datasets.append(ResidentImageDataset(fixture['driving/frames'], fixture['driving/angles']))           # 23: five batches
    for dataset in datasets:
        loader = ResidentImageLoader(dataset, 4, seed=9)
        for epoch in range(2):
            batches = list(loader)
            order = loader._order.cpu().tolist()
            assert len(batches) == len(dataset) // 4 and sorted(order) == list(range(len(dataset)))
            for number, (images, labels) in enumerate(batches):
                assert images.dtype == labels.dtype == torch.float32 and images.is_cuda and labels.is_cuda
                assert tuple(images.shape) == (4, 3, 8, 8) and tuple(labels.shape) == (4,)
                for position, index in enumerate(order[4 * number:4 * number + 4]):
                    image, label = dataset[index]
                    assert torch.equal(images[position].cpu(), image), (epoch, number, position)          # bit for bit
                    assert float(labels[position]) == float(label)
        walked = list(loader.in_order())
        assert [len(images) for images, _ in walked] == [4] * (len(dataset) // 4) + ([len(dataset) % 4] if len(dataset) % 4 else [])
        stacked = torch.cat([images for images, _ in walked]).cpu()
        assert torch.equal(stacked, torch.stack([dataset[index][0] for index in range(len(dataset))]))
    resized = ResidentImageLoader(datasets[0], 4, image_size=(4, 12), seed=9)
    images, labels = next(iter(resized))
    assert tuple(images.shape) == (4, 3, 4, 12) and bool(torch.isfinite(images).all())
    source = torch.stack([datasets[0][index][0] for index in resized._order.cpu().tolist()[:4]])
    expected = torch.nn.functional.interpolate(source, size=(4, 12), mode='bilinear', align_corners=False)
    assert float((images.cpu() - expected).abs().max()) <= 4 * float(np.spacing(source.abs().max().numpy()))


def run_experiment(experiment_class, fixture, size, step_graph, steps=3):
    """``steps`` training iterations on one stream from the experiment's own loaders (batch 4: every epoch of the five
    labeled examples is one batch, so the loaders are re-iterated), then the validation summaries."""
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all
    settings = Settings()
    for name, value in vars(settings_for(fixture, 'A')).items():
        setattr(settings, name, value)
    settings.matching_loss_multiplier, settings.contrasting_loss_multiplier = 1e2, 1e1
    settings.gradient_penalty_multiplier = 1e2
    settings.step_graph, settings.step_graph_warmup, settings.steps_to_run = step_graph, 1, 10 ** 9
    experiment = experiment_class(settings)
    experiment.image_size = size
    seed_all(0)
    experiment.dataset_setup()
    experiment.model_setup()
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    finish_setup(experiment)
    for optimizer in (experiment.d_optimizer, experiment.g_optimizer, experiment.dnn_optimizer):
        optimizer.count_on_device()              # both runs through the device-counted Adam entry point, as a capture needs
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.summary_period, writer.steps_to_run = 10 ** 9, 10 ** 9
    seed_all(5)                                  # the host streams the noise draws come from
    labeled = experiment.infinite_iter(experiment.train_dataset_loader)
    unlabeled = experiment.infinite_iter(experiment.unlabeled_dataset_loader)
    losses = []
    for step in range(1, steps + 1):
        examples, labels = next(labeled)
        assert tuple(examples.shape) == (4, 3) + ((size, size) if isinstance(size, int) else tuple(size))
        experiment.training_iteration(examples, labels, next(unlabeled)[0], step)
        losses.append({name: float(value.item()) for name, value in experiment.last_losses.items() if value is not None})
    torch.cuda.synchronize()
    return experiment, losses


def check_summaries(experiment, sizes):
    """The logged MAEs against ``network(in_order batches)`` computed here, over every example of the split."""
    from srgan_amd.srgan import as_var
    from srgan_amd.tape import no_grad
    experiment.eval_mode()
    with no_grad():
        experiment.validation_summaries(0)
        for tag, loader, size in (('1 Validation Error/MAE', experiment.validation_dataset_loader, sizes[1]),
                                  ('2 Train Error/MAE', experiment.train_dataset_loader, sizes[0])):
            for network, writer in ((experiment.D, experiment.gan_summary_writer), (experiment.DNN, experiment.dnn_summary_writer)):
                predictions, labels = [], []
                for images, batch_labels in loader.in_order():
                    predictions.append(network(as_var(images)).cpu().numpy().reshape(-1).astype(np.float64))
                    labels.append(batch_labels.cpu().numpy().astype(np.float64))
                predictions, labels = np.concatenate(predictions), np.concatenate(labels)
                assert len(predictions) == len(labels) == size == len(loader.dataset)     # the split, not a multiple of the batch
                np.testing.assert_array_equal(labels.astype(np.float32), loader.dataset.labels)
                mae = float(np.abs(predictions - labels).mean())
                logged = writer.scalars[tag][-1][1]
                print(f'{tag}: logged {logged!r} computed {mae!r} over {size} examples')
                assert np.isfinite(mae) and abs(logged - mae) <= 1e-6 * abs(mae)


def test_driving_trains_and_validates_on_a_database(lib, fixture, databases, monkeypatch):
    from srgan_amd.driving.srgan import DrivingExperiment
    from srgan_amd.data import ResidentImageLoader
    monkeypatch.setenv('SRGAN_DRIVING_DATABASE', databases['driving'])
    eager, eager_losses = run_experiment(DrivingExperiment, fixture, 16, step_graph=False)
    assert isinstance(eager.train_dataset_loader, ResidentImageLoader)
    assert all(np.isfinite(value) for step in eager_losses for value in step.values()) and len(eager_losses[-1]) >= 5
    assert eager_losses[-1] != eager_losses[-2]
    replayed, replayed_losses = run_experiment(DrivingExperiment, fixture, 16, step_graph=True)
    captured = replayed._captured_iteration
    assert captured.eager_iterations == 1 and captured.replays == 2
    assert eager_losses == replayed_losses
    for name in ('D', 'DNN', 'G'):
        a, b = getattr(eager, name)._srgan_arena.data, getattr(replayed, name)._srgan_arena.data
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    check_summaries(eager, sizes=(5, 4))
    assert '1 Validation Error/NMAE' in eager.gan_summary_writer.scalars
    assert '1 Validation Error/Ratio MAE GAN DNN' in eager.gan_summary_writer.scalars


def test_driving_trains_on_rectangular_frames_resampled_by_the_loader(lib, fixture, databases, monkeypatch):
    """8 x 8 stored frames delivered as 16 x 48: one axis of the driving shape's ratio each way is in the kernel test; here
    the experiment's own ``image_size`` pair reaches the loader."""
    from srgan_amd.driving.srgan import DrivingExperiment
    monkeypatch.setenv('SRGAN_DRIVING_DATABASE', databases['driving'])
    experiment, losses = run_experiment(DrivingExperiment, fixture, (16, 48), step_graph=False, steps=1)
    assert all(np.isfinite(value) for value in losses[-1].values())


def test_age_trains_and_validates_on_a_database_of_images(lib, fixture, databases, monkeypatch):
    import srgan_amd.age.srgan as age
    from srgan_amd.age.srgan import AgeExperiment
    monkeypatch.setattr(age, 'model_architecture', 'dcgan')
    monkeypatch.setenv('SRGAN_AGE_DATABASE', databases['age'])
    experiment, losses = run_experiment(AgeExperiment, fixture, 16, step_graph=False)
    assert experiment.train_dataset.images.dtype == np.uint8
    assert all(np.isfinite(value) for step in losses for value in step.values()) and len(losses[-1]) >= 5
    check_summaries(experiment, sizes=(5, 4))
