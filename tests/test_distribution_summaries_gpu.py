"""Distribution summaries on the MI355X (settings.distribution_summaries; csrc/distribution_summaries.hip):
``srgan_wasserstein_1d``, ``srgan_kde_curves`` and ``srgan_curve_frame`` against scipy and the tests' NumPy restatement
(distribution_summaries_reference.py, pinned on the CPU against scipy, hand-written frames and the reference's own summary step
in golden g18), the composed ``Distributions`` frame, and the summaries of tiny coefficient experiments -- the reference's logged
Wasserstein scalar, tags and shapes, and that switching the summaries on leaves the training bits alone.

Outputs are pre-filled with NaN and sit between NaN guards at a start that is not 16-byte aligned: every output element is
written exactly once and nothing else is.  Bounds that the precision of fp32 sets are taken from the float32 restatement's own
distance to scipy on the same inputs, computed here; every test prints the observed figures before it asserts."""
import datetime
import os

import numpy as np
import pytest
import torch
from scipy.stats import gaussian_kde, wasserstein_distance

import distribution_summaries_reference as R
from helpers import load_golden, golden_state
from test_steps_gpu import finish_setup

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 5                                   # floats of NaN on either side of an output (an odd count: an unaligned start)
FRAME_SETS = ('fake_coefficients', 'unlabeled_predictions', 'gan_validation', 'gan_train', 'dnn_validation', 'dnn_train')
TAG = 'Generator/Predicted Label Wasserstein'


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    _lib.library()
    return _lib


@pytest.fixture(scope='module')
def module():
    import srgan_amd  # noqa: F401
    from srgan_amd import distribution_summaries
    return distribution_summaries


@pytest.fixture(scope='module')
def g18():
    return load_golden('g18_coefficient_distributions')


def guarded(count):
    return torch.full((count + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')


def unguard(buffer, shape):
    host = buffer.cpu().numpy()
    count = int(np.prod(shape, dtype=np.int64))
    assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + count:]).all(), 'a write outside the output'
    return host[GUARD:GUARD + count].reshape(shape)


def dev(array, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype)).cuda()


# ---- the Wasserstein distance ------------------------------------------------------------------------------------------------
def device_wasserstein(lib, u, v):
    buffer = guarded(1)
    du, dv = dev(u), dev(v)
    lib.check(lib.library().srgan_wasserstein_1d(du.data_ptr(), len(u), dv.data_ptr(), len(v), buffer.data_ptr() + 4 * GUARD,
                                                 lib.stream_handle()), 'srgan_wasserstein_1d')
    return unguard(buffer, (1,))[0]


@pytest.mark.parametrize('levels', [1024, 3], ids=['spread', 'tied'])
@pytest.mark.parametrize('n, m', [(1, 1), (2, 2), (32, 32), (64, 1), (512, 512), (1024, 1), (8192, 8192)])
def test_wasserstein_is_exact_on_dyadic_values(lib, module, n, m, levels):
    """Multiples of 2^-8 in [-4, 4] and power-of-two counts: every product and partial sum is exact in fp32, so the result is
    scipy's rounded to fp32, bit for bit.  ``tied``: seven distinct values, shared by the two sets."""
    if (n, m) == (8192, 8192):
        assert n + m == module.WASSERSTEIN_MAX_VALUES                               # the capacity itself
    generator = np.random.RandomState(n + 3 * m + levels)
    scale = 1024 // levels
    u = (generator.randint(-levels, levels + 1, size=n) * scale / 256.0).astype(np.float32)
    v = (generator.randint(-levels, levels + 1, size=m) * scale / 256.0).astype(np.float32)
    expected = np.float32(wasserstein_distance(u.astype(np.float64), v.astype(np.float64)))
    got = device_wasserstein(lib, u, v)
    print(f'wasserstein exact n={n} m={m} levels={levels}: device {got!r} scipy {expected!r}')
    assert got.view(np.uint32) == expected.view(np.uint32)
    assert R.wasserstein32(u, v).view(np.uint32) == expected.view(np.uint32)        # the restated tree is exact too


@pytest.mark.parametrize('n, m', [(3, 5), (37, 100), (1000, 1000)])
def test_wasserstein_on_ragged_sets(lib, n, m):
    """Normal against uniform samples.  Bound: 8 x the error of the float32 restatement (sorted values, the kernel's summation
    tree) against scipy on the same inputs; the margin covers a different but fixed tree."""
    generator = np.random.RandomState(100 * n + m)
    u = generator.normal(0.3, 0.8, size=n).astype(np.float32)
    v = generator.uniform(-2, 2, size=m).astype(np.float32)
    expected = wasserstein_distance(u.astype(np.float64), v.astype(np.float64))
    restated = R.wasserstein32(u, v)
    got, again = device_wasserstein(lib, u, v), device_wasserstein(lib, u, v)
    bound = 8 * abs(float(restated) - expected)
    print(f'wasserstein ragged n={n} m={m}: device error {abs(float(got) - expected):.3e}, restatement error '
          f'{abs(float(restated) - expected):.3e}, bound {bound:.3e}, same bits as the restatement: '
          f'{got.view(np.uint32) == restated.view(np.uint32)}')
    assert np.isfinite(got) and got.view(np.uint32) == again.view(np.uint32)
    assert abs(float(got) - expected) <= bound


# ---- the kernel-density curves -----------------------------------------------------------------------------------------------
def device_curves(lib, sets, gridsize, factor=0.1, cut=3.0):
    count = len(sets)
    samples = dev(np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in sets]))
    offsets = dev(np.concatenate([[0], np.cumsum([np.size(x) for x in sets])]), np.int32)
    buffers = [guarded(count * gridsize), guarded(count * gridsize), guarded(count * 4)]
    lib.check(lib.library().srgan_kde_curves(samples.data_ptr(), offsets.data_ptr(), count, gridsize, factor, cut,
                                             *(buffer.data_ptr() + 4 * GUARD for buffer in buffers), lib.stream_handle()),
              'srgan_kde_curves')
    return unguard(buffers[0], (count, gridsize)), unguard(buffers[1], (count, gridsize)), unguard(buffers[2], (count, 4))


def scipy_density(x, gridsize, factor=0.1, cut=3):
    x = np.asarray(x, dtype=np.float64)
    h = factor * x.std(ddof=1)
    support = np.linspace(x.min() - cut * h, x.max() + cut * h, gridsize)
    return support, gaussian_kde(x, bw_method=factor)(support), h


# |h / h_numpy - 1|: M2 passes through at most 4 Welford updates and 8 merges of the fixed tree, each a handful of fp32
# roundings (2^-24 relative each, on a sum of non-negative terms), the square root halves the total, and 0.1f is 1.5e-8 off 0.1
H_TOLERANCE = 64 * 2.0 ** -24


def check_curves(got, sets, expected_curves, what):
    """Rows against scipy in float64, relative to each curve's maximum; bound: 10 x the float32 restatement's own error."""
    support, density, stats = got
    gridsize = support.shape[1]
    restated = R.kde_curves(sets, gridsize, dtype=np.float32)
    assert np.isfinite(support).all() and np.isfinite(density).all() and np.isfinite(stats).all()
    for c, x in enumerate(sets):
        x = np.asarray(x, dtype=np.float32)
        assert stats[c, 0] == x.size
        assert (stats[c, 1], stats[c, 2]) == ((x.min(), x.max()) if x.size else (0.0, 0.0))
        if expected_curves[c] is None:                                                 # cannot be fitted
            assert stats[c, 3] == 0 and not support[c].any() and not density[c].any(), (what, c)
            continue
        expected_support, expected_density, h = expected_curves[c]
        peak = expected_density.max()
        error = np.abs(density[c] - expected_density).max() / peak
        own = np.abs(restated[1][c] - expected_density).max() / peak
        print(f'{what} curve {c} ({x.size} samples, G={gridsize}): device error {error:.3e} of the maximum, restatement error '
              f'{own:.3e}, h off by {abs(stats[c, 3] / h - 1):.3e}')
        assert abs(stats[c, 3] / h - 1) <= H_TOLERANCE, (what, c)
        # lo, top, top - lo, the division, g * step and the sum: ten roundings of quantities up to 2 max|s|, and 3 h of h's own
        assert np.abs(support[c] - expected_support).max() <= 16 * 2.0 ** -24 * np.abs(expected_support).max() + 4 * abs(h) * \
            H_TOLERANCE, (what, c)
        assert error <= 10 * own, (what, c, error, own)


@pytest.mark.parametrize('gridsize', [2, 100, 130])
def test_kde_curves_of_many_sizes_in_one_call(lib, gridsize):
    generator = np.random.RandomState(11)
    sets = [generator.normal(0.3, 0.8, size=size).astype(np.float32) for size in (2, 7, 64, 65, 257, 1000)]
    sets.insert(3, np.array([1.25], dtype=np.float32))                                 # one sample: cannot be fitted
    sets.insert(4, np.full(9, -0.5, dtype=np.float32))                                 # no spread: cannot be fitted
    for x in sets:
        assert np.abs(x).max() <= 4 and (x.size < 2 or x.std(ddof=1) == 0 or x.std(ddof=1) >= 0.05)
    expected = [None if c in (3, 4) else scipy_density(x, gridsize) for c, x in enumerate(sets)]
    got = device_curves(lib, sets, gridsize)
    check_curves(got, sets, expected, 'kde')
    again = device_curves(lib, sets, gridsize)
    for first, second in zip(got, again):
        assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


def test_kde_curves_of_the_references_arrays(lib, g18):
    sets = [g18[name].astype(np.float32) for name in FRAME_SETS]
    expected = [(g18[f'kde/{name}/support'], g18[f'kde/{name}/density'], 0.1 * g18[name].astype(np.float64).std(ddof=1))
                for name in FRAME_SETS]
    check_curves(device_curves(lib, sets, 100), sets, expected, 'g18')


# ---- the frame ---------------------------------------------------------------------------------------------------------------
def frame_case():
    """Polylines over x in [-4, 4], y in [0, 1]: a step with vertical edges, one with a duplicate vertex, one that leaves the
    top, a single vertex (skipped), and two curves that overlap, so that the order matters."""
    x = np.linspace(-3.5, 3.5, 29)
    polylines = [
        [(-4, 0), (-2, 0), (-2, 0.5), (-1, 0.5), (-1, 0), (4, 0)],
        [(-3, 0.9), (-1, 0.7), (-1, 0.7), (0.5, 0.8), (0.5, 0.8), (3, 0.1)],
        [(-3.7, 0.2), (-0.3, 3.0), (2.2, -0.4)],
        [(0.0, 0.5)],
        np.stack([x, 0.6 * np.exp(-0.5 * x ** 2)], axis=1),
        np.stack([x, 0.6 * np.exp(-0.5 * (x - 0.4) ** 2)], axis=1),
    ]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in polylines])]).astype(np.int32)
    vertices = np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in polylines])
    colours = np.array([(0.3, 0.45, 0.69), (0.87, 0.52, 0.32), (0.33, 0.66, 0.41), (1, 0, 0), (0.77, 0.31, 0.32), (0.5, 0.45, 0.7)],
                       dtype=np.float32)
    widths = np.array([2.0, 1.0, 3.5, 2.0, 2.5, 0.7], dtype=np.float32)
    return vertices, offsets, colours, widths


@pytest.mark.parametrize('height, width', [(48, 64), (33, 50)])
def test_curve_frame_against_the_restatement(lib, height, width):
    vertices, offsets, colours, widths = frame_case()
    background, grid = np.array([0.918, 0.918, 0.949], dtype=np.float32), np.ones(3, dtype=np.float32)
    x_ticks, y_ticks = np.arange(-4, 5, dtype=np.float32), (np.arange(6) * 0.2).astype(np.float32)
    buffer = guarded(3 * height * width)
    held = [dev(vertices), dev(offsets, np.int32), dev(colours), dev(widths), dev(background), dev(grid), dev(x_ticks), dev(y_ticks)]
    lib.check(lib.library().srgan_curve_frame(held[0].data_ptr(), held[1].data_ptr(), len(offsets) - 1, held[2].data_ptr(),
                                              held[3].data_ptr(), height, width, -4.0, 4.0, 0.0, 1.0, held[4].data_ptr(),
                                              held[5].data_ptr(), held[6].data_ptr(), len(x_ticks), held[7].data_ptr(),
                                              len(y_ticks), buffer.data_ptr() + 4 * GUARD, lib.stream_handle()),
              'srgan_curve_frame')
    got = unguard(buffer, (3, height, width))
    expected = R.curve_frame(vertices, offsets, colours, widths, height, width, (-4, 4), (0, 1), background, grid, x_ticks, y_ticks)
    check_frame(got, expected, f'frame {height} x {width}')
    # the order matters: the two overlapping curves swapped give another picture
    swapped = R.curve_frame(vertices, offsets, colours[[0, 1, 2, 3, 5, 4]], widths, height, width, (-4, 4), (0, 1), background, grid,
                            x_ticks, y_ticks)
    assert np.abs(swapped - expected).max() > 0.1


def check_frame(got, expected, what):
    """The project's parity tolerance 1e-3, and no 8-bit level more than one off."""
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    levels = np.abs(np.round(got.astype(np.float64) * 255) - np.round(expected * 255))
    print(f'{what}: largest difference {np.abs(got - expected).max():.3e}, {int((levels > 0).sum())} of {levels.size} values on '
          f'another 8-bit level, at most {int(levels.max())} off')
    assert np.abs(got - expected).max() <= 1e-3
    assert levels.max() <= 1


# ---- the module --------------------------------------------------------------------------------------------------------------
def test_the_module_takes_device_tensors_only(lib, module):
    with pytest.raises(lib.HipLibraryError):
        module.wasserstein_distance(torch.zeros(3), torch.zeros(4).cuda())
    with pytest.raises(lib.HipLibraryError):
        module.kde_curves([torch.zeros(3).cuda(), torch.zeros(3)])
    u, v = np.array([0.0, 1.0, 3.0], dtype=np.float32), np.array([5.0, 6.0, 8.0], dtype=np.float32)
    distance = module.wasserstein_distance(dev(u), dev(v))
    assert distance.is_cuda and distance.dim() == 0 and float(distance) == 5.0
    support, density, stats = module.kde_curves([dev(u), dev(v)], gridsize=7)
    assert support.shape == density.shape == (2, 7) and stats.shape == (2, 4) and stats[:, 0].tolist() == [3.0, 3.0]


def test_the_distribution_frame_of_the_references_arrays(lib, module, g18):
    sets = [g18[name] for name in FRAME_SETS]
    got = module.distribution_frame(*(dev(x) for x in sets))
    assert got.is_cuda and got.shape == (3, 480, 640)
    expected = R.distribution_frame(module, [np.asarray(x, dtype=np.float32) for x in sets])
    check_frame(got.cpu().numpy(), expected, 'distribution frame')
    assert np.abs(expected - module.DARKGRID_BACKGROUND[:, None, None]).max() > 0.3   # something is drawn
    # a set that cannot be fitted is left out, as the reference leaves it out
    without = module.distribution_frame(dev(np.zeros(4)), *(dev(x) for x in sets[1:])).cpu().numpy()
    expected = R.distribution_frame(module, [np.zeros(4, dtype=np.float32)] + [np.asarray(x, dtype=np.float32) for x in sets[1:]])
    check_frame(without, expected, 'distribution frame without the fake curve')
    coefficients = module.fake_coefficients(dev(g18['fake_examples'])).cpu().numpy()
    assert coefficients.shape == (4,) and np.abs(coefficients - g18['fake_coefficients']).max() <= 1e-5


# ---- the experiments ---------------------------------------------------------------------------------------------------------
def coefficient_experiment(g18, experiment_class=None, **overrides):
    """The coefficient experiment at the sizes of golden g18 (hidden 10, batch 64, labeled 32, unlabeled 256, validation 64)."""
    from srgan_amd.coefficient.srgan import CoefficientExperiment
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all
    settings = Settings()
    for key in ('batch_size', 'hidden_size', 'labeled_dataset_size', 'unlabeled_dataset_size', 'validation_dataset_size',
                'labeled_dataset_seed', 'mean_offset'):
        setattr(settings, key, int(g18[key]))
    for key, value in dict(steps_to_run=10 ** 9, summary_step_period=1, pin_memory=False, **overrides).items():
        setattr(settings, key, value)
    experiment = (experiment_class or CoefficientExperiment)(settings)
    seed_all(0)
    experiment.dataset_setup()
    experiment.model_setup()
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    return experiment


def summary_step(experiment, step):
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.step = step
    experiment.end_of_step(step, experiment.gan_summary_writer, datetime.datetime.now())
    torch.cuda.synchronize()


def value_predictions(experiment, examples):
    from srgan_amd.srgan import as_var
    from srgan_amd.tape import no_grad
    with no_grad():
        return experiment.predicted_values(experiment.D, as_var(examples)).data.cpu().numpy()


def generated_examples(experiment, z):
    from srgan_amd.srgan import as_var
    from srgan_amd.tape import no_grad
    with no_grad():
        return experiment.G(as_var(torch.from_numpy(z))).data


def test_the_coefficient_experiment_logs_the_references_scalar_and_frame(lib, module, g18):
    experiment = coefficient_experiment(g18, distribution_summaries=True)
    assert np.array_equal(experiment.unlabeled_dataset.labels[:64], g18['unlabeled_labels'])
    for name in ('D', 'DNN', 'G'):
        getattr(experiment, name).load_state_dict(golden_state(g18, f'weights/{name}'))
    finish_setup(experiment)
    experiment.injected_draws = {'z_summary': torch.from_numpy(g18['z'])}
    host_stream = np.random.get_state()[1].copy()
    summary_step(experiment, int(g18['step']))
    assert np.array_equal(np.random.get_state()[1], host_stream)                      # the injected z was used: no draw
    logged = experiment.gan_summary_writer.scalars[TAG]
    assert len(logged) == 1 and logged[0][0] == int(g18['step']) and TAG not in experiment.dnn_summary_writer.scalars
    # the ragged rule on the inputs the kernel saw, against the value the reference logged
    predicted = value_predictions(experiment, generated_examples(experiment, g18['z']))
    labels = g18['unlabeled_labels'].astype(np.float32)
    own = abs(float(R.wasserstein32(predicted, labels)) - wasserstein_distance(predicted.astype(np.float64), labels.astype(np.float64)))
    print(f'experiment: logged {logged[0][1]!r}, reference {float(g18["wasserstein"])!r}, difference '
          f'{abs(logged[0][1] - float(g18["wasserstein"])):.3e}, restatement error {own:.3e}')
    assert abs(logged[0][1] - float(g18['wasserstein'])) <= 8 * own
    step, image = experiment.gan_summary_writer.images['Distributions']
    assert step == int(g18['step']) and image.shape == (3, 480, 640) and image.dtype == np.float32
    assert experiment.dnn_summary_writer.images == {}
    expected = R.distribution_frame(module, [g18[name].astype(np.float32) for name in FRAME_SETS])
    print(f'experiment frame: largest difference from the frame of the reference\'s arrays {np.abs(image - expected).max():.3e}')
    assert np.isfinite(image).all() and np.abs(image - expected).mean() <= 1e-3        # the predictions are the device's own
    # without an injected z the summary draws it from NumPy's global stream, as the reference does
    summary_step(experiment, int(g18['step']) + 1)
    assert not np.array_equal(np.random.get_state()[1], host_stream) and len(experiment.gan_summary_writer.scalars[TAG]) == 2


def test_the_dggan_experiment_logs_the_same_tags(lib, module, g18):
    from srgan_amd.coefficient.dggan import CoefficientDgganExperiment
    experiment = coefficient_experiment(g18, CoefficientDgganExperiment, distribution_summaries=True)
    finish_setup(experiment)
    z = np.random.RandomState(3).normal(size=(64, 10)).astype(np.float32)
    experiment.injected_draws = {'z_summary': torch.from_numpy(z)}
    summary_step(experiment, 4)
    logged = experiment.gan_summary_writer.scalars[TAG]
    predicted = value_predictions(experiment, generated_examples(experiment, z))
    labels = experiment.unlabeled_dataset.labels[:64].astype(np.float32)
    expected = wasserstein_distance(predicted.astype(np.float64), labels.astype(np.float64))
    own = abs(float(R.wasserstein32(predicted, labels)) - expected)
    print(f'dggan: logged {logged[0][1]!r}, scipy {expected!r}, restatement error {own:.3e}')
    assert len(logged) == 1 and logged[0][0] == 4 and abs(logged[0][1] - expected) <= 8 * own
    step, image = experiment.gan_summary_writer.images['Distributions']
    assert step == 4 and image.shape == (3, 480, 640) and np.isfinite(image).all()
    assert '1 Validation Error/Ratio MAE GAN DNN' in experiment.gan_summary_writer.scalars


def train_two_iterations(g18, **overrides):
    """Two iterations on the recorded batches and draws of golden g3b, a summary step after each."""
    from srgan_amd.utility import seed_all
    g3b = load_golden('g3b_coefficient_srgan_gp_active')
    experiment = coefficient_experiment(g18, **overrides)
    for module, prefix in ((experiment.D, 'init/D'), (experiment.DNN, 'init/DNN'), (experiment.G, 'init/G')):
        module.load_state_dict(golden_state(g3b, prefix))
    finish_setup(experiment)
    seed_all(5)
    for step in range(2):
        x, y, u = (dev(g3b[f's{step}/{k}']) for k in ('x', 'y', 'u'))
        experiment.injected_draws = {k: torch.from_numpy(g3b[f's{step}/{k}']) for k in ('z_d', 'z_g', 'alpha')}
        experiment.training_iteration(x, y, u, step)
        for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
            writer.step = step
        experiment.end_of_step(step, experiment.gan_summary_writer, datetime.datetime.now())
    torch.cuda.synchronize()
    return experiment


def test_the_summaries_do_not_perturb_training_and_are_off_by_default(lib, g18, monkeypatch):
    """With z_D, alpha and z_G injected the extra NumPy draw of the summary cannot shift them: the same weights, bit for bit.
    With the switch off: no new tag, no picture, no launch of the three entry points, no draw from NumPy's stream."""
    from srgan_amd import functional as F
    launched = []
    original = F._call
    monkeypatch.setattr(F, '_call', lambda name, *arguments: (launched.append(name), original(name, *arguments))[1])
    without = train_two_iterations(g18)
    assert not hasattr(without.settings, 'distribution_summaries') and not without.distribution_summaries_on()
    host_stream_after = np.random.get_state()
    new = {'srgan_wasserstein_1d', 'srgan_kde_curves', 'srgan_curve_frame'}
    assert not new & set(launched) and TAG not in without.gan_summary_writer.scalars and without.gan_summary_writer.images == {}
    launches_without = len(launched)
    np.random.seed(5)
    reference_stream = np.random.get_state()[1].copy()
    assert np.array_equal(host_stream_after[1], reference_stream) and host_stream_after[2] == np.random.get_state()[2]
    del launched[:]
    with_summaries = train_two_iterations(g18, distribution_summaries=True)
    assert new <= set(launched) and len(launched) > launches_without
    assert len(with_summaries.gan_summary_writer.scalars[TAG]) == 2 and with_summaries.gan_summary_writer.images['Distributions'][0] == 1
    for name in ('D', 'G', 'DNN'):
        first, second = getattr(without, name).state_dict(), getattr(with_summaries, name).state_dict()
        for key in first:
            assert torch.equal(first[key], second[key]), (name, key)
    scalars = {tag: values for tag, values in with_summaries.gan_summary_writer.scalars.items() if tag != TAG}
    assert scalars == without.gan_summary_writer.scalars
