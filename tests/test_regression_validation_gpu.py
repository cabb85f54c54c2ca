"""Age / driving validation summaries on the GPU: ``srgan_regression_evaluation_sums`` bit for bit against the NumPy
restatement on inputs whose sums are exact in fp64 (one row to more rows than threads, class logits with bins, padded rows,
a record that already holds a batch, the label extremes in the first row, the last row and the last wave, ties, infinities),
the rounded square, normal inputs within the summation-order bound; and the experiments on the tiny databases of
tests/golden/g15_image_databases.npz: the device path's scalars against the host path's, its one 256-byte download, the age
SGAN's summary step on both paths, training bits that do not move with the attribute, and an fp16 run evaluated on its own
data path."""
import numpy as np
import pytest
import torch

from crowd_validation_reference import contraction_cases
from image_database_fixture import golden, settings_for, write_age_database, write_driving_database
from regression_validation_reference import EMPTY_RECORD, evaluation_scalars, evaluation_sums, order_bounds
from test_steps_gpu import finish_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def device_sums(lib, predictions, row_stride, K, bins, labels, sums=None):
    """One call on uploaded copies; ``sums``: a device tensor to update (default: a new empty record)."""
    upload = lambda array: None if array is None else torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32).reshape(-1)).cuda()
    tensors = [upload(predictions), upload(bins), upload(labels)]
    if sums is None:
        sums = torch.tensor(EMPTY_RECORD, dtype=torch.float64, device='cuda')
    pointer = lambda tensor: None if tensor is None else tensor.data_ptr()
    lib.check(lib.library().srgan_regression_evaluation_sums(
        pointer(tensors[0]), row_stride, K, pointer(tensors[1]), pointer(tensors[2]), len(labels), sums.data_ptr(),
        lib.stream_handle()), 'srgan_regression_evaluation_sums')
    torch.cuda.synchronize()
    return sums


def exact_batch(generator, batch, K=1, row_stride=None, with_bins=False):
    """Inputs whose every term and partial sum is a multiple of 2^-6 far below 2^53: any order of additions is exact.  The
    padding of a row wider than K holds large values that must not be read."""
    row_stride = row_stride or K
    rows = np.full((batch, row_stride), 1000.0, dtype=np.float32)
    rows[:, :K] = generator.randint(-64, 65, size=(batch, K)) / 8
    bins = (generator.randint(-320, 321, size=K) / 8).astype(np.float32) if with_bins else None
    labels = (generator.randint(-320, 321, size=batch) / 8).astype(np.float32)
    return rows, row_stride, K, bins, labels


def assert_same_bits(got, expected):
    got = got.cpu().numpy() if hasattr(got, 'cpu') else got
    assert got.tobytes() == np.asarray(expected, dtype=np.float64).tobytes(), (got, expected)


# ---- the kernel -----------------------------------------------------------------------------------------------------------
# one row | the last lane of a wave | a whole wave | one row into the second wave | one short of the workgroup | the workgroup
# | a second pass of thread 0 | several passes, the last one ragged
@pytest.mark.parametrize('batch', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_plain_predictions_are_exact_on_exact_inputs(lib, batch):
    generator = np.random.RandomState(batch)
    first, second = exact_batch(generator, batch), exact_batch(generator, batch)
    preloaded = np.array([1.5, -2.0, 3.25, 4.0, 100.0, -100.0, 7.0, 8.25])           # min / max that no label reaches
    sums = torch.from_numpy(preloaded.copy()).cuda()
    expected_first = evaluation_sums(*first, sums=preloaded)
    assert_same_bits(device_sums(lib, *first, sums=sums), expected_first)
    assert expected_first[4] < 100.0 and expected_first[5] > -100.0 and expected_first[3] == 4.0 + batch
    expected_second = evaluation_sums(*second, sums=expected_first)                   # a second batch accumulates
    assert_same_bits(device_sums(lib, *second, sums=sums), expected_second)
    assert expected_second[6:].tolist() == [7.0, 8.25]                               # the reserved slots are not touched
    assert_same_bits(device_sums(lib, *first), evaluation_sums(*first))               # from an empty record


@pytest.mark.parametrize('batch', [1, 65, 257])
@pytest.mark.parametrize('K', [1, 2, 10, 13])
def test_class_logits_with_bins_are_exact_on_exact_inputs(lib, batch, K):
    generator = np.random.RandomState(100 * batch + K)
    inputs = exact_batch(generator, batch, K, with_bins=True)
    assert_same_bits(device_sums(lib, *inputs), evaluation_sums(*inputs))
    padded = exact_batch(generator, batch, K, row_stride=K + 3, with_bins=True)       # row_stride > K
    assert_same_bits(device_sums(lib, *padded), evaluation_sums(*padded))


def test_rows_wider_than_their_prediction(lib):
    """``row_stride > K`` without bins: column 0 of a wider tensor."""
    inputs = exact_batch(np.random.RandomState(5), 300, 1, row_stride=7)
    assert_same_bits(device_sums(lib, *inputs), evaluation_sums(*inputs))


def test_accumulation_carries_the_label_range_over(lib):
    generator = np.random.RandomState(11)
    first, second = exact_batch(generator, 70), exact_batch(generator, 5)
    first[4][:], second[4][:] = np.clip(first[4], -10, 10), np.clip(second[4], -3, 3)
    first[4][17], first[4][40] = -30.0, 35.0                                          # the range comes from the first batch
    sums = device_sums(lib, *first)
    expected = evaluation_sums(*second, sums=evaluation_sums(*first))
    assert_same_bits(device_sums(lib, *second, sums=sums), expected)
    assert expected[4] == -30.0 and expected[5] == 35.0 and expected[3] == 75.0
    wider = exact_batch(generator, 3)
    wider[4][:] = [-31.0, 0.0, 36.0]                                                  # ... and a later batch widens it
    expected = evaluation_sums(*wider, sums=expected)
    assert_same_bits(device_sums(lib, *wider, sums=sums), expected)
    assert expected[4] == -31.0 and expected[5] == 36.0


# rows 192-255 belong to the last wave; row 448 = 192 + 256 is that wave's second pass
@pytest.mark.parametrize('low,high', [(0, 499), (499, 0), (200, 255), (448, 192), (0, 0)])
def test_the_label_extremes_wherever_they_sit(lib, low, high):
    inputs = exact_batch(np.random.RandomState(low + high), 500)
    inputs[4][:] = np.clip(inputs[4], -20, 20)
    inputs[4][high] = 39.5
    if low != high:
        inputs[4][low] = -39.25
    got = device_sums(lib, *inputs).cpu().numpy()
    assert_same_bits(got, evaluation_sums(*inputs))
    assert got[5] == 39.5 and got[4] == (-39.25 if low != high else inputs[4].min())


def test_ties_zeros_the_last_column_and_infinities(lib):
    K = 10
    bins = np.linspace(10, 95, K).astype(np.float32)
    logits = np.full((8, K), -1.0, dtype=np.float32)
    logits[0, [3, 7]] = 2.5                                      # a tie: the lowest index, 3
    logits[1, :] = -3.0
    logits[1, 2], logits[1, 5] = -0.0, 0.0                       # +0.0 and -0.0 compare equal: 2
    logits[2, 5], logits[2, 2] = -0.0, 0.0                       # ... in either order: 2
    logits[3, K - 1] = 4.0                                       # the maximum in column K - 1
    logits[4, :] = 0.25                                          # every column ties: 0
    logits[5, :] = -np.inf
    logits[5, 6] = -3e38                                         # the only finite value: 6
    logits[6, [1, 8]] = np.inf                                   # a tie of +inf: 1
    logits[7, :] = -np.inf                                       # nothing but -inf: 0
    expected_columns = [3, 2, 2, K - 1, 0, 6, 1, 0]
    assert torch.from_numpy(logits).max(dim=1)[1].tolist() == expected_columns        # torch.max's own choice
    labels = np.zeros(8, dtype=np.float32)                       # d = the chosen bin: sums[0] names the columns
    got = device_sums(lib, logits, K, K, bins, labels).cpu().numpy()
    assert_same_bits(got, evaluation_sums(logits, K, K, bins, labels))
    assert got[0] == got[1] == float(bins[expected_columns].astype(np.float64).sum())
    for row, column in enumerate(expected_columns):             # ... and row by row
        single = device_sums(lib, logits[row], K, K, bins, labels[:1]).cpu().numpy()
        assert single[0] == float(bins[column]), (row, column, single[0])


def test_the_squares_are_rounded_before_they_are_added(lib):
    """Differences with 30 significant bits, whose squares are inexact in fp64: ``fl(fl(d1 * d1) + fl(d2 * d2))``, NumPy's
    value, is one unit in the last place away from what a fused multiply-add leaves.  The x of ``contraction_cases``; here the
    two rows are 0 and 256, both thread 0's, so that the second square meets the first in that thread's running sum; every
    other row is zero, every other addition exact."""
    for (counts, labels, _, _), unfused, fused in contraction_cases(4, 1):
        x = labels[0, 0]
        predictions, row_labels = np.zeros(257, dtype=np.float32), np.zeros(257, dtype=np.float32)
        predictions[0], predictions[256] = counts[0], counts[-1]                      # 1 and 1.5
        row_labels[0] = row_labels[256] = x
        # the SGAN form of the same differences: rows 0 (a tie) and 1-255 choose bin 0 = 1, row 256 chooses bin 1 = 1.5;
        # rows 1-255 have the label 1, so their difference is zero
        logits = np.zeros((257, 2), dtype=np.float32)
        logits[1:256, 0], logits[256, 1] = 1.0, 1.0
        sgan_labels = np.full(257, 1.0, dtype=np.float32)
        sgan_labels[0] = sgan_labels[256] = x
        for inputs in ((predictions, 1, 1, None, row_labels),
                       (logits, 2, 2, np.array([1.0, 1.5], dtype=np.float32), sgan_labels)):
            got = device_sums(lib, *inputs).cpu().numpy()
            print('sums[2] %r rounded squares %r fused %r' % (got[2], unfused, fused))
            assert got[2] == unfused != fused
            assert_same_bits(got, evaluation_sums(*inputs))


def test_normal_inputs_within_the_summation_order_bound(lib):
    """``n * 2^-53 * sum |term|`` per sum (derived in ``order_bounds``, not measured); and the same bits on every run."""
    generator = np.random.RandomState(7)
    for batch, K in ((1000, 1), (777, 10)):
        rows = generator.standard_normal((batch, K)).astype(np.float32)
        bins = None if K == 1 else (generator.standard_normal(K) * 30).astype(np.float32)
        labels = (generator.standard_normal(batch) * 20).astype(np.float32)
        inputs = (rows, K, K, bins, labels)
        got = device_sums(lib, *inputs).cpu().numpy()
        expected, bounds = evaluation_sums(*inputs), order_bounds(*inputs)
        for index in range(8):
            print('B %d K %d sums[%d] device %.17g restatement %.17g |difference| %.3g bound %.3g' % (
                batch, K, index, got[index], expected[index], abs(got[index] - expected[index]), bounds[index]))
        for index in range(8):
            assert abs(got[index] - expected[index]) <= bounds[index], index
        assert got[3] == batch and got[4] == labels.min() and got[5] == labels.max() and got[6] == got[7] == 0.0
        assert_same_bits(device_sums(lib, *inputs), got)                              # two calls, the same bits


def test_an_empty_batch_and_argument_errors_leave_the_sums_untouched(lib):
    rows = torch.ones((4, 10), dtype=torch.float32, device='cuda')
    bins = torch.arange(10, dtype=torch.float32, device='cuda')
    labels = torch.zeros(4, dtype=torch.float32, device='cuda')
    preloaded = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    sums = torch.tensor(preloaded, dtype=torch.float64, device='cuda')
    good = dict(predictions=rows.data_ptr(), row_stride=10, K=10, bins=bins.data_ptr(), labels=labels.data_ptr(), B=4,
                sums=sums.data_ptr())

    def call(**changes):
        a = dict(good, **changes)
        return lib.library().srgan_regression_evaluation_sums(a['predictions'], a['row_stride'], a['K'], a['bins'], a['labels'],
                                                              a['B'], a['sums'], lib.stream_handle())
    assert call(B=0) == 0                                                             # B == 0: succeeds
    for name in ('predictions', 'labels', 'sums'):
        assert call(**{name: None}) == lib.EINVAL, name
    assert call(B=-1) == lib.EINVAL and call(K=0) == lib.EINVAL and call(bins=None) == lib.EINVAL
    assert call(row_stride=9) == lib.EINVAL and call(sums=sums.data_ptr() + 4) == lib.EINVAL
    assert call(K=1025, row_stride=1025) == lib.ERANGE and call(B=2 ** 22) == lib.ERANGE
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == preloaded
    assert call() == 0                                                                # ... and the good call does update
    torch.cuda.synchronize()                                                          # every row: bin 0 = 0.0, label 0
    assert sums.cpu().tolist() == [1.0, 2.0, 3.0, 8.0, 0.0, 6.0, 7.0, 8.0]


# ---- the experiments ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixture():
    return golden()


@pytest.fixture(scope='module')
def databases(fixture, tmp_path_factory):
    root = tmp_path_factory.mktemp('regression_validation_databases')
    return {'driving': write_driving_database(fixture, root / 'driving'), 'age': write_age_database(fixture, root / 'age')}


def applications():
    from srgan_amd.age.sgan import AgeSganExperiment
    from srgan_amd.age.srgan import AgeExperiment
    from srgan_amd.driving.srgan import DrivingExperiment
    return {'driving': (DrivingExperiment, 'SRGAN_DRIVING_DATABASE', 'driving'), 'age': (AgeExperiment, 'SRGAN_AGE_DATABASE', 'age'),
            'age_sgan': (AgeSganExperiment, 'SRGAN_AGE_DATABASE', 'age')}


def make_experiment(name, fixture, databases, monkeypatch, size=16, attributes=(), **overrides):
    """The experiment of ``run_experiment`` in test_image_batches_gpu.py (image size 16, batch 4, splits of 5 and 4
    examples), set up and in training mode, with ``attributes`` set on the instance.  (D and the DNN start from the same
    weights, so before an iteration their errors are equal; the training test below compares the two paths after one.)"""
    import srgan_amd.age.srgan as age
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all
    experiment_class, variable, database = applications()[name]
    monkeypatch.setattr(age, 'model_architecture', 'dcgan')
    monkeypatch.setenv(variable, databases[database])
    settings = Settings()
    for key, value in vars(settings_for(fixture, 'A')).items():
        setattr(settings, key, value)
    settings.matching_loss_multiplier, settings.contrasting_loss_multiplier = 1e2, 1e1
    settings.gradient_penalty_multiplier = 1e2
    settings.steps_to_run = 10 ** 9
    for key, value in overrides.items():
        setattr(settings, key, value)
    experiment = experiment_class(settings)
    experiment.image_size = size
    for key, value in dict(attributes).items():
        setattr(experiment, key, value)
    seed_all(0)
    experiment.dataset_setup()
    experiment.model_setup()
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    finish_setup(experiment)
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.summary_period, writer.steps_to_run = 10 ** 9, 10 ** 9
    seed_all(5)                                                   # the host streams the noise draws come from
    experiment.batches = (experiment.infinite_iter(experiment.train_dataset_loader),
                          experiment.infinite_iter(experiment.unlabeled_dataset_loader))
    return experiment


def train_one_iteration(experiment, step):
    labeled, unlabeled = experiment.batches
    examples, labels = next(labeled)
    experiment.training_iteration(examples, labels, next(unlabeled)[0], step)
    torch.cuda.synchronize()


def summary_step(experiment):
    """What ``end_of_step`` does at a summary step, with fresh writers; returns ``[(writer name, tag, value)]`` in logging
    order per writer."""
    from srgan_amd.tape import no_grad
    from srgan_amd.utility import SummaryWriter
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    experiment.join_dnn_stream()
    experiment.eval_mode()
    with no_grad():
        experiment.validation_summaries(0)
    experiment.train_mode()
    torch.cuda.synchronize()
    return [(name, tag, values[-1][1]) for name, writer in (('dnn', experiment.dnn_summary_writer), ('gan', experiment.gan_summary_writer))
            for tag, values in writer.scalars.items()]


def count_downloads(experiment, monkeypatch):
    """Wraps the one download site; and counts every ``Tensor.cpu()`` / ``.item()`` of a device tensor besides."""
    seen = {'records': [], 'tensor_downloads': 0}
    download = experiment.download_evaluation_records
    tensor_cpu, tensor_item = torch.Tensor.cpu, torch.Tensor.item

    def wrapped(records):
        assert records.is_cuda
        seen['records'].append((tuple(records.shape), records.dtype, records.numel() * records.element_size(),
                                records.is_contiguous()))
        return download(records)

    def counting(original):
        def method(tensor, *arguments, **keywords):
            seen['tensor_downloads'] += bool(tensor.is_cuda)
            return original(tensor, *arguments, **keywords)
        return method
    monkeypatch.setattr(experiment, 'download_evaluation_records', wrapped, raising=False)
    monkeypatch.setattr(torch.Tensor, 'cpu', counting(tensor_cpu))
    monkeypatch.setattr(torch.Tensor, 'item', counting(tensor_item))
    return seen


def assert_paths_agree(host, device):
    """The tags and their order are identical; every scalar agrees to 1e-12 relative (at most five fp64 terms per sum: the
    order bound is below 1e-15, the margin is for the divisions)."""
    assert [entry[:2] for entry in device] == [entry[:2] for entry in host]
    for (name, tag, expected), (_, _, got) in zip(host, device):
        print('%s %s host %.17g device %.17g' % (name, tag, expected, got))
        assert np.isfinite(expected) and abs(got - expected) <= 1e-12 * abs(expected), (name, tag, got, expected)


@pytest.mark.parametrize('name', ['driving', 'age'])
def test_the_device_path_logs_what_the_host_path_logs(lib, fixture, databases, monkeypatch, name):
    experiment = make_experiment(name, fixture, databases, monkeypatch)
    host = summary_step(experiment)
    tags = ['MAE', 'NMAE', 'MSE'] if name == 'driving' else ['MAE', 'MSE']
    per_writer = ['2 Train Error/' + tag for tag in tags] + ['1 Validation Error/' + tag for tag in tags]
    assert [tag for writer, tag, _ in host if writer == 'dnn'] == per_writer
    assert [tag for writer, tag, _ in host if writer == 'gan'] == per_writer + ['1 Validation Error/Ratio MAE GAN DNN']
    experiment.regression_validation = 'device'
    seen = count_downloads(experiment, monkeypatch)
    device = summary_step(experiment)
    monkeypatch.undo()
    assert seen['records'] == [((4, 8), torch.float64, 256, True)]            # exactly one device-to-host copy, of 256 bytes
    assert seen['tensor_downloads'] == 1                                      # ... and no other tensor came back
    assert_paths_agree(host, device)
    # the MAE under the ratio is the DNN's validation MAE, as on the host path
    scalars = {(writer, tag): value for writer, tag, value in device}
    ratio = scalars[('gan', '1 Validation Error/MAE')] / scalars[('dnn', '1 Validation Error/MAE')]
    assert scalars[('gan', '1 Validation Error/Ratio MAE GAN DNN')] == ratio
    # every example of the splits was evaluated: 5 train (a ragged second batch) and 4 validation
    assert [len(loader.dataset) for loader in (experiment.train_dataset_loader, experiment.validation_dataset_loader)] == [5, 4]


def test_the_age_sgan_takes_a_summary_step_on_both_paths(lib, fixture, databases, monkeypatch):
    """Without ``predicted_labels`` the host epoch subtracts B labels from 10 * B logits and NumPy raises."""
    experiment = make_experiment('age_sgan', fixture, databases, monkeypatch, number_of_bins=10)
    host = summary_step(experiment)
    experiment.regression_validation = 'device'
    device = summary_step(experiment)
    assert_paths_agree(host, device)
    for entries in (host, device):
        scalars = {(writer, tag): value for writer, tag, value in entries}
        for key in (('dnn', '1 Validation Error/MAE'), ('dnn', '1 Validation Error/MSE'), ('gan', '1 Validation Error/MAE'),
                    ('gan', '1 Validation Error/MSE'), ('gan', '2 Train Error/MAE'),
                    ('gan', '1 Validation Error/Ratio MAE GAN DNN')):
            assert np.isfinite(scalars[key]) and scalars[key] > 0, key
    # every prediction is a bin value: the MAE of one example is |bin - age| for some bin
    from srgan_amd.srgan import as_var
    from srgan_amd.tape import no_grad
    experiment.eval_mode()
    with no_grad():
        images, ages = next(iter(experiment.validation_dataset_loader.in_order()))
        predicted = experiment.predicted_labels(experiment.D, as_var(images))
        logits = experiment.D(as_var(images)).data
    bins = torch.linspace(10, 95, 10).cuda()
    assert tuple(predicted.shape) == (4,) and torch.equal(predicted, bins[logits.max(dim=1)[1]])


def train_with_a_summary_step(mode, fixture, databases, monkeypatch):
    experiment = make_experiment('driving', fixture, databases, monkeypatch, attributes={'regression_validation': mode})
    logged = None
    for step in range(1, 4):
        train_one_iteration(experiment, step)
        if step == 1:
            writers = experiment.dnn_summary_writer, experiment.gan_summary_writer
            logged = summary_step(experiment)
            experiment.dnn_summary_writer, experiment.gan_summary_writer = writers
    torch.cuda.synchronize()
    return experiment, logged


def test_the_attribute_does_not_perturb_training(lib, fixture, databases, monkeypatch):
    host, host_logged = train_with_a_summary_step('host', fixture, databases, monkeypatch)
    device, device_logged = train_with_a_summary_step('device', fixture, databases, monkeypatch)
    assert_paths_agree(host_logged, device_logged)
    for name in ('D', 'G', 'DNN'):
        a, b = getattr(host, name)._srgan_arena.data, getattr(device, name)._srgan_arena.data
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


def test_an_fp16_run_is_evaluated_on_its_own_data_path(lib, fixture, databases, monkeypatch):
    """``validation_precision = 'step'``: the device scalars against host arithmetic on predictions taken HERE from forwards
    under ``experiment.precision()``, to the same 1e-12; the fp32 evaluation's MAE is printed next to it (both finite: no
    bound on their difference is fixed, profiles/regression_validation.md records what was observed)."""
    from srgan_amd import functional as F
    from srgan_amd.srgan import as_var
    from srgan_amd.tape import no_grad
    experiment = make_experiment('driving', fixture, databases, monkeypatch, compute_dtype='f16', storage_dtype='f16',
                                 attributes={'regression_validation': 'device', 'validation_precision': 'step'})
    device = summary_step(experiment)
    expected, storage_seen = [], set()
    experiment.eval_mode()
    with no_grad():
        for writer, network in (('dnn', experiment.DNN), ('gan', experiment.D)):
            for summary_name, loader in (('2 Train Error', experiment.train_dataset_loader),
                                         ('1 Validation Error', experiment.validation_dataset_loader)):
                predictions, plain_predictions, labels = [], [], []
                for images, batch_labels in loader.in_order():
                    with experiment.precision():
                        storage_seen.add(F.STORAGE_DTYPE)
                        predicted = network(as_var(images))
                    assert predicted.data.dtype == torch.float32
                    predictions.append(predicted.data.cpu().numpy().reshape(-1))
                    plain_predictions.append(network(as_var(images)).data.cpu().numpy().reshape(-1))
                    labels.append(batch_labels.cpu().numpy().reshape(-1))
                predictions, labels = np.concatenate(predictions), np.concatenate(labels)
                plain_predictions = np.concatenate(plain_predictions)
                print('%s %s predictions: largest |fp16 data path - fp32| %.3g, largest |fp32| %.3g, largest |label| %.3g' % (
                    writer, summary_name, np.abs(predictions - plain_predictions).max(), np.abs(plain_predictions).max(),
                    np.abs(labels).max()))
                record = evaluation_sums(predictions, 1, 1, None, labels)
                comparison = None
                if writer == 'gan' and summary_name == '1 Validation Error':
                    comparison = dict((entry[:2], entry[2]) for entry in expected)[('dnn', '1 Validation Error/MAE')]
                expected += [(writer, summary_name + '/' + tag, value)
                             for tag, value in evaluation_scalars(record, comparison, normalized=True)]
    experiment.train_mode()
    assert storage_seen and None not in storage_seen and 0 not in storage_seen, storage_seen      # a 16-bit data path was active
    assert_paths_agree(expected, device)
    experiment.validation_precision = 'f32'
    fp32 = summary_step(experiment)
    experiment.regression_validation = 'host'
    experiment.validation_precision = 'step'
    assert_paths_agree(device, summary_step(experiment))                      # the host path honours the switch too
    for (writer, tag, own), (_, _, plain) in zip(device, fp32):
        if tag.endswith('/MAE'):
            print('%s %s: fp16 data path %.9g, fp32 evaluation %.9g, relative difference %.3g' % (
                writer, tag, own, plain, abs(own - plain) / abs(plain)))
        assert np.isfinite(own) and np.isfinite(plain)


def test_without_the_attributes_nothing_of_the_device_path_runs(lib, fixture, databases, monkeypatch):
    """The defaults: the entry point is never called, nothing is downloaded through the device path's site, and the logged
    values are host arithmetic on ``network(in_order batches)`` (which test_image_batches_gpu.py pins to 1e-6 besides)."""
    from srgan_amd.srgan import as_var
    from srgan_amd.tape import no_grad
    experiment = make_experiment('driving', fixture, databases, monkeypatch)
    assert experiment.regression_validation == 'host' and experiment.validation_precision == 'f32'
    calls = []
    library = lib.library()
    entry_point = library.srgan_regression_evaluation_sums

    class Counting:
        def __call__(self, *arguments):
            calls.append(arguments)
            return entry_point(*arguments)
    monkeypatch.setattr(library, 'srgan_regression_evaluation_sums', Counting())
    monkeypatch.setattr(experiment, 'download_evaluation_records', lambda records: calls.append('download'), raising=False)
    monkeypatch.setattr(experiment, 'precision', lambda *a, **k: calls.append('precision'))
    logged = summary_step(experiment)
    monkeypatch.undo()
    assert calls == []
    scalars = {(writer, tag): value for writer, tag, value in logged}
    experiment.eval_mode()
    with no_grad():
        predictions, labels = [], []
        for images, batch_labels in experiment.validation_dataset_loader.in_order():
            predictions.append(experiment.D(as_var(images)).cpu().numpy().reshape(-1).astype(np.float64))
            labels.append(batch_labels.cpu().numpy().astype(np.float64))
    predictions, labels = np.concatenate(predictions), np.concatenate(labels)
    assert scalars[('gan', '1 Validation Error/MAE')] == float(np.abs(predictions - labels).mean())       # the parent's arithmetic
    assert scalars[('gan', '1 Validation Error/MSE')] == float((np.abs(predictions - labels) ** 2).mean())
    assert scalars[('gan', '1 Validation Error/NMAE')] == float(np.abs(predictions - labels).mean()) / float(labels.max() - labels.min())
