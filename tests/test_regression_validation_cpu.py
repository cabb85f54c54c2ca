"""Age / driving validation summaries, the parts that need no GPU: the NumPy restatement of
``srgan_regression_evaluation_sums`` against what the reference's own ``evaluation_epoch`` logged
(tests/golden/g20_regression_evaluation.npz), ``logits_to_bin_values`` against ``torch.max``, the entry point's plumbing and
argument checks (made before any device work), the two attributes of ``Experiment``, and the prediction hook -- the age
SGAN's host epoch on a stub network included."""
import os
import re

import numpy as np
import pytest
import torch

from regression_validation_reference import EMPTY_RECORD, evaluation_scalars, evaluation_sums, order_bounds, row_predictions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g20_regression_evaluation.npz')
PTR = 16        # a non-NULL, 16-byte aligned "pointer" for calls that must fail before touching memory


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def golden_inputs(golden, application):
    """(predictions, row_stride, K, bins, labels) of one recorded application."""
    if application == 'sgan':
        return golden['sgan/logits'], 10, 10, golden['sgan/bins'], golden['sgan/labels']
    return golden[application + '/predictions'], 1, 1, None, golden[application + '/labels']


def scalar_tolerance(value, terms):
    """The reference takes ``mean()`` of the same float64 terms (all of one sign) in NumPy's order, the restatement their sum
    over the count: ``terms * 2^-53`` relative for the order of the additions, and one rounding for each of at most eight
    operations behind it (the divisions, the range, the ratio)."""
    return (terms + 8) * 2.0 ** -53 * abs(value)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_the_restatement_on_a_hand_written_case():
    predictions = np.array([1.0, 9.0, 3.5, 9.0, -2.0, 9.0], dtype=np.float32)            # row_stride 2: the 9s are never read
    labels = np.array([0.5, 4.0, -1.0], dtype=np.float32)                                # d = 0.5, -0.5, -1
    sums = evaluation_sums(predictions, 2, 1, None, labels)
    assert sums.tolist() == [-1.0, 2.0, 1.5, 3.0, -1.0, 4.0, 0.0, 0.0]
    again = evaluation_sums(np.array([2.0], dtype=np.float32), 1, 1, None, np.array([7.0], dtype=np.float32), sums=sums)
    assert again.tolist() == [-6.0, 7.0, 26.5, 4.0, -1.0, 7.0, 0.0, 0.0]                  # min carried over, max replaced
    assert evaluation_sums(predictions[:0], 1, 1, None, labels[:0], sums=again).tolist() == again.tolist()   # B == 0
    assert evaluation_sums(predictions, 2, 1, None, labels, sums=[0, 0, 0, 0, 9, -9, 6.5, 7.5])[6:].tolist() == [6.5, 7.5]
    assert tuple(EMPTY_RECORD) == (0.0, 0.0, 0.0, 0.0, np.inf, -np.inf, 0.0, 0.0)
    logits = np.array([[1, 5, 5], [-0.0, 0.0, -1], [0, 1, 2]], dtype=np.float32)
    bins = np.array([10.0, 20.0, 30.0], dtype=np.float32)
    assert row_predictions(logits, 3, 3, bins).tolist() == [20.0, 10.0, 30.0]           # a tie, the zeros, the last column
    binned = evaluation_sums(logits, 3, 3, bins, np.array([20.0, 20.0, 20.0], dtype=np.float32))
    assert binned.tolist() == [0.0, 20.0, 200.0, 3.0, 20.0, 20.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        evaluation_sums(logits, 3, 3, None, labels)
    assert [tag for tag, _ in evaluation_scalars(again, 2.0, normalized=True)] == ['MAE', 'NMAE', 'MSE', 'Ratio MAE GAN DNN']
    assert [value for _, value in evaluation_scalars(again, 2.0, normalized=True)] == [1.75, 1.75 / 8, 26.5 / 4, 0.875]
    assert [tag for tag, _ in evaluation_scalars(again)] == ['MAE', 'MSE']
    bounds = order_bounds(predictions, 2, 1, None, labels)
    assert all(0 < bounds[k] < 1e-14 for k in (0, 1, 2)) and not bounds[3:].any()


@pytest.mark.parametrize('application', ['age', 'driving', 'sgan'])
def test_the_restatement_gives_what_the_reference_logged(golden, application):
    inputs = golden_inputs(golden, application)
    batch = int(golden['batch_size'])
    labels = inputs[4]
    whole = evaluation_sums(*inputs)
    record = None
    for first in range(0, len(labels), batch):                             # batch by batch, as an epoch accumulates
        rows = np.asarray(inputs[0]).reshape(len(labels), -1)[first:first + batch]
        record = evaluation_sums(rows, inputs[1], inputs[2], inputs[3], labels[first:first + batch], sums=record)
    assert record[3] == whole[3] == len(labels) and record[4] == whole[4] and record[5] == whole[5]
    assert all(abs(record[k] - whole[k]) <= order_bounds(*inputs)[k] for k in range(3))
    normalized = application == 'driving'
    for tags, values, comparison in ((golden[application + '/tags'], golden[application + '/values'], None),
                                     (golden[application + '/compared_tags'], golden[application + '/compared_values'],
                                      float(golden['comparison_value']))):
        scalars = evaluation_scalars(record, comparison, normalized=normalized)
        assert ['1 Validation Error/' + tag for tag, _ in scalars] == list(tags)          # the same tags in the same order
        for (tag, value), expected in zip(scalars, values):
            print('%s %s restatement %.17g reference %.17g' % (application, tag, value, expected))
            assert abs(value - expected) <= scalar_tolerance(expected, len(labels)), tag
    if application == 'sgan':
        assert np.array_equal(row_predictions(*inputs[:4]), golden['sgan/predicted_ages'])   # bit for bit


def test_logits_to_bin_values_takes_the_first_maximal_index(golden):
    from srgan_amd.utility import logits_to_bin_values
    bins = torch.linspace(10, 95, 10)
    logits = torch.from_numpy(golden['sgan/logits'])
    assert torch.equal(logits_to_bin_values(logits, bins), torch.from_numpy(golden['sgan/predicted_ages']))
    cases = torch.full((4, 10), -1.0)
    cases[0, 3] = cases[0, 7] = 2.5                                        # a tie
    cases[1, :] = -3.0
    cases[1, 2], cases[1, 5] = -0.0, 0.0                                   # +0.0 and -0.0 compare equal
    cases[2, 9] = 4.0                                                      # the maximum in the last column
    cases[3, :] = 0.0                                                      # every column ties
    picked = cases.max(dim=1)[1]
    assert picked.tolist() == [3, 2, 9, 0]
    assert torch.equal(logits_to_bin_values(cases, bins), bins[picked])
    assert np.array_equal(row_predictions(cases.numpy(), 10, 10, bins.numpy()), bins[picked].numpy())


# ---- the entry point ------------------------------------------------------------------------------------------------------
def test_the_library_advertises_and_binds_the_entry_point():
    from srgan_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_REGRESSION_EVALUATION\s+0x40000u', header)
    assert _lib.capabilities().features & 0x40000
    assert _lib.library().srgan_version() == 110
    assert 'srgan_regression_evaluation_sums' in _lib.SIGNATURES
    assert 'srgan_regression_evaluation_sums' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def evaluation_call(lib, **changes):
    a = dict(dict(predictions=PTR, row_stride=10, K=10, bins=PTR, labels=PTR, B=5, sums=PTR), **changes)
    return lib.library().srgan_regression_evaluation_sums(a['predictions'], a['row_stride'], a['K'], a['bins'], a['labels'],
                                                          a['B'], a['sums'], None)


def test_argument_errors_are_reported_before_any_device_work():
    """Fake pointers throughout: a call that got as far as a launch would fault, and ``sums`` is never dereferenced."""
    from srgan_amd import _lib
    for name in ('predictions', 'labels', 'sums'):
        assert evaluation_call(_lib, **{name: None}) == _lib.EINVAL, name
        assert b'srgan_regression_evaluation_sums' in _lib.library().srgan_last_error()
    assert evaluation_call(_lib, B=-1) == _lib.EINVAL
    assert evaluation_call(_lib, K=0) == _lib.EINVAL and evaluation_call(_lib, K=-3) == _lib.EINVAL
    assert evaluation_call(_lib, bins=None) == _lib.EINVAL                                 # K > 1 without bins
    assert evaluation_call(_lib, bins=None, K=2, row_stride=2) == _lib.EINVAL
    assert evaluation_call(_lib, row_stride=9) == _lib.EINVAL and evaluation_call(_lib, row_stride=-1) == _lib.EINVAL
    assert evaluation_call(_lib, row_stride=0, K=1, bins=None) == _lib.EINVAL
    assert evaluation_call(_lib, sums=PTR + 4) == _lib.EINVAL
    # the capacity of the one-workgroup design: K <= 1024 and B * K <= 2^22
    assert evaluation_call(_lib, K=1025, row_stride=1025, B=1) == _lib.ERANGE
    assert b'2^22' in _lib.library().srgan_last_error()
    assert evaluation_call(_lib, K=1, row_stride=1, bins=None, B=2 ** 22 + 1) == _lib.ERANGE
    assert evaluation_call(_lib, K=1024, row_stride=1024, B=2 ** 12 + 1) == _lib.ERANGE
    assert evaluation_call(_lib, K=1, row_stride=2 ** 40, bins=None, B=2 ** 31 - 1) == _lib.ERANGE     # no 32-bit overflow
    # zero rows: a successful no-op at the limits too (nothing is launched, the fake pointers are never used)
    assert evaluation_call(_lib, B=0) == 0 and evaluation_call(_lib, B=0, K=1, row_stride=1, bins=None) == 0
    assert evaluation_call(_lib, B=0, K=1024, row_stride=1024) == 0


# ---- the experiment -------------------------------------------------------------------------------------------------------
def bare_experiment(experiment_class=None):
    from srgan_amd import srgan
    from srgan_amd.settings import Settings

    class _Experiment(experiment_class or srgan.Experiment):
        def dataset_setup(self):
            pass

        def model_setup(self):
            pass

        def validation_summaries(self, step):
            pass

    return _Experiment(Settings())


def test_the_switches_are_attributes_with_defaults_and_are_checked():
    from srgan_amd import settings, srgan
    from srgan_amd.age.srgan import AgeExperiment
    from srgan_amd.driving.srgan import DrivingExperiment
    assert srgan.Experiment.regression_validation == 'host' and srgan.Experiment.validation_precision == 'f32'
    experiment = bare_experiment()
    assert experiment.regression_validation == 'host' and experiment.validation_precision == 'f32'
    assert not {'regression_validation', 'validation_precision'} & set(vars(experiment))       # class attributes
    assert AgeExperiment.regression_validation == DrivingExperiment.regression_validation == 'host'
    names = {name for name, _, _ in settings.EXTENSIONS} | set(dict(settings.DEFAULTS))
    assert not {'regression_validation', 'validation_precision'} & names                        # not settings
    experiment.train_dataset_loader = experiment.validation_dataset_loader = []
    for name, value in (('regression_validation', 'gpu'), ('regression_validation', None), ('validation_precision', 'bf16'),
                        ('validation_precision', True)):
        broken = bare_experiment()
        broken.train_dataset_loader = broken.validation_dataset_loader = []
        setattr(broken, name, value)
        with pytest.raises(ValueError, match=name):
            broken.regression_validation_summaries()


def test_the_default_prediction_hook_is_the_network():
    experiment = bare_experiment()
    examples = torch.arange(6.0).reshape(3, 2)
    network = lambda x: x * 2
    assert torch.equal(experiment.predicted_labels(network, examples), examples * 2)
    rows, bins = experiment.prediction_rows(network, examples)
    assert torch.equal(rows, examples * 2) and bins is None


def test_a_downloaded_record_logs_what_the_reference_logged(golden):
    """``log_regression_record`` on the restatement's record: the host half of the device path."""
    from srgan_amd.srgan import Experiment
    from srgan_amd.utility import SummaryWriter
    assert tuple(Experiment.EVALUATION_RECORD) == tuple(EMPTY_RECORD)
    for application in ('age', 'driving', 'sgan'):
        record = evaluation_sums(*golden_inputs(golden, application))
        writer = SummaryWriter()
        mae = Experiment.log_regression_record(record, writer, '1 Validation Error',
                                               comparison_value=float(golden['comparison_value']),
                                               normalized=application == 'driving')
        assert list(writer.scalars) == list(golden[application + '/compared_tags'])
        expected = golden[application + '/compared_values']
        for (tag, values), value in zip(writer.scalars.items(), expected):
            assert abs(values[-1][1] - value) <= scalar_tolerance(value, int(record[3])), tag
        assert mae == writer.scalars['1 Validation Error/MAE'][-1][1]
        assert abs(mae - float(golden[application + '/returned_mae'])) <= scalar_tolerance(mae, 11)
    with pytest.raises(ValueError, match='empty'):
        Experiment.log_regression_record(np.array(EMPTY_RECORD), SummaryWriter(), '1 Validation Error')


def test_the_age_sgan_predicts_bin_values_and_takes_a_host_epoch(golden):
    """The age SGAN's hook on a stub network that returns the recorded class logits, and its host evaluation epoch against
    what the reference's logged for the same logits.  (Without the hook the epoch subtracts B labels from 10 * B logits.)"""
    from srgan_amd.age.sgan import AgeSganExperiment
    from srgan_amd.tape import Var
    from srgan_amd.utility import SummaryWriter
    experiment = bare_experiment(AgeSganExperiment)
    assert np.array_equal(experiment.bins.numpy(), golden['sgan/bins'])
    experiment.bins = Var(experiment.bins)                  # (as the first training step leaves them, but on the CPU)
    logits = torch.from_numpy(golden['sgan/logits'])
    labels = torch.from_numpy(golden['sgan/labels'])
    network = lambda examples: Var(logits[examples.data.long()])
    rows = Var(torch.arange(len(labels)))                   # the "images" are the row numbers; a Var enters the tape as it is
    predicted = experiment.predicted_labels(network, rows)
    assert predicted.dtype == torch.float32 and np.array_equal(predicted.numpy(), golden['sgan/predicted_ages'])
    device_rows, bins = experiment.prediction_rows(network, rows)
    assert torch.equal(device_rows.data, logits) and np.array_equal(bins.data.numpy(), golden['sgan/bins'])
    batch = int(golden['batch_size'])
    batches = [(Var(rows.data[first:first + batch]), labels[first:first + batch]) for first in range(0, len(labels), batch)]
    writer = SummaryWriter()
    mae = experiment.regression_evaluation_epoch(network, batches, writer, '1 Validation Error',
                                                 comparison_value=float(golden['comparison_value']))
    assert list(writer.scalars) == list(golden['sgan/compared_tags'])
    for (tag, values), expected in zip(writer.scalars.items(), golden['sgan/compared_values']):
        assert abs(values[-1][1] - expected) <= scalar_tolerance(expected, len(labels)), tag
    assert abs(mae - float(golden['sgan/returned_mae'])) <= scalar_tolerance(mae, len(labels))
