"""Generate tests/golden/g20_regression_evaluation.npz by running the UNMODIFIED upstream reference on CPU.

Test infrastructure only, like make_goldens.py: it needs the reference checkout and never travels to the GPU box; the
emitted fixture holds data only.  Fixed predictions, class logits, bins and labels go through the reference's own
``AgeExperiment.evaluation_epoch``, ``DrivingExperiment.evaluation_epoch`` and ``AgeSganExperiment.images_to_predicted_ages``
with a stub network that returns the recorded outputs (its "images" are the row numbers) and a stub writer that records what
is logged: per application the tags in logging order and their values, once without and once with a comparison value.  Usage::

    python tests/golden/make_regression_validation_goldens.py

The archive is written with fixed member times, so the same inputs give the same bytes.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstubs  # noqa: E402

_refstubs.install()
for missing in ('requests', 'patoolib'):
    try:
        __import__(missing)
    except ImportError:
        sys.modules[missing] = types.ModuleType(missing)

import torch  # noqa: E402
from torch.utils.data import TensorDataset  # noqa: E402
from make_image_database_goldens import save  # noqa: E402
from settings import Settings  # noqa: E402
from age.srgan import AgeExperiment  # noqa: E402
from age.sgan import AgeSganExperiment  # noqa: E402
from driving.srgan import DrivingExperiment  # noqa: E402

BATCH = 4                       # 11 and 9 examples: a ragged last batch
COMPARISON = 7.25               # the "DNN's MAE" of the second epoch


class RecordedNetwork(torch.nn.Module):
    """Returns the recorded output rows the "images" (row numbers) name."""

    def __init__(self, outputs):
        super().__init__()
        self.outputs = torch.from_numpy(outputs)

    def forward(self, images):
        return self.outputs[images.reshape(-1).long()]


def logged(experiment, outputs, labels):
    """The tags (in order) and values the reference's ``evaluation_epoch`` logs, without and then with a comparison value."""
    settings = experiment.settings
    dataset = TensorDataset(torch.arange(len(labels), dtype=torch.float32), torch.from_numpy(labels))
    writer = _refstubs.RecordingSummaryWriter()
    first = experiment.evaluation_epoch(settings, RecordedNetwork(outputs), dataset, writer, '1 Validation Error')
    plain = [(tag, values[-1][1]) for tag, values in writer.scalars.items()]
    writer = _refstubs.RecordingSummaryWriter()
    second = experiment.evaluation_epoch(settings, RecordedNetwork(outputs), dataset, writer, '1 Validation Error',
                                         comparison_value=COMPARISON)
    compared = [(tag, values[-1][1]) for tag, values in writer.scalars.items()]
    assert first == second
    return {'tags': np.array([tag for tag, _ in plain]), 'values': np.array([value for _, value in plain], dtype=np.float64),
            'compared_tags': np.array([tag for tag, _ in compared]),
            'compared_values': np.array([value for _, value in compared], dtype=np.float64),
            'returned_mae': np.array(float(first), dtype=np.float64)}


def sgan_logits(generator, rows, columns):
    """Class logits with the cases the selection must get right in the first rows: a tie (the lowest index wins), +0.0
    against -0.0 (equal), the maximum in the last column, infinities."""
    logits = generator.standard_normal((rows, columns)).astype(np.float32)
    logits[0, :] = -1.0
    logits[0, [3, 7]] = 2.5                                   # a tie: column 3
    logits[1, :] = -3.0
    logits[1, 2], logits[1, 5] = -0.0, 0.0                    # equal: column 2
    logits[2, :] = np.linspace(-2, 2, columns)                # the last column
    logits[3, :] = -np.inf
    logits[3, 6] = -1e30                                      # the only finite value
    logits[4, [1, 8]] = np.inf                                # a tie of infinities: column 1
    return logits


def main():
    settings = Settings()
    settings.batch_size = BATCH
    generator = np.random.RandomState(20)
    arrays = {'torch_version': np.array(torch.__version__), 'batch_size': np.array(BATCH),
              'comparison_value': np.array(COMPARISON, dtype=np.float64)}

    ages = generator.randint(10, 96, 11).astype(np.float32)
    predicted_ages = (ages + 9 * generator.standard_normal(11)).astype(np.float32)[:, None]
    arrays.update({'age/predictions': predicted_ages, 'age/labels': ages})
    arrays.update({'age/' + key: value for key, value in logged(AgeExperiment(settings), predicted_ages, ages).items()})

    angles = generator.uniform(-1.5, 1.5, 9).astype(np.float32)
    predicted_angles = (angles + 0.3 * generator.standard_normal(9)).astype(np.float32)[:, None]
    arrays.update({'driving/predictions': predicted_angles, 'driving/labels': angles})
    arrays.update({'driving/' + key: value
                   for key, value in logged(DrivingExperiment(settings), predicted_angles, angles).items()})

    sgan = AgeSganExperiment(settings)
    logits = sgan_logits(generator, 11, 10)
    bin_ages = sgan.images_to_predicted_ages(RecordedNetwork(logits), torch.arange(11, dtype=torch.float32))
    arrays.update({'sgan/logits': logits, 'sgan/bins': sgan.bins.numpy().astype(np.float32), 'sgan/labels': ages,
                   'sgan/predicted_ages': bin_ages.numpy().astype(np.float32)})
    arrays.update({'sgan/' + key: value for key, value in logged(sgan, logits, ages).items()})
    save(os.path.join(HERE, 'g20_regression_evaluation.npz'), arrays)


if __name__ == '__main__':
    main()
