"""Generate tests/golden/g18_coefficient_distributions.npz by running the UNMODIFIED upstream reference on CPU.

Test infrastructure only, like make_goldens.py: it needs the reference checkout, scipy and matplotlib and never travels to the
GPU box; the emitted fixture holds data only.  The reference's ``CoefficientExperiment`` (hidden 10, batch 64, labeled 32,
unlabeled 256, validation 64) trains three steps and then runs its own ``validation_summaries`` (coefficient/srgan.py:40-78)
with ``generate_display_frame`` replaced by a function that keeps its arguments (seaborn is not installed).  Recorded: the z of
the summary, the generated examples, the five prediction arrays the frame is drawn from, the unlabeled labels, the weights the
summaries ran with, the logged ``Generator/Predicted Label Wasserstein``, and for every array of the frame
``scipy.stats.gaussian_kde(x, bw_method=0.1)`` on ``linspace(min - 3 h, max + 3 h, 100)``, h = 0.1 std(x, ddof=1).  Usage::

    python tests/golden/make_distribution_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstubs  # noqa: E402


class RecordClass:
    """Stand-in for ``recordclass.RecordClass`` that takes the fields as keywords (``evaluation_epoch`` builds one; the stub of
    _refstubs.py, which no other fixture instantiates, takes none)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


_refstubs._module('recordclass', RecordClass=RecordClass)
_refstubs.install()

import torch  # noqa: E402
from scipy.stats import gaussian_kde  # noqa: E402

import make_goldens  # noqa: E402  (installs nothing more; its helpers)
import utility as ref_utility  # noqa: E402
from settings import Settings  # noqa: E402

STEPS, GRIDSIZE, BANDWIDTH, CUT = 3, 100, 0.1, 3
FRAME_ARGUMENTS = ('fake_examples', 'unlabeled_predictions', 'gan_validation', 'dnn_validation', 'gan_train', 'dnn_train')


def scipy_curve(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    h = BANDWIDTH * x.std(ddof=1)
    support = np.linspace(x.min() - CUT * h, x.max() + CUT * h, GRIDSIZE)
    return support, gaussian_kde(x, bw_method=BANDWIDTH)(support)


def main():
    import coefficient.srgan as ref_coefficient
    settings = Settings()
    settings.batch_size, settings.hidden_size = 64, 10
    settings.labeled_dataset_size, settings.unlabeled_dataset_size, settings.validation_dataset_size = 32, 256, 64
    settings.pin_memory, settings.number_of_data_workers = False, 0
    settings.summary_step_period = 1
    experiment = ref_coefficient.CoefficientExperiment(settings)
    ref_utility.seed_all(0)
    experiment.dataset_setup()
    experiment.model_setup()
    experiment.prepare_optimizers()
    experiment.train_mode()
    make_goldens.attach_writers(experiment)
    labeled = experiment.infinite_iter(experiment.train_dataset_loader)
    unlabeled = experiment.infinite_iter(experiment.unlabeled_dataset_loader)
    for step in range(STEPS):
        x, y = next(labeled)
        experiment.dnn_training_step(x, y, step)
        experiment.gan_training_step(x, y, next(unlabeled)[0], step)
    out = {name: np.array(getattr(settings, name)) for name in
           ('batch_size', 'hidden_size', 'labeled_dataset_size', 'unlabeled_dataset_size', 'validation_dataset_size',
            'labeled_dataset_seed', 'mean_offset')}
    for name in ('D', 'DNN', 'G'):
        out.update(make_goldens.state_arrays(f'weights/{name}', getattr(experiment, name)))

    captured = {}

    class RecordingMixture(ref_coefficient.MixtureModel):
        def rvs(self, size):
            values = super().rvs(size)
            captured['z'] = np.asarray(values).astype(np.float32)
            return values

    def keep_arguments(*arguments):
        for name, value in zip(FRAME_ARGUMENTS, arguments):
            captured[name] = np.array(value)
        captured['step'] = np.array(arguments[-1])
        return np.zeros((4, 6, 3), dtype=np.uint8)

    ref_coefficient.MixtureModel = RecordingMixture
    ref_coefficient.generate_display_frame = keep_arguments
    # (the conversion of the figure for TensorBoard uses an alias current NumPy has dropped; the stand-in figure needs none)
    ref_coefficient.standard_image_format_to_tensorboard_image_format = lambda image: image
    experiment.eval_mode()
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.step = STEPS
    with torch.no_grad():
        experiment.validation_summaries(STEPS)
    assert set(FRAME_ARGUMENTS) <= set(captured) and captured['z'].shape == (64, experiment.G.input_size)
    out.update(captured)
    out['unlabeled_labels'] = np.array(experiment.unlabeled_dataset.labels[:settings.validation_dataset_size])
    out['unlabeled_examples'] = np.array(experiment.unlabeled_dataset.examples[:settings.validation_dataset_size])
    out['wasserstein'] = np.array(make_goldens.last_scalars(experiment.gan_summary_writer)['Generator/Predicted Label Wasserstein'])
    # what presentation.py:24,33 plots as the fake curve: the four coefficients fitted to the first generated example
    fake_a3 = np.transpose(np.polyfit(np.linspace(-1, 1, num=10), np.transpose(captured['fake_examples'][:, :10]), 3))
    out['fake_coefficients'] = fake_a3[0, :]
    for name in ('fake_coefficients',) + FRAME_ARGUMENTS[1:]:
        out[f'kde/{name}/support'], out[f'kde/{name}/density'] = scipy_curve(out[name])
    make_goldens.save('g18_coefficient_distributions', **out)


if __name__ == '__main__':
    main()
