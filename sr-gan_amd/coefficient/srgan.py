"""Coefficient application (surface of reference coefficient/srgan.py:17-101): toy datasets, MLP D / DNN and generator, the
MAE / MSE summaries and, with ``settings.distribution_summaries``, the reference's two distribution outputs built on the device
(``distribution_summaries.py``): the scalar ``Generator/Predicted Label Wasserstein`` and the ``Distributions`` frame of
kernel-density curves -- without the figure's text."""
import numpy as np
import torch
from scipy.stats import norm
from torch.utils.data import DataLoader

from .. import distribution_summaries
from .. import functional as F
from ..settings import option
from ..srgan import Experiment, as_var
from ..tape import no_grad
from ..utility import MixtureModel, current_device
from .data import ToyDataset
from .models import Generator, MLP, observation_count


class CoefficientExperiment(Experiment):
    """The coefficient application."""

    def dataset_setup(self):
        """Labeled / unlabeled / validation toy datasets with the reference's seeds (labeled: the settings' seed, unlabeled
        100, validation 101; reference coefficient/srgan.py:20-33); the two training sets are shuffled each epoch."""
        settings = self.settings

        def toy(size, seed):
            return ToyDataset(dataset_size=size, observation_count=observation_count, settings=settings, seed=seed)

        def shuffled(dataset):
            return DataLoader(dataset, batch_size=settings.batch_size, shuffle=True, pin_memory=settings.pin_memory)
        self.train_dataset = toy(settings.labeled_dataset_size, settings.labeled_dataset_seed)
        self.train_dataset_loader = shuffled(self.train_dataset)
        self.unlabeled_dataset = toy(settings.unlabeled_dataset_size, 100)
        self.unlabeled_dataset_loader = shuffled(self.unlabeled_dataset)
        self.validation_dataset = toy(settings.validation_dataset_size, 101)

    def model_setup(self):
        self.DNN = MLP(self.settings.hidden_size)
        self.D = MLP(self.settings.hidden_size)
        self.G = Generator(self.settings.hidden_size)

    def predicted_values(self, network, examples):
        """The value predictions of D or the DNN (the dual-goal networks return a score beside them)."""
        return network(examples)

    def validation_summaries(self, step):
        """MAE / MSE / RMSE of DNN and D on the train and validation sets, and the GAN/DNN ratios (reference
        coefficient/srgan.py:40-55,87-101); then, with ``settings.distribution_summaries``, :56-78."""
        dnn_validation = None
        for network, writer in ((self.DNN, self.dnn_summary_writer), (self.D, self.gan_summary_writer)):
            value_head = lambda examples, network=network: self.predicted_values(network, examples)
            for dataset, name in ((self.train_dataset, '2 Train Error'), (self.validation_dataset, '1 Validation Error')):
                values = self.evaluation_epoch(value_head, dataset, writer, name,
                                               dnn_validation if (network is self.D and name.startswith('1')) else None)
                if network is self.DNN and name.startswith('1'):
                    dnn_validation = values
        self.distribution_summaries(step)

    def evaluation_epoch(self, network, dataset, summary_writer, summary_name, comparison_values=None):
        with no_grad():
            on_device = network(as_var(torch.from_numpy(dataset.examples.astype(np.float32))))
        if self.distribution_summaries_on():
            # the frame of ``distribution_summaries`` reads the four prediction sets where they are: no second upload
            # ((GAN writer?, summary name) -> the device predictions of the latest evaluation_epoch)
            predictions = self.__dict__.setdefault('device_predictions', {})
            predictions[(summary_writer is self.gan_summary_writer, summary_name)] = on_device.data
        predicted = on_device.cpu().numpy()
        errors = predicted - dataset.labels
        values = dict(mae=float(np.mean(np.abs(errors))), mse=float(np.mean(np.power(errors, 2))))
        values['rmse'] = values['mse'] ** 0.5
        for key, value in values.items():
            summary_writer.add_scalar(f'{summary_name}/{key.upper()}', value)
        if comparison_values:
            # (the reference's "Ratio MSE" divides the MAE by the DNN's MSE, coefficient/srgan.py:96; kept as it logs it)
            for key, numerator in (('mae', 'mae'), ('mse', 'mae'), ('rmse', 'rmse')):
                summary_writer.add_scalar(f'{summary_name}/Ratio {key.upper()} GAN DNN',
                                          values[numerator] / comparison_values[key])
        values['predicted_labels'] = predicted
        return values

    # ``settings.distribution_summaries``: the reference's distribution outputs of a summary step, computed on the device.
    # Unlike the image summaries this one DOES draw from a host stream -- the reference draws its z from NumPy's global stream
    # at every summary step, and so does this -- which is one more reason it is off by default: switching it on moves every
    # later host draw of z_D.  (Under ``settings.device_random_draws`` the training draws do not come from that stream, and a
    # run trains the same bits with the setting on and off.)
    def distribution_summaries_setting(self):
        return bool(option(self.settings, 'distribution_summaries'))

    def distribution_summaries_on(self):
        """Under data parallelism only the rank that writes the trial's event files launches anything."""
        return self.distribution_summaries_setting() and (self.dp is None or self.dp.rank == 0)

    def summary_set_on_device(self, name, make):
        """A fixed array of a summary step (a slice of a dataset), uploaded once and kept."""
        cache = self.__dict__.setdefault('_summary_sets', {})
        if name not in cache:
            cache[name] = torch.from_numpy(np.ascontiguousarray(make(), dtype=np.float32)).to(current_device())
        return cache[name]

    def distribution_summaries(self, step):
        """Reference coefficient/srgan.py:56-78 as written: z from the two-Gaussian mixture on NumPy's global stream, G without
        noise, D on the generated examples and on the first ``validation_dataset_size`` unlabeled examples; the Wasserstein
        distance between D's predictions on the generated examples and those unlabeled examples' true labels as a scalar of
        the GAN writer (the only download: the finished scalar); and, when the step is a multiple of
        ``summary_step_period``, the ``Distributions`` frame.  Every data-parallel rank draws z -- the ranks' host streams
        stay identical -- and rank 0 alone computes."""
        if not self.distribution_summaries_setting():
            return
        settings = self.settings
        z = self._take_draw('z_summary')
        if z is None:
            z = torch.tensor(MixtureModel([norm(-settings.mean_offset, 1), norm(settings.mean_offset, 1)]).rvs(
                size=[settings.batch_size, self.G.input_size]).astype(np.float32))
        if not self.distribution_summaries_on():
            return
        count = settings.validation_dataset_size
        unlabeled_labels = self.summary_set_on_device('unlabeled labels', lambda: self.unlabeled_dataset.labels[:count])
        unlabeled_examples = self.summary_set_on_device('unlabeled examples', lambda: self.unlabeled_dataset.examples[:count])
        with no_grad():
            fake_examples = self.G(as_var(z), add_noise=False)
            fake_predicted_labels = self.predicted_values(self.D, fake_examples)
            unlabeled_predictions = self.predicted_values(self.D, as_var(unlabeled_examples))
        distance = distribution_summaries.wasserstein_distance(fake_predicted_labels, unlabeled_labels)
        self.gan_summary_writer.add_scalar('Generator/Predicted Label Wasserstein', float(distance))
        if self.dnn_summary_writer.step % settings.summary_step_period == 0:
            predictions = self.device_predictions
            # (the "fake" curve is the four coefficients fitted to the FIRST generated example, presentation.py:24,33 -- not
            # the cubic coefficient of every example; kept as the reference draws it: distribution_summaries.fake_coefficients)
            frame = distribution_summaries.distribution_frame(
                distribution_summaries.fake_coefficients(fake_examples), unlabeled_predictions,
                predictions[(True, '1 Validation Error')], predictions[(True, '2 Train Error')],
                predictions[(False, '1 Validation Error')], predictions[(False, '2 Train Error')])
            self.gan_summary_writer.add_image('Distributions', frame)
