"""Driving (steering-angle) application (surface of reference driving/srgan.py:17-46): DCGAN D / G.  The
reference resizes frames to 128x128 (driving/data.py:56,123); ``image_size`` may be set to (64, 192) for the
66x200-derived rectangular shape of BASELINE config 5.  With ``SRGAN_DRIVING_DATABASE`` it trains on a
preprocessed steering-angle directory resident on the device (``driving/data.py``), resampled to ``image_size`` when the
stored frames differ."""
import math
import os

from ..srgan import Experiment
from ..synthetic import SyntheticLoader
from .models import Generator, Discriminator


class DrivingExperiment(Experiment):
    image_size = 128

    DATABASE_ENV = 'SRGAN_DRIVING_DATABASE'      # a directory with meta.pkl and the preprocessed frames

    def dataset_setup(self):
        settings = self.settings
        directory = os.environ.get(self.DATABASE_ENV)
        if directory:
            from ..data import database_loaders
            from .data import driving_datasets
            database_loaders(self, driving_datasets(directory, settings), self.image_size)
            return
        angle = math.pi / 2
        self.train_dataset_loader = SyntheticLoader.images(settings.batch_size, self.image_size, (-angle, angle),
                                                           seed=settings.labeled_dataset_seed, dp=self.dp)
        self.unlabeled_dataset_loader = SyntheticLoader.images(settings.batch_size, self.image_size, (-angle, angle),
                                                               seed=100, dp=self.dp)
        self.validation_dataset_loader = SyntheticLoader.images(settings.batch_size, self.image_size, (-angle, angle),
                                                                seed=101, dp=self.dp, pool=1)

    def model_setup(self):
        d_norm = self.discriminator_norm_arguments()
        self.G = Generator(image_size=self.image_size, **self.generator_norm_arguments())
        self.D = Discriminator(image_size=self.image_size, **d_norm)
        self.DNN = Discriminator(image_size=self.image_size, **d_norm)

    def validation_summaries(self, step):
        """MAE / NMAE / MSE of DNN and D on the train and validation batches (reference driving/srgan.py:48-67,87-104)
        and, with ``settings.image_summaries``, the ``Real`` / ``Fake/Standard`` / ``Fake/Offset`` grids (:68-85)."""
        self.regression_validation_summaries(normalized=True)
        self.regression_image_summaries()
