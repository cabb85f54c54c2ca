"""Age application (surface of reference age/srgan.py:17-51).  Without a database ``dataset_setup`` yields synthetic
faces of the reference's batch contract (image f32[3,S,S] in [-1,1], age in [10, 95]); with ``SRGAN_AGE_DATABASE`` it
trains on a preprocessed IMDB-WIKI / LAP directory resident on the device (``age/data.py``; the downloads are out of
scope)."""
import os

from ..srgan import Experiment
from ..synthetic import SyntheticLoader
from .models import Generator, Discriminator
from .vgg import vgg16

model_architecture = 'dcgan'  # dcgan or vgg (reference age/srgan.py:14)


class AgeExperiment(Experiment):
    """The age estimation application."""
    image_size = None      # None = the architecture's native size (128 dcgan / 224 vgg)

    def _size(self):
        if self.image_size is not None:
            return self.image_size
        return 224 if model_architecture == 'vgg' else 128

    DATABASE_ENV = 'SRGAN_AGE_DATABASE'          # a directory with meta.json and the preprocessed images

    def dataset_setup(self):
        settings = self.settings
        directory = os.environ.get(self.DATABASE_ENV)
        if directory:
            from ..data import database_loaders
            from .data import age_datasets
            database_loaders(self, age_datasets(directory, settings), self._size())
            return
        self.train_dataset_loader = SyntheticLoader.images(settings.batch_size, self._size(), (10.0, 95.0),
                                                           seed=settings.labeled_dataset_seed, dp=self.dp)
        self.unlabeled_dataset_loader = SyntheticLoader.images(settings.batch_size, self._size(), (10.0, 95.0),
                                                               seed=100, dp=self.dp)
        self.validation_dataset_loader = SyntheticLoader.images(settings.batch_size, self._size(), (10.0, 95.0),
                                                                seed=101, dp=self.dp, pool=1)

    def model_setup(self):
        """reference age/srgan.py:42-51 (``pretrained=True`` VGG weights need a download: load a checkpoint)."""
        size = self._size()
        d_norm = self.discriminator_norm_arguments()
        if model_architecture == 'vgg':
            self.G = Generator(image_size=size, **self.generator_norm_arguments())
            self.D = vgg16(num_classes=1, image_size=size)
            self.DNN = vgg16(num_classes=1, image_size=size)
        else:
            self.G = Generator(image_size=size, **self.generator_norm_arguments())
            self.D = Discriminator(image_size=size, **d_norm)
            self.DNN = Discriminator(image_size=size, **d_norm)

    def validation_summaries(self, step):
        """MAE / MSE of DNN and D on the train and validation batches (reference age/srgan.py:52-71,92-107) and, with
        ``settings.image_summaries``, the ``Real`` / ``Fake/Standard`` / ``Fake/Offset`` grids (:73-90)."""
        self.regression_validation_summaries()
        self.regression_image_summaries()
