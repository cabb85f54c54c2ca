"""DNN-only crowd experiment (reference crowd/dnn.py:20): ``DnnExperiment`` mixed into the crowd application."""
from ..dnn import DnnExperiment
from .models import KnnDenseNetCat
from .srgan import CrowdExperiment


class CrowdDnnExperiment(DnnExperiment, CrowdExperiment):
    """The DNN-only version of the crowd application."""

    def model_setup(self):
        self.DNN = KnnDenseNetCat(image_size=self.settings.image_patch_size, drop_rate=self.dense_drop_rate())

    def validation_summaries(self, step):
        """The DNN's scalar epochs and, with ``settings.image_summaries``, its map comparisons ``Real`` / ``Validation`` when
        evaluation datasets are attached (reference crowd/dnn.py:71-91; the full-image test summaries of :93 are not part of
        the DNN-only trial here)."""
        train_dataset = getattr(self, 'train_dataset', None)
        validation_dataset = getattr(self, 'validation_dataset', None)
        if train_dataset is None or validation_dataset is None:
            return
        self.evaluation_epoch(self.settings, self.DNN, train_dataset, self.dnn_summary_writer, '2 Train Error', shuffle=False)
        self.evaluation_epoch(self.settings, self.DNN, validation_dataset, self.dnn_summary_writer, '1 Validation Error',
                              shuffle=False)
        if self.image_summaries_on():
            self.map_comparison_summaries(((self.DNN, self.dnn_summary_writer),))
