"""Crowd application glue (surface of reference crowd/srgan.py): model setup, the crowd labeled loss on HIP kernels
and the sliding-window inference of a full image.  Dataset loading and the evaluation plots of the
reference are out of scope for the hot path; ``dataset_setup`` provides synthetic
ShanghaiTech-shaped batches."""
import numpy as np
import torch

from .. import functional as F
from .. import image_summaries
from ..settings import option
from ..srgan import Experiment, as_var
from ..tape import no_grad
from .data import CrowdDataset, CrowdExample, DeviceSlidingWindows, ImageSlidingWindowDataset
from .models import DCGenerator, KnnDenseNetCat
from ..synthetic import SyntheticLoader


class CrowdExperiment(Experiment):
    """The crowd application."""

    DATABASE_ENV = 'SRGAN_CROWD_DATABASE'       # e.g. .../ShanghaiTech ; SRGAN_CROWD_DATABASE_PART e.g. part_A

    def dataset_setup(self):
        """Without a database on disk: synthetic (image, head-count label, ikNN map) batches of the reference's batch
        contract (crowd/shanghai_tech_data.py:99-104): image f32[3,S,S] in [-1,1], label f32[S,S], map f32[S,S].
        With ``SRGAN_CROWD_DATABASE`` pointing at a database preprocessed by the reference: the
        ShanghaiTech branch of reference crowd/srgan.py:54-69 -- labeled / unlabeled scenes resident in HBM and cut into
        random patches on the device, the test split behind ``dataset_class`` for the full-image summaries; with
        ``settings.crowd_dataset`` ``'UCF QNRF'`` the UCF-QNRF branch (``ucf_qnrf_dataset_setup``).  With
        ``settings.crowd_validation = 'device'`` (needs the database) the evaluation sets of
        ``validation_summaries`` are attached as well (``attach_evaluation_sets``)."""
        import os
        settings = self.settings
        size = settings.image_patch_size
        directory = os.environ.get(self.DATABASE_ENV)
        validation = option(settings, 'crowd_validation')
        if validation is not None and validation != 'device':
            raise ValueError("settings.crowd_validation is unset or 'device', not {!r}".format(validation))
        if validation is not None and not directory:
            raise ValueError('settings.crowd_validation cuts its evaluation sets from a resident database: it needs {} '
                             '(the synthetic batches have no scenes)'.format(self.DATABASE_ENV))
        if directory and settings.crowd_dataset in (CrowdDataset.ucf_qnrf, CrowdDataset.ucf_qnrf.value):
            self.ucf_qnrf_dataset_setup(directory)
            return
        if directory:
            from .data import DeviceCrowdPatchLoader, PreprocessedCrowdDataset
            part = os.environ.get(self.DATABASE_ENV + '_PART') or None
            maps = settings.map_directory_name

            def scenes(count):
                return PreprocessedCrowdDataset(directory, 'train', part, number_of_examples=count,
                                                map_directory_name=maps).examples()
            labeled, unlabeled = self.patch_loader_arguments()
            self.train_dataset_loader = DeviceCrowdPatchLoader(scenes(settings.labeled_dataset_size), settings.batch_size,
                                                               size, dp=self.dp, **labeled)
            self.unlabeled_dataset_loader = DeviceCrowdPatchLoader(scenes(settings.unlabeled_dataset_size),
                                                                   settings.batch_size, size, dp=self.dp, **unlabeled)
            self.dataset_class = lambda dataset, map_directory_name: PreprocessedCrowdDataset(
                directory, dataset, part, map_directory_name=map_directory_name)
            self.attach_evaluation_sets(lambda count: PreprocessedCrowdDataset(
                directory, 'test', part, number_of_examples=count, map_directory_name=maps).examples())
            return
        self.train_dataset_loader = SyntheticLoader.crowd(settings.batch_size, size, seed=settings.labeled_dataset_seed,
                                                          dp=self.dp)
        self.unlabeled_dataset_loader = SyntheticLoader.crowd(settings.batch_size, size, seed=100, dp=self.dp)

    def patch_loader_arguments(self):
        """``(labeled, unlabeled)`` keyword arguments of the two database loaders under ``self.crowd_patch_draws``.  ``'host'``:
        the private generators' seeds, as ever.  ``'device'``: positions from the counter-based stream under
        ``settings.device_random_seed``, one draw id per loader, so that a batch is a function of ``(seed, step)``
        (``training_loop`` puts the loaders at ``starting_step``)."""
        from .data import CROWD_DRAW_LABELED, CROWD_DRAW_UNLABELED
        if self.crowd_patch_draws not in ('host', 'device'):
            raise ValueError("crowd_patch_draws is 'host' or 'device', not {!r}".format(self.crowd_patch_draws))
        if self.crowd_patch_draws == 'host':
            return dict(seed=self.settings.labeled_dataset_seed), dict(seed=100)
        seed = option(self.settings, 'device_random_seed')
        return (dict(seed=seed, draws='device', draw_id=CROWD_DRAW_LABELED),
                dict(seed=seed, draws='device', draw_id=CROWD_DRAW_UNLABELED))

    def ucf_qnrf_dataset_setup(self, directory):
        """The UCF-QNRF branch of reference crowd/srgan.py:34-52 (``settings.crowd_dataset`` ``CrowdDataset.ucf_qnrf`` or
        ``'UCF QNRF'``): ``<directory>/<Train|Test>/...``, one seeded permutation of the training scenes of which the
        labeled loader keeps the first ``labeled_dataset_size`` and the unlabeled loader the ``unlabeled_dataset_size``
        behind them.  (The full-image walk behind ``dataset_class`` reads the test split in a fixed order -- the
        reference's is unseeded; the totals do not depend on it.)"""
        from .data import DeviceCrowdPatchLoader, UcfQnrfCrowdDataset
        settings = self.settings
        size, maps = settings.image_patch_size, settings.map_directory_name

        def scenes(count, start=None):
            return UcfQnrfCrowdDataset(directory, 'train', seed=settings.labeled_dataset_seed, number_of_examples=count,
                                       map_directory_name=maps, examples_start=start).examples()
        labeled, unlabeled = self.patch_loader_arguments()
        self.train_dataset_loader = DeviceCrowdPatchLoader(scenes(settings.labeled_dataset_size), settings.batch_size, size,
                                                           dp=self.dp, **labeled)
        self.unlabeled_dataset_loader = DeviceCrowdPatchLoader(
            scenes(settings.unlabeled_dataset_size, settings.labeled_dataset_size), settings.batch_size, size, dp=self.dp,
            **unlabeled)
        self.dataset_class = lambda dataset, map_directory_name: UcfQnrfCrowdDataset(
            directory, dataset, seed=0, map_directory_name=map_directory_name)
        self.attach_evaluation_sets(lambda count: UcfQnrfCrowdDataset(
            directory, 'test', seed=101, number_of_examples=count, map_directory_name=maps).examples())

    def attach_evaluation_sets(self, validation_scenes):
        """With ``settings.crowd_validation = 'device'`` (unset: nothing happens here): the
        ``train_dataset`` / ``validation_dataset`` that ``validation_summaries`` evaluates, as fixed patch lists cut on the
        device -- the train set over the labeled loader's resident scenes (seed ``labeled_dataset_seed``, flips), the
        validation set over the test split (seed 101, no flips; reference crowd/srgan.py:36-38,51,55-57,69), of which
        ``settings.crowd_validation_scenes`` (default all) scenes are uploaded.  Under data parallelism only
        the rank that writes the trial's event files holds and evaluates them (the rule of ``image_summaries_on``)."""
        settings = self.settings
        if option(settings, 'crowd_validation') != 'device' or (self.dp is not None and self.dp.rank != 0):
            return
        from .data import ResidentCrowdEvaluationSet
        size = settings.image_patch_size
        self.train_dataset = ResidentCrowdEvaluationSet(self.train_dataset_loader, settings.batch_size, size,
                                                        seed=settings.labeled_dataset_seed, flip=True)
        self.validation_dataset = ResidentCrowdEvaluationSet(
            validation_scenes(option(settings, 'crowd_validation_scenes')), settings.batch_size, size, seed=101,
            flip=False, device=self.train_dataset_loader.device, draws=self.train_dataset_loader.draw_mode)

    def model_setup(self):
        """reference crowd/srgan.py:92-96 (``pretrained=True`` there downloads torchvision weights; offline the
        networks are freshly initialised and a checkpoint can be loaded instead)."""
        size = self.settings.image_patch_size
        self.G = DCGenerator(image_size=size, **self.generator_norm_arguments())
        self.D = KnnDenseNetCat(image_size=size, drop_rate=self.dense_drop_rate())
        self.DNN = KnnDenseNetCat(image_size=size, drop_rate=self.dense_drop_rate())

    def validation_summaries(self, step):
        """The scalar summaries of reference crowd/srgan.py:98-147 when evaluation datasets are attached
        (``train_dataset`` / ``validation_dataset``: indexable, items ``(image, label, map)``; ``dataset_class`` for the
        full-image test summaries).  With ``settings.image_summaries`` the pictures of :119-145 follow the scalars: the map
        comparisons ``Real`` / ``Validation`` of both networks when the datasets are attached (``map_comparison_summaries``)
        and G's samples ``Fake/Standard`` / ``Fake/Offset`` over (-1, 1)."""
        train_dataset = getattr(self, 'train_dataset', None)
        validation_dataset = getattr(self, 'validation_dataset', None)
        if train_dataset is not None and validation_dataset is not None:
            settings = self.settings
            self.evaluation_epoch(settings, self.DNN, train_dataset, self.dnn_summary_writer, '2 Train Error', shuffle=False)
            dnn_validation_count_mae = self.evaluation_epoch(settings, self.DNN, validation_dataset,
                                                             self.dnn_summary_writer, '1 Validation Error', shuffle=False)
            self.evaluation_epoch(settings, self.D, train_dataset, self.gan_summary_writer, '2 Train Error', shuffle=False)
            self.evaluation_epoch(settings, self.D, validation_dataset, self.gan_summary_writer, '1 Validation Error',
                                  comparison_value=dnn_validation_count_mae, shuffle=False)
        if self.image_summaries_on():
            if train_dataset is not None and validation_dataset is not None:
                self.map_comparison_summaries(((self.D, self.gan_summary_writer), (self.DNN, self.dnn_summary_writer)))
            self.generated_image_summaries(range=(-1, 1))
        if getattr(self, 'dataset_class', None) is not None:
            self.test_summaries()

    def map_comparison_summaries(self, networks_and_writers):
        """``Real`` from the first three items of ``train_dataset`` and ``Validation`` from the first three of
        ``validation_dataset``, for every ``(network, writer)``: image | ikNN map | predicted maps (reference
        crowd/srgan.py:119-135, crowd/dnn.py:82-91).  The reference reads ``train_dataset`` for ``Validation`` too (:128) -- a
        slip, the tag says validation -- which is not reproduced."""
        for tag, dataset in (('Real', self.train_dataset), ('Validation', self.validation_dataset)):
            items = [dataset[index] for index in range(min(3, len(dataset)))]
            images = as_var(torch.stack([torch.as_tensor(item[0]) for item in items]).float())
            maps = as_var(torch.stack([torch.as_tensor(item[2]) for item in items]).float())
            for network, writer in networks_and_writers:
                with no_grad():
                    _, _, predicted_maps = self.images_to_predicted_labels(network, images)
                writer.add_image(tag, self.create_map_comparison_image(images, maps, predicted_maps))

    def convert_density_maps_to_heatmaps(self, label, predicted_label):
        """The reference's name (crowd/srgan.py:193-217) for one (map, predicted map) pair ``[h, w]``: the two inferno
        heatmaps ``[3, P, P]`` at ``settings.image_patch_size`` under the pair's common range, on the device."""
        tiles, _ = image_summaries.density_heatmaps(as_var(label).data[None], as_var(predicted_label).data[None, None],
                                                    self.settings.image_patch_size)
        return tiles[0, 0], tiles[0, 1]

    def create_map_comparison_image(self, images, labels, predicted_labels, number_of_images=3):
        """The reference's name (crowd/srgan.py:219-245) for ``image_summaries.map_comparison_image``."""
        return image_summaries.map_comparison_image(images, labels, predicted_labels, number_of_images)

    def images_to_predicted_labels(self, network, images):
        """reference crowd/srgan.py:256-259"""
        predicted_densities, predicted_counts, predicted_maps = network(images)
        return predicted_densities, predicted_counts, predicted_maps

    def evaluation_epoch(self, settings, network, dataset, summary_writer, summary_name, comparison_value=None,
                         shuffle=True):
        """Count ME / MAE / MSE and kNN-map MAE / MSE of ``network`` over batches of ``dataset`` (reference
        crowd/srgan.py:149-191), stopping once more than 100 examples have been seen.  As in the reference, the map
        errors cover the FIRST batch only (its concatenation of the maps sits inside the "still empty" branch).  A dataset
        that offers ``device_batches`` (``ResidentCrowdEvaluationSet``) is evaluated by ``evaluation_epoch_device``."""
        if hasattr(dataset, 'device_batches'):
            return self.evaluation_epoch_device(network, dataset, summary_writer, summary_name, comparison_value)
        self.join_dnn_stream()
        order = np.random.permutation(len(dataset)) if shuffle else np.arange(len(dataset))
        predicted_counts, label_counts = [], []
        maps = predicted_maps = None
        for index, start in enumerate(range(0, len(order), settings.batch_size)):
            items = [dataset[int(i)] for i in order[start:start + settings.batch_size]]
            images = torch.stack([torch.as_tensor(item[0]) for item in items])
            labels = torch.stack([torch.as_tensor(item[1]) for item in items])
            with no_grad():
                _, batch_predicted_counts, batch_predicted_maps = self.images_to_predicted_labels(network, as_var(images))
            predicted_counts.append(batch_predicted_counts.cpu().numpy().reshape(-1).astype(np.float64))
            label_counts.append(labels.cpu().numpy().astype(np.float64).sum(axis=(1, 2)))
            if maps is None:
                maps = np.stack([np.asarray(torch.as_tensor(item[2]).cpu(), dtype=np.float64) for item in items])
                predicted_maps = batch_predicted_maps.cpu().numpy().astype(np.float64)
            if index * settings.batch_size >= 100:
                break
        predicted_counts, label_counts = np.concatenate(predicted_counts), np.concatenate(label_counts)
        maps = np.expand_dims(maps, axis=1)
        count_mae = np.abs(predicted_counts - label_counts).mean()
        summary_writer.add_scalar('{}/ME'.format(summary_name), (predicted_counts - label_counts).mean())
        summary_writer.add_scalar('{}/MAE'.format(summary_name), count_mae)
        summary_writer.add_scalar('{}/kNN MAE'.format(summary_name), np.abs(predicted_maps - maps).mean())
        summary_writer.add_scalar('{}/MSE'.format(summary_name), (np.abs(predicted_counts - label_counts) ** 2).mean())
        summary_writer.add_scalar('{}/kNN MSE'.format(summary_name), (np.abs(predicted_maps - maps) ** 2).mean())
        if comparison_value is not None:
            summary_writer.add_scalar('{}/Ratio MAE GAN DNN'.format(summary_name), count_mae / comparison_value)
        return count_mae

    def evaluation_epoch_device(self, network, dataset, summary_writer, summary_name, comparison_value=None):
        """``evaluation_epoch`` over the device batches of ``dataset`` with nothing but 64 bytes going back to the host:
        per batch the forward pass and one ``srgan_crowd_evaluation_sums`` call into eight doubles on the device (the maps
        are passed for the first batch only, as the reference accumulates them), one download at the end.  The same six
        scalars under the same tags in the same order; returns the count MAE.  The dataset fixes the number of batches
        (``evaluation_batch_count``: the reference's 100-example rule)."""
        from .. import _lib
        self.join_dnn_stream()
        lib = _lib.library()
        sums = scratch = None
        for index, (images, labels, maps) in enumerate(dataset.device_batches()):
            with no_grad():
                _, predicted_counts, predicted_maps = self.images_to_predicted_labels(network, as_var(images))
            predicted_counts = predicted_counts.data.float().reshape(-1).contiguous()
            labels = labels.float().contiguous()
            batch, plane = labels.shape[0], labels.shape[1] * labels.shape[2]
            if predicted_counts.shape[0] != batch:
                raise ValueError('one predicted count per example is evaluated')
            channels = 0
            if index == 0:
                predicted_maps, maps = predicted_maps.data.float().contiguous(), maps.float().contiguous()
                channels = predicted_maps.shape[1]
                if tuple(predicted_maps.shape) != (batch, channels) + tuple(maps.shape[1:]) or maps.shape != labels.shape:
                    raise ValueError('predicted maps {} do not match the maps {}'.format(tuple(predicted_maps.shape),
                                                                                         tuple(maps.shape)))
                sums = torch.zeros(8, dtype=torch.float64, device=labels.device)
            needed = lib.srgan_crowd_evaluation_scratch_bytes(batch, channels, plane)
            if needed < 0:
                _lib.check(int(needed), 'srgan_crowd_evaluation_scratch_bytes')
            if scratch is None or scratch.numel() * 8 < needed:
                scratch = torch.empty((needed + 7) // 8, dtype=torch.float64, device=labels.device)
            _lib.check(lib.srgan_crowd_evaluation_sums(
                predicted_counts.data_ptr(), labels.data_ptr(), predicted_maps.data_ptr() if index == 0 else None,
                maps.data_ptr() if index == 0 else None, batch, channels, plane, sums.data_ptr(), scratch.data_ptr(),
                _lib.stream_handle()), 'srgan_crowd_evaluation_sums')
        if sums is None:
            raise ValueError('the evaluation set is empty')
        difference, absolute, square, examples, map_absolute, map_square, map_elements, _ = sums.cpu().numpy()
        count_mae = absolute / examples
        summary_writer.add_scalar('{}/ME'.format(summary_name), difference / examples)
        summary_writer.add_scalar('{}/MAE'.format(summary_name), count_mae)
        summary_writer.add_scalar('{}/kNN MAE'.format(summary_name), map_absolute / map_elements)
        summary_writer.add_scalar('{}/MSE'.format(summary_name), square / examples)
        summary_writer.add_scalar('{}/kNN MSE'.format(summary_name), map_square / map_elements)
        if comparison_value is not None:
            summary_writer.add_scalar('{}/Ratio MAE GAN DNN'.format(summary_name), count_mae / comparison_value)
        return count_mae

    def test_summaries(self):
        """Full-image test errors of both networks through ``predict_full_example`` (reference crowd/srgan.py:261-300):
        NAE / MAE / RMSE of the count, MAE / RMSE of the density sum, and the GAN-to-DNN ratios."""
        import random
        test_dataset = self.dataset_class(dataset='test', map_directory_name=self.settings.map_directory_name)
        if self.settings.test_summary_size is not None:
            indexes = random.sample(range(test_dataset.length), self.settings.test_summary_size)
        else:
            indexes = range(test_dataset.length)
        dnn_mae_count = dnn_rmse_count = None
        for network in (self.DNN, self.D):
            totals = dict.fromkeys(('Count error', 'NAE', 'Density sum error', 'SE count', 'SE density'), 0.0)
            for index in indexes:
                full_image, full_label, _ = test_dataset[index]
                full_example = CrowdExample(image=full_image, label=full_label)
                predicted_count, predicted_label = self.predict_full_example(full_example, network)
                true_count = full_example.label.sum()
                totals['Count error'] += np.abs(predicted_count - true_count)
                totals['NAE'] += np.abs(predicted_count - true_count) / true_count
                totals['Density sum error'] += np.abs(predicted_label.sum() - true_count)
                totals['SE count'] += (predicted_count - true_count) ** 2
                totals['SE density'] += (predicted_label.sum() - true_count) ** 2
            summary_writer = self.dnn_summary_writer if network is self.DNN else self.gan_summary_writer
            mae_count = totals['Count error'] / len(indexes)
            rmse_count = (totals['SE count'] / len(indexes)) ** 0.5
            summary_writer.add_scalar('0 Test Error/NAE count', totals['NAE'] / len(indexes))
            summary_writer.add_scalar('0 Test Error/MAE count', mae_count)
            summary_writer.add_scalar('0 Test Error/MAE density', totals['Density sum error'] / len(indexes))
            summary_writer.add_scalar('0 Test Error/RMSE count', rmse_count)
            summary_writer.add_scalar('0 Test Error/RMSE density', (totals['SE density'] / len(indexes)) ** 0.5)
            if network is self.DNN:
                dnn_mae_count, dnn_rmse_count = mae_count, rmse_count
            else:
                summary_writer.add_scalar('0 Test Error/Ratio MAE GAN DNN', mae_count / dnn_mae_count)
                summary_writer.add_scalar('0 Test Error/Ratio RMSE GAN DNN', rmse_count / dnn_rmse_count)

    def labeled_loss_function(self, predicted_labels, labels, order=2):
        """count loss + map_multiplier * map loss (reference crowd/srgan.py:247-254)."""
        head_labels, map_labels = labels
        _, predicted_count_labels, predicted_maps = predicted_labels
        map_rows = F.crowd_map_l1(predicted_maps, map_labels)
        map_loss = self.batch_mean_of_examples(F.pow_scalar(map_rows, order))
        head_counts = F.row_sum(head_labels)
        count_loss = self.batch_mean_of_examples(F.pow_scalar(F.abs_(F.sub(predicted_count_labels, head_counts)), order))
        return F.add(count_loss, F.scale(map_loss, self.settings.map_multiplier))

    def predict_full_example(self, full_example, network):
        """Count and density prediction of one full crowd image: every sliding-window patch goes through ``network``
        (batches of ``settings.batch_size``), each patch's density and uniformly spread count are accumulated at its
        position (clipped at the image borders) and divided by the number of patches covering each pixel
        (reference crowd/srgan.py:332-395).  Returns ``(count, density[H, W])`` like the reference.

        The reference resizes every predicted density patch to the patch size with ``scipy.misc.imresize`` (removed
        from SciPy); ``KnnDenseNetCat`` already predicts at the patch size, where that resize is the identity, and
        only that case is supported here; ``predict_full_example_device`` (chosen by ``settings.full_image_inference =
        'device'``; the default is this host path) resizes on the device."""
        if option(self.settings, 'full_image_inference') == 'device':
            return self.predict_full_example_device(full_example, network)
        settings = self.settings
        patch_size = settings.image_patch_size
        half = patch_size // 2
        height, width = full_example.label.shape[0], full_example.label.shape[1]
        sum_density = np.zeros((height, width), dtype=np.float32)
        sum_count = np.zeros((height, width), dtype=np.float32)
        hits = np.zeros((height, width), dtype=np.int32)
        dataset = ImageSlidingWindowDataset(full_example, patch_size, settings.test_sliding_window_size)
        self.join_dnn_stream()
        for start in range(0, len(dataset), settings.batch_size):
            items = [dataset[i] for i in range(start, min(start + settings.batch_size, len(dataset)))]
            images = torch.stack([item[0] for item in items])
            with no_grad():
                densities, counts, _ = network(as_var(images))
            densities, counts = densities.cpu().numpy(), counts.cpu().numpy().reshape(-1)
            for (_, x, y), density, count in zip(items, densities, counts):
                if density.shape != (patch_size, patch_size):
                    raise NotImplementedError('density predictions at another resolution than the patch need '
                                              'scipy.misc.imresize, which SciPy removed (predict_full_example_device '
                                              'resizes them on the device)')
                count_array = np.full(density.shape, count / density.size, dtype=np.float32)
                y_start = half - y if y - half < 0 else 0
                y_end = y + half - height if y + half > height else 0
                x_start = half - x if x - half < 0 else 0
                x_end = x + half - width if x + half > width else 0
                target = (slice(y - half + y_start, y + half - y_end), slice(x - half + x_start, x + half - x_end))
                source = (slice(y_start, density.shape[0] - y_end), slice(x_start, density.shape[1] - x_end))
                sum_density[target] += density[source]
                sum_count[target] += count_array[source]
                hits[target] += 1
        hits[hits == 0] = 1
        full_density = sum_density / hits.astype(np.float32)
        full_count = np.sum(sum_count / hits.astype(np.float32))
        return full_count, full_density

    def predict_full_example_device(self, full_example, network):
        """``predict_full_example`` with everything around the network on the device: the scene is uploaded once, the
        windows are cut by ``DeviceSlidingWindows``, per-window counts and densities stay in device buffers (a density
        predicted below the patch resolution goes through ``srgan_crowd_resize_bilinear``, the float-mode resize the
        reference's ``imresize(..., mode='F')`` meant), one ``srgan_crowd_blend_windows`` launch averages the overlaps,
        and count and density come back in one download.  Same return contract: ``(count, density[H, W])``.

        A network whose density is the all-zero placeholder (``density_is_placeholder``: ``KnnDenseNetCat``) has none
        stored or read; both output arities work (``(density, count, maps)`` and ``JointDCDiscriminator``'s
        ``(density, count)``)."""
        from .. import _lib
        settings = self.settings
        patch_size = settings.image_patch_size
        height, width = full_example.label.shape[0], full_example.label.shape[1]
        windows = DeviceSlidingWindows(full_example, settings.batch_size, patch_size, settings.test_sliding_window_size)
        if len(windows) == 0:           # (an image of at most half a patch has no window: nothing is predicted)
            return np.float32(0.0), np.zeros((height, width), dtype=np.float32)
        self.join_dnn_stream()
        lib, device = _lib.library(), windows.upload().device
        placeholder = getattr(network, 'density_is_placeholder', False)
        counts = torch.empty(len(windows), dtype=torch.float32, device=device)
        densities = None if placeholder else torch.empty((len(windows), patch_size, patch_size), dtype=torch.float32,
                                                         device=device)
        for first, images in windows:
            with no_grad():
                outputs = network(as_var(images))
            density, count = outputs[0].data, outputs[1].data
            batch = images.shape[0]
            counts[first:first + batch].copy_(count.reshape(-1))
            if placeholder:
                continue
            if tuple(density.shape[1:]) == (patch_size, patch_size):
                densities[first:first + batch].copy_(density)
            else:
                density = density.float().contiguous()
                _lib.check(lib.srgan_crowd_resize_bilinear(
                    density.data_ptr(), batch, density.shape[1], density.shape[2], patch_size,
                    densities[first:first + batch].data_ptr(), _lib.stream_handle()), 'srgan_crowd_resize_bilinear')
        result = torch.empty(height * width + 1, dtype=torch.float32, device=device)     # [density | count]: one download
        _lib.check(lib.srgan_crowd_blend_windows(
            0 if placeholder else densities.data_ptr(), counts.data_ptr(), windows.device_ys.data_ptr(), len(windows.ys),
            windows.device_xs.data_ptr(), len(windows.xs), height, width, patch_size, result.data_ptr(),
            result.data_ptr() + 4 * height * width, _lib.stream_handle()), 'srgan_crowd_blend_windows')
        result = result.cpu().numpy()
        return result[-1], result[:-1].reshape(height, width)

    def inference(self, input_):
        """Count and density of one uint8 image ``[H, W, 3]`` through ``inference_network`` (reference
        crowd/srgan.py:424-436, without its timing print), on the device path."""
        example = CrowdExample(image=input_, label=np.zeros(input_.shape[:2], dtype=np.float32))
        return self.predict_full_example_device(example, self.inference_network)

    def evaluate(self, during_training=False, step=None, number_of_examples=None):
        """The full-image test totals of the DNN and the GAN discriminator (reference crowd/srgan.py:302-330) over
        ``self.dataset_class(dataset='test', ...)``, printed as there and returned as ``{'DNN': {...}, 'GAN': {...}}``:
        the reference's totals plus 'MAE count', 'MAE density', 'MSE count', 'MSE density'.  ``during_training``: the
        networks are already set up, nothing is loaded; ``number_of_examples`` limits the walk to the first examples."""
        if not during_training:
            super().evaluate()
        results = {}
        for name, network in (('DNN', self.DNN), ('GAN', self.D)):
            test_dataset = self.dataset_class(dataset='test', map_directory_name=self.settings.map_directory_name)
            length = test_dataset.length if number_of_examples is None else min(number_of_examples, test_dataset.length)
            totals = dict.fromkeys(('Count', 'Density error', 'Count error', 'Density sum error', 'Predicted count',
                                    'Predicted density sum', 'SE count', 'SE density'), 0.0)
            for index in range(length):
                full_image, full_label = test_dataset[index][:2]
                full_example = CrowdExample(image=full_image, label=full_label)
                predicted_count, predicted_label = self.predict_full_example(full_example, network)
                true_count = full_example.label.sum()
                totals['Count'] += true_count
                totals['Density error'] += np.abs(predicted_label - full_example.label).sum()
                totals['Count error'] += np.abs(predicted_count - true_count)
                totals['Density sum error'] += np.abs(predicted_label.sum() - true_count)
                totals['Predicted count'] += predicted_count
                totals['Predicted density sum'] += predicted_label.sum()
                totals['SE count'] += (predicted_count - true_count) ** 2
                totals['SE density'] += (predicted_label.sum() - true_count) ** 2
            print('=== {} ==='.format(name))
            summary = {'MAE count': totals['Count error'] / length, 'MAE density': totals['Density sum error'] / length,
                       'MSE count': totals['SE count'] / length, 'MSE density': totals['SE density'] / length}
            for key, value in summary.items():
                print('{}: {}'.format(key, value))
            for key, value in totals.items():
                print('Total {}: {}'.format(key, value))
            results[name] = {key: float(value) for key, value in {**totals, **summary}.items()}
        return results
