"""A database of equally sized frames with one scalar label each, resident on the device, and the loader that
assembles training batches from it there (age and driving; the crowd application's counterpart is
``crowd.data.DeviceCrowdPatchLoader``).  The reference reads every example from disk in ``Dataset.__getitem__`` and
collates batches in a ``DataLoader`` with worker processes (age/data.py:52-60, driving/data.py:44-51, age/srgan.py:29-31);
here the whole split is uploaded once and a batch is one ``srgan_image_batch_gather`` launch: a shuffled gather, the
[-1, 1] normalisation and an optional bilinear resize, with no host-to-device copy per batch."""
import numpy as np
import torch


class ResidentImageDataset:
    """``images``: an array or a list of ``[C, h, w]`` frames of one shape with values in the 0..255 range; an integer
    dtype is stored as uint8, a float dtype as float32 (the reference's driving frames are float64 with non-integer
    values, and it converts them to float32 before normalising: rounding them to uint8 would change the result).
    ``labels``: one float per frame.  ``dataset[i]`` is the reference's item: ``(image f32[C, h, w] in [-1, 1], label)``
    as host tensors (utility.py:129-132).  The device copies are made once, on first use (``upload``)."""

    def __init__(self, images, labels, device=None, names=None):
        images = np.asarray(images)
        if images.ndim != 4:
            raise ValueError('frames must share one [C, h, w] shape')
        self.images = np.ascontiguousarray(images, dtype=np.uint8 if images.dtype.kind in 'iub' else np.float32)
        self.labels = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
        if len(self.labels) != len(self.images):
            raise ValueError('one label per frame')
        self.names = None if names is None else np.asarray(names)
        self.device = device
        self.device_images = self.device_labels = None

    def __len__(self):
        return len(self.images)

    def __getitem__(self, index):
        image = torch.from_numpy(self.images[index].astype(np.float32))
        return (image / 127.5) - 1, torch.tensor(self.labels[index], dtype=torch.float32)

    @property
    def frame_shape(self):
        return tuple(self.images.shape[1:])

    def upload(self):
        if self.device_images is None:
            from .utility import current_device
            self.device = self.device or current_device()
            self.device_images = torch.from_numpy(self.images).to(self.device)
            self.device_labels = torch.from_numpy(self.labels).to(self.device)
        return self


class ResidentImageLoader:
    """Batches ``(image f32[B, C, H, W], label f32[B])`` gathered on the device -- ``SyntheticLoader.images``' contract.

    Iterating is ONE epoch of the reference's ``DataLoader(shuffle=True, drop_last=True)``: a fresh permutation from a
    private CPU ``torch.Generator`` (seeded once, so the next epoch's order differs) is uploaded as one int32 tensor, then
    ``len(dataset) // batch_size`` batches follow, each one launch reading its slice of that tensor.
    ``Experiment.infinite_iter`` re-iterates for the next epoch.  ``in_order()`` walks the dataset once in stored order
    and keeps the short last batch: the reference's ``DataLoader(dataset, batch_size)`` of ``evaluation_epoch``.

    ``image_size`` (an int or ``(H, W)``; default: the frames' own) is the size the kernel delivers; it resamples when
    the stored size differs.  ``batch_size`` is the GLOBAL batch: under data parallelism (``dp``) every rank draws the
    same permutation from the shared seed and gathers only its own contiguous slice; ``in_order()`` is not sharded."""
    # The DATABASE is resident, the batches are not: each is a fresh tensor that a kernel on the current stream fills.  A
    # consumer on another stream has to wait for that stream, and the batch must outlive its DNN step -- which is what
    # Experiment does for a loader that is not ``resident`` in SyntheticLoader's sense (pre-built batches, never freed).
    resident = False

    def __init__(self, dataset, batch_size, image_size=None, shuffle=True, seed=0, dp=None):
        self.dp = dp if dp is not None and dp.world_size > 1 else None
        self.local_batch = self.dp.local_batch(batch_size) if self.dp is not None else batch_size    # raises unless it divides
        self.dataset, self.batch_size, self.shuffle = dataset, batch_size, shuffle
        if image_size is None:
            image_size = dataset.frame_shape[1:]
        self.image_size = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        self.generator = torch.Generator().manual_seed(seed)
        self._order = self._stored_order = None

    def __len__(self):
        return len(self.dataset) // self.batch_size

    def epoch_order(self):
        """The next epoch's index list (host, int32)."""
        count = len(self.dataset)
        order = torch.randperm(count, generator=self.generator) if self.shuffle else torch.arange(count)
        return order.to(torch.int32)

    def to_device(self, order):
        return order.to(self.dataset.upload().device)

    def gather(self, order, first, count):
        """Examples ``order[first : first + count]`` (``order``: an int32 device tensor) as one device batch."""
        from . import _lib
        dataset = self.dataset.upload()
        channels, stored_height, stored_width = dataset.frame_shape
        height, width = self.image_size
        images = torch.empty((count, channels, height, width), dtype=torch.float32, device=dataset.device)
        labels = torch.empty((count,), dtype=torch.float32, device=dataset.device)
        _lib.check(_lib.library().srgan_image_batch_gather(
            dataset.device_images.data_ptr(), 0 if dataset.images.dtype == np.uint8 else 1, len(dataset), channels,
            stored_height, stored_width, dataset.device_labels.data_ptr(), order.data_ptr(), first, count, height, width,
            images.data_ptr(), labels.data_ptr(), _lib.stream_handle()), 'srgan_image_batch_gather')
        return images, labels

    def __iter__(self):
        if len(self) == 0:
            raise ValueError(f'{len(self.dataset)} examples do not fill one batch of {self.batch_size}')
        # the kernel reads the index list asynchronously: it stays referenced until the next epoch replaces it
        self._order = order = self.to_device(self.epoch_order())
        offset = self.dp.rank * self.local_batch if self.dp is not None else 0
        for batch in range(len(self)):
            yield self.gather(order, batch * self.batch_size + offset, self.local_batch)

    def in_order(self):
        """An iterable over the whole dataset in stored order, ``ceil(len / batch_size)`` batches."""
        return _InOrder(self)


class _InOrder:
    def __init__(self, loader):
        self.loader = loader

    def __iter__(self):
        loader, count = self.loader, len(self.loader.dataset)
        if loader._stored_order is None:
            loader._stored_order = loader.to_device(torch.arange(count, dtype=torch.int32))
        for first in range(0, count, loader.batch_size):
            yield loader.gather(loader._stored_order, first, min(loader.batch_size, count - first))


def split_slices(labeled, validation, unlabeled, unlabeled_starts_after_validation_size):
    """The reference's three slices of the shuffled database as Python slices ``(train, unlabeled, validation)``.
    Driving (driving/srgan.py:21-37) starts the unlabeled slice at ``labeled + validation``; age (age/srgan.py:27-40)
    starts it at ``labeled``.  ``unlabeled=None`` ends it where the validation tail begins (driving/srgan.py:33-34; the
    reference's age code has no value for that case, it adds ``None``)."""
    start = labeled + (validation if unlabeled_starts_after_validation_size else 0)
    end = start + unlabeled if unlabeled is not None else -validation
    return slice(0, labeled), slice(start, end), slice(-validation, None)


def repeat_to_batch(names, labels, batch_size):
    """A slice shorter than the batch is repeated element by element -- a a b b, not a b a b -- ``ceil(batch / n)``
    times (age/data.py:43-46, driving/data.py:34-37)."""
    if len(names) < batch_size:
        repeats = int(np.ceil(batch_size / len(names)))
        names, labels = np.repeat(names, repeats), np.repeat(labels, repeats)
    return names, labels


def database_loaders(experiment, datasets, image_size):
    """The three loaders of an experiment from its ``(train, unlabeled, validation)`` datasets, and the
    ``train_dataset`` / ``validation_dataset`` attributes the reference sets (age/srgan.py:27-40)."""
    settings = experiment.settings
    train, unlabeled, validation = datasets
    experiment.train_dataset, experiment.unlabeled_dataset, experiment.validation_dataset = train, unlabeled, validation
    experiment.train_dataset_loader = ResidentImageLoader(train, settings.batch_size, image_size,
                                                          seed=settings.labeled_dataset_seed, dp=experiment.dp)
    experiment.unlabeled_dataset_loader = ResidentImageLoader(unlabeled, settings.batch_size, image_size, seed=100,
                                                              dp=experiment.dp)
    experiment.validation_dataset_loader = ResidentImageLoader(validation, settings.batch_size, image_size, shuffle=False,
                                                               dp=experiment.dp)
