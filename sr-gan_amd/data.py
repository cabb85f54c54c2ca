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


# The draw ids of the two loaders' device draws (SRGAN_IMAGE_BATCH_DRAW_* in include/srgan_hip.h), next to the crowd loaders'
# 0x30000 / 0x30001, and the most frames ``srgan_epoch_order`` ranks (SRGAN_EPOCH_ORDER_MAX).
IMAGE_DRAW_LABELED, IMAGE_DRAW_UNLABELED = 0x30002, 0x30003
EPOCH_ORDER_MAX = 1 << 20


class ResidentImageLoader:
    """Batches ``(image f32[B, C, H, W], label f32[B])`` gathered on the device -- ``SyntheticLoader.images``' contract.

    Iterating is ONE epoch of the reference's ``DataLoader(shuffle=True, drop_last=True)``: a fresh permutation from a
    private CPU ``torch.Generator`` (seeded once, so the next epoch's order differs) is uploaded as one int32 tensor, then
    ``len(dataset) // batch_size`` batches follow, each one launch reading its slice of that tensor.
    ``Experiment.infinite_iter`` re-iterates for the next epoch.  ``in_order()`` walks the dataset once in stored order
    and keeps the short last batch: the reference's ``DataLoader(dataset, batch_size)`` of ``evaluation_epoch``.

    ``image_size`` (an int or ``(H, W)``; default: the frames' own) is the size the kernel delivers; it resamples when
    the stored size differs.  ``batch_size`` is the GLOBAL batch: under data parallelism (``dp``) every rank draws the
    same permutation from the shared seed and gathers only its own contiguous slice; ``in_order()`` is not sharded.

    ``draws='device'`` takes the epoch order off the host: epoch ``e`` orders the frames by the 64-bit
    keys of draw ``draw_id`` of the port's counter-based stream under ``seed`` (``srgan_epoch_order``, include/srgan_hip.h),
    and the batch of training step ``t`` is rows ``(t % len(self)) * batch_size ...`` of the order of epoch
    ``t // len(self)``: a function of ``(seed, t)``.  ``device_batch()`` is one batch -- the rebuild of the order at an
    epoch start, ``srgan_epoch_batch_indices``, the gather and ``srgan_random_advance``: at most four launches, no copy, no
    argument that depends on the step, so they can be recorded in a HIP graph.  ``start_at(step)`` puts the loader at a
    step (a continued run: its ``starting_step``), ``last_table`` is the ``int32 [local batch]`` index table of the latest
    batch.  Iterating yields ``len(self)`` such batches.  Under ``dp`` every rank rebuilds the whole order (the same bits)
    and takes its own rows of the global batch."""
    # The DATABASE is resident, the batches are not: each is a fresh tensor that a kernel on the current stream fills.  A
    # consumer on another stream has to wait for that stream, and the batch must outlive its DNN step -- which is what
    # Experiment does for a loader that is not ``resident`` in SyntheticLoader's sense (pre-built batches, never freed).
    resident = False

    def __init__(self, dataset, batch_size, image_size=None, shuffle=True, seed=0, dp=None, draws='host',
                 draw_id=IMAGE_DRAW_LABELED):
        if draws not in ('host', 'device'):
            raise ValueError("draws is 'host' or 'device', not {!r}".format(draws))
        self.dp = dp if dp is not None and dp.world_size > 1 else None
        self.local_batch = self.dp.local_batch(batch_size) if self.dp is not None else batch_size    # raises unless it divides
        self.dataset, self.batch_size, self.shuffle = dataset, batch_size, shuffle
        if image_size is None:
            image_size = dataset.frame_shape[1:]
        self.image_size = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        self.generator = torch.Generator().manual_seed(seed) if draws == 'host' else None      # (a device seed has 64 bits)
        self._order = self._stored_order = None
        self.draw_mode, self.draw_id, self.seed = draws, int(draw_id), seed
        self.state = self.order = self.last_table = None
        self._step = None              # device draws: the host's copy of the state's iteration word
        self._rebuild = True           # ... and whether ``order`` has yet to be built for the epoch of that step
        if draws == 'device':
            if not shuffle:
                raise ValueError("draws='device' is a shuffled order: a loader with shuffle=False walks the stored order")
            if not 0 <= self.draw_id < 2 ** 31:
                raise ValueError('draw_id is a non-negative 32-bit integer')
            if len(self) == 0:
                raise ValueError(f'{len(dataset)} examples do not fill one batch of {batch_size}')
            if len(dataset) > EPOCH_ORDER_MAX:
                raise ValueError(f'draws=\'device\' orders at most {EPOCH_ORDER_MAX} frames, not {len(dataset)}')

    def __len__(self):
        return len(self.dataset) // self.batch_size

    # ---- draws='device' ---------------------------------------------------------------------------------------------
    def _require_device_draws(self, what):
        if self.draw_mode != 'device':
            raise ValueError(f"{what} belongs to draws='device': the host generator has no position to set")

    def prepare_capture(self):
        """Device draws: the persistent buffers -- the 16-byte state and ``order`` -- exist, and ``order`` holds the epoch
        of the current step.  Called before a HIP graph capture that records ``device_batch()``: inside a capture nothing
        may be uploaded, these two must not live in the graph's memory pool (they carry the loader from replay to replay),
        and the recorded rebuild is the conditional one, which leaves an order alone in the middle of an epoch."""
        self._require_device_draws('prepare_capture')
        if self.state is None:
            self.start_at(0)
        if self._rebuild:
            self._build_order(conditional=0)
        return self

    def start_at(self, step):
        """Device draws: the next batch is that of training step ``step``; the order is rebuilt before it is cut."""
        self._require_device_draws('start_at')
        from .nn import draw_state
        state = draw_state(self.seed, step).to(self.dataset.upload().device)
        if self.state is None:         # allocated once: a recorded launch keeps reading these addresses
            self.state = state
            self.order = torch.empty((len(self.dataset),), dtype=torch.int32, device=state.device)
        else:
            self.state.copy_(state)
        self._step, self._rebuild = int(step) & 0xffffffff, True

    def _build_order(self, conditional):
        from . import _lib
        _lib.check(_lib.library().srgan_epoch_order(len(self.dataset), len(self), conditional, self.draw_id,
                                                     self.state.data_ptr(), self.order.data_ptr(), _lib.stream_handle()),
                   'srgan_epoch_order')
        self._rebuild = False

    def batch_shapes(self):
        """The shapes of one batch ``(images, labels)`` of this rank."""
        return (self.local_batch, self.dataset.frame_shape[0]) + self.image_size, (self.local_batch,)

    def device_batch(self):
        """Device draws: one batch -- rebuild at an epoch start, index table, gather, advance -- enqueued on the current
        stream.  The host skips the rebuild when it knows that the step is not an epoch start; while a HIP graph is being
        captured it records the conditional rebuild, which decides that on the device (``replayed()`` keeps the host's
        count of the steps in line with the replays)."""
        self._require_device_draws('device_batch')
        from . import _lib
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and (self.state is None or self._rebuild):
            raise RuntimeError('prepare_capture() comes before a capture that records device_batch()')
        if self.state is None:
            self.start_at(0)
        if capturing:
            self._build_order(conditional=1)
        elif self._rebuild or self._step % len(self) == 0:
            self._build_order(conditional=0)
        lib, stream = _lib.library(), _lib.stream_handle()
        table = torch.empty((self.local_batch,), dtype=torch.int32, device=self.order.device)
        _lib.check(lib.srgan_epoch_batch_indices(
            self.order.data_ptr(), len(self.dataset), self.batch_size, len(self),
            self.dp.rank * self.local_batch if self.dp is not None else 0, self.local_batch, self.state.data_ptr(),
            table.data_ptr(), stream), 'srgan_epoch_batch_indices')
        batch = self.gather(table, 0, self.local_batch)
        _lib.check(lib.srgan_random_advance(self.state.data_ptr(), stream), 'srgan_random_advance')
        self.last_table = table
        if not capturing:              # (a capture records the launches, it does not run them)
            self._step = (self._step + 1) & 0xffffffff
        return batch

    def replayed(self, count=1):
        """``count`` recorded ``device_batch()`` calls have been replayed: the device state moved on without the host."""
        self._step = (self._step + count) & 0xffffffff

    def epoch_order(self):
        """The next epoch's index list (host, int32)."""
        if self.draw_mode != 'host':
            raise ValueError("epoch_order belongs to draws='host': the device order is the loader's ``order`` tensor")
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
        if self.draw_mode == 'device':
            for _ in range(len(self)):
                yield self.device_batch()
            return
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
    # experiment.image_batch_draws: 'host' -- the private generators' seeds, as ever; 'device' -- the epoch orders from the
    # counter-based stream under settings.device_random_seed, one draw id per loader, so that a batch is a function of
    # (seed, step) (training_loop puts the loaders at starting_step)
    draws = getattr(experiment, 'image_batch_draws', 'host')
    if draws not in ('host', 'device'):
        raise ValueError("image_batch_draws is 'host' or 'device', not {!r}".format(draws))
    if draws == 'host':
        labeled_arguments, unlabeled_arguments = dict(seed=settings.labeled_dataset_seed), dict(seed=100)
    else:
        from .settings import option
        seed = option(settings, 'device_random_seed')
        labeled_arguments = dict(seed=seed, draws='device', draw_id=IMAGE_DRAW_LABELED)
        unlabeled_arguments = dict(seed=seed, draws='device', draw_id=IMAGE_DRAW_UNLABELED)
    experiment.train_dataset_loader = ResidentImageLoader(train, settings.batch_size, image_size, dp=experiment.dp,
                                                          **labeled_arguments)
    experiment.unlabeled_dataset_loader = ResidentImageLoader(unlabeled, settings.batch_size, image_size, dp=experiment.dp,
                                                              **unlabeled_arguments)
    experiment.validation_dataset_loader = ResidentImageLoader(validation, settings.batch_size, image_size, shuffle=False,
                                                               dp=experiment.dp)
