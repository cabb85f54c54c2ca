"""Inference-side data handling of the crowd application: the sliding-window patches of one full
image (reference crowd/data.py:370-453,521-560) and the uint8 -> [-1, 1] normalisation (crowd/data.py:115-128).
``ImageSlidingWindowDataset`` is the host-side NumPy form and the single source of the window positions;
``DeviceSlidingWindows`` cuts the same windows on the device from a scene resident in HBM, as ``DeviceCrowdPatchLoader``
does for training batches; ``ResidentCrowdEvaluationSet`` holds the fixed patches a validation epoch scores (DESIGN.md
section 3h).  The reference's training datasets / preprocessors stay out of scope."""
from enum import Enum

import numpy as np
import torch


class CrowdExample:
    """Image (H, W, 3) and optional per-pixel label / map of one crowd scene (reference crowd/data.py:21-40)."""

    def __init__(self, image, label=None, roi=None, perspective=None, patch_center_y=None, patch_center_x=None, map_=None):
        self.image, self.label, self.roi, self.perspective, self.map = image, label, roi, perspective, map_
        self.patch_center_y, self.patch_center_x = patch_center_y, patch_center_x


def extract_padded_patch(image, y, x, patch_size):
    """The ``patch_size`` square centred on (y, x), zero-padded where it leaves the image, with the reference's
    order of operations (crowd/data.py:390-407: pad top / left first and move the centre, then pad bottom / right)."""
    half = int(patch_size // 2)
    if y - half < 0:
        image = np.pad(image, ((half - y, 0), (0, 0), (0, 0)), 'constant')
        y = half
    if y + half > image.shape[0]:
        image = np.pad(image, ((0, y + half - image.shape[0]), (0, 0), (0, 0)), 'constant')
    if x - half < 0:
        image = np.pad(image, ((0, 0), (half - x, 0), (0, 0)), 'constant')
        x = half
    if x + half > image.shape[1]:
        image = np.pad(image, ((0, 0), (0, x + half - image.shape[1]), (0, 0)), 'constant')
    return image[y - half:y + half, x - half:x + half, :]


def negative_one_to_one(image):
    """uint8 [0, 255] -> float32 [-1, 1] (crowd/data.py:127)."""
    return (image.astype(np.float32) / (255 / 2)) - 1


class ImageSlidingWindowDataset:
    """Every sliding-window patch of one full example: ``(image f32[3, P, P], x, y)`` per index (reference
    crowd/data.py:521-560).  Window centres run from half a patch in steps of ``window_step_size``; one more centre
    sits half a patch from the far edge, so an image smaller than a patch still yields one (padded) patch."""

    def __init__(self, full_example, image_patch_size=128, window_step_size=32):
        self.image = full_example.image
        self.window_step_size, self.image_patch_size = window_step_size, image_patch_size
        half = int(image_patch_size // 2)
        height, width = self.image.shape[0], self.image.shape[1]
        self.y_positions = list(range(half, height - half + 1, window_step_size))
        if height - half > 0:
            self.y_positions = sorted(set(self.y_positions + [height - half]))
        self.x_positions = list(range(half, width - half + 1, window_step_size))
        if width - half > 0:
            self.x_positions = sorted(set(self.x_positions + [width - half]))
        self.positions_shape = np.array([len(self.y_positions), len(self.x_positions)])
        self.length = int(self.positions_shape.prod())

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        y_index, x_index = np.unravel_index(index, self.positions_shape)
        y, x = self.y_positions[y_index], self.x_positions[x_index]
        patch = negative_one_to_one(extract_padded_patch(self.image, y, x, self.image_patch_size))
        return torch.from_numpy(np.ascontiguousarray(patch.transpose((2, 0, 1)))), x, y


class PreprocessedCrowdDataset:
    """Full-image examples of a crowd database in the on-disk layout the reference's preprocessors write and its
    ``ShanghaiTechFullImageDataset`` / ``UcfQnrfFullImageDataset`` read (crowd/shanghai_tech_data.py:18-44,
    crowd/ucf_qnrf_data.py): ``<database_directory>/[<part>/]<dataset>_data/{images,labels,<map_directory_name>}/*.npy``
    (image u8[H, W, 3], head-count label f32[H, W], ikNN map f32[H, W]).  ``__getitem__`` returns ``(image, label,
    map)`` like the reference; ``examples()`` gives the ``CrowdExample``s that ``DeviceCrowdPatchLoader`` keeps resident
    (training) and ``CrowdExperiment.test_summaries`` walks (evaluation).  The database directory is passed in (the
    reference takes it from its preprocessor object)."""

    def __init__(self, database_directory, dataset='train', part=None, number_of_examples=None,
                 map_directory_name='knn_maps'):
        import os
        pieces = [database_directory] + ([part] if part else []) + ['{}_data'.format(dataset)]
        self.dataset_directory = os.path.join(*pieces)
        names = [name for name in os.listdir(os.path.join(self.dataset_directory, 'labels')) if name.endswith('.npy')]
        self.file_names = sorted(names)[:number_of_examples]       # (the reference keeps the directory's own order)
        self.length = len(self.file_names)
        self.map_directory_name = map_directory_name

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        import os
        file_name = self.file_names[index]
        return tuple(np.load(os.path.join(self.dataset_directory, directory, file_name))
                     for directory in ('images', 'labels', self.map_directory_name))

    def examples(self):
        return [CrowdExample(image=image, label=label, map_=map_) for image, label, map_ in
                (self[index] for index in range(self.length))]


class CrowdDataset(Enum):
    """Selects the crowd dataset (``settings.crowd_dataset``; reference crowd/data.py:13-18)."""
    ucf_qnrf = 'UCF QNRF'
    shanghai_tech = 'ShanghaiTech'
    world_expo = 'World Expo'


class UcfQnrfCrowdDataset:
    """Full-image examples of a UCF-QNRF database as the reference's preprocessor writes it and its
    ``UcfQnrfFullImageDataset`` reads it (crowd/ucf_qnrf_data.py:18-53): ``<database_directory>/<Train|Test>/{images,
    labels,<map_directory_name>}/*.npy``.  The ``.npy`` names of ``labels`` are sorted and then shuffled by
    ``random.Random(seed)`` -- the permutation the reference's ``seed_all(seed); random.shuffle(...)`` gives on a sorted
    listing (it shuffles the directory's own order) -- and sliced ``[examples_start : examples_start +
    number_of_examples]`` with the reference's ``None`` rules: the labeled scenes are the first ``labeled_dataset_size``
    of the permutation, the unlabeled ones those behind them.  ``__getitem__`` / ``examples()`` as
    ``PreprocessedCrowdDataset``."""

    def __init__(self, database_directory, dataset='train', seed=None, number_of_examples=None,
                 map_directory_name='maps', examples_start=None):
        import os
        import random
        if examples_start is None:
            examples_end = number_of_examples
        elif number_of_examples is None:
            examples_end = None
        else:
            examples_end = examples_start + number_of_examples
        self.dataset_directory = os.path.join(database_directory, dataset.capitalize())
        names = sorted(name for name in os.listdir(os.path.join(self.dataset_directory, 'labels')) if name.endswith('.npy'))
        random.Random(seed).shuffle(names)
        self.file_names = names[examples_start:examples_end]
        self.length = len(self.file_names)
        self.map_directory_name = map_directory_name

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        import os
        file_name = self.file_names[index]
        return tuple(np.load(os.path.join(self.dataset_directory, directory, file_name))
                     for directory in ('images', 'labels', self.map_directory_name))

    def examples(self):
        return [CrowdExample(image=image, label=label, map_=map_) for image, label, map_ in
                (self[index] for index in range(self.length))]


def draw_example(generator, length, start_indexes, shapes, patch_size, flip):
    """One ``(scene index, y, x, flip)`` from ``generator`` (a ``np.random.RandomState``): a uniform draw over all
    ``length`` valid patch centres of the scenes (reference crowd/shanghai_tech_data.py:83-98) and, with ``flip``, a fair
    coin (crowd/data.py:104; no coin is drawn without).  The one rule of ``DeviceCrowdPatchLoader.draw_positions`` and of
    ``ResidentCrowdEvaluationSet``'s fixed list."""
    half = patch_size // 2
    index = int(generator.randint(length))
    scene = int(np.searchsorted(start_indexes, index, side='right') - 1)
    height, width = shapes[scene]
    columns = width - 2 * half + 1
    y_index, x_index = divmod(index - start_indexes[scene], columns)
    return scene, half + y_index, half + x_index, int(flip and generator.randint(2))


def evaluation_batch_count(batch_size):
    """Batches one evaluation epoch walks: the smallest ``n`` with ``(n - 1) * batch_size >= 100`` -- the reference's
    ``if index * batch_size >= 100: break`` behind batch ``index`` (crowd/srgan.py:176)."""
    return -(-100 // batch_size) + 1


# The draw ids of the two loaders' device draws (SRGAN_CROWD_PATCH_DRAW_* in include/srgan_hip.h): above the dropout ranges
# [0x10000, 0x30000), away from an iteration's draws 0, 1, 2 and the summary draws 8 and 9.
CROWD_DRAW_LABELED, CROWD_DRAW_UNLABELED = 0x30000, 0x30001


class DeviceCrowdPatchLoader:
    """Endless training batches cut ON THE DEVICE from full crowd scenes that stay resident in HBM:
    the reference's ``ShanghaiTechTransformedDataset`` + ``DataLoader(num_workers=4)`` pipeline (random position
    uniform over every valid patch centre of every scene, ``RandomHorizontalFlip``, [-1, 1] normalisation, CHW layout;
    crowd/shanghai_tech_data.py:47-107) with one kernel launch per batch instead of per-example NumPy work.

    ``examples``: ``CrowdExample``s with uint8 ``image`` (H, W, 3) and float ``label`` / ``map`` (H, W).  Yields
    ``(image f32[B, 3, P, P], label f32[B, P, P], map f32[B, P, P])`` device tensors -- the batch contract of
    ``CrowdExperiment``.  Positions and flips come from a private ``numpy`` generator (the reference's
    multi-process workers make its own stream irreproducible anyway).

    ``draws='device'`` takes the host out of a batch: the positions come from the port's
    counter-based stream (``srgan_crowd_draw_patches``: example ``e`` of the batch of iteration ``i`` is a function of
    ``(seed, i, draw_id, e)``), the scenes' pointers, shapes and running centre counts are uploaded ONCE, and a batch is the
    draw, ``srgan_crowd_extract_patches_indexed`` and ``srgan_random_advance`` -- three launches, no host-to-device copy.
    ``start_at(step)`` puts the stream at an iteration (a continued run: its ``starting_step``), ``last_table`` is the
    ``int32 [local batch, 4]`` table ``(scene, y, x, flip)`` of the latest batch, ``batch_for_table`` cuts an explicit
    device table.  Under ``dp`` a rank draws only its own rows of the global table."""

    def __init__(self, examples, batch_size, image_patch_size=224, seed=0, device=None, flip=True, dp=None, draws='host',
                 draw_id=CROWD_DRAW_LABELED):
        """``batch_size`` is the GLOBAL batch; under data parallelism (``dp``) every rank draws the positions of the whole
        batch from the shared seed and cuts only its own contiguous slice (same examples as one device would see).
        ``draws``: ``'host'`` (the private ``numpy`` generator) or ``'device'`` (draw ``draw_id`` of the counter-based stream
        under ``seed``, taken modulo 2^64)."""
        from .. import _lib
        if draws not in ('host', 'device'):
            raise ValueError("draws is 'host' or 'device', not {!r}".format(draws))
        self.dp = dp if dp is not None and dp.world_size > 1 else None
        if self.dp is not None:
            self.dp.local_batch(batch_size)           # raises unless the global batch divides over the ranks
        from ..utility import current_device
        self._lib = _lib
        self.device = device or current_device()
        self.batch_size, self.patch_size, self.flip = batch_size, image_patch_size, flip
        self.generator = np.random.RandomState(seed) if draws == 'host' else None      # (a device seed has 64 bits)
        half = image_patch_size // 2
        self.images, self.labels, self.maps, self.shapes, self.start_indexes = [], [], [], [], []
        self.length = 0
        for example in examples:
            height, width = example.image.shape[0], example.image.shape[1]
            self.images.append(torch.from_numpy(np.ascontiguousarray(example.image, dtype=np.uint8)).to(self.device))
            self.labels.append(torch.from_numpy(np.ascontiguousarray(example.label, dtype=np.float32)).to(self.device))
            self.maps.append(torch.from_numpy(np.ascontiguousarray(example.map, dtype=np.float32)).to(self.device))
            self.shapes.append((height, width))
            self.start_indexes.append(self.length)
            # every centre whose patch lies inside the scene; a scene smaller than a patch has none, as upstream
            self.length += max(height - 2 * half + 1, 0) * max(width - 2 * half + 1, 0)
        if self.length == 0:
            raise ValueError('no scene is as large as one patch')
        self.draw_mode, self.draw_id, self.seed = draws, int(draw_id), seed
        self.state = self.last_table = self.scene_pointers = None
        if draws == 'device':
            if image_patch_size < 2 or image_patch_size % 2:
                raise ValueError('device draws need an even patch size')
            self.upload_scene_table()

    def upload_scene_table(self):
        """The per-SCENE tables of the indexed entry points, uploaded once: ``scene_pointers`` int64 ``[3, S]`` (images,
        labels, maps), ``scene_heights`` / ``scene_widths`` int32 ``[S]`` and ``scene_starts`` int64 ``[S + 1]``, the running
        count of valid centres (``scene_starts[S] == length``)."""
        if self.scene_pointers is None:
            pointers = [[tensor.data_ptr() for tensor in tensors] for tensors in (self.images, self.labels, self.maps)]
            self.scene_pointers = torch.tensor(pointers, dtype=torch.int64).to(self.device)
            self.scene_heights = torch.tensor([shape[0] for shape in self.shapes], dtype=torch.int32).to(self.device)
            self.scene_widths = torch.tensor([shape[1] for shape in self.shapes], dtype=torch.int32).to(self.device)
            self.scene_starts = torch.tensor(self.start_indexes + [self.length], dtype=torch.int64).to(self.device)
            # the leading arguments of the two calls, as plain integers: nothing is looked up per batch
            self._draw_arguments = (self.scene_starts.data_ptr(), self.scene_heights.data_ptr(),
                                    self.scene_widths.data_ptr(), len(self.shapes))
            self._cut_arguments = tuple(self.scene_pointers[row].data_ptr() for row in range(3)) + self._draw_arguments[1:]
        return self

    @property
    def local_batch_size(self):
        """The rows of the global batch this rank cuts."""
        return self.batch_size if self.dp is None else self.batch_size // self.dp.world_size

    def start_at(self, step):
        """Device draws: the next batch is that of iteration ``step`` (``state`` = ``nn.draw_state(seed, step)``)."""
        if self.draw_mode != 'device':
            raise ValueError("start_at belongs to draws='device': the host generator has no position to set")
        from ..nn import draw_state
        self.state = draw_state(self.seed, step).to(self.device)

    def prepare_capture(self):
        """Device draws: the state exists before a HIP graph capture that records ``device_batch()`` (made inside it, it
        would be a host copy)."""
        if self.draw_mode != 'device':
            raise ValueError("prepare_capture belongs to draws='device'")
        if self.state is None:
            self.start_at(0)
        return self

    def batch_shapes(self):
        """The shapes of one batch ``(image, label, map)`` of this rank."""
        local, size = self.local_batch_size, self.patch_size
        return (local, 3, size, size), (local, size, size), (local, size, size)

    def _stream(self):
        return torch._C._cuda_getCurrentRawStream(self.device.index if self.device.index is not None
                                                  else torch._C._cuda_getDevice())

    def draw_table(self):
        """Device draws: this rank's rows of the current iteration's table, ``int32 [local batch, 4]`` on the device (the
        state is not advanced)."""
        if self.state is None:
            self.start_at(0)
        local = self.local_batch_size
        first = self.dp.rank * local if self.dp is not None else 0
        table = torch.empty((local, 4), dtype=torch.int32, device=self.device)
        self._lib.check(self._lib.library().srgan_crowd_draw_patches(
            *self._draw_arguments, self.patch_size, int(bool(self.flip)), first, local, self.draw_id, self.state.data_ptr(),
            table.data_ptr(), self._stream()), 'srgan_crowd_draw_patches')
        return table

    def batch_for_table(self, table):
        """The device batch of an explicit DEVICE table ``int32 [count, 4]`` of ``(scene, y, x, flip)`` rows -- the device
        counterpart of ``batch_for``: one launch, nothing uploaded.  A row whose scene is outside ``[0, S)`` gives an
        all-padding patch."""
        if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 4 or not table.is_contiguous():
            raise ValueError('a table is a contiguous int32 [count, 4] tensor')
        self.upload_scene_table()
        count, size = table.shape[0], self.patch_size
        image = torch.empty((count, 3, size, size), dtype=torch.float32, device=self.device)
        label = torch.empty((count, size, size), dtype=torch.float32, device=self.device)
        map_ = torch.empty((count, size, size), dtype=torch.float32, device=self.device)
        self._lib.check(self._lib.library().srgan_crowd_extract_patches_indexed(
            *self._cut_arguments, table.data_ptr(), count, size, image.data_ptr(), label.data_ptr(), map_.data_ptr(),
            self._stream()), 'srgan_crowd_extract_patches_indexed')
        return image, label, map_

    def device_batch(self):
        """Device draws: one batch -- draw, cut, advance -- enqueued on the current stream."""
        table = self.draw_table()
        batch = self.batch_for_table(table)
        self._lib.check(self._lib.library().srgan_random_advance(self.state.data_ptr(), self._stream()),
                        'srgan_random_advance')
        self.last_table = table
        return batch

    def draw_positions(self):
        """(scene index, y, x, flip) of one batch: a uniform draw over all valid centres (reference
        crowd/shanghai_tech_data.py:83-98) and a fair coin per example (crowd/data.py:104)."""
        if self.generator is None:
            raise ValueError("draw_positions belongs to draws='host': device draws are read from last_table")
        draws = [draw_example(self.generator, self.length, self.start_indexes, self.shapes, self.patch_size, self.flip)
                 for _ in range(self.batch_size)]
        if self.dp is not None:
            local = self.batch_size // self.dp.world_size
            draws = draws[self.dp.rank * local:(self.dp.rank + 1) * local]
        return draws

    def batch_for(self, draws):
        """The device batch of explicit ``(scene, y, x, flip)`` draws."""
        count, size = len(draws), self.patch_size
        pointers = lambda tensors: torch.tensor([tensors[d[0]].data_ptr() for d in draws], dtype=torch.int64)
        table = torch.stack([pointers(self.images), pointers(self.labels), pointers(self.maps)]).to(self.device)
        numbers = torch.tensor([[self.shapes[d[0]][0] for d in draws], [self.shapes[d[0]][1] for d in draws],
                                [d[1] for d in draws], [d[2] for d in draws], [d[3] for d in draws]],
                               dtype=torch.int32).to(self.device)
        image = torch.empty((count, 3, size, size), dtype=torch.float32, device=self.device)
        label = torch.empty((count, size, size), dtype=torch.float32, device=self.device)
        map_ = torch.empty((count, size, size), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream().cuda_stream
        self._lib.check(self._lib.library().srgan_crowd_extract_patches(
            table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), numbers[0].data_ptr(), numbers[1].data_ptr(),
            numbers[2].data_ptr(), numbers[3].data_ptr(), numbers[4].data_ptr(), count, size, image.data_ptr(),
            label.data_ptr(), map_.data_ptr(), stream), 'srgan_crowd_extract_patches')
        self._keep_alive = (table, numbers)          # the kernel reads the tables asynchronously
        return image, label, map_

    def __iter__(self):
        while True:
            yield self.device_batch() if self.draw_mode == 'device' else self.batch_for(self.draw_positions())


class ResidentCrowdEvaluationSet:
    """The fixed patches one evaluation epoch walks, cut ON THE DEVICE from resident scenes: the stand-in for the reference's
    ``...TransformedDataset`` as ``evaluation_epoch`` and the map comparisons use it (crowd/srgan.py:51,69,149-191).  The
    reference draws fresh random patches at every evaluation; here the ``evaluation_batch_count(batch_size) * batch_size``
    draws ``(scene, y, x, flip)`` are made ONCE, at construction, from a private ``np.random.RandomState(seed)`` with
    ``draw_example`` -- the loader's per-example rule -- so that successive summary steps score the same patches and no
    stream that training uses moves.

    ``source``: a ``DeviceCrowdPatchLoader`` whose resident scenes are shared (the train set: no second upload; its
    generator is not touched) or a list of ``CrowdExample``s that are uploaded here (the test split).  Nothing but the
    scenes and the draw list is kept between evaluations: every batch is one ``srgan_crowd_extract_patches`` launch.

    Over a loader in device mode (``draws='device'``; for scenes uploaded here: the ``draws`` argument) the list -- still
    drawn by the host rule -- is uploaded once as ``table``, int32 ``[N, 4]``, and every batch is a slice of it cut by
    ``batch_for_table``: the same bits as ``batch_for``, no per-evaluation upload.  The loader's state is not touched."""

    def __init__(self, source, batch_size, image_patch_size=224, seed=0, flip=False, device=None, draws='host'):
        if isinstance(source, DeviceCrowdPatchLoader):
            if source.patch_size != image_patch_size:
                raise ValueError('the evaluation set shares the scenes of a loader with another patch size')
            self.scenes = source
        else:       # a loader of its own is the upload; one device, and its generator is never drawn from
            self.scenes = DeviceCrowdPatchLoader(source, batch_size, image_patch_size, seed=seed, device=device, flip=flip,
                                                 draws=draws)
        self.batch_size, self.patch_size, self.flip, self.seed = batch_size, image_patch_size, flip, seed
        generator = np.random.RandomState(seed)
        scenes = self.scenes
        self.draws = [draw_example(generator, scenes.length, scenes.start_indexes, scenes.shapes, image_patch_size, flip)
                      for _ in range(evaluation_batch_count(batch_size) * batch_size)]
        self.table = None
        if scenes.draw_mode == 'device':
            self.table = torch.tensor(self.draws, dtype=torch.int32).to(scenes.device)

    def __len__(self):
        return len(self.draws)

    def device_batches(self):
        """``(image f32[B, 3, P, P], label f32[B, P, P], map f32[B, P, P])`` device batches, in list order."""
        for start in range(0, len(self.draws), self.batch_size):
            if self.table is not None:
                yield self.scenes.batch_for_table(self.table[start:start + self.batch_size])
            else:
                yield self.scenes.batch_for(self.draws[start:start + self.batch_size])

    def __getitem__(self, index):
        """Example ``index`` of the list as device tensors ``(image[3, P, P], label[P, P], map[P, P])``."""
        if self.table is not None:
            index = range(len(self.draws))[index]             # negative indices and IndexError as the list's
            image, label, map_ = self.scenes.batch_for_table(self.table[index:index + 1])
        else:
            image, label, map_ = self.scenes.batch_for([self.draws[index]])
        return image[0], label[0], map_[0]


class DeviceSlidingWindows:
    """The sliding-window patches of one full example cut ON THE DEVICE: the scene is uploaded once as uint8 and every
    batch of ``batch_size`` windows is one ``srgan_crowd_extract_windows`` launch -- no per-window NumPy padding,
    normalisation, transposition or upload.  The centres are ``ImageSlidingWindowDataset``'s (``ys`` / ``xs``: its
    ``y_positions`` / ``x_positions`` as int32; window ``i`` is centred on ``(ys[i // len(xs)], xs[i % len(xs)])``, the
    dataset's own index order), so the extra edge centre and images smaller than a patch follow the one rule.

    Iterating yields ``(first window index, images f32[count, 3, P, P])`` device batches in window order.  Nothing
    touches the device before the first batch is asked for."""

    def __init__(self, full_example, batch_size, image_patch_size=128, window_step_size=32, device=None):
        if image_patch_size % 2:
            raise ValueError('the window slices only line up for an even patch size')
        positions = ImageSlidingWindowDataset(full_example, image_patch_size, window_step_size)
        self.image = full_example.image
        self.height, self.width = self.image.shape[0], self.image.shape[1]
        self.batch_size, self.patch_size = batch_size, image_patch_size
        self.ys = np.asarray(positions.y_positions, dtype=np.int32)
        self.xs = np.asarray(positions.x_positions, dtype=np.int32)
        self.length = positions.length
        self.device = device
        self.scene = self.device_ys = self.device_xs = None

    def __len__(self):
        return self.length

    def centre(self, index):
        """``(y, x)`` of window ``index`` -- what the kernels compute from the uploaded table."""
        return int(self.ys[index // len(self.xs)]), int(self.xs[index % len(self.xs)])

    def upload(self):
        if self.scene is None:
            from ..utility import current_device
            self.device = self.device or current_device()
            self.scene = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.uint8)).to(self.device)
            self.device_ys = torch.from_numpy(self.ys).to(self.device)
            self.device_xs = torch.from_numpy(self.xs).to(self.device)
        return self

    def batch(self, first, count):
        """Windows ``first .. first + count - 1`` as one device tensor."""
        from .. import _lib
        self.upload()
        size = self.patch_size
        images = torch.empty((count, 3, size, size), dtype=torch.float32, device=self.device)
        _lib.check(_lib.library().srgan_crowd_extract_windows(
            self.scene.data_ptr(), self.height, self.width, self.device_ys.data_ptr(), len(self.ys),
            self.device_xs.data_ptr(), len(self.xs), first, count, size, images.data_ptr(), _lib.stream_handle()),
            'srgan_crowd_extract_windows')
        return images

    def __iter__(self):
        for first in range(0, self.length, self.batch_size):
            yield first, self.batch(first, min(self.batch_size, self.length - first))
