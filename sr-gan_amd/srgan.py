"""Semi-supervised regression GAN training on MI355X: the ``Experiment`` surface of reference srgan.py with
the training step (dnn_training_step / gan_training_step and the loss calculations, srgan.py:259-391)
running on the HIP tape.

Differences from the reference that are deliberate (each keeps results identical to 1e-3):

* ``settings.reference_schedule = False`` (default) shares the discriminator forward of the labeled batch
  between the labeled and unlabeled losses and that of the unlabeled batch between the unlabeled and fake
  losses, and back-propagates their sum once: the reference recomputes those forwards (Appendix A.2).
  ``True`` replays the reference's exact forward / backward order.
* the discriminator's weight gradients are not computed during the generator update (the reference computes
  and discards them, srgan.py:304 then :278).
* one process per GPU: an optional data-parallel context shards the three batches and exchanges feature
  sums and gradients over RCCL (``parallel.py``).  The gradient all-reduces are asynchronous: each starts during the
  last backward pass into its network's arena (reference srgan.py:264 for the DNN, :295 for D, :304 for G are where those
  gradients complete) and the optimizer update that needs it is applied when the weights are next used
  (``finish_update``): the DNN's exchange runs under the whole GAN step, D's under the generator forward, G's under
  the next iteration's DNN step.  The arithmetic is unchanged.
"""
import contextlib
import datetime
import os
import re
import select
import sys
from abc import ABC, abstractmethod

import numpy as np
import torch
from scipy.stats import norm

from . import _lib
from . import functional as F
from . import nn
from .optim import Adam
from .settings import Settings, option
from .tape import Var, backward, no_grad
from . import image_summaries
from .utility import SummaryWriter, MixtureModel, current_device, make_directory_name_unique, norm_squared, seed_all, \
    to_image_range


def as_var(value, staged=False):
    """Device tensors from the data pipeline enter the tape as constants.  ``staged``: a small host tensor goes through a
    pinned staging buffer (the three random draws of an iteration ask for it; nothing else does)."""
    if isinstance(value, Var) or value is None:
        return value
    if isinstance(value, (tuple, list)):
        return tuple(as_var(v) for v in value)
    if isinstance(value, np.ndarray):
        value = torch.from_numpy(value)
    if staged and value.device.type == 'cpu' and torch.cuda.is_available() and value.dtype == torch.float32 and \
            0 < value.numel() <= _STAGING_LIMIT and not torch.cuda.is_current_stream_capturing():
        return F.constant(_through_pinned_staging(value))
    return F.constant(value.to(current_device(), non_blocking=True))


# The three random draws of an iteration (srgan.py:286-289,301,364) reach the device through PINNED staging buffers: a copy
# from pageable memory is staged by the runtime and its blit kernel sat 0.55 ms on the stream per draw (rocprofv3, round 3:
# three __amd_rocclr_copyBuffer launches of 555 us per iteration, the first in front of the generator's forward pass).  A ring
# of buffers per size; a buffer is reused only after the copy that read it has finished.  Only the draw call sites stage
# (`as_var(..., staged=True)`), never while a stream is capturing (a captured copy would re-read whatever the reusable slot
# holds at replay time), and the rings of at most _STAGING_SIZES distinct sizes are kept (least recently used dropped), so
# pinned memory stays bounded when batch sizes vary.
_STAGING_LIMIT = 1 << 20
_STAGING_RING = 8
_STAGING_SIZES = 6
_staging = {}


def _through_pinned_staging(value):
    device = current_device()
    key = (value.numel(), str(device))
    ring = _staging.pop(key, None)
    if ring is None:
        while len(_staging) >= _STAGING_SIZES:
            oldest = _staging.pop(next(iter(_staging)))
            for _, event in oldest['slots']:
                if event is not None:
                    event.synchronize()             # its copies are done before the pinned pages go away
        ring = {'next': 0, 'slots': [[torch.empty(value.numel(), dtype=torch.float32).pin_memory(), None]
                                     for _ in range(_STAGING_RING)]}
    _staging[key] = ring                            # (re-inserted last: the dict's order is the recency order)
    slot = ring['slots'][ring['next']]
    ring['next'] = (ring['next'] + 1) % _STAGING_RING
    if slot[1] is not None:
        slot[1].synchronize()                     # (eight copies ago: long done)
    slot[0].copy_(value.reshape(-1))
    out = torch.empty(value.shape, dtype=torch.float32, device=device)
    out.view(-1).copy_(slot[0], non_blocking=True)
    slot[1] = torch.cuda.Event()
    slot[1].record()
    return out


def examples_on_gpu():
    return torch.cuda.is_available()


DRAW_Z_D, DRAW_ALPHA, DRAW_Z_G = 0, 1, 2      # the draw ids of an iteration's three device draws (settings.device_random_draws)
# The draw ids of the dropout masks (settings.drop_rate; SRGAN_DROPOUT_DRAWS_* in include/srgan_hip.h): call k of a network's
# step of an iteration takes base + k under that network's own state.  Two disjoint ranges, clear of the draws above and of
# the summary draws 8 and 9.
DROPOUT_DRAWS_D, DROPOUT_DRAWS_DNN, DROPOUT_DRAW_RANGE = 0x10000, 0x20000, 0x10000
DROPOUT_DRAW_BASES = {'D': DROPOUT_DRAWS_D, 'DNN': DROPOUT_DRAWS_DNN}
# Optional settings (None or a callable) that replace Experiment.feature_distance_loss: see there.
FEATURE_LOSS_SETTINGS = ('matching_feature_loss', 'contrasting_feature_loss')
# Passes of D whose place in the host's program order depends on a side-stream setting number their dropout calls in a section
# of D's range of their own (nn.DropoutStream.section), so the masks do not depend on the stream settings.
DROPOUT_SECTION_PENALTY, DROPOUT_SECTION_GENERATOR_UNLABELED = 1, 2


def device_draw_window(global_rows, columns, world_size=1, rank=0):
    """(rows, first) of the window of a ``[global_rows, columns]`` device draw that rank ``rank`` of ``world_size`` fills:
    its contiguous rows of the global tensor, starting at element ``first`` of the draw.  The ranks' windows tile the
    global tensor, and an element's value depends on its index in the draw alone (``srgan_random_fill``), so together the
    ranks hold exactly what one device draws at the global batch size."""
    if not 0 <= rank < world_size:
        raise ValueError(f'rank {rank} outside a world of {world_size}')
    if global_rows % world_size:
        raise ValueError(f'{global_rows} rows are not divisible by {world_size} ranks')
    rows = global_rows // world_size
    return rows, rank * rows * columns


class Experiment(ABC):
    """Manages one experimental trial (reference srgan.py:24-469)."""
    # How the age and driving applications take their validation summaries (``regression_validation_summaries``).  A run sets
    # them on the instance or in a subclass; any other value is a ValueError when the summaries are first taken.
    regression_validation = 'host'     # 'device': the summary step's errors from sums taken on the device
    validation_precision = 'f32'       # 'step': the evaluation's forward passes run under self.precision()
    # How the crowd application's database loaders draw their patch positions (``crowd.data.DeviceCrowdPatchLoader``); the
    # same kind of switch: an attribute, checked (``ValueError``) in the crowd ``dataset_setup``.
    crowd_patch_draws = 'host'         # 'device': positions from the counter-based stream, a function of (seed, step)
    # The age / driving counterpart (``data.ResidentImageLoader``, checked in ``data.database_loaders``), and whether the two
    # training loaders are recorded WITH a captured iteration (``settings.step_graph`` on a single device: both must then draw
    # on the device; ``captured_loaders``).
    image_batch_draws = 'host'         # 'device': the epoch orders from the counter-based stream, a function of (seed, step)
    capture_loaders = False            # True: a replayed iteration cuts its own batches, nothing is copied into the graph

    def __init__(self, settings: Settings):
        self.settings = settings
        self.trial_directory = None
        self.dnn_summary_writer = None
        self.gan_summary_writer = None
        self.dataset_class = None
        self.train_dataset = None
        self.train_dataset_loader = None
        self.unlabeled_dataset = None
        self.unlabeled_dataset_loader = None
        self.validation_dataset = None
        self.DNN = None
        self.dnn_optimizer = None
        self.D = None
        self.d_optimizer = None
        self.G = None
        self.g_optimizer = None
        self.signal_quit = False
        self.starting_step = 0

        self.labeled_features = None
        self.unlabeled_features = None
        self.fake_features = None
        self.interpolates_features = None
        self.gradient_norm = None

        self.dp = None                 # optional parallel.DataParallel context
        self._pending_updates = {}     # network name -> (gradient exchange in flight, optimizer to step after it)
        self.injected_draws = None     # tests: dict with 'z_d', 'z_g', 'alpha' device/CPU tensors, used once
        self.last_losses = {}          # device scalars of the latest step (no host sync)
        self._draw_state = None        # settings.device_random_draws: device int32 x 4 {seed_lo, seed_hi, iteration, 0}
        self._dropout_streams = {}     # 'D' / 'DNN' -> (network, its nn.DropoutStream or None), made at the first training step
        self._captured_iteration = None          # settings.step_graph: the graph.CapturedIteration, made at the first iteration
        self._single_compute_stream = False      # captured under data parallelism: the side streams are off for this run
        self._graph_note = False                 # why a data-parallel run with step_graph stays eager: said once
        self._typed_commands = set()             # rank 0: 'save' / 'quit' typed since the ranks last exchanged them
        self._dnn_stream = self._aux_stream = self._gp_stream = None       # the side streams, each made at first use
        self._stack_too_large = False            # the stacked discriminator pass passed the kernels' 2^31 elements once

    @property
    def parallel(self):
        """True when the data-parallel exchanges run: more than one rank, or one rank with ``dp.force`` (the whole
        collective path -- feature sums, bucketed gradient exchange, broadcasts -- on a world of one: how the RCCL
        backend is exercised on a one-GPU box, ``bench.py --force-dp``)."""
        return self.dp is not None and self.dp.active

    # ------------------------------------------------------------------------------------------ lifecycle
    def _trial_decision(self):
        """What reference srgan.py:54-70 decides from the file system before a trial starts: skip it, its (unique)
        directory, and where to load a model from.  Taken on rank 0 only and broadcast, so that every rank of a
        data-parallel run trains the same trial from the same checkpoint."""
        settings = self.settings
        trial_directory = os.path.join(settings.logs_directory, settings.trial_name)
        decision = dict(skip=False, trial_directory=trial_directory, load_model_path=settings.load_model_path,
                        continue_existing_experiments=settings.continue_existing_experiments)
        if (settings.skip_completed_experiment and os.path.exists(trial_directory) and
                '/check' not in trial_directory and not settings.continue_existing_experiments):
            decision['skip'] = True
            return decision
        if not settings.continue_existing_experiments:
            decision['trial_directory'] = make_directory_name_unique(trial_directory)
        else:
            if os.path.exists(trial_directory) and settings.load_model_path is not None:
                raise ValueError('Cannot load from path and continue existing at the same time.')
            elif settings.load_model_path is None:
                decision['load_model_path'] = trial_directory
            elif not os.path.exists(trial_directory):
                decision['continue_existing_experiments'] = False
        os.makedirs(os.path.join(decision['trial_directory'], settings.temporary_directory), exist_ok=True)
        return decision

    def train(self):
        """Run the SRGAN training for the experiment (reference srgan.py:52-86)."""
        settings = self.settings
        parallel = self.parallel
        if parallel and settings.batch_size % self.dp.world_size:
            raise ValueError(f'batch_size {settings.batch_size} is the GLOBAL batch and must be divisible by the '
                             f'{self.dp.world_size} data-parallel ranks')
        decision = self._trial_decision() if not parallel or self.dp.rank == 0 else None
        if parallel:
            decision = self.dp.broadcast_object(decision)
        self.trial_directory = decision['trial_directory']
        if decision['skip']:
            print('`{}` experiment already exists. Skipping...'.format(self.trial_directory))
            return
        settings.load_model_path = decision['load_model_path']
        settings.continue_existing_experiments = decision['continue_existing_experiments']
        print(self.trial_directory)
        self.prepare_summary_writers()
        seed_all(0)

        self.dataset_setup()
        self.model_setup()
        self.gpu_mode()              # parameters move into flat device arenas before the optimizers bind
        self.prepare_optimizers()
        self.load_models()
        if parallel:                 # every rank starts from rank 0's weights (and the checkpoint it may have loaded)
            for module in (self.D, self.DNN, self.G):
                if module is not None and getattr(module, '_srgan_arena', None) is not None:
                    self.dp.broadcast_parameters(module._srgan_arena)
        self.train_mode()

        self.training_loop()

        print('Completed {}'.format(self.trial_directory))
        if settings.should_save_models:
            self.save_models(step=settings.steps_to_run)
        self.close()

    # (network attribute, optimizer attribute): also the keys of the checkpoint dictionary (reference srgan.py:88-97)
    CHECKPOINT_PARTS = (('DNN', 'dnn_optimizer'), ('D', 'd_optimizer'), ('G', 'g_optimizer'))

    def save_models(self, step):
        """One torch.save dict with the reference's keys (srgan.py:88-97); written by rank 0 only."""
        self.join_dnn_stream()         # also applies optimizer updates still waiting for their gradient exchange
        if self.dp is not None and self.dp.rank != 0:
            return
        model = {'step': step}
        for network, optimizer in self.CHECKPOINT_PARTS:
            model[network] = getattr(self, network).state_dict()
            model[optimizer] = getattr(self, optimizer).state_dict()
        torch.save(model, os.path.join(self.trial_directory, f'model_{step}.pth'))
        self.flush_summary_writers()

    @staticmethod
    def unpack_labeled(samples):
        """(examples, labels) of a labeled batch; a third element is a secondary label (the crowd maps)."""
        if len(samples) == 2:
            return as_var(samples[0]), as_var(samples[1])
        examples, primary_labels, secondary_labels = samples
        return as_var(examples), as_var((primary_labels, secondary_labels))

    def end_of_step(self, step, summary_writer, step_time_start):
        """Periodic validation summaries, the stdin commands and periodic checkpoints (reference srgan.py:120-129);
        returns the time stamp the next progress line is measured from."""
        if summary_writer.is_summary_step() or step == self.settings.steps_to_run - 1:
            print('\rStep {}, {}...'.format(step, datetime.datetime.now() - step_time_start), end='')
            step_time_start = datetime.datetime.now()
            self.join_dnn_stream()
            self.eval_mode()
            with no_grad():
                self.validation_summaries(step)
            self.train_mode()
            self.flush_summary_writers()       # a summary step's records are in the event files when the step is over
        self.handle_user_input(step)
        if self.settings.save_step_period and step % self.settings.save_step_period == 0 and step != 0:
            self.save_models(step=step)
        return step_time_start

    def training_loop(self):
        """The per-step hot loop (reference srgan.py:99-129)."""
        self.start_loaders_at(self.starting_step)
        loaders = self.captured_loaders()
        train_dataset_generator = self.infinite_iter(self.train_dataset_loader)
        unlabeled_dataset_generator = self.infinite_iter(self.unlabeled_dataset_loader)
        step_time_start = datetime.datetime.now()
        for step in range(self.starting_step, self.settings.steps_to_run):
            self.adjust_learning_rate(step)
            if loaders is not None:        # the iteration draws its own batches: eagerly, or as part of the graph
                self.captured_iteration().run(None, None, None, step, loaders=loaders)
            else:
                labeled_examples, labels = self.unpack_labeled(next(train_dataset_generator))
                unlabeled_examples = as_var(next(unlabeled_dataset_generator)[0])
                self.training_iteration(labeled_examples, labels, unlabeled_examples, step)
            step_time_start = self.end_of_step(step, self.gan_summary_writer, step_time_start)

    def captured_loaders(self):
        """``(train loader, unlabeled loader)`` when the iteration is to take its batches from the loaders itself
        (``capture_loaders`` with ``settings.step_graph`` on a single device), else None: today's path.  Both loaders must
        then make a batch from launches whose arguments do not depend on the step -- ``draw_mode == 'device'`` with a
        ``device_batch()``: the resident image loaders under ``image_batch_draws = 'device'``, the crowd patch loaders under
        ``crowd_patch_draws = 'device'`` -- or a ``ValueError`` is raised before the first step."""
        if not self.capture_loaders or not option(self.settings, 'step_graph') or not examples_on_gpu() or \
                self.parallel or (self.dp is not None and self.dp.world_size > 1):
            return None
        loaders = self.train_dataset_loader, self.unlabeled_dataset_loader
        for loader in loaders:
            if getattr(loader, 'draw_mode', None) != 'device' or not hasattr(loader, 'device_batch'):
                raise ValueError('capture_loaders needs both training loaders in device mode (image_batch_draws / '
                                 "crowd_patch_draws = 'device'), not {}".format(type(loader).__name__))
        return loaders

    def captured_iteration(self):
        if self._captured_iteration is None:
            from .graph import CapturedIteration
            self._captured_iteration = CapturedIteration(self)
        return self._captured_iteration

    def training_iteration(self, labeled_examples, labels, unlabeled_examples, step):
        """The body of the reference's loop (srgan.py:104-118): the DNN step, then the GAN step.  With
        ``settings.step_graph`` on a single device (fp32 or the 16-bit path; data parallel: fp32 only) the iteration is captured
        once as a HIP graph and replayed
        (``graph.CapturedIteration``); summary steps and the first ``settings.step_graph_warmup`` iterations run eagerly."""
        if option(self.settings, 'step_graph') and examples_on_gpu() and self._exchanges_are_capturable():
            return self.captured_iteration().run(labeled_examples, labels, unlabeled_examples, step)
        self.dnn_training_step(labeled_examples, labels, step)
        self.gan_training_step(labeled_examples, labels, unlabeled_examples, step)

    def _stream_setting(self, name):
        """A side-stream switch of ``settings`` as THIS iteration sees it: off while the iteration is captured / replayed as a
        HIP graph under data parallelism (``_single_compute_stream``), without touching ``settings`` itself."""
        if self._single_compute_stream:
            return False
        return option(self.settings, name)

    def _exchanges_are_capturable(self):
        """True when this run's iterations can be captured as HIP graphs.  Single device: always.  Data parallel: fp32 only (settings.storage_dtype
        keeps such a run eager, with a note), and only when the
        caller OPTED IN with ``settings.step_graph_collectives = 'abi'`` -- the exchanges then run through the C ABI's RCCL entry
        points on a stream this process owns (``DataParallel.use_abi_collectives``, the default device transport; destroyed by
        ``close()``) and are captured with the iteration; collectives that go through a host-side process group
        (gloo, torch's own NCCL work queue) keep the run eager.  No setting is modified: the compute side streams are switched
        off for such a run through ``_stream_setting`` (hipStreamEndCapture crashes -- ROCm 7.0 runtime, a segmentation fault
        inside capture_end, round 5; re-tested in round 6 with the process on four streams: gpurun_out/r6u -- when a capture holds
        the compute side streams AND the communication stream)."""
        if not self.parallel:
            return True
        if option(self.settings, 'storage_dtype'):
            if not self._graph_note:
                print('[srgan_amd] step_graph with settings.storage_dtype replays on a single device only; running eagerly '
                      'under data parallelism')
                self._graph_note = True
            return False
        if option(self.settings, 'step_graph_collectives') != 'abi':
            if not self._graph_note:
                print('[srgan_amd] step_graph under data parallelism needs settings.step_graph_collectives = "abi" '
                      '(the C ABI\'s RCCL entry points); running eagerly')
                self._graph_note = True
            return False
        if getattr(self.dp, 'abi', None) is None and getattr(self.dp, 'device_backend', None) == 'nccl':
            self.dp.use_abi_collectives()
        if getattr(self.dp, 'abi', None) is None:
            return False
        if not self._single_compute_stream:
            self.join_dnn_stream()                  # an eager iteration may have left work on a side stream
            self._single_compute_stream = True
            print('[srgan_amd] step_graph under data parallelism: one compute stream + RCCL\'s (side streams off for this run)')
        return True

    def close(self):
        """Releases what the experiment created outside torch: the C ABI's RCCL communicator (before the process group goes)."""
        self.join_dnn_stream()
        abi = getattr(self.dp, 'abi', None) if self.dp is not None else None
        if abi is not None:
            torch.cuda.synchronize()
            abi.close()
            self.dp.abi = None
        for writer in self.summary_writers():
            writer.close()

    def prepare_optimizers(self):
        """Adam for D (with coupled L2), G and DNN (reference srgan.py:131-138) on the flat arenas."""
        if getattr(self.D, '_srgan_arena', None) is None:
            self.gpu_mode()
        d_lr = self.settings.learning_rate
        weight_decay = self.settings.weight_decay
        self.d_optimizer = Adam(self.D._srgan_arena, lr=d_lr, weight_decay=weight_decay)
        self.g_optimizer = Adam(self.G._srgan_arena, lr=d_lr)
        self.dnn_optimizer = Adam(self.DNN._srgan_arena, lr=d_lr, weight_decay=weight_decay)

    def summary_directory(self, name):
        """Rank 0 writes the trial's event files; the other ranks of a data-parallel run log in memory only."""
        if self.dp is not None and self.dp.rank != 0:
            return None
        return os.path.join(self.trial_directory, name)

    def summary_writers(self):
        """The writers this experiment has (a DNN-only trial has one)."""
        return [writer for writer in (self.dnn_summary_writer, self.gan_summary_writer) if writer is not None]

    def flush_summary_writers(self):
        for writer in self.summary_writers():
            writer.flush()

    def arena_histogram_summaries(self, bins=30):
        """Histograms of the flat parameter and gradient arenas, taken on the device: ``Parameters/<D|G|DNN>`` and
        ``Gradients/<D|G|DNN>``, the DNN's to the DNN writer and the others to the GAN writer.  Called by nothing here: a
        subclass that wants them calls it from its ``validation_summaries``."""
        for name, writer in (('DNN', self.dnn_summary_writer), ('D', self.gan_summary_writer), ('G', self.gan_summary_writer)):
            arena = getattr(getattr(self, name, None), '_srgan_arena', None)
            if arena is None or writer is None:
                continue
            writer.add_histogram(f'Parameters/{name}', arena.data, bins=bins)
            writer.add_histogram(f'Gradients/{name}', arena.grad, bins=bins)

    def prepare_summary_writers(self):
        self.dnn_summary_writer = SummaryWriter(self.summary_directory('DNN'))
        self.gan_summary_writer = SummaryWriter(self.summary_directory('GAN'))
        for writer in (self.dnn_summary_writer, self.gan_summary_writer):
            writer.summary_period = self.settings.summary_step_period
            writer.steps_to_run = self.settings.steps_to_run

    USER_INPUT_EXCHANGE_PERIOD = 50     # data-parallel runs agree on typed commands every this many steps

    def _poll_stdin(self):
        """'save' / 'quit' typed on stdin since the last poll, without blocking (reference srgan.py:149-163)."""
        commands = set()
        try:
            ready = sys.stdin in select.select([sys.stdin], [], [], 0)[0]
        except (ValueError, OSError):
            return commands
        while ready:
            line = sys.stdin.readline()
            if not line:
                break
            commands.update(word for word in ('save', 'quit') if word in line)
            ready = sys.stdin in select.select([sys.stdin], [], [], 0)[0]
        return commands

    def handle_user_input(self, step):
        """Acts on 'save' / 'quit' (reference srgan.py:149-163).  Under data parallelism rank 0 reads stdin and the ranks
        exchange what it saw every ``USER_INPUT_EXCHANGE_PERIOD`` steps, so that all of them save / stop together
        (one rank leaving the loop alone would leave the others hanging in their next collective)."""
        parallel = self.parallel
        if not parallel:
            commands = self._poll_stdin()
        else:
            if self.dp.rank == 0:
                self._typed_commands |= self._poll_stdin()
            if step % self.USER_INPUT_EXCHANGE_PERIOD != 0 and step != self.settings.steps_to_run - 1:
                return
            commands = self.dp.broadcast_object(sorted(self._typed_commands))
            self._typed_commands = set()
        if 'save' in commands:
            self.save_models(step)
            print('\rSaved model for step {}...'.format(step))
        if 'quit' in commands:
            self.signal_quit = True
            print('\rQuit requested after current experiment...')

    def train_mode(self):
        for module in (self.D, self.DNN, self.G):
            module.train()

    def eval_mode(self):
        for module in (self.D, self.DNN, self.G):
            module.eval()

    def generator_norm_arguments(self):
        """The norm-layer arguments of a DCGAN generator, for every ``model_setup`` that builds one:
        ``settings.generator_batch_norm`` (norm layers with batch statistics) and ``settings.blocked_batch_norm`` (such a
        generator stays on the blocked data path that ``settings.storage_dtype`` / ``settings.blocked_fp32`` select; without
        either of them it changes nothing).  With the latter off the generator with norm layers keeps the fp32 graph, which
        the 16-bit storage test of the batch-norm step pins."""
        return dict(batch_norm=self.settings.generator_batch_norm,
                    blocked_batch_norm=option(self.settings, 'blocked_batch_norm'))

    def discriminator_norm_arguments(self):
        """The norm-layer arguments of a DCGAN discriminator (D and DNN), for every ``model_setup`` that builds one:
        ``settings.discriminator_batch_norm`` (frozen norm layers) and ``settings.blocked_frozen_norm`` (such a discriminator
        stays on the blocked data path that ``settings.storage_dtype`` / ``settings.blocked_fp32`` select; without either of
        them it changes nothing).  With the latter off: the fp32 NCHW graph."""
        return dict(batch_norm=self.settings.discriminator_batch_norm,
                    blocked_frozen_norm=option(self.settings, 'blocked_frozen_norm'))

    def gpu_mode(self):
        """Moves each network into its flat parameter / gradient arena on this rank's device."""
        if self.dp is not None and self.dp.world_size > 1 and self.G is not None and \
                any(isinstance(module, nn.BatchStatNorm2d) for module in self.G.modules()):
            # per-rank statistics and unsynchronised running buffers would silently differ from one device on the global batch
            raise NotImplementedError('a generator with batch-statistics normalisation (settings.generator_batch_norm) runs on '
                                      'one device only: statistics synchronised across the data-parallel ranks are future work')
        self.refuse_dropout_under_data_parallelism()
        self.refuse_feature_loss_hooks_under_data_parallelism()
        device = current_device()
        for module in (self.D, self.DNN, self.G):
            if getattr(module, '_srgan_arena', None) is None:
                nn.flatten_parameters(module, device)

    def refuse_dropout_under_data_parallelism(self):
        if self.dp is not None and self.dp.world_size > 1 and \
                any(nn.active_dropout_layers(getattr(self, name, None)) for name in DROPOUT_DRAW_BASES):
            # a rank would have to mask its rows of the GLOBAL batch's activations (a `first` per call and per layer)
            raise NotImplementedError('a network with dropout layers (settings.drop_rate > 0) runs on one device only: masks '
                                      'windowed over the data-parallel ranks are future work')

    def refuse_feature_loss_hooks_under_data_parallelism(self):
        if self.dp is not None and self.dp.world_size > 1 and \
                any(option(self.settings, name) is not None for name in FEATURE_LOSS_SETTINGS):
            # a hook sees this rank's rows only: the batch means / Gram matrices of a sharded batch need collectives of their own
            raise NotImplementedError('settings.matching_feature_loss / settings.contrasting_feature_loss run on one device '
                                      'only: feature losses over a batch sharded across data-parallel ranks are future work')

    def cpu_mode(self):
        raise RuntimeError('the MI355X training step has no CPU mode')

    @staticmethod
    def compare_model_path_for_latest(model_path1, model_path2):
        """Later step wins; a file without a step number wins over all (reference srgan.py:197-219)."""
        if model_path1 is None:
            return model_path2
        if model_path1.group(1) is None:
            return model_path1
        if model_path2.group(1) is None:
            return model_path2
        return model_path1 if int(model_path1.group(1)) > int(model_path2.group(1)) else model_path2

    def latest_checkpoint_path(self):
        """The ``model[_<step>].pth`` with the highest step in ``settings.load_model_path`` (None if there is none)."""
        latest_model = None
        for file_name in os.listdir(self.settings.load_model_path):
            match = re.search(r'model_?(\d+)?\.pth', file_name)
            if match:
                latest_model = self.compare_model_path_for_latest(latest_model, match)
        return os.path.join(self.settings.load_model_path, latest_model.group(0)) if latest_model else None

    def load_models(self, with_optimizers=True):
        """Loads the latest checkpoint of ``settings.load_model_path`` (reference srgan.py:221-251)."""
        if not self.settings.load_model_path:
            return
        model_path = self.latest_checkpoint_path()
        if model_path is None:
            return
        loaded_model = torch.load(model_path, map_location='cpu')
        for network, optimizer in self.CHECKPOINT_PARTS:
            getattr(self, network).load_state_dict(loaded_model[network])
        if with_optimizers:
            for network, optimizer in self.CHECKPOINT_PARTS:
                getattr(self, optimizer).load_state_dict(loaded_model[optimizer])
        print('Model loaded from `{}`.'.format(model_path))
        if self.settings.continue_existing_experiments:
            self.starting_step = loaded_model['step'] + 1
            print(f'Continuing from step {self.starting_step}')

    # ------------------------------------------------------------------------------------------ random draws
    def _take_draw(self, key):
        if self.injected_draws is not None and self.injected_draws.get(key) is not None:
            value = self.injected_draws[key]
            self.injected_draws[key] = None
            return value
        return None

    def _global_draw(self, local_batch, draw):
        """Under data parallelism every rank draws the tensor for the GLOBAL batch from its (identically seeded) host
        stream and keeps its own shard: the ranks' examples differ, and together they are exactly what the
        single-device reference draws at the global batch size."""
        if not self.parallel:
            return draw(local_batch)
        return self.dp.shard(draw(self.dp.global_batch(local_batch)))

    def draw_discriminator_noise(self, batch_size):
        """Host tensor: float64 two-Gaussian mixture from NumPy's global stream cast to float32 (srgan.py:286-289)."""
        offset = self.settings.mean_offset
        return self._global_draw(batch_size, lambda count: torch.tensor(
            MixtureModel([norm(-offset, 1), norm(offset, 1)]).rvs(size=[count, self.G.input_size]).astype(np.float32)))

    def draw_generator_noise(self, batch_size):
        """Host tensor: N(0, 1) from torch's CPU stream (srgan.py:301)."""
        return self._global_draw(batch_size, lambda count: torch.randn(count, self.G.input_size))

    def draw_interpolation_alpha(self, batch_size):
        """Host tensor: U[0, 1) per example.  The reference draws on the device (srgan.py:364), which is not
        reproducible across devices; here it comes from torch's CPU stream and is copied over."""
        return self._global_draw(batch_size, lambda count: torch.rand(count))

    # ``settings.device_random_draws`` (seed: ``settings.device_random_seed``): the three draws come from the counter-based
    # generator of csrc/random_draws.hip instead of the host streams -- kernel launches on the stream that uses them, nothing
    # staged, and a HIP graph captures them with the step.  Element e of draw d of iteration t is a pure function of
    # (seed, t, d, e); t lives in a device state that ``gan_training_step`` advances once per iteration.  The stream is NOT
    # the reference's (host draws stay the default and the only stream pinned against it); an injected draw still wins.
    def device_random_draws(self):
        return bool(option(self.settings, 'device_random_draws'))

    def device_draw_state(self):
        """The draws' device state, created at first use with ``iteration = starting_step`` (a resumed run continues its
        stream; checkpoints keep the reference's keys, the seed comes from the settings)."""
        if self._draw_state is None:
            self._draw_state = nn.draw_state(option(self.settings, 'device_random_seed'), self.starting_step)
        return self._draw_state

    def _device_draw(self, draw, local_rows, columns, kind, offset=0.0):
        """This rank's ``[local_rows, columns]`` window of a draw of the global batch (no global draw, no shard); one value
        per example (``columns`` None) is a vector."""
        world_size, rank = (self.dp.world_size, self.dp.rank) if self.dp is not None else (1, 0)
        rows, first = device_draw_window(local_rows * world_size, columns or 1, world_size, rank)
        return F.random_fill((rows,) if columns is None else (rows, columns), kind, offset, draw, self.device_draw_state(), first)

    def sample_discriminator_noise(self, batch_size):
        z = self._take_draw('z_d')
        if z is None and self.device_random_draws():
            return self._device_draw(DRAW_Z_D, batch_size, self.G.input_size, 1, self.settings.mean_offset)
        return as_var(self.draw_discriminator_noise(batch_size) if z is None else z, staged=True)

    def sample_generator_noise(self, batch_size):
        z = self._take_draw('z_g')
        if z is None and self.device_random_draws():
            return self._device_draw(DRAW_Z_G, batch_size, self.G.input_size, 1)
        return as_var(self.draw_generator_noise(batch_size) if z is None else z, staged=True)

    def sample_interpolation_alpha(self, batch_size):
        alpha = self._take_draw('alpha')
        if alpha is None and self.device_random_draws():
            return self._device_draw(DRAW_ALPHA, batch_size, None, 0)
        return as_var((self.draw_interpolation_alpha(batch_size) if alpha is None else alpha).reshape(-1), staged=True)

    # ``settings.drop_rate`` (0: no dropout layer exists and none of this runs): dropout on the new features of every dense
    # layer of D and DNN (reference crowd/models.py:336-353).  The masks come from the counter-based stream of the device
    # draws and are never stored: a network owns a ``nn.DropoutStream`` -- a device state {seed, iteration} of its own (seed:
    # ``settings.device_random_seed``; iteration: ``starting_step`` at first use, so a resumed run continues its masks) and a
    # host-side call counter.  The counter is reset when the network's step of an iteration begins, each training-mode dropout
    # call takes the next draw id of the network's range, and the state is advanced once per iteration behind the last launch
    # that reads it (the ordering edges).  The draws' own state is untouched.
    def dense_drop_rate(self):
        return float(option(self.settings, 'drop_rate') or 0)

    def dropout_stream(self, name):
        """The dropout stream of network ``name`` ('D' / 'DNN'), or None when it has no active dropout layer."""
        network = getattr(self, name, None)
        streams = self._dropout_streams
        known = streams.get(name)
        if known is None or known[0] is not network:
            stream = None
            if nn.active_dropout_layers(network):
                stream = nn.DropoutStream(DROPOUT_DRAW_BASES[name], option(self.settings, 'device_random_seed'),
                                          self.starting_step, DROPOUT_DRAW_RANGE)
                nn.attach_dropout_stream(network, stream)
            known = streams[name] = (network, stream)
        return known[1]

    def dropout_section(self, name, index):
        """Context manager: the dropout calls of network ``name`` inside it take their draw ids from section ``index``."""
        stream = self.dropout_stream(name)
        return contextlib.nullcontext() if stream is None else stream.section(index)

    def prepare_dropout_streams(self):
        """The device states exist (a HIP graph capture must not be the first to need them: made inside it, a state would be
        a copy from the host)."""
        for name in DROPOUT_DRAW_BASES:
            stream = self.dropout_stream(name)
            if stream is not None:
                stream.state()

    # ------------------------------------------------------------------------------------------ batch reductions
    def _global_batch(self, local):
        return local if self.dp is None else self.dp.global_batch(local)

    def batch_mean_of_features(self, features, rank_specific_use=False):
        """Mean over the (global) batch -> shape features.shape[1:] (the ``mean(0)`` of srgan.py:442-443).
        ``rank_specific_use``: what is computed from the mean differs between the ranks (see ``all_reduce_sum_var``)."""
        sums = F.col_sum(features)
        if self.parallel:
            sums = self.dp.all_reduce_sum_var(sums, reduce_backward=rank_specific_use)
        return F.scale(sums, 1.0 / self._global_batch(features.shape[0]))

    def batch_mean_of_examples(self, per_example):
        """Mean over the (global) batch of per-example scalars.  Under data parallelism this is the rank's
        partial sum / global batch: gradients add up over ranks, and logged values are summed over ranks."""
        return F.scale(F.sum_all(per_example), 1.0 / self._global_batch(per_example.shape[0]))

    # ------------------------------------------------------------------------------------------ the hot path
    def dnn_training_step(self, examples, labels, step):
        """One round of DNN training (reference srgan.py:259-271).

        The DNN baseline and the GAN networks never exchange anything inside an iteration, so with
        ``settings.overlap_dnn_step = True`` this step is only ENQUEUED here, on a second HIP stream: its ~3000
        launches -- mostly small kernels on 32x32 / 16x16 planes that cannot fill 256 CUs on their own -- then run
        concurrently with the discriminator / generator step on the main stream (measured: 316.6 -> 306.1 ms per
        step, +3.4 % images/s).  ``gan_training_step`` joins the two streams before it returns; anything else that
        touches the DNN first calls ``join_dnn_stream()``.  Off by default: with two streams in flight a kernel's
        duration no longer measures the kernel (bench.py's per-kernel roofline would read 34 % instead of 40 %)."""
        examples, labels = as_var(examples), as_var(labels)
        self._apply_stream_settings()
        side = self._dnn_side_stream()
        if side is None:
            return self._dnn_training_step(examples, labels, step)
        if not self._batches_are_resident() or torch.cuda.is_current_stream_capturing():
            # the batch was produced on the main stream; while a HIP graph is being captured the wait is also what
            # FORKS the side stream into the capture (the batches then are the graph's static input copies, and the
            # chain is joined again before the capture ends, gan_training_step)
            side.wait_stream(torch.cuda.current_stream())
        # (resident batches, eager: the DNN step of iteration i + 1 may start while iteration i's generator step still runs
        # -- the DNN shares nothing with the GAN networks, so its stream only ever waits for its own previous step)
        with torch.cuda.stream(side):
            self._dnn_training_step(examples, labels, step)

    def _dnn_side_stream(self):
        if not self._stream_setting('overlap_dnn_step') or not examples_on_gpu():
            return None
        if self._dnn_stream is None:
            self._dnn_stream = torch.cuda.Stream()
        return self._dnn_stream

    def _auxiliary_stream(self):
        """A second stream for forward passes that nothing differentiates (``settings.overlap_generator_forwards``)."""
        if not self._stream_setting('overlap_generator_forwards') or not examples_on_gpu() or self.parallel:
            # (under data parallelism the chains run on THREE streams -- main, gradient penalty, DNN step -- so that RCCL's
            # communication stream gets the fourth hardware queue of the HIP runtime to itself: a fifth stream aliases onto a
            # queue and couples two chains)
            return None
        if self._aux_stream is None:
            self._aux_stream = torch.cuda.Stream()
        return self._aux_stream

    def _penalty_stream(self):
        """A stream of its own for the gradient-penalty chain (``settings.overlap_gradient_penalty``; shared-forwards
        schedule; while a HIP graph is captured the fork / join below become edges of the graph; under data parallelism D's gradient exchange then starts after the
        two chains have joined and runs under the generator forward instead of under the penalty's backward): D(interpolates), the recorded gradient w.r.t. them, the double
        backward and the backward through the forward graph (reference srgan.py:294-295) are a chain of batch-sized kernels
        that depends on nothing of the stacked pass over [x, u, fake] (srgan.py:279-292) but the generated images -- the two
        chains run next to each other, each into its own gradient buffer of D's arena."""
        if not self._stream_setting('overlap_gradient_penalty') or not examples_on_gpu() or \
                getattr(self.D, '_srgan_arena', None) is None:
            return None
        if self._gp_stream is None:
            # (default priority: a high-priority stream for this, the longest chain, is one more hardware queue and lost 18-47 %
            # under graph replay and data parallelism, profiles/r05_stream_priority.txt)
            self._gp_stream = torch.cuda.Stream(priority=0)
        return self._gp_stream

    def _gradient_penalty_on_its_own_stream(self, stream, fake_examples, unlabeled_examples):
        main = torch.cuda.current_stream()
        stream.wait_stream(main)                          # the generated images, the batch, last step's weight update
        arena = self.D._srgan_arena
        with torch.cuda.stream(stream):
            with arena.gradients_into_alternate() as alternate:
                F.fill_(alternate, 0.0)
                with self.precision('penalty'):
                    gradient_penalty = self.gradient_penalty_calculation(fake_examples, unlabeled_examples)
                    self.scaled_backward(gradient_penalty)
        for var in (gradient_penalty, self.gradient_norm, self.interpolates_features):
            if var is not None:
                var.data.record_stream(main)              # read on the main stream after the join (summaries)
        return gradient_penalty

    def _apply_stream_settings(self):
        """``settings.wgrad_stream`` (None: leave the module attribute as it is) -> ``fused.WGRAD_STREAM``."""
        wanted = option(self.settings, 'wgrad_stream')
        if self._single_compute_stream:
            wanted = False
        if wanted is not None:
            from . import fused
            fused.WGRAD_STREAM = bool(wanted)

    def _batches_are_resident(self):
        return bool(getattr(self.train_dataset_loader, 'resident', False))

    def _join_side_stream(self):
        if self._dnn_stream is not None:
            torch.cuda.current_stream().wait_stream(self._dnn_stream)

    def join_dnn_stream(self):
        """Settle the networks before anything outside the training step reads them: the current stream waits for an
        enqueued DNN step, and optimizer updates still waiting for their gradient exchange are applied."""
        self.finish_update()
        self._join_side_stream()

    # ---- data-parallel gradient exchange, overlapped with the step (no-ops on one device) ----------------------
    def gradient_exchange(self, module):
        """The asynchronous all-reduce of ``module``'s gradient arena for the LAST backward pass into it (handed to
        ``tape.backward(grad_ready=...)``); None on a single device."""
        if not self.parallel:
            return None
        # settings.gradient_wire_dtype ('f32' | 'bf16': buckets travel as bf16, the master gradients stay fp32) and
        # settings.gradient_exchange_form ('all_reduce' | 'reduce_scatter'), opt-in per configuration
        return self.dp.gradient_exchange(module._srgan_arena, wire=option(self.settings, 'gradient_wire_dtype'),
                                         form=option(self.settings, 'gradient_exchange_form'))

    # ---- mixed precision (BASELINE.json configs 2 and 5; the reference is fp32-only) --------------------------------
    def precision(self, phase='step'):
        """The MFMA operand type of a phase as a context manager: ``settings.compute_dtype`` ('f32' default, 'bf16',
        'f16') for the step, ``settings.gradient_penalty_dtype`` (default 'f32': "fp16 with fp32 GP") for the
        gradient-penalty chain -- its forward, the recorded inner gradient and the penalty's own backward."""
        name = option(self.settings, 'compute_dtype')
        if phase == 'penalty':
            name = option(self.settings, 'gradient_penalty_dtype')
        # settings.storage_dtype ('bf16' / 'f16' / None): the networks with a 16-bit data path (blocked16) keep activations
        # and gradients in that type while the phase computes in it; a phase in another type (an fp32 penalty chain) does not
        storage = option(self.settings, 'storage_dtype')
        if storage and F.COMPUTE_DTYPES[storage] == F.COMPUTE_DTYPES[name]:
            return _Contexts(F.compute_dtype(name), F.storage_dtype(storage))
        # settings.blocked_fp32: a phase that computes in fp32 runs the DCGAN stacks' 4x4 / stride 2 stages on fp32 tensors in
        # the blocked layout (exact arithmetic on the LDS-DMA kernels of csrc/blocked16_k4s2.hip)
        if F.COMPUTE_DTYPES[name] == 0 and option(self.settings, 'blocked_fp32'):
            return _Contexts(F.compute_dtype(name), F.storage_dtype('f32b'))
        return _Contexts(F.compute_dtype(name), F.storage_dtype(None))

    def scaled_backward(self, root, **arguments):
        """``backward(root)`` with the root gradient set to ``settings.loss_scale`` (static loss scaling for the fp16 mode:
        gradients of 1e-6 would otherwise reach the fp16 operands as subnormals); ``apply_update`` divides it out."""
        scale = float(option(self.settings, 'loss_scale'))
        return backward(root, grad=None if scale == 1.0 else F.full_like(root, scale), **arguments)

    def apply_update(self, optimizer):
        scale = float(option(self.settings, 'loss_scale'))
        if scale != 1.0:
            F._unary_raw(F.U_AFFINE, optimizer.arena.grad, 1.0 / scale, 0.0, out=optimizer.arena.grad)
        optimizer.step()

    def start_update(self, name, optimizer, exchange):
        """The optimizer step of network ``name``: at once on a single device; under data parallelism after its gradient
        exchange, i.e. in ``finish_update`` -- the rest of the arena goes out now and the step continues meanwhile."""
        if exchange is None:
            self.apply_update(optimizer)
            return
        exchange.finish()
        if not option(self.settings, 'overlap_gradient_exchange'):
            exchange.wait()
            self.apply_update(optimizer)
            return
        self._pending_updates[name] = (exchange, optimizer)

    def finish_update(self, *names):
        """Wait for the gradient exchange of the named networks (default: all) and apply their optimizer updates."""
        for name in (names or tuple(self._pending_updates)):
            pending = self._pending_updates.pop(name, None)
            if pending is None:
                continue
            exchange, optimizer = pending
            side = self._dnn_side_stream() if name == 'DNN' else None
            if side is not None:                    # the DNN's step and exchange live on the side stream
                with torch.cuda.stream(side):
                    exchange.wait()
                    self.apply_update(optimizer)
            else:
                exchange.wait()
                self.apply_update(optimizer)

    def _dnn_training_step(self, examples, labels, step):
        self.DNN.apply(disable_batch_norm_updates)
        self.dnn_summary_writer.step = step
        self.finish_update('DNN')
        self.dnn_optimizer.zero_grad()
        dropout = self.dropout_stream('DNN')
        if dropout is not None:
            dropout.begin_step()
        exchange = self.gradient_exchange(self.DNN)
        with self.precision():
            dnn_loss = self.dnn_loss_calculation(examples, labels)
            self.scaled_backward(dnn_loss, grad_ready=exchange)
        if dropout is not None:
            # the DNN's masks of this iteration are all drawn: every launch that reads the state -- the forward's and the
            # backward's dropout kernels -- is on this stream, in front of this line
            dropout.advance()
        self.start_update('DNN', self.dnn_optimizer, exchange)       # finished at the end of gan_training_step
        self.last_losses['dnn_loss'] = dnn_loss
        if self.dnn_summary_writer.is_summary_step():
            self.dnn_summary_writer.add_scalar('Discriminator/Labeled Loss', self.loss_value(dnn_loss, partial=True))
            if getattr(self.DNN, 'features', None) is not None:
                norms = F.row_norm(F.flatten2d(self.DNN.features.detach()))
                self.dnn_summary_writer.add_scalar('Feature Norm/Labeled', F.mean_all(norms).item())

    def gan_training_step(self, labeled_examples, labels, unlabeled_examples, step):
        """One round of GAN training (reference srgan.py:273-320)."""
        settings = self.settings
        labeled_examples, labels = as_var(labeled_examples), as_var(labels)
        unlabeled_examples = as_var(unlabeled_examples)
        self._apply_stream_settings()
        self.D.apply(disable_batch_norm_updates)
        self.gan_summary_writer.step = step
        self.finish_update('G', 'D')         # the previous iteration's generator update (its exchange ran under the DNN step)
        self.d_optimizer.zero_grad()
        dropout = self.dropout_stream('D')
        if dropout is not None:
            dropout.begin_step()
        batch_size = unlabeled_examples.shape[0]
        penalty_stream = None
        with self.precision():
            if option(settings, 'reference_schedule'):
                labeled_loss = self.labeled_loss_calculation(labeled_examples, labels)
                self.scaled_backward(labeled_loss)
                unlabeled_loss = self.unlabeled_loss_calculation(labeled_examples, unlabeled_examples)
                self.scaled_backward(unlabeled_loss)
                z = self.sample_discriminator_noise(batch_size)
                with no_grad():
                    fake_examples = self.G(z)
                fake_loss = self.fake_loss_calculation(unlabeled_examples, fake_examples)
                self.scaled_backward(fake_loss)
            else:
                z = self.sample_discriminator_noise(batch_size)
                with no_grad():
                    fake_examples = self.G(z)
                penalty_stream = self._penalty_stream()
                if penalty_stream is not None:
                    gradient_penalty = self._gradient_penalty_on_its_own_stream(penalty_stream, fake_examples,
                                                                                unlabeled_examples)
                labeled_loss, unlabeled_loss, fake_loss = self.discriminator_losses_shared_forwards(
                    labeled_examples, labels, unlabeled_examples, fake_examples)
                self.scaled_backward(F.add(F.add(labeled_loss, unlabeled_loss), fake_loss))
        generator_phase = step % settings.generator_training_step_period == 0
        generator_fake = None
        if generator_phase and penalty_stream is not None:
            # The generator's forward pass of the generator step (srgan.py:300-302) depends on nothing the discriminator step
            # produces -- only D(fake) needs the updated discriminator -- so it is enqueued HERE, behind the stacked pass's
            # backward: the main stream would otherwise idle until the (longer) penalty chain has joined (measured: the
            # stacked chain ends 16 ms before the penalty chain).  The random draws keep the reference's order (z_D, alpha, z_G).
            self.g_optimizer.zero_grad()
            with self.precision():
                generator_fake = self.G(self.sample_generator_noise(batch_size))
        exchange = self.gradient_exchange(self.D)
        if penalty_stream is not None:
            # the penalty chain accumulated into the arena's second gradient buffer on its own stream: join and add
            torch.cuda.current_stream().wait_stream(penalty_stream)
            arena = self.D._srgan_arena
            F._binary_raw(F.B_ADD, arena.grad, arena._alternate, out=arena.grad)
        else:
            with self.precision('penalty'):
                gradient_penalty = self.gradient_penalty_calculation(fake_examples, unlabeled_examples)
                self.scaled_backward(gradient_penalty, grad_ready=exchange)   # the last backward pass into D's arena (srgan.py:295)
        self.start_update('D', self.d_optimizer, exchange)
        generator_loss = None
        if generator_phase:
            with self.precision():
                if generator_fake is None:
                    self.g_optimizer.zero_grad()
                    generator_fake = self.G(self.sample_generator_noise(batch_size))   # runs while D's gradients are still being exchanged
                self.finish_update('D')
                generator_loss = self.generator_loss_calculation(generator_fake, unlabeled_examples)
                exchange = self.gradient_exchange(self.G)
                self.scaled_backward(generator_loss, grad_ready=exchange)
            self.start_update('G', self.g_optimizer, exchange)      # finished when G is next used (next iteration)
        if self.device_random_draws():
            # ONE advance of the draws' iteration count per iteration (also when the generator does not train), on the main
            # stream.  Every fill of iteration t lies between the advances of t - 1 and t: z_D and z_G are filled on this
            # stream, in front of this line; alpha is filled on the penalty stream, which waited for this stream (behind the
            # previous advance) before its chain started and which this stream waited for above, before the arenas were
            # added; the DNN chain and the auxiliary forward draw nothing.  A captured step holds the same edges.
            F.random_advance(self.device_draw_state())
        if dropout is not None:
            # ONE advance of D's dropout state per iteration, on the main stream, behind every launch that reads it: the
            # stacked pass, D(fake) of the generator step and their backwards run on this stream; the penalty chain (forward,
            # recorded backward, double backward) runs on the penalty stream, which waited for this stream (behind the
            # previous advance) before it started and which this stream waited for before the arenas were added; D(u) of
            # the generator step runs on the auxiliary stream between its wait for this stream and this stream's wait for it
            # (generator_loss_calculation).  A captured step holds the same edges.
            dropout.advance()
        self.finish_update('D', 'DNN')
        self.last_losses.update(labeled_loss=labeled_loss, unlabeled_loss=unlabeled_loss, fake_loss=fake_loss,
                                gradient_penalty=gradient_penalty, generator_loss=generator_loss)
        if not self._batches_are_resident() or self.gan_summary_writer.is_summary_step() or \
                self.dnn_summary_writer.is_summary_step() or torch.cuda.is_current_stream_capturing():
            # (a batch that is freed after the iteration must outlive its DNN step; resident batches let the DNN stream
            # run on into the next iteration -- everything that reads the DNN joins it first, join_dnn_stream(); a HIP
            # graph capture must end with every forked stream joined)
            self._join_side_stream()
        if self.gan_summary_writer.is_summary_step():
            writer = self.gan_summary_writer
            if generator_loss is not None:
                writer.add_scalar('Generator/Loss', self.loss_value(generator_loss))
            writer.add_scalar('Discriminator/Labeled Loss', self.loss_value(labeled_loss, partial=True))
            writer.add_scalar('Discriminator/Unlabeled Loss', self.loss_value(unlabeled_loss))
            writer.add_scalar('Discriminator/Fake Loss', self.loss_value(fake_loss))
            writer.add_scalar('Discriminator/Gradient Penalty', self.loss_value(gradient_penalty, partial=True))
            writer.add_scalar('Discriminator/Gradient Norm', self.loss_value(
                self.batch_mean_of_examples(self.gradient_norm.detach()), partial=True))
            if self.labeled_features is not None and self.unlabeled_features is not None:
                with no_grad():
                    for tag, features in (('Labeled', self.labeled_features), ('Unlabeled', self.unlabeled_features)):
                        mean = self.batch_mean_of_features(features.detach())
                        writer.add_scalar('Feature Norm/' + tag, F.sqrt(F.sum_all(F.square(mean))).item())

    def _distance_over_the_ranks_rows(self, distance_function, difference):
        from . import utility
        mean_type = (utility.abs_mean, utility.abs_mean_neg, utility.abs_plus_one_log_mean_neg,
                     utility.abs_plus_one_sqrt_mean_neg, utility.square_mean)
        if distance_function in mean_type:
            return F.scale(self.dp.all_reduce_sum_var(distance_function(difference)), 1.0 / self.dp.world_size)
        if distance_function is utility.norm_mean:
            return F.sqrt(self.dp.all_reduce_sum_var(F.sum_all(F.square(difference))))
        raise NotImplementedError(f'normalize_feature_norm under data parallelism: no rule to assemble '
                                  f'{getattr(distance_function, "__name__", distance_function)} from the ranks\' rows')

    def loss_value(self, loss, partial=False):
        """Host value of a device scalar; ``partial`` scalars are per-rank partial sums under data parallelism."""
        value = float(loss.item())
        if partial and self.parallel:
            value = self.dp.all_reduce_sum_float(value)
        return value

    def synchronize_gradients(self, module):
        """Blocking form of the gradient exchange (methods that do not overlap it: the DNN-only experiment)."""
        if self.parallel:
            self.dp.all_reduce_gradients(module._srgan_arena)

    def discriminator_losses_shared_forwards(self, labeled_examples, labels, unlabeled_examples, fake_examples):
        """Labeled + unlabeled + fake losses from ONE discriminator pass over the three batches stacked along the
        batch dimension; same mathematics as srgan.py:329-358, which runs five separate forwards (the discriminator
        acts per example: its batch-norm layers are frozen, srgan.py:276).  One pass over 3B examples instead of
        three over B triples the work per kernel launch, which is what the 16x16 / 32x32 dense blocks lack."""
        settings = self.settings
        sizes = (labeled_examples.shape[0], unlabeled_examples.shape[0], fake_examples.shape[0])
        stackable = option(settings, 'batched_discriminator') and not self._stack_too_large and \
            tuple(labeled_examples.shape[1:]) == tuple(unlabeled_examples.shape[1:]) == tuple(fake_examples.shape[1:])
        if stackable:
            # Stacking triples the batch of every activation; one of them may then pass the 2^31-element limit of the
            # kernels' 32-bit offsets although the three batches fit on their own (e.g. VGG-16 at batch 600: 1800 x 64 x
            # 128 x 128).  The library reports that as SRGAN_ERANGE; the three separate passes are the same mathematics.
            try:
                stacked = F.cat_rows([labeled_examples, unlabeled_examples, fake_examples.detach()])
                predicted = self.D(stacked)
                features = self.D.features
            except _lib.HipLibraryError as error:
                if error.status != _lib.ERANGE:
                    raise
                print(f'stacked discriminator pass too large ({error}); using three separate passes')
                self._stack_too_large = True
                stackable = False
        if stackable:
            take = lambda value, first, count: (tuple(F.narrow_rows(v, first, count) for v in value)
                                                if isinstance(value, (tuple, list)) else F.narrow_rows(value, first, count))
            predicted_labels = take(predicted, 0, sizes[0])
            self.labeled_features = F.narrow_rows(features, 0, sizes[0])
            self.unlabeled_features = F.narrow_rows(features, sizes[0], sizes[1])
            self.fake_features = F.narrow_rows(features, sizes[0] + sizes[1], sizes[2])
        else:
            predicted_labels = self.D(labeled_examples)
            self.labeled_features = self.D.features
            _ = self.D(unlabeled_examples)
            self.unlabeled_features = self.D.features
            _ = self.D(fake_examples.detach())
            self.fake_features = self.D.features
        labeled_loss = self.labeled_loss_function(predicted_labels, labels, order=settings.labeled_loss_order)
        labeled_loss = F.scale(labeled_loss, settings.labeled_loss_multiplier)
        unlabeled_loss = self.feature_distance_loss(self.unlabeled_features, self.labeled_features)
        unlabeled_loss = F.scale(unlabeled_loss, settings.matching_loss_multiplier * settings.srgan_loss_multiplier)
        fake_loss = self.feature_distance_loss(self.unlabeled_features, self.fake_features,
                                               distance_function=settings.contrasting_distance_function)
        fake_loss = F.scale(fake_loss, settings.contrasting_loss_multiplier * settings.srgan_loss_multiplier)
        return labeled_loss, unlabeled_loss, fake_loss

    def dnn_loss_calculation(self, labeled_examples, labels):
        """reference srgan.py:322-327."""
        predicted_labels = self.DNN(labeled_examples)
        labeled_loss = self.labeled_loss_function(predicted_labels, labels, order=self.settings.labeled_loss_order)
        return F.scale(labeled_loss, self.settings.labeled_loss_multiplier)

    def labeled_loss_calculation(self, labeled_examples, labels):
        """reference srgan.py:329-335."""
        predicted_labels = self.D(labeled_examples)
        self.labeled_features = self.D.features
        labeled_loss = self.labeled_loss_function(predicted_labels, labels, order=self.settings.labeled_loss_order)
        return F.scale(labeled_loss, self.settings.labeled_loss_multiplier)

    def unlabeled_loss_calculation(self, labeled_examples, unlabeled_examples):
        """reference srgan.py:337-346."""
        _ = self.D(labeled_examples)
        self.labeled_features = self.D.features
        _ = self.D(unlabeled_examples)
        self.unlabeled_features = self.D.features
        unlabeled_loss = self.feature_distance_loss(self.unlabeled_features, self.labeled_features)
        return F.scale(unlabeled_loss, self.settings.matching_loss_multiplier * self.settings.srgan_loss_multiplier)

    def fake_loss_calculation(self, unlabeled_examples, fake_examples):
        """reference srgan.py:348-358."""
        _ = self.D(unlabeled_examples)
        self.unlabeled_features = self.D.features
        _ = self.D(fake_examples.detach())
        self.fake_features = self.D.features
        fake_loss = self.feature_distance_loss(self.unlabeled_features, self.fake_features,
                                               distance_function=self.settings.contrasting_distance_function)
        return F.scale(fake_loss, self.settings.contrasting_loss_multiplier * self.settings.srgan_loss_multiplier)

    def gradient_penalty_calculation(self, fake_examples, unlabeled_examples):
        """Interpolated-sample gradient penalty with its double backward (reference srgan.py:360-375).
        alpha has ``settings.batch_size`` entries as in the reference (:363), i.e. the unlabeled batch must
        have exactly that many examples (per rank under data parallelism)."""
        settings = self.settings
        expected = settings.batch_size if self.dp is None else self.dp.local_batch(settings.batch_size)
        alpha = self.sample_interpolation_alpha(expected)
        interpolates = F.gp_interpolate(unlabeled_examples.detach(), fake_examples.detach(), alpha)
        with self.dropout_section('D', DROPOUT_SECTION_PENALTY):
            interpolates_loss = self.interpolate_loss_calculation(interpolates)
        gradients, = backward(interpolates_loss, grad=F.full_like(interpolates_loss, 1.0), inputs=[interpolates],
                              create_graph=True)
        gradient_norm = F.row_norm(F.flatten2d(gradients))
        self.gradient_norm = gradient_norm
        norm_excesses = F.relu(F.add_scalar(gradient_norm, -1.0))
        penalty = self.batch_mean_of_examples(F.square(norm_excesses))
        return F.scale(penalty, settings.gradient_penalty_multiplier)

    def interpolate_loss_calculation(self, interpolates):
        """Per-example feature norm of the interpolates (reference srgan.py:377-381)."""
        _ = self.D(interpolates)            # differentiated twice: every node's backward is itself recorded
        self.interpolates_features = self.D.features
        return F.row_norm(F.flatten2d(self.interpolates_features))

    def generator_loss_calculation(self, fake_examples, unlabeled_examples):
        """reference srgan.py:383-391 (no srgan_loss_multiplier, Appendix A.4)."""
        with nn.frozen_parameters(self.D):
            side = self._auxiliary_stream()
            if side is None:
                _ = self.D(fake_examples)
                self.fake_features = self.D.features
                with no_grad(), self.dropout_section('D', DROPOUT_SECTION_GENERATOR_UNLABELED):
                    _ = self.D(unlabeled_examples)
                    detached_unlabeled_features = self.D.features.detach()
            else:
                # D(u) needs no gradient and shares nothing with D(fake) but the (frozen) weights: its batch-sized kernels
                # run on a second stream next to D(fake)'s, which on their own cannot fill the GPU on the small planes
                main = torch.cuda.current_stream()
                side.wait_stream(main)                   # the discriminator update and the batch are enqueued on main
                with torch.cuda.stream(side), no_grad(), self.dropout_section('D', DROPOUT_SECTION_GENERATOR_UNLABELED):
                    _ = self.D(unlabeled_examples)
                    detached_unlabeled_features = self.D.features.detach()
                detached_unlabeled_features.data.record_stream(main)
                _ = self.D(fake_examples)
                self.fake_features = self.D.features
                main.wait_stream(side)
        generator_loss = self.feature_distance_loss(detached_unlabeled_features, self.fake_features)
        return F.scale(generator_loss, self.settings.matching_loss_multiplier)

    # ------------------------------------------------------------------------------------------ plug-in hooks
    @abstractmethod
    def dataset_setup(self):
        """Prepares the datasets and loaders (reference srgan.py:393-400)."""

    @abstractmethod
    def model_setup(self):
        """Assigns self.DNN, self.D and self.G (reference srgan.py:402-407)."""

    @abstractmethod
    def validation_summaries(self, step: int):
        """Per-application evaluation summaries (reference srgan.py:409-412)."""

    def labeled_loss_function(self, predicted_labels, labels, order=2):
        """mean(|p - y| ** order) (reference srgan.py:414-417).  A (B, 1) prediction against (B) labels
        broadcasts to (B, B) exactly as in the reference's VGG path (Appendix A.12)."""
        if len(predicted_labels.shape) == 2 and predicted_labels.shape[1] == 1 and len(labels.shape) == 1:
            batch = predicted_labels.shape[0]
            rows = F.row_broadcast(F.view(predicted_labels, (batch,)), (batch, batch))
            columns = F.col_broadcast(labels, batch)
            difference = F.sub(rows, columns)
            return F.scale(F.sum_all(F.pow_scalar(F.abs_(difference), order)),
                           1.0 / (batch * self._global_batch(batch)))
        difference = F.sub(predicted_labels, F.view(labels, predicted_labels.shape))
        return self.batch_mean_of_examples(F.pow_scalar(F.abs_(difference), order))

    def evaluate(self):
        self.model_setup()
        self.gpu_mode()
        self.load_models(with_optimizers=False)
        self.eval_mode()

    def predicted_labels(self, network, examples):
        """The labels ``network`` predicts for ``examples``, one per example (the reference's ``images_to_predicted_ages`` /
        ``images_to_predicted_angles``, age/srgan.py:109-112, driving/srgan.py:106-110).  An application whose networks return
        something else overrides it (the age SGAN's class logits)."""
        return network(examples)

    def prediction_rows(self, network, examples):
        """``(rows, bins)`` for the device evaluation: ``bins`` None and one prediction per row -- ``predicted_labels`` -- or
        ``[B, K]`` class logits with the ``K`` bin values, of which ``srgan_regression_evaluation_sums`` takes the first
        maximal one's on the device."""
        return self.predicted_labels(network, examples), None

    def validation_forward_context(self):
        """``validation_precision = 'step'``: the evaluation's forward passes run on the data path the run trains on."""
        return self.precision() if self.validation_precision == 'step' else contextlib.nullcontext()

    def regression_evaluation_epoch(self, network, dataset, summary_writer, summary_name, comparison_value=None,
                                    normalized=False):
        """MAE / MSE (and NMAE = MAE / label range with ``normalized``) of ``network`` over ``dataset`` -- any
        iterable of ``(examples, labels)`` batches -- as summary scalars; ratio to ``comparison_value`` (the DNN's MAE)
        when given.  Forward passes only (reference age/srgan.py:92-107, driving/srgan.py:87-104)."""
        predictions, labels = [], []
        self.join_dnn_stream()
        with no_grad(), self.validation_forward_context():
            for examples, batch_labels in dataset:
                predicted = self.predicted_labels(network, as_var(examples))
                predictions.append(predicted.cpu().numpy().reshape(-1).astype(np.float64))
                labels.append(np.asarray(batch_labels.cpu() if hasattr(batch_labels, 'cpu') else batch_labels,
                                         dtype=np.float64).reshape(-1))
        predictions, labels = np.concatenate(predictions), np.concatenate(labels)
        mae = float(np.abs(predictions - labels).mean())
        summary_writer.add_scalar('{}/MAE'.format(summary_name), mae)
        if normalized:
            summary_writer.add_scalar('{}/NMAE'.format(summary_name), mae / float(labels.max() - labels.min()))
        summary_writer.add_scalar('{}/MSE'.format(summary_name), float((np.abs(predictions - labels) ** 2).mean()))
        if comparison_value is not None:
            summary_writer.add_scalar('{}/Ratio MAE GAN DNN'.format(summary_name), mae / comparison_value)
        return mae

    def regression_evaluation_epoch_device(self, network, dataset, record):
        """One evaluation epoch with nothing going back to the host: per batch one forward pass and one
        ``srgan_regression_evaluation_sums`` call, on the stream the forward ran on, into ``record`` -- eight doubles on the
        device that start as ``EVALUATION_RECORD``.  Batches of a resident loader (``in_order``) and of ``SyntheticLoader`` are
        on the device already; a host tensor is uploaded.  No collective: under data parallelism every rank evaluates what it
        evaluates on the host path."""
        self.join_dnn_stream()
        lib = _lib.library()
        device = record.device
        with no_grad(), self.validation_forward_context():
            for examples, batch_labels in dataset:
                rows, bins = self.prediction_rows(network, as_var(examples))
                rows = (rows.data if isinstance(rows, Var) else rows).float()
                rows = rows.reshape(rows.shape[0], -1).contiguous()
                batch, width = rows.shape
                labels = torch.as_tensor(batch_labels).to(device, dtype=torch.float32, non_blocking=True)
                labels = labels.reshape(-1).contiguous()
                if labels.shape[0] != batch:
                    raise ValueError('{} labels for {} predicted rows'.format(labels.shape[0], batch))
                if bins is None:
                    if width != 1:
                        raise ValueError('one prediction per example is evaluated, the network gave {}'.format(width))
                else:
                    bins = (bins.data if isinstance(bins, Var) else bins).to(device, dtype=torch.float32).reshape(-1).contiguous()
                    if bins.shape[0] < width:
                        raise ValueError('{} class logits but {} bins'.format(width, bins.shape[0]))
                _lib.check(lib.srgan_regression_evaluation_sums(
                    rows.data_ptr(), width, width, None if bins is None else bins.data_ptr(), labels.data_ptr(), batch,
                    record.data_ptr(), _lib.stream_handle()), 'srgan_regression_evaluation_sums')

    EVALUATION_RECORD = (0.0, 0.0, 0.0, 0.0, float('inf'), float('-inf'), 0.0, 0.0)      # an epoch's eight doubles before its
    # first batch: sum d, sum |d|, sum d * d, examples, smallest label, largest label, two reserved (include/srgan_hip.h)

    @staticmethod
    def download_evaluation_records(records):
        """The one device-to-host copy of a summary step on the device path: its four 64-byte records."""
        return records.cpu().numpy()

    @staticmethod
    def log_regression_record(record, summary_writer, summary_name, comparison_value=None, normalized=False):
        """The scalars of ``regression_evaluation_epoch`` from an epoch's downloaded record, under the same tags in the same
        order; returns the MAE."""
        _, absolute, square, examples, smallest, largest = (float(value) for value in record[:6])
        if examples == 0:
            raise ValueError('the evaluation set is empty')
        mae = absolute / examples
        summary_writer.add_scalar('{}/MAE'.format(summary_name), mae)
        if normalized:
            summary_writer.add_scalar('{}/NMAE'.format(summary_name), mae / (largest - smallest))
        summary_writer.add_scalar('{}/MSE'.format(summary_name), square / examples)
        if comparison_value is not None:
            summary_writer.add_scalar('{}/Ratio MAE GAN DNN'.format(summary_name), mae / comparison_value)
        return mae

    def regression_validation_summaries(self, normalized=False):
        """DNN and D on the train and validation batches, D's validation MAE relative to the DNN's (reference
        age/srgan.py:52-71, driving/srgan.py:48-67; the image grids: ``regression_image_summaries``).  A loader over a database
        (``in_order``) is walked once in stored order, every example of the split as upstream; any other loader is iterated.

        ``regression_validation = 'device'``: the four epochs leave their sums in four consecutive 64-byte records of one device
        tensor (``regression_evaluation_epoch_device``), one download of those 256 bytes ends the step, and the scalars are
        formed from the records -- the same tags in the same order as the host path, the DNN's validation MAE under D's ratio."""
        if self.regression_validation not in ('host', 'device'):
            raise ValueError("regression_validation is 'host' or 'device', not {!r}".format(self.regression_validation))
        if self.validation_precision not in ('f32', 'step'):
            raise ValueError("validation_precision is 'f32' or 'step', not {!r}".format(self.validation_precision))
        train, validation = (loader.in_order() if hasattr(loader, 'in_order') else loader
                             for loader in (self.train_dataset_loader, self.validation_dataset_loader))
        epochs = ((self.DNN, train, self.dnn_summary_writer, '2 Train Error'),
                  (self.DNN, validation, self.dnn_summary_writer, '1 Validation Error'),
                  (self.D, train, self.gan_summary_writer, '2 Train Error'),
                  (self.D, validation, self.gan_summary_writer, '1 Validation Error'))
        records = None
        if self.regression_validation == 'device':
            records = torch.tensor([self.EVALUATION_RECORD] * len(epochs), dtype=torch.float64, device=current_device())
            for record, (network, dataset, _, _) in zip(records, epochs):
                self.regression_evaluation_epoch_device(network, dataset, record)
            records = self.download_evaluation_records(records)
        dnn_mae = None
        for index, (network, dataset, summary_writer, summary_name) in enumerate(epochs):
            comparison_value = dnn_mae if index == 3 else None
            if records is None:
                mae = self.regression_evaluation_epoch(network, dataset, summary_writer, summary_name,
                                                       comparison_value=comparison_value, normalized=normalized)
            else:
                mae = self.log_regression_record(records[index], summary_writer, summary_name,
                                                 comparison_value=comparison_value, normalized=normalized)
            if index == 1:
                dnn_mae = mae

    # ``settings.image_summaries``: the pictures the reference writes at every summary step -- grids of training images and
    # of G's samples, the crowd map comparison -- built on the device (``image_summaries.py``) and downloaded once each by
    # ``SummaryWriter.add_image``.  Nothing here draws from a host stream or advances a loader's schedule, so a run trains the
    # same bits with the setting on and off.
    SUMMARY_DRAW_STANDARD, SUMMARY_DRAW_OFFSET = 8, 9      # draw ids of the two summary z (the training draws are 0, 1, 2)

    def image_summaries_on(self):
        """Under data parallelism only the rank that writes the trial's event files launches anything (no collective is
        involved: G in eval mode and the two image kernels are local)."""
        return bool(option(self.settings, 'image_summaries')) and (self.dp is None or self.dp.rank == 0)

    def real_image_summary(self, examples, range):
        """``Real`` on the GAN writer: the first ``min(9, B)`` of ``examples`` in a grid three wide (reference
        age/srgan.py:74-78).  The callers pass the train loader's first batch in STORED order: the reference shows a shuffled
        batch, which would consume torch's generator."""
        examples = examples.data if isinstance(examples, Var) else examples
        self.gan_summary_writer.add_image('Real', image_summaries.make_grid(examples[:9], nrow=3, normalize=True, range=range))

    def first_train_batch(self):
        """The examples of the train loader's first batch, in stored order where the loader can walk it (``in_order``)."""
        loader = self.train_dataset_loader
        return next(iter(loader.in_order() if hasattr(loader, 'in_order') else loader))[0]

    def generated_image_summaries(self, range, to_images=None):
        """``Fake/Standard`` and ``Fake/Offset`` on the GAN writer (reference age/srgan.py:79-90): G on ``min(9, batch_size)``
        z drawn on the device -- N(0, 1), and the mixture at ``settings.mean_offset`` -- from a state of its own,
        ``{device_random_seed, the writer's step}``, and draws 8 and 9: not the training draws' state, whether or not
        ``settings.device_random_draws`` is set.  ``to_images`` maps G's output to the value range ``range`` names."""
        count = min(9, self.settings.batch_size)
        state = self.summary_draw_state(self.gan_summary_writer.step)
        for tag, draw, offset in (('Fake/Standard', self.SUMMARY_DRAW_STANDARD, 0.0),
                                  ('Fake/Offset', self.SUMMARY_DRAW_OFFSET, self.settings.mean_offset)):
            z = F.random_fill((count, self.G.input_size), 1, offset, draw, state)
            with no_grad():
                fake = self.G(z).data
            if to_images is not None:
                fake = to_images(fake)
            self.gan_summary_writer.add_image(tag, image_summaries.make_grid(fake, nrow=3, normalize=True, range=range))

    def summary_draw_state(self, step):
        """Device int32 x 4 {seed_lo, seed_hi, step, 0} for the summary draws of ``step`` (``srgan_random_fill``'s state)."""
        return nn.draw_state(option(self.settings, 'device_random_seed'), step)

    def regression_image_summaries(self):
        """The image grids of the age and driving applications (reference age/srgan.py:73-90, driving/srgan.py:68-85): images
        in 0..255 through ``to_image_range``, normalised over (0, 255)."""
        if not self.image_summaries_on():
            return
        self.real_image_summary(to_image_range(self.first_train_batch()[:9]), range=(0, 255))
        self.generated_image_summaries(range=(0, 255), to_images=to_image_range)

    def start_loaders_at(self, step):
        """Before the first batch: a loader whose batches are a function of ``(seed, step)`` (``start_at``: the crowd loaders
        and the resident image loaders with device draws) is put at ``step``, so that a continued run cuts what the uninterrupted run cuts there."""
        for loader in (self.train_dataset_loader, self.unlabeled_dataset_loader):
            if getattr(loader, 'draw_mode', 'device') == 'device' and hasattr(loader, 'start_at'):
                loader.start_at(step)

    @staticmethod
    def infinite_iter(dataset):
        while True:
            for examples in dataset:
                yield examples

    def adjust_learning_rate(self, step):
        """lr * 0.1 ** (step // 100000), applied to the DNN optimizer only (reference srgan.py:432-436)."""
        lr = self.settings.learning_rate * (0.1 ** (step // 100000))
        for param_group in self.dnn_optimizer.param_groups:
            param_group['lr'] = lr

    def feature_distance_loss(self, base_features, other_features, distance_function=None):
        """distance(mean_b(base) - mean_b(other)) (reference srgan.py:438-449).

        ``settings.matching_feature_loss`` / ``settings.contrasting_feature_loss`` replace it: each is a callable
        ``(base_features, other_features) -> scalar Var``, e.g. ``feature_covariance_loss`` or ``feature_angle_loss`` below.
        A call without ``distance_function`` (the unlabeled loss and the generator loss) uses the matching one, the call that
        passes ``settings.contrasting_distance_function`` (the fake loss) the contrasting one.  A hook gets the features as
        the discriminator left them and decides about means and norms itself: ``settings.normalize_feature_norm`` is
        ignored.  One device only (``gpu_mode`` refuses them under data parallelism)."""
        hook = None
        if distance_function is None:
            hook = option(self.settings, 'matching_feature_loss')
        elif distance_function is self.settings.contrasting_distance_function:
            hook = option(self.settings, 'contrasting_feature_loss')
        if hook is not None:
            return hook(base_features, other_features)
        if distance_function is None:
            distance_function = self.settings.matching_distance_function
        normalize = self.settings.normalize_feature_norm
        base_mean_features = self.batch_mean_of_features(base_features, rank_specific_use=normalize)
        other_mean_features = self.batch_mean_of_features(other_features, rank_specific_use=normalize)
        if normalize:
            # The reference's branch AS WRITTEN (srgan.py:444-447): the base mean is divided by its norm, but line 447
            # divides the un-meaned ``other_features`` (B, F) by the norm of their mean, so the difference broadcasts to
            # (B, F) and the distance function averages over examples as well.  Off by default (settings.py:39).
            # Under data parallelism a rank holds its own rows of that (B, F) difference: the distance is assembled from the
            # ranks' parts (a mean over all elements = the mean of the equally sized shards' means; a norm = the root of the
            # summed squares), and the two batch means pass their gradients through an all-reduce of their own.
            epsilon = 1e-5

            def inverse_norm(vector):
                norm = F.sqrt(F.sum_all(F.square(vector)))
                return F.div(F.full_like(norm, 1.0), F.add_scalar(norm, epsilon))
            base_normalized = F.scalar_mul(base_mean_features, inverse_norm(base_mean_features))
            other_rows = F.flatten2d(other_features)
            other_normalized = F.scalar_mul(other_rows, inverse_norm(other_mean_features))
            difference = F.sub(F.col_broadcast(base_normalized, other_rows.shape[0]), other_normalized)
            if self.parallel:
                return self._distance_over_the_ranks_rows(distance_function, difference)
            return distance_function(difference)
        return distance_function(F.sub(base_mean_features, other_mean_features))

    @property
    def inference_network(self):
        return self.D

    def inference_setup(self):
        self.model_setup()
        self.gpu_mode()
        self.load_models(with_optimizers=False)
        self.eval_mode()

    def inference(self, input_):
        raise NotImplementedError


class _Contexts:
    """Several context managers entered / left together."""

    def __init__(self, *managers):
        self.managers = managers

    def __enter__(self):
        for manager in self.managers:
            manager.__enter__()
        return self

    def __exit__(self, *exc):
        for manager in reversed(self.managers):
            manager.__exit__(*exc)


# --------------------------------------------------------------------- alternative feature losses (reference srgan.py:472-535)
# Tape functions of two feature batches [B, F...]; any of them can be a settings.matching_feature_loss /
# settings.contrasting_feature_loss (Experiment.feature_distance_loss).  Scalars have shape [1], as everywhere on the tape.
def _batch_mean(features):
    rows = F.flatten2d(features)
    return F.scale(F.col_sum(rows), 1.0 / rows.shape[0])


def unit_vector(vector):
    """vector / (|vector| + 1e-10) (reference srgan.py:472-474)."""
    flat = F.view(vector, (vector.numel(),))
    norm_plus_epsilon = F.add_scalar(F.sqrt(F.sum_all(F.square(flat))), 1e-10)
    return F.view(F.scalar_mul(flat, F.div(F.full_like(norm_plus_epsilon, 1.0), norm_plus_epsilon)), vector.shape)


def angle_between(vector0, vector1):
    """The angle between two vectors, their cosine clamped to +-(1 - 1e-6) (reference srgan.py:477-482)."""
    epsilon = 1e-6
    cosine = F.sum_all(F.mul(unit_vector(vector0), unit_vector(vector1)))
    return F.acos(F.clamp(cosine, -1.0 + epsilon, 1.0 - epsilon))


def square(tensor):
    """Squares the tensor value (reference srgan.py:485-487)."""
    return F.square(tensor)


def feature_distance_loss_unmeaned(base_features, other_features, distance_function=square):
    """mean(distance(mean_b(base) - other)): only the base is averaged over the batch (reference srgan.py:490-494)."""
    other_rows = F.flatten2d(other_features)
    difference = F.sub(F.col_broadcast(_batch_mean(base_features), other_rows.shape[0]), other_rows)
    return F.mean_all(distance_function(difference))


def feature_distance_loss_both_unmeaned(base_features, other_features, distance_function=norm_squared):
    """mean(distance(base - other)), example by example (reference srgan.py:497-500)."""
    return F.mean_all(distance_function(F.sub(F.flatten2d(base_features), F.flatten2d(other_features))))


def feature_angle_loss(base_features, other_features, target=0, summary_writer=None):
    """|angle(mean_b(base), mean_b(other)) - target|^2 (reference srgan.py:503-508).  A ``summary_writer`` logs
    ``Feature Vector/Angle`` -- through ``.item()``, a host synchronisation: pass none inside a captured step."""
    angle = angle_between(_batch_mean(base_features), _batch_mean(other_features))
    if summary_writer:
        summary_writer.add_scalar('Feature Vector/Angle', angle.item())
    return F.square(F.abs_(F.add_scalar(angle, -float(target))))


def _correlation(xm, observations_in_rows):
    count = xm.shape[0] if observations_in_rows else xm.shape[1]
    covariance = F.scale(F.mm(xm, xm, transpose_a=observations_in_rows, transpose_b=not observations_in_rows), 1.0 / (count - 1))
    # (the diagonal of the covariance as the sums of squares it is made of: the tape has no diag(); equal in exact arithmetic)
    squares = F.col_sum(F.square(xm)) if observations_in_rows else F.row_sum(F.square(xm))
    stddev = F.sqrt(F.scale(squares, 1.0 / (count - 1)))
    inverse = F.div(F.full_like(stddev, 1.0), stddev)
    size = covariance.shape[0]
    by_columns = F.chan_affine(covariance, None, inverse, None, None, dims=(size, size, 1))
    return F.clamp(F.row_scale(by_columns, inverse), -1.0, 1.0)


def corrcoef(x):
    """The correlation coefficients of the ROWS of ``x`` [variables, observations] as a MATERIALISED matrix, composed of
    ``F.mm`` and elementwise tape operations (reference srgan.py:517-528): for a small number of variables and for callers
    who want the matrix.  ``feature_covariance_loss`` does NOT go through it."""
    mean = F.scale(F.row_sum(x), 1.0 / x.shape[1])
    return _correlation(F.sub(x, F.row_broadcast(mean, x.shape)), observations_in_rows=False)


def feature_corrcoef(x):
    """``corrcoef`` of the features (columns) of ``x`` [B, F] -> [F, F] (reference srgan.py:511-514), materialised; the
    transposition is folded into the contraction."""
    rows = F.flatten2d(x)
    xm = F.sub(rows, F.col_broadcast(_batch_mean(rows), rows.shape[0]))
    return _correlation(xm, observations_in_rows=True)


def feature_covariance_loss(base_features, other_features):
    """sum |feature_corrcoef(base) - feature_corrcoef(other)| (reference srgan.py:531-535) as ONE fused operation
    (``F.feature_corrcoef_l1``): the two F x F matrices are formed tile by tile on the fp32 MFMA and never stored, so it runs
    at F = 4096 (VGG) and F = 32768 (the DCGAN discriminators) too.  The diagonal contributes exactly 0; first order only."""
    return F.feature_corrcoef_l1(F.flatten2d(base_features), F.flatten2d(other_features))


def disable_batch_norm_updates(module):
    """Every batch-norm layer in eval mode (reference srgan.py:538-542).  The HIP batch-norm always uses the
    running statistics, so this only keeps ``module.training`` flags consistent with the reference."""
    if isinstance(module, torch.nn.modules.batchnorm._BatchNorm):
        module.eval()


def enable_batch_norm_updates(module):
    """reference srgan.py:545-549 (never used on the hot path: the re-enable is commented out upstream)."""
    if isinstance(module, torch.nn.modules.batchnorm._BatchNorm):
        module.train()
