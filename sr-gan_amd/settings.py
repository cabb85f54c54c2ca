"""Run settings: the attribute bag the experiments read, with the reference's names, defaults, attribute order and
list-expansion semantics (reference settings.py:12-127).  The defaults live in one table; ``Settings()`` instantiates it
in order, because ``convert_to_settings_list`` expands list-valued attributes in attribute order.  The settings this port adds
live in a second table, ``EXTENSIONS``, which ``Settings()`` does not instantiate; ``option`` reads them."""
import platform
import random
from copy import deepcopy
from enum import Enum

from .utility import abs_plus_one_sqrt_mean_neg, abs_mean

# (name, default) in the reference's declaration order; grouped as it groups them.
DEFAULTS = (
    # the run
    ('trial_name', 'base'), ('steps_to_run', 200000), ('temporary_directory', 'temporary'), ('logs_directory', 'logs'),
    ('batch_size', 1000), ('summary_step_period', 2000), ('labeled_dataset_size', 50), ('unlabeled_dataset_size', 50000),
    ('validation_dataset_size', 1000), ('learning_rate', 1e-4), ('weight_decay', 0),
    # the losses
    ('labeled_loss_multiplier', 1e0), ('matching_loss_multiplier', 1e0), ('contrasting_loss_multiplier', 1e0),
    ('srgan_loss_multiplier', 1e0), ('dggan_loss_multiplier', 1e1), ('gradient_penalty_on', True),
    ('gradient_penalty_multiplier', 1e1), ('mean_offset', 0), ('labeled_loss_order', 2),
    ('generator_training_step_period', 1), ('labeled_dataset_seed', 0), ('normalize_fake_loss', False),
    ('normalize_feature_norm', False), ('contrasting_distance_function', abs_plus_one_sqrt_mean_neg),
    ('matching_distance_function', abs_mean),
    # checkpoints, data loading, resuming
    ('load_model_path', None), ('should_save_models', True), ('skip_completed_experiment', True),
    ('number_of_data_workers', 4), ('pin_memory', True), ('continue_from_previous_trial', False),
    ('continue_existing_experiments', False), ('save_step_period', None),
    # coefficient application
    ('hidden_size', 10),
    # crowd application
    ('crowd_dataset', 'World Expo'), ('number_of_cameras', 5), ('number_of_images_per_camera', 5),
    ('test_summary_size', None), ('test_sliding_window_size', 128), ('image_patch_size', 224), ('label_patch_size', 224),
    ('map_multiplier', 1e-6), ('map_directory_name', 'i1nn_maps'),
    # SGAN models
    ('number_of_bins', 10),
    # DCGAN networks: the ``batch_norm`` switch of the reference's age / driving / crowd models.py, per network.  G's norm
    # layers use batch statistics in training mode, D's and DNN's are frozen (reference srgan.py:171,261,276).
    ('generator_batch_norm', False), ('discriminator_batch_norm', False),
)

# (name, default, what it is) of every setting that is NOT the reference's.  ``Settings()`` does not carry them (it mirrors the
# reference's attributes and order): a run sets the ones it wants as plain attributes, and every reader asks ``option``.
EXTENSIONS = (
    # the schedule of an iteration
    ('step_graph', False, 'capture the iteration once as a HIP graph and replay it (graph.py)'),
    ('step_graph_warmup', 2, 'eager iterations before the first capture'),
    ('step_graph_collectives', None, "'abi': capture the data-parallel exchanges too, through the C ABI's RCCL entry points"),
    ('reference_schedule', False, "the reference's exact forward / backward order instead of the shared forwards"),
    ('batched_discriminator', True, 'one discriminator pass over the labeled, unlabeled and fake batches stacked'),
    ('overlap_dnn_step', False, 'the DNN step on a stream of its own'),
    ('overlap_generator_forwards', False, "the generator step's D(unlabeled) on a stream of its own"),
    ('overlap_gradient_penalty', False, 'the gradient-penalty chain on a stream of its own'),
    ('overlap_gradient_exchange', True, 'optimizer updates wait for their gradient exchange only when the weights are next used'),
    ('wgrad_stream', None, 'True / False -> fused.WGRAD_STREAM; None leaves it alone'),
    # precision and layout
    ('compute_dtype', 'f32', "the MFMA operand type of the step: 'f32', 'bf16' or 'f16'"),
    ('gradient_penalty_dtype', 'f32', 'the same for the gradient-penalty chain'),
    ('storage_dtype', None, "'bf16' / 'f16': activations and gradients of the blocked data path in that type"),
    ('blocked_fp32', False, 'fp32 phases run the DCGAN 4x4 / stride 2 stages on blocked fp32 tensors'),
    ('blocked_batch_norm', False, 'a generator with batch-statistics norm layers stays on the blocked data path'),
    ('blocked_frozen_norm', False, 'a discriminator with frozen norm layers stays on the blocked data path'),
    ('loss_scale', 1.0, 'static loss scale: the root gradient of every backward, divided out before the update'),
    # data parallelism
    ('gradient_wire_dtype', None, "'f32' | 'bf16': the type the gradient buckets travel in"),
    ('gradient_exchange_form', None, "'all_reduce' | 'reduce_scatter'"),
    # randomness on the device
    ('device_random_draws', False, 'z_D, alpha and z_G from the counter-based generator instead of the host streams'),
    ('device_random_seed', 0, 'its 64-bit seed; also seeds the dropout masks and the summary draws'),
    ('drop_rate', 0, 'dropout on the new features of every dense layer of D and DNN'),
    # summaries and losses
    ('image_summaries', False, "the reference's image grids and crowd map comparisons, built on the device"),
    ('distribution_summaries', False, "the coefficient application's Wasserstein / KDE summaries, on the device"),
    ('matching_feature_loss', None, 'callable (base, other) -> scalar Var replacing the unlabeled and generator feature loss'),
    ('contrasting_feature_loss', None, 'the same for the fake loss'),
    # crowd application
    ('crowd_validation', None, "'device': validation summaries from evaluation sets cut from the resident database"),
    ('crowd_validation_scenes', None, 'how many test scenes that uploads (None: all)'),
    ('full_image_inference', 'host', "'device': the sliding-window inference of a full image on the device"),
)
_EXTENSION_DEFAULTS = {name: default for name, default, _ in EXTENSIONS}


def option(settings, name):
    """The value of extension ``name``: the attribute when ``settings`` has it (a set ``None`` stays ``None``), else the
    default of ``EXTENSIONS``.  A name the table does not have is a KeyError; ``settings`` is never written."""
    default = _EXTENSION_DEFAULTS[name]
    return getattr(settings, name, default)


# what ``local_setup`` shrinks on the reference author's laptop (settings.py:69-79)
LAPTOP_OVERRIDES = {'labeled_dataset_seed': 0, 'summary_step_period': 10, 'labeled_dataset_size': 10,
                    'unlabeled_dataset_size': 10, 'validation_dataset_size': 10, 'skip_completed_experiment': False,
                    'number_of_data_workers': 0}


class Settings:
    """One run's settings; any attribute may hold a list / tuple of alternatives (see ``convert_to_settings_list``)."""

    def __init__(self):
        for name, default in DEFAULTS:
            setattr(self, name, default)

    def local_setup(self):
        if 'Carbon' not in platform.node():
            return
        self.batch_size = min(10, self.batch_size)
        for name, value in LAPTOP_OVERRIDES.items():
            setattr(self, name, value)


def _first_alternative(settings):
    """(attribute name, alternatives) of the first list- or tuple-valued attribute, or None."""
    for name, value in vars(settings).items():
        if isinstance(value, (list, tuple)):
            return name, value
    return None


def convert_to_settings_list(settings, shuffle=True):
    """Cartesian expansion of every list / tuple valued attribute into separate deep copies, in attribute order,
    optionally shuffled (reference settings.py:82-111)."""
    expanded, pending = [], [settings]
    while pending:
        current = pending.pop(0)
        alternative = _first_alternative(current)
        if alternative is None:
            expanded.append(current)
            continue
        name, alternatives = alternative
        for value in alternatives:
            variant = deepcopy(current)
            setattr(variant, name, value)
            pending.append(variant)
    if shuffle:
        random.seed()
        random.shuffle(expanded)
    return expanded


ApplicationName = Enum('ApplicationName', {name: name for name in ('coefficient', 'age', 'crowd', 'driving')})
MethodName = Enum('MethodName', {name: name for name in ('srgan', 'dnn', 'dggan', 'sgan')})
