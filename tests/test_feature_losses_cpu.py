"""The alternative feature losses (srgan_amd.srgan: feature_angle_loss, feature_distance_loss_unmeaned,
feature_distance_loss_both_unmeaned, feature_covariance_loss), the parts that need no GPU: the tests' NumPy restatement
(feature_losses_reference.py) is pinned to the fixture recorded from the reference and obeys the correlation loss's rules; the
library advertises and binds the fused entry points and refuses bad arguments before any device work; the two settings are
optional, select the hooks, and are refused under data parallelism."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import feature_losses_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g19_feature_losses.npz')
PTR = 16      # a non-NULL, 16-byte aligned "pointer" that is never dereferenced: argument errors come first


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def keys(golden, group):
    return ['%dx%d' % tuple(shape) for shape in golden[group]]


def relative(got, expected):
    return np.abs(np.asarray(got) - expected).max() / max(np.abs(expected).max(), 1e-300)


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(R.LOSSES))
def test_the_restatement_reproduces_the_reference_to_1e_12(golden, name):
    checked_gradients = 0
    for key in keys(golden, 'gradient_shapes') + keys(golden, 'loss_only_shapes') + ['parallel']:
        if f'{key}/{name}/value' not in golden:
            continue                                                   # (parallel has no correlation loss: its signs are noise)
        value, grad_base, grad_other = R.LOSSES[name](golden[f'{key}/base'], golden[f'{key}/other'])
        expected = float(golden[f'{key}/{name}/value'])
        # (the floor: (2, 3) has every correlation at +-1 with equal signs on both sides -- a loss of 2^-52, the rounding of
        # entries of magnitude 1, where "relative" says nothing)
        features = golden[f'{key}/base'].shape[1]
        assert abs(value - expected) <= 1e-12 * abs(expected) + features * (features - 1) * 2.0 ** -52, key
        if f'{key}/{name}/grad_base' in golden:
            assert relative(grad_base, golden[f'{key}/{name}/grad_base']) <= 1e-12, key
            assert relative(grad_other, golden[f'{key}/{name}/grad_other']) <= 1e-12, key
            checked_gradients += 1
    assert checked_gradients >= 4


def test_the_fixture_keeps_every_entry_away_from_a_sign_flip(golden):
    for key in keys(golden, 'gradient_shapes'):
        base, other = golden[f'{key}/base'], golden[f'{key}/other']
        assert base.dtype == np.float32 and other.dtype == np.float32          # the device gets the reference's inputs bit for bit
        features = base.shape[1]
        gap = np.abs(R.corrcoef_rows(base, 0, features) - R.corrcoef_rows(other, 0, features))
        gap[np.diag_indices(features)] = np.inf
        assert gap.min() >= 1e-5 and gap.min() == pytest.approx(float(golden[f'{key}/min_gap']), rel=1e-6), key


def test_the_parallel_case_sits_on_the_clamp(golden):
    base, other = golden['parallel/base'], golden['parallel/other']
    expected = np.arccos(1.0 - R.ANGLE_EPSILON)
    assert R.angle_between(base.mean(0), other.mean(0)) == expected
    value, grad_base, grad_other = R.angle_loss(base, other)
    assert value == expected ** 2 and not grad_base.any() and not grad_other.any()


def test_blocks_of_any_size_give_the_same_loss_and_gradients(golden):
    base, other = golden['33x130/base'], golden['33x130/other']
    whole = R.covariance_loss(base, other, block=130)
    for block in (1, 7, 64, 129):
        for got, expected in zip(R.covariance_loss(base, other, block=block), whole):
            assert relative(got, expected) <= 1e-13


def test_one_changed_column_leaves_every_other_entry_at_exactly_zero():
    rng = np.random.default_rng(0)
    base = rng.standard_normal((17, 70)).astype(np.float32)
    for k in (0, 31, 32, 69):
        other = base.copy()
        other[:, k] = rng.standard_normal(17).astype(np.float32)
        difference = R.corrcoef_rows(base, 0, 70) - R.corrcoef_rows(other, 0, 70)
        outside = np.delete(np.delete(difference, k, 0), k, 1)
        assert not outside.any()
        row = np.delete(difference[k], k)
        assert R.covariance_loss(base, other, gradients=False)[0] == pytest.approx(2.0 * np.abs(row).sum(), rel=1e-14)


def test_a_constant_column_gives_nan_and_a_duplicated_column_a_finite_value():
    rng = np.random.default_rng(1)
    base, other = rng.standard_normal((9, 12)), rng.standard_normal((9, 12))
    constant = base.copy()
    constant[:, 5] = 0.75
    value, grad_base, grad_other = R.covariance_loss(constant, other)
    assert np.isnan(value) and np.isnan(grad_base).all() and np.isnan(grad_other).all()
    duplicated = base.copy()
    duplicated[:, 7] = duplicated[:, 2]
    value, grad_base, grad_other = R.covariance_loss(duplicated, other)
    assert np.isfinite(value) and np.isfinite(grad_base).all() and np.isfinite(grad_other).all()
    assert R.covariance_loss(base, base)[0] == 0.0


# ---- the entry points -----------------------------------------------------------------------------------------------------
def test_the_library_advertises_and_binds_the_entry_points():
    from srgan_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_FEATURE_LOSSES\s+0x8000u', header)
    assert _lib.capabilities().features & 0x8000
    assert _lib.library().srgan_version() == 110
    for name in ('srgan_feature_corrcoef_l1_fwd', 'srgan_feature_corrcoef_l1_bwd', 'srgan_feature_corrcoef_l1_scratch_bytes'):
        assert name in _lib.SIGNATURES
    assert 'SRGAN_FEATURE_FEATURE_LOSSES' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_the_unary_op_codes_of_the_host_are_the_librarys():
    from srgan_amd import functional as F
    source = open(os.path.join(ROOT, 'sr-gan_amd', 'csrc', 'elementwise.hip')).read()
    names = re.search(r'enum UnaryOp \{(.*?)\}', source, flags=re.DOTALL).group(1).replace('= 0', '').split(',')
    names = [name.strip() for name in names]
    assert names.index('U_ACOS') == F.U_ACOS == 20 and names.index('U_CLAMP') == F.U_CLAMP == 21
    assert names.index('U_IN_RANGE') == F.U_IN_RANGE == 22 and names.index('U_COUNT') == 23


CAPACITY_SHAPES = ((5000, 10), (600, 4096), (600, 32768), (16, 32768), (8192, 128), (2, 2 ** 20))
BEYOND_CAPACITY = ((8193, 10), (2, 2 ** 20 + 1), (4096, 32768), (600, 2 ** 17))


def test_the_scratch_query_covers_the_applications_and_refuses_the_rest():
    from srgan_amd import _lib
    query = _lib.library().srgan_feature_corrcoef_l1_scratch_bytes
    for batch, features in CAPACITY_SHAPES:
        padded = -(-features // 128) * 128 * (-(-batch // 32) * 32)
        assert padded <= 2 ** 26
        bytes_ = query(batch, features)
        assert 2 * padded * 4 <= bytes_ <= 2 * padded * 4 + (1 << 24), (batch, features)      # the two copies and the partial sums
    for batch, features in BEYOND_CAPACITY:
        assert query(batch, features) == _lib.ERANGE, (batch, features)
        message = _lib.library().srgan_last_error().decode()
        assert f'({batch}, {features})' in message and 'capacity' in message
    assert query(1, 10) == _lib.EINVAL and query(5, 0) == _lib.EINVAL and query(-3, 10) == _lib.EINVAL


def test_argument_errors_are_reported_before_any_device_work():
    from srgan_amd import _lib
    library = _lib.library()
    forward = dict(base=PTR, other=PTR, loss=PTR, saved=PTR, scratch=PTR, B=5, F=7)
    backward = dict(base=PTR, other=PTR, saved=PTR, scratch=PTR, g=PTR, grad_base=PTR, grad_other=PTR, B=5, F=7)

    def call_forward(**changes):
        a = dict(forward, **changes)
        return library.srgan_feature_corrcoef_l1_fwd(a['base'], a['other'], a['loss'], a['saved'], a['scratch'], a['B'], a['F'], None)

    def call_backward(**changes):
        a = dict(backward, **changes)
        return library.srgan_feature_corrcoef_l1_bwd(a['base'], a['other'], a['saved'], a['scratch'], a['g'], a['grad_base'],
                                                     a['grad_other'], a['B'], a['F'], None)
    for name in ('base', 'other', 'loss', 'saved', 'scratch'):
        assert call_forward(**{name: None}) == _lib.EINVAL, name
    for name in ('base', 'other', 'saved', 'scratch', 'g'):
        assert call_backward(**{name: None}) == _lib.EINVAL, name
    for call in (call_forward, call_backward):
        assert call(scratch=PTR + 4) == _lib.EINVAL                                            # a misaligned scratch
        assert call(B=1) == _lib.EINVAL and call(B=0) == _lib.EINVAL and call(F=0) == _lib.EINVAL
        for batch, features in BEYOND_CAPACITY:
            assert call(B=batch, F=features) == _lib.ERANGE
            assert f'({batch}, {features})' in library.srgan_last_error().decode()


# ---- the settings ---------------------------------------------------------------------------------------------------------
def test_the_settings_are_optional_and_outside_the_defaults():
    from srgan_amd import settings, srgan
    assert [name for name, _ in settings.DEFAULTS] == list(vars(settings.Settings()))          # a run that never sets them
    for name in srgan.FEATURE_LOSS_SETTINGS:
        assert name not in dict(settings.DEFAULTS) and not hasattr(settings.Settings(), name)
    assert srgan.FEATURE_LOSS_SETTINGS == ('matching_feature_loss', 'contrasting_feature_loss')


def stand_in_experiment(**hooks):
    """What Experiment.feature_distance_loss reads, with the legacy path's first call recording that it was reached."""
    from srgan_amd import srgan, settings as S
    settings = S.Settings()
    for name, hook in hooks.items():
        setattr(settings, name, hook)
    reached = []

    def batch_mean_of_features(features, rank_specific_use=False):
        reached.append(features)
        raise LookupError('the legacy path')
    experiment = SimpleNamespace(settings=settings, batch_mean_of_features=batch_mean_of_features, parallel=False)
    return (lambda *arguments, **keywords: srgan.Experiment.feature_distance_loss(experiment, *arguments, **keywords)), reached, settings


def test_without_the_settings_every_call_takes_the_legacy_path():
    for hooks in ({}, dict(matching_feature_loss=None, contrasting_feature_loss=None)):
        loss, reached, settings = stand_in_experiment(**hooks)
        for keywords in ({}, dict(distance_function=settings.contrasting_distance_function), dict(distance_function=abs)):
            with pytest.raises(LookupError):
                loss('base', 'other', **keywords)
        assert reached == ['base'] * 3


def test_each_setting_replaces_its_own_calls_only():
    loss, reached, settings = stand_in_experiment(matching_feature_loss=lambda base, other: ('matching', base, other))
    assert loss('b', 'o') == ('matching', 'b', 'o') and not reached
    with pytest.raises(LookupError):
        loss('b', 'o', distance_function=settings.contrasting_distance_function)
    loss, reached, settings = stand_in_experiment(contrasting_feature_loss=lambda base, other: ('contrasting', base, other))
    assert loss('b', 'o', distance_function=settings.contrasting_distance_function) == ('contrasting', 'b', 'o') and not reached
    with pytest.raises(LookupError):
        loss('b', 'o')
    with pytest.raises(LookupError):
        loss('b', 'o', distance_function=abs)                                                  # any other distance: the legacy path


def test_the_public_names_and_defaults_are_the_references():
    import inspect
    from srgan_amd import srgan, utility
    for name in ('unit_vector', 'angle_between', 'square', 'feature_distance_loss_unmeaned', 'feature_distance_loss_both_unmeaned',
                 'feature_angle_loss', 'feature_corrcoef', 'corrcoef', 'feature_covariance_loss'):
        assert callable(getattr(srgan, name)), name
    signature = inspect.signature
    assert list(signature(srgan.feature_angle_loss).parameters) == ['base_features', 'other_features', 'target', 'summary_writer']
    assert signature(srgan.feature_angle_loss).parameters['target'].default == 0
    assert signature(srgan.feature_distance_loss_unmeaned).parameters['distance_function'].default is srgan.square
    assert signature(srgan.feature_distance_loss_both_unmeaned).parameters['distance_function'].default is utility.norm_squared
    assert list(signature(srgan.angle_between).parameters) == ['vector0', 'vector1']
    assert list(signature(srgan.feature_covariance_loss).parameters) == ['base_features', 'other_features']


@pytest.mark.parametrize('name', ['matching_feature_loss', 'contrasting_feature_loss'])
def test_gpu_mode_refuses_the_settings_under_data_parallelism(name):
    from srgan_amd import srgan, settings as S
    settings = S.Settings()
    setattr(settings, name, srgan.feature_covariance_loss)
    experiment = SimpleNamespace(settings=settings, dp=SimpleNamespace(world_size=2, rank=0, active=True))
    with pytest.raises(NotImplementedError, match='one device only'):
        srgan.Experiment.refuse_feature_loss_hooks_under_data_parallelism(experiment)
    experiment.dp.world_size = 1
    srgan.Experiment.refuse_feature_loss_hooks_under_data_parallelism(experiment)              # one rank: nothing to refuse
    setattr(settings, name, None)
    experiment.dp.world_size = 2
    srgan.Experiment.refuse_feature_loss_hooks_under_data_parallelism(experiment)              # None is "not set"
