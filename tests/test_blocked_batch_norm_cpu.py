"""Batch-statistics norm on blocked tensors, the parts that need no GPU: the library advertises and binds the four
``srgan_h_batch_norm_*`` entry points and they refuse bad arguments before any device work; the opt-in setting defaults to
off; and ``Generator(blocked_batch_norm=True)`` changes which path the forward takes, not the module tree."""
import re
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 16      # a non-NULL "pointer" that is never dereferenced: argument errors come first


def test_the_library_advertises_and_binds_the_entry_points():
    from srgan_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_BLOCKED_BATCH_NORM\s+0x100u', header)
    assert _lib.capabilities().features & 0x100
    assert _lib.library().srgan_version() == 110
    for name in ('stats', 'fwd', 'bwd_reduce', 'bwd_apply'):
        assert f'srgan_h_batch_norm_{name}' in _lib.SIGNATURES


def _calls(library, n, c, hw, dtype, missing=False):
    """The status of each of the four entry points for one shape and dtype (``missing``: the first required pointer NULL)."""
    x = None if missing else PTR
    return {
        'stats': library.srgan_h_batch_norm_stats(x, PTR, PTR, None, None, None, 0.1, 1e-5, n, c, hw, dtype, None),
        'fwd': library.srgan_h_batch_norm_fwd(x, PTR, PTR, PTR, PTR, 1.0, PTR, n, c, hw, dtype, None),
        'bwd_reduce': library.srgan_h_batch_norm_bwd_reduce(x, PTR, PTR, PTR, PTR, None, None, n, c, hw, dtype, None),
        'bwd_apply': library.srgan_h_batch_norm_bwd_apply(x, PTR, PTR, PTR, PTR, PTR, None, 1.0, PTR, n, c, hw, dtype, None),
    }


def test_argument_errors_are_reported_before_any_device_work():
    from srgan_amd import _lib
    library = _lib.library()
    for dtype in (0, 1, 2):
        assert set(_calls(library, 2, 3, 4, dtype, missing=True).values()) == {_lib.EINVAL}, dtype      # a NULL required pointer
        assert set(_calls(library, 1, 3, 1, dtype).values()) == {_lib.EINVAL}, dtype                    # one value per channel
        assert set(_calls(library, 2, 3, 2 ** 24, dtype).values()) == {_lib.ERANGE}, dtype              # 2^25 values per channel
        assert set(_calls(library, 1, 3, 2 ** 24 + 1, dtype).values()) == {_lib.ERANGE}, dtype
        assert set(_calls(library, 1, 3, 2 ** 40, dtype).values()) == {_lib.ERANGE}, dtype
    for dtype in (-1, 3, 7):
        assert set(_calls(library, 2, 3, 4, dtype).values()) == {_lib.EINVAL}, dtype                    # unknown dtype
    # every other required pointer, one at a time
    assert library.srgan_h_batch_norm_stats(PTR, None, PTR, None, None, None, 0.1, 1e-5, 2, 3, 4, 1, None) == _lib.EINVAL
    assert library.srgan_h_batch_norm_stats(PTR, PTR, None, None, None, None, 0.1, 1e-5, 2, 3, 4, 1, None) == _lib.EINVAL
    for position in range(6):                       # x, mean, inv_std, gamma, beta, y
        p = [PTR] * 6
        p[position] = None
        assert library.srgan_h_batch_norm_fwd(p[0], p[1], p[2], p[3], p[4], 1.0, p[5], 2, 3, 4, 2, None) == _lib.EINVAL, position
    for position in range(5):                       # s, x, mean, inv_std, sums
        p = [PTR] * 5
        p[position] = None
        assert library.srgan_h_batch_norm_bwd_reduce(*p, None, None, 2, 3, 4, 0, None) == _lib.EINVAL, position
    for position in range(7):                       # s, x, mean, inv_std, gamma, sums, gx
        p = [PTR] * 7
        p[position] = None
        assert library.srgan_h_batch_norm_bwd_apply(*p[:6], None, 1.0, p[6], 2, 3, 4, 0, None) == _lib.EINVAL, position


def test_the_setting_defaults_to_off_and_is_not_a_declared_default():
    from srgan_amd import settings
    assert getattr(settings.Settings(), 'blocked_batch_norm', False) is False
    assert 'blocked_batch_norm' not in dict(settings.DEFAULTS)


def test_the_flag_opens_the_blocked_path_for_a_generator_with_norms_only():
    from srgan_amd.age.models import Generator, Discriminator, _blocked_stack_ok
    from srgan_amd.crowd.models import DCGenerator
    assert _blocked_stack_ok(Generator(image_size=32, conv_dim=8))                                    # no norms: as before
    assert _blocked_stack_ok(Generator(image_size=32, conv_dim=8, blocked_batch_norm=True))
    assert not _blocked_stack_ok(Generator(image_size=32, conv_dim=8, batch_norm=True))
    assert _blocked_stack_ok(Generator(image_size=32, conv_dim=8, batch_norm=True, blocked_batch_norm=True))
    assert not _blocked_stack_ok(DCGenerator(image_size=32, conv_dim=8, batch_norm=True))
    assert _blocked_stack_ok(DCGenerator(image_size=32, conv_dim=8, batch_norm=True, blocked_batch_norm=True))
    # the discriminator's frozen norm has no blocked kernels, whatever is set on it
    with_norms = Discriminator(image_size=32, conv_dim=8, batch_norm=True)
    assert not _blocked_stack_ok(with_norms)
    with_norms.blocked_batch_norm = True
    assert not _blocked_stack_ok(with_norms)
    assert _blocked_stack_ok(Discriminator(image_size=32, conv_dim=8))


def test_the_flag_leaves_the_state_dict_alone():
    import torch
    from srgan_amd.age.models import Generator
    plain = Generator(image_size=32, conv_dim=8, batch_norm=True).state_dict()
    flagged = Generator(image_size=32, conv_dim=8, batch_norm=True, blocked_batch_norm=True).state_dict()
    assert list(plain) == list(flagged)
    assert all(torch.equal(plain[key], flagged[key]) for key in plain)


def test_model_setups_hand_the_setting_over():
    from srgan_amd.settings import Settings
    from srgan_amd.driving.srgan import DrivingExperiment
    for wanted in (False, True):
        settings = Settings()
        settings.generator_batch_norm = True
        if wanted:
            settings.blocked_batch_norm = True
        experiment = DrivingExperiment(settings)
        experiment.image_size = 32
        experiment.model_setup()
        assert experiment.G.blocked_batch_norm is wanted
        assert not hasattr(experiment.D, 'blocked_batch_norm')
