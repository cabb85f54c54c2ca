"""The frozen norm of the DCGAN discriminators on blocked tensors, the parts that need no GPU: the library advertises and binds
``srgan_h_frozen_norm_bwd`` and the entry point refuses bad arguments before any device work; the opt-in setting defaults to
off and reaches D and DNN; ``Discriminator(blocked_frozen_norm=True)`` changes which path the forward takes, not the module
tree."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 16      # a non-NULL "pointer" that is never dereferenced: argument errors come first


def test_the_library_advertises_and_binds_the_entry_point():
    from srgan_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_BLOCKED_FROZEN_NORM\s+0x200u', header)
    assert _lib.capabilities().features & 0x200
    assert _lib.library().srgan_version() == 110
    assert 'srgan_h_frozen_norm_bwd' in _lib.SIGNATURES


def _call(library, dtype, s=PTR, x=PTR, mean=PTR, inv_std=PTR, gamma=PTR, ref=None, gx=PTR, g_gamma=PTR, g_beta=PTR, n=2, c=3, hw=4):
    return library.srgan_h_frozen_norm_bwd(s, x, mean, inv_std, gamma, ref, 0.25, gx, g_gamma, g_beta, n, c, hw, dtype, None)


def test_argument_errors_are_reported_before_any_device_work():
    from srgan_amd import _lib
    library = _lib.library()
    for dtype in (-1, 3, 7):                                                        # unknown dtype, whatever else is passed
        assert _call(library, dtype) == _lib.EINVAL, dtype
        assert _call(library, dtype, gx=None, g_gamma=None) == _lib.EINVAL, dtype
    for dtype in (0, 1, 2):
        for required in ('s', 'inv_std', 'gamma'):                                  # a NULL required pointer
            assert _call(library, dtype, **{required: None}) == _lib.EINVAL, (dtype, required)
            assert b'srgan_h_frozen_norm_bwd' in library.srgan_last_error()
        assert _call(library, dtype, gx=None, g_gamma=None, g_beta=None) == _lib.EINVAL, dtype       # nothing to compute
        assert _call(library, dtype, x=None) == _lib.EINVAL, dtype                                   # g_gamma without x
        assert _call(library, dtype, x=None, gx=None, g_beta=None) == _lib.EINVAL, dtype
        for n, c, hw in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (-1, 3, 4)):                               # empty / negative extents
            assert _call(library, dtype, n=n, c=c, hw=hw) == _lib.EINVAL, (dtype, n, c, hw)
        # above max_tensor_elements = 2^31 - 1 (the product is formed without overflow)
        limit = _lib.capabilities().max_tensor_elements
        assert limit == 2 ** 31 - 1
        for n, c, hw in ((1, 1, 2 ** 31), (2, 4, 2 ** 28), (2 ** 15, 2 ** 15, 2), (1, 3, 2 ** 40), (2 ** 30, 2 ** 30, 2 ** 62)):
            assert n * c * hw > limit
            assert _call(library, dtype, n=n, c=c, hw=hw) == _lib.ERANGE, (dtype, n, c, hw)
            assert b'2^31' in library.srgan_last_error()
        assert _call(library, dtype, s=None, n=1, c=1, hw=2 ** 31) == _lib.EINVAL, dtype             # EINVAL comes before ERANGE


def test_the_setting_defaults_to_off_and_is_not_a_declared_default():
    from srgan_amd import settings
    assert getattr(settings.Settings(), 'blocked_frozen_norm', False) is False
    assert 'blocked_frozen_norm' not in dict(settings.DEFAULTS)


def test_the_flag_leaves_the_state_dict_alone():
    import torch
    from srgan_amd.age.models import Discriminator
    plain = Discriminator(32, 8, batch_norm=True).state_dict()
    flagged = Discriminator(32, 8, batch_norm=True, blocked_frozen_norm=True).state_dict()
    assert list(plain) == list(flagged) and any('running_var' in key for key in plain)
    assert all(plain[key].shape == flagged[key].shape and torch.equal(plain[key], flagged[key]) for key in plain)
    modules = lambda network: [(name, type(module)) for name, module in network.named_modules()]
    assert modules(Discriminator(32, 8, batch_norm=True)) == modules(Discriminator(32, 8, batch_norm=True, blocked_frozen_norm=True))


def test_the_flag_opens_the_blocked_path_for_a_discriminator_with_frozen_norms_only():
    from srgan_amd import nn
    from srgan_amd.age.models import Generator, Discriminator, _blocked_stack_ok
    assert _blocked_stack_ok(Discriminator(32, 8))                                                   # no norms: as before
    assert _blocked_stack_ok(Discriminator(32, 8, blocked_frozen_norm=True))
    assert not _blocked_stack_ok(Discriminator(32, 8, batch_norm=True))
    flagged = Discriminator(32, 8, batch_norm=True, blocked_frozen_norm=True)
    assert flagged.blocked_frozen_norm is True and _blocked_stack_ok(flagged)
    # exactly the frozen class: a norm with batch statistics behind a convolution has no such path
    flagged.layer3[1] = nn.BatchStatNorm2d(flagged.layer3[0].out_channels)
    assert not _blocked_stack_ok(flagged)
    # the flag is the discriminator's: on a generator with norms it opens nothing
    generator = Generator(image_size=32, conv_dim=8, batch_norm=True)
    generator.blocked_frozen_norm = True
    assert not _blocked_stack_ok(generator)


def test_model_setups_hand_the_setting_over():
    from srgan_amd.settings import Settings
    from srgan_amd.age.srgan import AgeExperiment
    from srgan_amd.age.sgan import AgeSganExperiment
    from srgan_amd.driving.srgan import DrivingExperiment
    for experiment_class in (AgeExperiment, AgeSganExperiment, DrivingExperiment):
        for wanted in (False, True):
            settings = Settings()
            settings.discriminator_batch_norm = True
            if wanted:
                settings.blocked_frozen_norm = True
            experiment = experiment_class(settings)
            experiment.image_size = 32
            experiment.model_setup()
            for network in (experiment.D, experiment.DNN):
                assert network.blocked_frozen_norm is wanted, (experiment_class.__name__, wanted)
                assert len(network.layer2) == 2
            assert not hasattr(experiment.G, 'blocked_frozen_norm')
