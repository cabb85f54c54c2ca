"""The DCGAN networks' ``batch_norm`` switch on the CPU (no GPU): with it on, the generator has the reference's modules,
``state_dict`` keys and initial tensors (golden g16, generated from the unmodified reference with its switch forced on,
tests/golden/make_batch_norm_goldens.py); with it off nothing changed; and the fixture's running statistics are what plain
torch batch-norm computes, so the fixture is pinned without the reference."""
import numpy as np
import torch

from helpers import load_golden, golden_state, assert_close

LEAK = 0.05


def test_generator_with_the_switch_on_has_the_reference_keys_and_initial_tensors():
    from srgan_amd import nn
    from srgan_amd.age.models import Generator
    expected = golden_state(load_golden('g16_tiny_dcgan_batch_norm'), 'init/G')
    generator = Generator(image_size=32, conv_dim=8, batch_norm=True)
    state = generator.state_dict()
    assert list(state) == list(expected)
    assert any(key.endswith('1.running_var') for key in state) and 'layer4.1.weight' not in state and 'fc.1.weight' not in state
    for key, value in expected.items():
        assert tuple(state[key].shape) == tuple(value.shape) and state[key].dtype == value.dtype, key
        assert torch.equal(state[key], value), key      # same seed_all(0) construction order; batch-norm init draws nothing
    norms = [module for module in generator.modules() if isinstance(module, torch.nn.BatchNorm2d)]
    assert len(norms) == 3 and all(isinstance(module, nn.BatchStatNorm2d) for module in norms)


def test_discriminator_with_the_switch_on_has_frozen_norms_and_the_reference_keys():
    from srgan_amd import nn
    from srgan_amd.age.models import Discriminator
    g = load_golden('g16_tiny_dcgan_batch_norm')
    discriminator = Discriminator(image_size=32, conv_dim=8, batch_norm=True)
    assert list(discriminator.state_dict()) == list(golden_state(g, 'init/D'))
    for key, value in golden_state(g, 'init/DNN').items():       # (init/D is this times the fixture's d_scale)
        assert torch.equal(discriminator.state_dict()[key], value), key
    norms = [module for module in discriminator.modules() if isinstance(module, torch.nn.BatchNorm2d)]
    assert len(norms) == 3 and not any(isinstance(module, nn.BatchStatNorm2d) for module in norms)


def test_default_arguments_build_the_networks_without_norm_layers():
    from srgan_amd.age import models
    from srgan_amd.crowd.models import DCGenerator
    from srgan_amd.settings import Settings
    g5 = load_golden('g5_tiny_dcgan')
    assert list(models.Generator(image_size=32, conv_dim=8).state_dict()) == list(golden_state(g5, 'init/G'))
    assert list(models.Discriminator(image_size=32, conv_dim=8).state_dict()) == list(golden_state(g5, 'init/D'))
    assert not any('running_mean' in key for key in DCGenerator(image_size=32, conv_dim=8).state_dict())
    assert Settings().generator_batch_norm is False and Settings().discriminator_batch_norm is False


def test_the_module_level_switch_is_read_when_a_network_is_built(monkeypatch):
    from srgan_amd.age import models
    from srgan_amd.crowd.models import DCGenerator
    monkeypatch.setattr(models, 'batch_norm', True)
    expected = list(golden_state(load_golden('g16_tiny_dcgan_batch_norm'), 'init/G'))
    assert list(models.Generator(image_size=32, conv_dim=8).state_dict()) == expected
    assert list(DCGenerator(image_size=32, conv_dim=8).state_dict()) == expected
    assert list(models.Generator(image_size=32, conv_dim=8, batch_norm=False).state_dict()) == \
        [key for key in expected if '.1.' not in key]


def test_model_setups_pass_the_settings_through():
    from srgan_amd import nn
    from srgan_amd.settings import Settings
    from srgan_amd.driving.srgan import DrivingExperiment
    settings = Settings()
    settings.generator_batch_norm, settings.discriminator_batch_norm = True, True
    experiment = DrivingExperiment(settings)
    experiment.image_size = 32
    experiment.model_setup()
    assert sum(isinstance(m, nn.BatchStatNorm2d) for m in experiment.G.modules()) == 3
    for network in (experiment.D, experiment.DNN):
        assert sum(type(m) is nn.BatchNorm2d for m in network.modules()) == 3


def test_data_parallel_ranks_refuse_a_generator_with_batch_statistics():
    import pytest
    from types import SimpleNamespace
    from srgan_amd.settings import Settings
    from srgan_amd.driving.srgan import DrivingExperiment
    settings = Settings()
    settings.generator_batch_norm = True
    experiment = DrivingExperiment(settings)
    experiment.image_size = 32
    experiment.model_setup()
    experiment.dp = SimpleNamespace(world_size=2, active=True)
    with pytest.raises(NotImplementedError, match='synchronised'):
        experiment.gpu_mode()


def test_the_fixtures_running_statistics_are_plain_torch_batch_norm():
    """G's buffers after the first step = two training-mode forwards (z_d under no_grad, then z_g; reference srgan.py:290,302)
    through plain torch layers holding ``init/G`` -- the generator is updated only at the end of the step."""
    g = load_golden('g16_tiny_dcgan_batch_norm')
    state = golden_state(g, 'init/G')
    buffers = {key: value.clone() for key, value in state.items() if 'running' in key or 'tracked' in key}

    def forward(z):
        functional = torch.nn.functional
        out = functional.conv_transpose2d(z.view(z.shape[0], -1, 1, 1), state['fc.0.weight'], state['fc.0.bias'])
        for index in (1, 2, 3):
            prefix = f'layer{index}'
            out = functional.conv_transpose2d(out, state[f'{prefix}.0.weight'], state[f'{prefix}.0.bias'], stride=2, padding=1)
            out = functional.batch_norm(out, buffers[f'{prefix}.1.running_mean'], buffers[f'{prefix}.1.running_var'],
                                        state[f'{prefix}.1.weight'], state[f'{prefix}.1.bias'], training=True, momentum=0.1,
                                        eps=1e-5)
            buffers[f'{prefix}.1.num_batches_tracked'] += 1
            out = functional.leaky_relu(out, LEAK)
        return out

    with torch.no_grad():
        forward(torch.from_numpy(g['s0/z_d']))
        forward(torch.from_numpy(g['s0/z_g']))
    assert len(buffers) == 9
    for key, value in buffers.items():
        recorded = g[f's0/G_buffers/{key}']
        if 'tracked' in key:
            assert int(recorded) == int(value) == 2
        else:
            assert_close(value.numpy(), recorded, rtol=1e-5, atol=1e-7, what=key)
            assert np.abs(recorded - (0.0 if 'mean' in key else 1.0)).max() > 1e-3, f'{key} did not move'


def test_the_library_advertises_the_entry_points():
    import re
    import os
    from srgan_amd import _lib
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'srgan_hip.h')
    assert re.search(r'#define\s+SRGAN_FEATURE_BATCH_NORM_TRAIN\s+0x80u', open(header).read())
    assert _lib.capabilities().features & 0x80
    assert _lib.library().srgan_version() == 110
    for name in ('stats', 'fwd', 'bwd_reduce', 'bwd_apply'):
        assert f'srgan_batch_norm_train_{name}' in _lib.SIGNATURES
    # argument errors are reported before any device work: one value per channel, a missing tensor
    assert _lib.library().srgan_batch_norm_train_stats(16, 16, 16, None, None, None, 0.1, 1e-5, 1, 3, 1, None) == _lib.EINVAL
    assert _lib.library().srgan_batch_norm_train_fwd(None, 16, 16, 16, 16, 1.0, 16, 2, 3, 4, None) == _lib.EINVAL
    # the partial counts are fp32: more than 2^24 values per channel are refused, not summed inexactly
    assert _lib.library().srgan_batch_norm_train_stats(16, 16, 16, None, None, None, 0.1, 1e-5, 2, 3, 2 ** 24, None) == _lib.ERANGE
