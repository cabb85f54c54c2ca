"""Device random draws (settings.device_random_draws; csrc/random_draws.hip), the parts that need no GPU: the tests' NumPy
reference of the stream is pinned to the published Philox4x32-10 known answers and produces the distributions it claims;
the library advertises and binds the two entry points and refuses bad arguments before any device work; the data-parallel
windows tile the global tensor; the setting defaults to off and, off, leaves the device state alone."""
import os
import re

import numpy as np
import pytest
from scipy import stats

import device_draws_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 16      # a non-NULL "pointer" that is never dereferenced: argument errors come first
TRIPLES = ((0, 0, 0), (5, 7, 1), (2 ** 40 + 3, 123456, 2))      # (seed, iteration, draw)
COUNT = 2 ** 18


def _words(text):
    return [int(word, 16) for word in text.split()]


@pytest.mark.parametrize('counter, key, output', [
    ('00000000 00000000 00000000 00000000', '00000000 00000000', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_the_reference_reproduces_the_published_known_answers(counter, key, output):
    assert R.philox4x32_10(_words(counter), _words(key)).tolist() == _words(output)


def test_the_element_mapping_across_the_32_bit_block_word():
    """Kind 0, seed 5, iteration 7, draw 1, elements 2^34 - 2 .. 2^34 + 1: blocks 2^32 - 1 and 2^32, so the high counter word
    is used; element e owns word e & 3 of block e >> 2."""
    values = R.expected(0, 5, 7, 1, 2 ** 34 - 2, 4)
    np.testing.assert_allclose(values, [0.86082083, 0.48128009, 0.46896261, 0.17401564], rtol=0, atol=1e-8)
    assert np.array_equal(values * 2 ** 24, np.round(values * 2 ** 24))              # multiples of 2^-24
    low = R.philox4x32_10([2 ** 32 - 1, 0, 1, 7], [5, 0])
    high = R.philox4x32_10([0, 1, 1, 7], [5, 0])
    assert R.own_words(5, 7, 1, 2 ** 34 - 2, 4).tolist() == [low[2], low[3], high[0], high[1]]
    # a window of a draw is the slice of the draw from 0, whatever its alignment
    whole = R.expected(1, 5, 7, 1, 0, 64, offset=0.5)
    for first, n in ((0, 1), (1, 3), (2, 4), (3, 5), (7, 50)):
        assert np.array_equal(R.expected(1, 5, 7, 1, first, n, offset=0.5), whole[first:first + n])


@pytest.mark.parametrize('seed, iteration, draw', TRIPLES)
def test_the_construction_has_the_distributions_it_claims(seed, iteration, draw):
    """Evaluated by the reference alone (deterministic): Kolmogorov-Smirnov against N(0, 1), the two-Gaussian mixture and
    U[0, 1); first two moments; the mixture's sign is independent of the normal part; no lag-1 correlation."""
    normal = R.expected(1, seed, iteration, draw, 0, COUNT)
    mixture = R.expected(1, seed, iteration, draw, 0, COUNT, offset=2.0)
    uniform = R.expected(0, seed, iteration, draw, 0, COUNT)
    sign = R.signs(seed, iteration, draw, 0, COUNT)
    assert stats.kstest(normal, 'norm').pvalue > 0.01
    assert stats.kstest(mixture, lambda x: 0.5 * (stats.norm.cdf(x + 2.0) + stats.norm.cdf(x - 2.0))).pvalue > 0.01
    assert stats.kstest(uniform, 'uniform').pvalue > 0.01
    assert uniform.min() >= 0.0 and uniform.max() < 1.0 and np.isfinite(normal).all()
    assert abs(normal.mean()) < 0.01 and abs(normal.var() - 1.0) < 0.01
    np.testing.assert_allclose(mixture - normal, 2.0 * sign, rtol=0, atol=1e-12)
    assert abs(sign.mean()) < 0.01                                                    # equal weights
    assert abs(np.corrcoef(sign, normal)[0, 1]) < 0.01
    assert abs(np.corrcoef(normal[:-1], normal[1:])[0, 1]) < 0.01


def test_the_library_advertises_and_binds_the_entry_points():
    from srgan_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_DEVICE_DRAWS\s+0x400u', header)
    assert _lib.capabilities().features & 0x400
    assert _lib.library().srgan_version() == 110
    assert 'srgan_random_fill' in _lib.SIGNATURES and 'srgan_random_advance' in _lib.SIGNATURES


def test_argument_errors_are_reported_before_any_device_work():
    from srgan_amd import _lib
    library = _lib.library()
    fill = library.srgan_random_fill
    assert fill(None, 4, 0, 0, 0.0, 0, PTR, None) == _lib.EINVAL                    # NULL out
    assert fill(PTR, 4, 0, 0, 0.0, 0, None, None) == _lib.EINVAL                    # NULL state
    assert fill(PTR, -1, 0, 0, 0.0, 0, PTR, None) == _lib.EINVAL                    # n < 0
    assert fill(PTR, 4, -1, 0, 0.0, 0, PTR, None) == _lib.EINVAL                    # first < 0
    for kind in (-1, 2, 7):
        assert fill(PTR, 4, 0, kind, 0.0, 0, PTR, None) == _lib.EINVAL, kind        # kind outside {0, 1}
    assert fill(PTR, 4, 0, 1, 0.0, -1, PTR, None) == _lib.EINVAL                    # draw < 0
    for offset in (float('nan'), float('inf'), -float('inf')):
        assert fill(PTR, 4, 0, 1, offset, 0, PTR, None) == _lib.EINVAL, offset      # a non-finite offset
    limit = _lib.capabilities().max_tensor_elements
    assert fill(PTR, limit + 1, 0, 0, 0.0, 0, PTR, None) == _lib.EINVAL             # n above max_tensor_elements
    assert fill(PTR, 2 ** 40, 0, 0, 0.0, 0, PTR, None) == _lib.EINVAL
    assert fill(PTR, 4, 2 ** 63 - 2, 0, 0.0, 0, PTR, None) == _lib.EINVAL           # first + n beyond 64 bits
    assert library.srgan_random_advance(None, None) == _lib.EINVAL
    for kind in (0, 1):
        assert fill(PTR, 0, 0, kind, 0.5, 2, PTR, None) == 0                        # n == 0: a successful no-op
        assert fill(PTR, 0, 2 ** 40 + 1, kind, 0.0, 0, PTR, None) == 0


def test_the_ranks_windows_tile_the_global_tensor():
    from srgan_amd.srgan import device_draw_window
    columns, global_rows = 10, 6
    for world_size in (1, 2, 3):
        covered = []
        for rank in range(world_size):
            rows, first = device_draw_window(global_rows, columns, world_size, rank)
            assert rows == global_rows // world_size and first == rank * rows * columns
            covered.extend(range(first, first + rows * columns))
        assert covered == list(range(global_rows * columns)), world_size             # no gap, no overlap, in rank order
    assert device_draw_window(4, 10) == (4, 0)
    assert device_draw_window(8, 1, 2, 1) == (4, 4)                                   # alpha: one value per example
    with pytest.raises(ValueError):
        device_draw_window(7, 10, 2, 0)
    with pytest.raises(ValueError):
        device_draw_window(6, 10, 2, 2)


def test_the_setting_defaults_to_off_and_is_not_a_declared_default():
    from srgan_amd import settings
    default = settings.Settings()
    assert not hasattr(default, 'device_random_draws') and not hasattr(default, 'device_random_seed')
    assert not {'device_random_draws', 'device_random_seed'} & set(dict(settings.DEFAULTS))


def test_with_the_setting_off_the_device_state_is_never_touched(monkeypatch):
    """The three ``sample_*`` methods hand the host draws on (``as_var`` is replaced: there is no device here) and neither
    create the state nor call the fill."""
    import torch
    from srgan_amd import srgan, functional as F
    from srgan_amd.settings import Settings
    from srgan_amd.coefficient.models import Generator

    class _Experiment(srgan.Experiment):
        def dataset_setup(self):
            pass

        def model_setup(self):
            self.G = Generator(10)

        def validation_summaries(self, step):
            pass

    def refuse(*arguments, **keywords):
        raise AssertionError('the device draws were used')
    monkeypatch.setattr(F, 'random_fill', refuse)
    monkeypatch.setattr(F, 'random_advance', refuse)
    monkeypatch.setattr(srgan.Experiment, 'device_draw_state', refuse)
    monkeypatch.setattr(srgan, 'as_var', lambda value, staged=False: value)
    experiment = _Experiment(Settings())
    experiment.model_setup()
    assert experiment.device_random_draws() is False and experiment._draw_state is None
    assert tuple(experiment.sample_discriminator_noise(4).shape) == (4, 10)
    assert tuple(experiment.sample_interpolation_alpha(4).shape) == (4,)
    assert tuple(experiment.sample_generator_noise(4).shape) == (4, 10)
    injected = torch.ones(4, 10)
    experiment.settings.device_random_draws = True                                   # an injected draw wins, setting on
    experiment.injected_draws = {'z_d': injected, 'z_g': None, 'alpha': None}
    assert experiment.sample_discriminator_noise(4) is injected
    assert experiment._draw_state is None
