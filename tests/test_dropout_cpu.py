"""Dropout with masks regenerated on the device (settings.drop_rate; csrc/dropout.hip), the parts that need no GPU: the
tests' NumPy restatement of ``srgan_dropout`` (built on the device draws' reference stream, device_draws_reference.py) keeps
the fraction it claims and is window-consistent; the library advertises and binds the entry point and refuses bad arguments
before any device work; the dense layers construct with ``drop_rate > 0``; the draw ids, the call counter, eval mode and the
data-parallel refusal, all on the host."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import device_draws_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 16      # a non-NULL "pointer" that is never dereferenced: argument errors come first
SEED, ITERATION, DRAW = 2 ** 40 + 3, 123456, 0x10000


def dropout_mask(n, p, seed, iteration, draw, first=0):
    """bool [n]: element e is kept when element ``first + e`` of the uniform draw is >= p (p as the fp32 the kernel gets)."""
    return R.expected(0, seed, iteration, draw, first, n) >= np.float64(np.float32(p))


def dropout_scale(p):
    """fp32 ``1.0f / (1.0f - p)`` as the host launcher computes it (inf at p == 1, where nothing is kept)."""
    with np.errstate(divide='ignore'):
        return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_reference(x, p, seed, iteration, draw, first=0):
    """``srgan_dropout`` on the contiguous fp32 array ``x`` (any shape, elements in C order): kept elements are the fp32
    product x * scale rounded once, dropped ones +0.0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.size == 0:
        return x.copy()
    keep = dropout_mask(x.size, p, seed, iteration, draw, first).reshape(x.shape)
    with np.errstate(invalid='ignore', over='ignore'):
        scaled = (x * dropout_scale(p)).astype(np.float32)
    return np.where(keep, scaled, np.float32(0.0)).astype(np.float32)


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
def test_the_kept_fraction_is_within_five_binomial_standard_deviations(p):
    n = 65536
    kept = dropout_mask(n, p, SEED, ITERATION, DRAW).mean()
    assert abs(kept - (1.0 - p)) <= 5.0 * np.sqrt(p * (1.0 - p) / n), (p, kept)


def test_p_zero_keeps_every_element_and_p_one_none():
    x = np.random.default_rng(0).standard_normal(4099).astype(np.float32)
    assert dropout_mask(4099, 0.0, SEED, ITERATION, DRAW).all()
    assert np.array_equal(dropout_reference(x, 0.0, SEED, ITERATION, DRAW), x)                 # a copy
    assert not dropout_mask(4099, 1.0, SEED, ITERATION, DRAW).any()                            # the uniforms are < 1
    out = dropout_reference(x, 1.0, SEED, ITERATION, DRAW)
    assert np.array_equal(out, np.zeros_like(x)) and not np.signbit(out).any()


def test_kept_elements_are_scaled_once_and_dropped_ones_are_positive_zero():
    x = np.array([1.0, -0.0, np.inf, -np.inf, 1e-45, 3.0, -7.5, np.nan] * 16, dtype=np.float32)
    out = dropout_reference(x, 0.25, SEED, ITERATION, DRAW)
    keep = dropout_mask(x.size, 0.25, SEED, ITERATION, DRAW)
    assert keep.any() and not keep.all()
    assert dropout_scale(0.25) == np.float32(4.0) / np.float32(3.0)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(out[keep], (x * dropout_scale(0.25))[keep], equal_nan=True)
    assert (out[~keep] == 0).all() and not np.signbit(out[~keep]).any()


def test_two_windows_of_a_draw_agree_with_the_whole_draw():
    x = np.random.default_rng(1).standard_normal(1027).astype(np.float32)
    whole = dropout_reference(x, 0.5, SEED, ITERATION, DRAW)
    for first, stop in ((0, 513), (513, 1027), (1, 4), (6, 1001)):
        assert np.array_equal(dropout_reference(x[first:stop], 0.5, SEED, ITERATION, DRAW, first), whole[first:stop])
    assert not np.array_equal(dropout_reference(x, 0.5, SEED, ITERATION, DRAW + 1), whole)     # another draw, another mask
    assert not np.array_equal(dropout_reference(x, 0.5, SEED, ITERATION + 1, DRAW), whole)     # another iteration


# ---- the entry point ------------------------------------------------------------------------------------------------------
def test_the_library_advertises_and_binds_the_entry_point():
    from srgan_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    assert re.search(r'#define\s+SRGAN_FEATURE_DROPOUT\s+0x4000u', header)
    assert _lib.capabilities().features & 0x4000
    assert _lib.library().srgan_version() == 110
    assert 'srgan_dropout' in _lib.SIGNATURES
    assert 'SRGAN_FEATURE_DROPOUT' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_the_draw_ranges_of_the_header_are_the_hosts():
    from srgan_amd import srgan
    header = open(os.path.join(ROOT, 'include', 'srgan_hip.h')).read()
    values = {name: int(re.search(r'#define\s+%s\s+(0x[0-9a-fA-F]+)' % name, header).group(1), 16)
              for name in ('SRGAN_DROPOUT_DRAWS_D', 'SRGAN_DROPOUT_DRAWS_DNN', 'SRGAN_DROPOUT_DRAW_RANGE')}
    assert (srgan.DROPOUT_DRAWS_D, srgan.DROPOUT_DRAWS_DNN, srgan.DROPOUT_DRAW_RANGE) == tuple(values.values())
    d = range(srgan.DROPOUT_DRAWS_D, srgan.DROPOUT_DRAWS_D + srgan.DROPOUT_DRAW_RANGE)
    dnn = range(srgan.DROPOUT_DRAWS_DNN, srgan.DROPOUT_DRAWS_DNN + srgan.DROPOUT_DRAW_RANGE)
    assert not set(d) & set(dnn) and min(d.start, dnn.start) >= 3                              # disjoint, clear of 0, 1, 2
    taken = {srgan.DRAW_Z_D, srgan.DRAW_ALPHA, srgan.DRAW_Z_G, srgan.Experiment.SUMMARY_DRAW_STANDARD,
             srgan.Experiment.SUMMARY_DRAW_OFFSET}
    assert not taken & (set(d) | set(dnn))
    assert max(d.stop, dnn.stop) <= 2 ** 31                                                    # a draw id is an int32


def test_argument_errors_are_reported_before_any_device_work():
    from srgan_amd import _lib
    dropout = _lib.library().srgan_dropout
    good = dict(x=PTR, y=PTR, rows=3, row_elems=5, x_stride=5, y_stride=5, first=0, p=0.5, draw=3, state=PTR)

    def call(**changes):
        a = dict(good, **changes)
        return dropout(a['x'], a['y'], a['rows'], a['row_elems'], a['x_stride'], a['y_stride'], a['first'], a['p'], a['draw'],
                       a['state'], None)
    for name in ('x', 'y', 'state'):
        assert call(**{name: None}) == _lib.EINVAL, name                                       # NULL pointers
    for name in ('rows', 'row_elems', 'first'):
        assert call(**{name: -1}) == _lib.EINVAL, name                                         # negative sizes
    assert call(x_stride=4) == _lib.EINVAL and call(y_stride=4) == _lib.EINVAL                 # a stride below row_elems
    assert call(draw=-1) == _lib.EINVAL
    for p in (-0.001, 1.001, float('nan'), float('inf'), -float('inf')):
        assert call(p=p) == _lib.EINVAL, p
    limit = _lib.capabilities().max_tensor_elements
    assert call(rows=1, row_elems=limit + 1, x_stride=limit + 1, y_stride=limit + 1) == _lib.ERANGE
    assert call(rows=2 ** 16, row_elems=2 ** 15, x_stride=2 ** 15, y_stride=2 ** 15) == _lib.ERANGE       # 2^31 elements
    assert call(rows=2 ** 40, row_elems=2 ** 40, x_stride=2 ** 40, y_stride=2 ** 40) == _lib.ERANGE       # no 64-bit overflow
    assert call(first=2 ** 63 - 2) == _lib.EINVAL                                              # first + n beyond 64 bits
    for changes in (dict(rows=0), dict(row_elems=0, x_stride=0, y_stride=0), dict(rows=0, first=2 ** 40 + 1, p=1.0)):
        assert call(**changes) == 0, changes                                                   # zero elements: a successful no-op


# ---- layers, streams, settings --------------------------------------------------------------------------------------------
def test_a_dense_layer_with_a_drop_rate_constructs():
    from srgan_amd import nn
    from srgan_amd.crowd.models import _DenseLayer, _DenseBlock, KnnDenseNetCat
    layer = _DenseLayer(8, 4, 2, drop_rate=0.25)
    assert isinstance(layer.dropout, nn.Dropout) and layer.dropout.p == 0.25
    plain = _DenseLayer(8, 4, 2)
    assert not hasattr(plain, 'dropout') and not nn.active_dropout_layers(plain)
    assert list(layer.state_dict()) == list(plain.state_dict())                                # the checkpoint format is unchanged
    block = _DenseBlock(2, 8, 2, 4, drop_rate=0.25)
    assert len(nn.active_dropout_layers(block)) == 2
    network = KnnDenseNetCat(growth_rate=4, block_config=(1, 1, 2, 1), num_init_features=8, bn_size=2, drop_rate=0.2, image_size=64)
    assert len(nn.active_dropout_layers(network)) == 5
    assert all(layer.p == pytest.approx(0.2) for layer in nn.active_dropout_layers(network))
    with pytest.raises(ValueError):
        nn.Dropout(1.5)


def test_eval_mode_and_p_zero_return_the_input_object_and_launch_nothing(monkeypatch):
    from srgan_amd import nn, functional as F

    def refuse(*arguments, **keywords):
        raise AssertionError('a kernel was launched')
    monkeypatch.setattr(F, 'dropout', refuse)
    x = SimpleNamespace(meta=None)
    layer = nn.Dropout(0.5)
    layer.eval()
    assert layer(x) is x
    zero = nn.Dropout(0.0)
    zero.train()
    assert zero(x) is x
    layer.train()
    with pytest.raises(RuntimeError, match='dropout stream'):                                  # no stream attached
        layer(x)
    with pytest.raises(NotImplementedError, match='blocked'):
        layer(SimpleNamespace(meta=object()))


def test_the_stream_numbers_the_calls_of_a_step(monkeypatch):
    from srgan_amd import nn, functional as F
    stream = nn.DropoutStream(0x10000, seed=SEED, iteration=7, draws=16)                       # four sections of four ids
    stream._state = 'state'                                                                    # no device here
    seen = []
    monkeypatch.setattr(F, 'dropout', lambda x, p, draw, state, first=0: seen.append((p, draw, state)) or x)
    block = nn.Sequential(nn.Dropout(0.5), nn.Dropout(0.0), nn.Dropout(0.25))
    assert nn.attach_dropout_stream(block, stream) == 2
    block.train()
    x = SimpleNamespace(meta=None)
    stream.begin_step()
    block(x), block(x)
    assert seen == [(0.5, 0x10000, 'state'), (0.25, 0x10001, 'state'), (0.5, 0x10002, 'state'), (0.25, 0x10003, 'state')]
    with pytest.raises(RuntimeError, match='range'):                                           # the section is used up
        block(x)
    stream.begin_step()                                                                        # the next iteration: the same ids
    block.eval()
    block(x)                                                                                   # eval mode takes no id
    block.train()
    block(x)
    assert seen[-2:] == [(0.5, 0x10000, 'state'), (0.25, 0x10001, 'state')]


def test_a_section_numbers_its_calls_wherever_it_stands_in_the_program_order(monkeypatch):
    """The penalty chain's forward comes before the stacked pass with the penalty stream on and after it with the stream
    off: in a section of its own it takes the same ids either way, and so does the rest of the step."""
    from srgan_amd import nn, functional as F
    seen = []
    monkeypatch.setattr(F, 'dropout', lambda x, p, draw, state, first=0: seen.append(draw) or x)
    layer = nn.Dropout(0.5)
    layer.train()
    x = SimpleNamespace(meta=None)

    def step(section_first):
        stream = nn.DropoutStream(0x10000, draws=16)
        stream._state = 'state'
        nn.attach_dropout_stream(layer, stream)
        del seen[:]
        stream.begin_step()
        order = ('section', 'main') if section_first else ('main', 'section')
        taken = {}
        for part in order:
            before = len(seen)
            if part == 'section':
                with stream.section(1):
                    layer(x), layer(x)
            else:
                layer(x), layer(x), layer(x)
            taken[part] = seen[before:]
        with stream.section(1):                                                                # entered again: it goes on
            layer(x)
        with stream.section(2):
            layer(x)
        layer(x)
        return taken, seen[-3:]
    first, second = step(True), step(False)
    assert first == second
    assert first[0] == {'section': [0x10004, 0x10005], 'main': [0x10000, 0x10001, 0x10002]}
    assert first[1] == [0x10006, 0x10008, 0x10003]
    stream = nn.DropoutStream(0, draws=16)
    with pytest.raises(ValueError):
        with stream.section(0):
            pass
    with pytest.raises(ValueError):
        with stream.section(4):
            pass


def experiment_with(drop_rate=None, world_size=1):
    from srgan_amd.settings import Settings
    from srgan_amd.crowd.srgan import CrowdExperiment
    from srgan_amd.crowd.models import KnnDenseNetCat, DCGenerator

    class Small(CrowdExperiment):
        def model_setup(self):
            arguments = dict(growth_rate=4, block_config=(1, 1, 1, 1), num_init_features=8, bn_size=2, image_size=64,
                             drop_rate=self.dense_drop_rate())
            self.G = DCGenerator(image_size=64, conv_dim=8)
            self.D, self.DNN = KnnDenseNetCat(**arguments), KnnDenseNetCat(**arguments)
    settings = Settings()
    if drop_rate is not None:
        settings.drop_rate = drop_rate
    experiment = Small(settings)
    experiment.model_setup()
    if world_size > 1:
        experiment.dp = SimpleNamespace(world_size=world_size, rank=0, active=True)
    return experiment


def test_the_setting_defaults_to_zero_and_reaches_both_networks():
    from srgan_amd import nn, settings
    assert not hasattr(settings.Settings(), 'drop_rate') and 'drop_rate' not in dict(settings.DEFAULTS)
    off = experiment_with()
    assert off.dense_drop_rate() == 0.0
    assert not nn.active_dropout_layers(off.D) and not nn.active_dropout_layers(off.DNN)
    assert off.dropout_stream('D') is None and off.dropout_stream('DNN') is None               # nothing is created
    on = experiment_with(0.2)
    assert len(nn.active_dropout_layers(on.D)) == 4 and len(nn.active_dropout_layers(on.DNN)) == 4
    on.starting_step = 5
    d, dnn = on.dropout_stream('D'), on.dropout_stream('DNN')
    assert (d.base, dnn.base, d.iteration, dnn.iteration) == (0x10000, 0x20000, 5, 5)
    assert on.dropout_stream('D') is d and all(layer.dropout_stream is d for layer in nn.active_dropout_layers(on.D))
    assert on._draw_state is None                                                              # the draws' state is another one
    on.eval_mode()
    assert not any(layer.training for layer in nn.active_dropout_layers(on.D) + nn.active_dropout_layers(on.DNN))


@pytest.mark.parametrize('module_name, class_name, networks', [('srgan', 'CrowdExperiment', 2), ('dnn', 'CrowdDnnExperiment', 1),
                                                              ('dggan', 'CrowdDgganExperiment', 2)])
def test_the_crowd_model_setups_pass_the_setting_through(monkeypatch, module_name, class_name, networks):
    """The model_setup of each crowd experiment that builds the dense networks hands ``settings.drop_rate`` to them (the
    constructors are replaced by recorders: the full-size networks are not built here)."""
    import importlib
    from srgan_amd.settings import Settings
    module = importlib.import_module('srgan_amd.crowd.' + module_name)
    built = []

    class Recorder:
        def __init__(self, *arguments, **keywords):
            built.append(keywords.get('drop_rate'))
    for name in ('KnnDenseNetCat', 'KnnDenseNetCatDggan', 'DCGenerator'):
        if hasattr(module, name):
            monkeypatch.setattr(module, name, Recorder)
    for drop_rate, expected in ((0.3, 0.3), (None, 0.0)):
        settings = Settings()
        if drop_rate is not None:
            settings.drop_rate = drop_rate
        del built[:]
        getattr(module, class_name)(settings).model_setup()
        assert built.count(expected) == networks, (class_name, built)


def test_gpu_mode_refuses_dropout_under_data_parallelism():
    with pytest.raises(NotImplementedError, match='one device'):
        experiment_with(0.2, world_size=2).gpu_mode()
