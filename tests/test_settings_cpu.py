"""The port's own settings (``settings.EXTENSIONS`` / ``settings.option``) and the state an ``Experiment`` declares: one
table that every reader goes through, checked against the package's source."""
import ast
import os
from types import SimpleNamespace

import pytest

# (name, default) of every setting that is not the reference's, as the readers have always defaulted them
EXPECTED = (
    ('step_graph', False), ('step_graph_warmup', 2), ('step_graph_collectives', None), ('reference_schedule', False),
    ('batched_discriminator', True), ('overlap_dnn_step', False), ('overlap_generator_forwards', False),
    ('overlap_gradient_penalty', False), ('overlap_gradient_exchange', True), ('wgrad_stream', None),
    ('compute_dtype', 'f32'), ('gradient_penalty_dtype', 'f32'), ('storage_dtype', None), ('blocked_fp32', False),
    ('blocked_batch_norm', False), ('blocked_frozen_norm', False), ('loss_scale', 1.0), ('gradient_wire_dtype', None),
    ('gradient_exchange_form', None), ('device_random_draws', False), ('device_random_seed', 0), ('drop_rate', 0),
    ('image_summaries', False), ('distribution_summaries', False), ('matching_feature_loss', None),
    ('contrasting_feature_loss', None), ('crowd_validation', None), ('crowd_validation_scenes', None),
    ('full_image_inference', 'host'),
)
DECLARED_STATE = ('_captured_iteration', '_single_compute_stream', '_graph_note', '_typed_commands', '_dnn_stream',
                  '_aux_stream', '_gp_stream', '_stack_too_large', '_draw_state', '_dropout_streams')


def same(value, expected):
    return type(value) is type(expected) and value == expected                  # (False is not 0, 1.0 is not 1)


def test_the_table_is_the_expected_one():
    from srgan_amd import settings
    names = [name for name, _, _ in settings.EXTENSIONS]
    assert len(set(names)) == len(names)
    assert not set(names) & set(dict(settings.DEFAULTS))
    assert sorted(names) == sorted(name for name, _ in EXPECTED)
    expected = dict(EXPECTED)
    for name, default, description in settings.EXTENSIONS:
        assert same(default, expected[name]), name
        assert isinstance(description, str) and description and '\n' not in description, name
    assert not set(names) & set(vars(settings.Settings()))                      # Settings() stays the reference's


def test_option():
    from srgan_amd import settings
    from srgan_amd.settings import option
    for bag in (settings.Settings(), SimpleNamespace()):
        before = dict(vars(bag))
        for name, default in EXPECTED:
            assert same(option(bag, name), default), name
        assert vars(bag) == before and not hasattr(bag, 'loss_scale')           # reading never writes
        bag.loss_scale, bag.batched_discriminator, bag.compute_dtype = 1024.0, None, None
        assert option(bag, 'loss_scale') == 1024.0
        assert option(bag, 'batched_discriminator') is None and option(bag, 'compute_dtype') is None   # set to None is None
        with pytest.raises(KeyError, match='los_scale'):
            option(bag, 'los_scale')
        with pytest.raises(KeyError, match='batch_size'):                       # the reference's are plain attributes
            option(bag, 'batch_size')
        assert set(vars(bag)) == set(before) | {'loss_scale', 'batched_discriminator', 'compute_dtype'}


def package_modules():
    import srgan_amd
    root = os.path.dirname(srgan_amd.__file__)
    for directory, _, files in os.walk(root):
        for file in sorted(files):
            if file.endswith('.py'):
                path = os.path.join(directory, file)
                with open(path) as handle:
                    yield os.path.relpath(path, root), ast.parse(handle.read(), path)


def called(node):
    """The name a call goes to: ``f(...)`` -> 'f', ``x.f(...)`` -> 'f'."""
    function = node.func
    return function.id if isinstance(function, ast.Name) else function.attr if isinstance(function, ast.Attribute) else None


def literal(node):
    return node.value if isinstance(node, ast.Constant) and isinstance(node.value, str) else None


def test_every_reader_goes_through_the_table():
    from srgan_amd import settings
    names = {name for name, _, _ in settings.EXTENSIONS}
    read, modules = set(), 0
    for module, tree in package_modules():
        modules += 1
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            where = f'{module}:{node.lineno}'
            if called(node) == 'getattr' and isinstance(node.func, ast.Name) and len(node.args) >= 2 and \
                    literal(node.args[1]) is not None:
                target = node.args[0]
                target_name = target.id if isinstance(target, ast.Name) else target.attr if isinstance(target, ast.Attribute) else ''
                assert not target_name.endswith('settings'), f'{where}: a setting read with getattr, not option()'
                if module == 'srgan.py' and target_name == 'self':
                    assert not literal(node.args[1]).startswith('_'), f'{where}: undeclared state read with getattr'
            for function, position in (('option', 1), ('_stream_setting', 0)):
                if called(node) == function and len(node.args) > position and literal(node.args[position]) is not None:
                    assert literal(node.args[position]) in names, f'{where}: {literal(node.args[position])!r} is not in EXTENSIONS'
                    read.add(literal(node.args[position]))
    assert modules > 20                                                         # the walk saw the package
    assert read == names                                                        # and no row of the table is dead


def test_an_experiment_declares_its_state():
    from srgan_amd import srgan
    from srgan_amd.settings import Settings

    class _Experiment(srgan.Experiment):
        def dataset_setup(self):
            pass

        def model_setup(self):
            pass

        def validation_summaries(self, step):
            pass

    state = vars(_Experiment(Settings()))
    for name in DECLARED_STATE:
        assert name in state, name
    assert state['_typed_commands'] == set() and state['_dropout_streams'] == {}
    assert state['_single_compute_stream'] is False and state['_graph_note'] is False and state['_stack_too_large'] is False
    for name in ('_captured_iteration', '_dnn_stream', '_aux_stream', '_gp_stream', '_draw_state'):
        assert state[name] is None, name


def test_the_three_draw_states_are_the_same_words(monkeypatch):
    import torch
    from srgan_amd import nn, srgan
    from srgan_amd.settings import Settings

    class _Experiment(srgan.Experiment):
        def dataset_setup(self):
            pass

        def model_setup(self):
            pass

        def validation_summaries(self, step):
            pass

    monkeypatch.setattr(nn, 'current_device', lambda: torch.device('cpu'))
    seed, iteration = 0xFEDCBA9876543210, 0x9ABCDEF0                            # above 2^32, above 2^31
    expected = [0x76543210, 0xFEDCBA98 - 2 ** 32, 0x9ABCDEF0 - 2 ** 32, 0]       # {seed_lo, seed_hi, iteration, 0} as int32
    settings = Settings()
    settings.device_random_seed = seed
    experiment = _Experiment(settings)
    experiment.starting_step = iteration
    states = {'draw_state': nn.draw_state(seed, iteration),
              'device_draw_state': experiment.device_draw_state(),
              'summary_draw_state': experiment.summary_draw_state(iteration),
              'DropoutStream.state': nn.DropoutStream(0x10000, seed, iteration).state()}
    for name, state in states.items():
        assert state.dtype == torch.int32 and tuple(state.shape) == (4,), name
        assert state.tolist() == expected, name
    assert nn.draw_state(seed + 2 ** 64, iteration + 2 ** 32).tolist() == expected          # both wrap at their width
    assert nn.draw_state(0, 0).tolist() == [0, 0, 0, 0]
