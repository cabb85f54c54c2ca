"""Dropout with masks regenerated on the MI355X (settings.drop_rate; csrc/dropout.hip): ``srgan_dropout`` against the tests'
NumPy restatement (test_dropout_cpu.py, built on the device draws' reference stream) bit for bit -- contiguous, ragged,
strided both ways, in place, across the 32-bit block word, on special values; the tape op to second order; a dense block
with dropout against CPU torch autograd in fp64 with the restatement's masks; and tiny crowd experiments with dropout in D and
DNN: reruns, a replayed HIP graph, a resumed run, a summary step in between, side streams, and the setting at 0.

Tolerances: the kernel is compared bit for bit (one fp32 product per element, the mask from exact multiples of 2^-24).  The
dense block and the side-stream comparison use 1e-3 relative, the project's tolerance against its oracles (measured against a
tensor's largest magnitude; the losses as the side-stream test of the dropout-free step measures them)."""
import numpy as np
import pytest
import torch

from helpers import assert_close, assert_close_norm
from test_dropout_cpu import dropout_reference, dropout_mask, dropout_scale

pytestmark = pytest.mark.gpu
SEED, ITERATION, DRAW = 2 ** 40 + 3, 123456, 0x10000
LOSSES = ('dnn_loss', 'labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss')
RTOL = 1e-3


def make_state(seed=SEED, iteration=ITERATION):
    words = np.array([seed & 0xffffffff, seed >> 32, iteration, 0], dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)).cuda()


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def launch(x, x_offset, y, y_offset, rows, row_elems, x_stride, y_stride, first, p, draw, state):
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib, functional as F
    _lib.check(_lib.library().srgan_dropout(x.data_ptr() + 4 * x_offset, y.data_ptr() + 4 * y_offset, rows, row_elems, x_stride,
                                            y_stride, first, p, draw, state.data_ptr(), F._stream()), 'srgan_dropout')


def check_kernel(rows, row_elems, first=0, p=0.25, x_stride=None, y_stride=None, x_offset=8, y_offset=8, in_place=False,
                 values=None, tail=8):
    """One ``srgan_dropout`` call from a buffer of normals into a NaN-filled buffer (or in place); every float of the output
    buffer -- the written rows and everything around and between them -- must hold the expected bits."""
    x_stride, y_stride = x_stride or row_elems, y_stride or row_elems
    generator = np.random.default_rng(rows * 1000003 + row_elems)
    x_host = generator.standard_normal(x_offset + (rows - 1) * x_stride + row_elems + tail).astype(np.float32)
    if values is not None:
        for r, row in enumerate(np.resize(values, (rows, row_elems))):
            x_host[x_offset + r * x_stride:x_offset + r * x_stride + row_elems] = row
    logical = np.stack([x_host[x_offset + r * x_stride:x_offset + r * x_stride + row_elems] for r in range(rows)])
    x = torch.from_numpy(x_host).cuda()
    if in_place:
        y, y_offset, y_stride = x, x_offset, x_stride
    else:
        y = torch.full((y_offset + (rows - 1) * y_stride + row_elems + tail,), float('nan'), dtype=torch.float32, device='cuda')
    want = y.cpu().numpy().copy()
    reference = dropout_reference(logical, p, SEED, ITERATION, DRAW, first)
    for r in range(rows):
        want[y_offset + r * y_stride:y_offset + r * y_stride + row_elems] = reference[r]
    launch(x, x_offset, y, y_offset, rows, row_elems, x_stride, y_stride, first, p, DRAW, make_state())
    got = y.cpu().numpy()
    wrong = np.flatnonzero(bits(got) != bits(want))
    assert wrong.size == 0, (rows, row_elems, first, p, x_stride, y_stride, x_offset, y_offset, in_place, wrong[:8],
                             got[wrong[:8]], want[wrong[:8]])
    if not in_place:
        assert np.array_equal(bits(x.cpu().numpy()), bits(x_host))      # the input is only read
    return reference


# ---- the kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.25, 0.5, 1.0])
@pytest.mark.parametrize('first', [0, 1, 2, 3, 6])
def test_contiguous_rows_against_the_restatement(first, p):
    """[3, 5, 7, 7] (rows of 245 floats: no multiple of 4, so Philox blocks straddle the rows) and 5 x 3 x 3 rows; buffers
    that start on a 16-byte boundary (offset 8) and off it (offset 5)."""
    for offset in (8, 5):
        out = check_kernel(3, 5 * 7 * 7, first, p, x_offset=offset, y_offset=offset)
        check_kernel(3, 5 * 3 * 3, first, p, x_offset=offset, y_offset=offset)
        check_kernel(2, 256, first, p, x_offset=offset, y_offset=8)     # rows of whole blocks: the 16-byte path when first % 4 == 0
    kept = np.count_nonzero(out) / out.size
    assert (kept == 1.0) if p == 0.0 else (kept == 0.0) if p == 1.0 else abs(kept - (1 - p)) < 0.1


@pytest.mark.parametrize('p', [0.25, 1.0])
@pytest.mark.parametrize('first', [0, 3])
def test_the_strided_forms_and_in_place(first, p):
    """Channels [8:13) of a [3, 16, 7, 7] buffer: written (the concatenation buffer), read (a slice of a wider gradient), both,
    and in place -- contiguous and inside the slice."""
    plane, row_elems, stride, offset = 49, 5 * 49, 16 * 49, 8 * 49
    check_kernel(3, row_elems, first, p, y_stride=stride, y_offset=offset)
    check_kernel(3, row_elems, first, p, x_stride=stride, x_offset=offset)
    check_kernel(3, row_elems, first, p, x_stride=stride, x_offset=offset, y_stride=stride, y_offset=offset + plane)
    check_kernel(3, row_elems, first, p, in_place=True)
    check_kernel(3, row_elems, first, p, x_stride=stride, x_offset=offset, in_place=True)
    check_kernel(4, 8 * 16, first, p, x_stride=32 * 16, x_offset=0, y_stride=16 * 16, y_offset=4)      # aligned slices: float4


def test_more_than_one_workgroup_and_the_grid_stride_loop():
    check_kernel(4, 8 * 40 * 40 + 3, first=5)                          # 51212 elements: 51 workgroups
    check_kernel(2, 1100003, first=2, p=0.5)                           # more Philox blocks than the grid has threads (2048 x 256)


def test_a_window_across_the_32_bit_block_word():
    """Elements 2^34 - 5 .. : blocks 2^32 - 2 .. 2^32 + 1, so the high counter word is used."""
    check_kernel(1, 12, first=2 ** 34 - 5, p=0.5)
    check_kernel(3, 7, first=2 ** 34 - 5, p=0.5, y_stride=11)


@pytest.mark.parametrize('p', [0.0, 0.25, 1.0])
def test_special_values(p):
    """-0.0, subnormals and infinities: a kept element is the IEEE product, a dropped one +0.0 whatever x holds."""
    values = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, 3.4e38, -3.4e38, 1.0, -1.5, 1.1754944e-38],
                      dtype=np.float32)
    out = check_kernel(2, 96, first=1, p=p, values=values)
    if p == 1.0:
        assert not np.signbit(out).any() and (out == 0).all()
    if p == 0.0:
        assert np.array_equal(bits(out), bits(np.resize(values, out.shape)))                   # a copy, signs of zero included


def test_another_draw_and_another_iteration_give_other_masks():
    x = torch.ones(1024, device='cuda')
    outputs = []
    for draw, iteration in ((DRAW, ITERATION), (DRAW + 1, ITERATION), (DRAW, ITERATION + 1)):
        y = torch.empty_like(x)
        launch(x, 0, y, 0, 1, 1024, 1024, 1024, 0, 0.5, draw, make_state(iteration=iteration))
        outputs.append(y.cpu().numpy())
        assert np.array_equal(outputs[-1], dropout_reference(np.ones(1024), 0.5, SEED, iteration, draw))
    assert not np.array_equal(outputs[0], outputs[1]) and not np.array_equal(outputs[0], outputs[2])


# ---- the tape op and the layers -------------------------------------------------------------------------------------------
def test_the_tape_op_to_second_order():
    """forward = mask * scale * x, its backward the same operation on the gradient, and the backward's backward again."""
    import srgan_amd  # noqa: F401
    from srgan_amd import functional as F
    from srgan_amd.tape import backward
    generator = torch.Generator().manual_seed(2)
    shape = (2, 3, 5, 5)
    x_host, g_host, h_host = (torch.randn(shape, generator=generator) for _ in range(3))
    state = make_state()
    x, g = F.leaf(x_host.cuda(), requires_grad=True), F.leaf(g_host.cuda(), requires_grad=True)
    y = F.dropout(x, 0.25, DRAW + 3, state, first=6)
    assert y.requires_grad and tuple(y.shape) == shape
    gx, = backward(y, grad=g, inputs=[x], create_graph=True)
    gg, = backward(gx, grad=F.constant(h_host.cuda()), inputs=[g])
    for got, source in ((y, x_host), (gx, g_host), (gg, h_host)):
        want = dropout_reference(source.numpy(), 0.25, SEED, ITERATION, DRAW + 3, first=6)
        assert np.array_equal(bits(got.data.cpu().numpy()), bits(want))
    flat = F.dropout(F.constant(x_host.reshape(2, 75).cuda()), 0.25, DRAW + 3, state, first=6)             # [N, F]
    assert not flat.requires_grad and np.array_equal(flat.data.cpu().numpy().reshape(shape), y.data.cpu().numpy())
    with pytest.raises(NotImplementedError):
        blocked = F.constant(x_host.cuda())
        blocked.meta = object()
        F.dropout(blocked, 0.25, DRAW, state)


def test_calls_and_iterations_get_masks_of_their_own_and_eval_mode_returns_the_input():
    import srgan_amd  # noqa: F401
    from srgan_amd import nn, functional as F
    stream = nn.DropoutStream(DRAW, seed=SEED, iteration=ITERATION)
    layer = nn.Dropout(0.5)
    nn.attach_dropout_stream(layer, stream)
    layer.train()
    x = F.constant(torch.ones(2, 4, 8, 8, device='cuda'))
    ones = np.ones((2, 4, 8, 8), dtype=np.float32)
    stream.begin_step()
    first, second = layer(x), layer(x)                                                         # two calls of one iteration
    assert np.array_equal(first.data.cpu().numpy(), dropout_reference(ones, 0.5, SEED, ITERATION, DRAW))
    assert np.array_equal(second.data.cpu().numpy(), dropout_reference(ones, 0.5, SEED, ITERATION, DRAW + 1))
    assert not torch.equal(first.data, second.data)
    stream.advance()
    stream.begin_step()
    again = layer(x)                                                                           # the same call, next iteration
    assert np.array_equal(again.data.cpu().numpy(), dropout_reference(ones, 0.5, SEED, ITERATION + 1, DRAW))
    assert not torch.equal(again.data, first.data)
    assert stream.state().cpu().tolist()[2] == ITERATION + 1
    layer.eval()
    assert layer(x) is x and stream.counter == 1


def _reference_block(x, parameters, masks, scale, layers=2):
    """The dense block in torch (float64): frozen norms, ReLU, 1x1 and 3x3 convolutions; dropout is the multiplication with
    the restatement's masks and scale in front of the concatenation."""
    features = x
    for index in range(1, layers + 1):
        get = lambda name: parameters[f'denselayer{index}.{name}']

        def norm(value, name):
            shape = (1, -1, 1, 1)
            inverse = 1.0 / torch.sqrt(get(name + '.running_var').reshape(shape) + 1e-5)
            return (value - get(name + '.running_mean').reshape(shape)) * inverse * get(name + '.weight').reshape(shape) + \
                get(name + '.bias').reshape(shape)
        hidden = torch.nn.functional.conv2d(torch.relu(norm(features, 'norm1')), get('conv1.weight'))
        hidden = torch.nn.functional.conv2d(torch.relu(norm(hidden, 'norm2')), get('conv2.weight'), padding=1)
        features = torch.cat([features, hidden * masks[index - 1] * scale], 1)
    return features


def test_a_dense_block_with_dropout_against_torch_autograd():
    """2 layers, 8 input channels, growth 4, bn_size 2 on [2, 8, 6, 6] at drop_rate 0.25: the output, the first-order gradients
    and the penalty-style second order (the gradient of sum_b ||d |y_b| / dx_b|| with respect to the weights)."""
    import srgan_amd  # noqa: F401
    from srgan_amd import nn, functional as F
    from srgan_amd.tape import backward
    from srgan_amd.crowd.models import _DenseBlock
    torch.manual_seed(0)
    block = _DenseBlock(2, 8, 2, 4, drop_rate=0.25)
    generator = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for module in block.modules():
            if isinstance(module, torch.nn.BatchNorm2d):
                module.running_mean.copy_(0.3 * torch.randn(module.num_features, generator=generator))
                module.running_var.copy_(0.5 + torch.rand(module.num_features, generator=generator))
                module.weight.copy_(0.5 + torch.rand(module.num_features, generator=generator))
                module.bias.copy_(0.2 * torch.randn(module.num_features, generator=generator))
            elif isinstance(module, torch.nn.Conv2d):
                module.weight.copy_(0.3 * torch.randn(module.weight.shape, generator=generator))
    assert all(module.eps == 1e-5 for module in block.modules() if isinstance(module, torch.nn.BatchNorm2d))
    names = [name for name, _ in block.named_parameters()]
    x_host = torch.randn(2, 8, 6, 6, generator=generator)
    weights_host = torch.randn(2, 16, 6, 6, generator=generator)
    masks = [torch.from_numpy(dropout_mask(2 * 4 * 6 * 6, 0.25, SEED, ITERATION, DRAW + call).reshape(2, 4, 6, 6).astype(np.float64))
             for call in range(2)]
    scale = float(dropout_scale(0.25))

    # the reference, float64 on the CPU
    parameters = {name: value.detach().double().clone() for name, value in block.state_dict().items()}
    for name in names:
        parameters[name].requires_grad_(True)
    x64 = x_host.double().requires_grad_(True)
    y64 = _reference_block(x64, parameters, masks, scale)
    first_order = torch.autograd.grad((y64 * weights_host.double()).sum(), [x64] + [parameters[name] for name in names],
                                      retain_graph=True)
    inner, = torch.autograd.grad(y64.flatten(1).norm(dim=1).sum(), x64, create_graph=True)
    second_order = torch.autograd.grad(inner.flatten(1).norm(dim=1).sum(), [parameters[name] for name in names])

    # the device
    arena = nn.flatten_parameters(block, torch.device('cuda'))
    block.train()
    stream = nn.DropoutStream(DRAW, seed=SEED, iteration=ITERATION)
    assert nn.attach_dropout_stream(block, stream) == 2
    gradients = lambda: [parameter.grad.detach().cpu().numpy().copy() for _, parameter in block.named_parameters()]
    stream.begin_step()
    x = F.leaf(x_host.cuda(), requires_grad=True)
    y = block(x)
    assert stream.counter == 2
    arena.zero_grad()
    backward(F.sum_all(F.mul(y, F.constant(weights_host.cuda()))))
    assert_close_norm(y.data.cpu().numpy(), y64.detach().numpy(), RTOL, 'output')
    dropped = y.data.cpu().numpy()[:, 8:] == 0
    assert np.array_equal(dropped, np.concatenate([mask.numpy() == 0 for mask in masks], axis=1))      # exactly the masks' zeros
    assert_close_norm(x.grad.data.cpu().numpy(), first_order[0].numpy(), RTOL, 'gradient of the input')
    for name, got, want in zip(names, gradients(), first_order[1:]):
        assert_close_norm(got, want.numpy(), RTOL, 'first order ' + name)
    stream.begin_step()                                                                        # the same iteration: the same masks
    x = F.leaf(x_host.cuda(), requires_grad=True)
    out = F.row_norm(F.flatten2d(block(x)))
    inner_gradient, = backward(out, grad=F.full_like(out, 1.0), inputs=[x], create_graph=True)
    assert_close_norm(inner_gradient.data.cpu().numpy(), inner.detach().numpy(), RTOL, 'recorded gradient')
    arena.zero_grad()
    backward(F.sum_all(F.row_norm(F.flatten2d(inner_gradient))))
    for name, got, want in zip(names, gradients(), second_order):
        assert float(want.abs().max()) > 0, name
        assert_close_norm(got, want.numpy(), RTOL, 'second order ' + name)


# ---- experiments ----------------------------------------------------------------------------------------------------------
SIZE, BATCH = 64, 2


def small_experiment(drop_rate=0.2, load_from=None, **overrides):
    """A ``CrowdExperiment`` whose ``model_setup`` builds the crowd networks with a small ``block_config`` at 64 x 64; its
    validation summaries run D and the DNN in eval mode on a stored batch (no dropout call may happen there)."""
    import srgan_amd  # noqa: F401
    from srgan_amd import nn
    from srgan_amd.settings import Settings
    from srgan_amd.crowd.srgan import CrowdExperiment
    from srgan_amd.crowd.models import DCGenerator, KnnDenseNetCat
    from srgan_amd.srgan import as_var
    from srgan_amd.utility import SummaryWriter, seed_all

    class Small(CrowdExperiment):
        def dataset_setup(self):
            pass

        def model_setup(self):
            arguments = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16, bn_size=2, image_size=SIZE,
                             drop_rate=self.dense_drop_rate())
            self.G = DCGenerator(image_size=SIZE, conv_dim=16)
            self.D, self.DNN = KnnDenseNetCat(**arguments), KnnDenseNetCat(**arguments)

        def validation_summaries(self, step):
            counters = [(stream.counter, dict(stream._resume)) for stream in (self.dropout_stream('D'), self.dropout_stream('DNN'))
                        if stream is not None]
            for network in (self.D, self.DNN):
                assert not network.training
                _, count, _ = network(as_var(self.validation_examples))
                self.validation_counts.append(count.data.clone())
            assert counters == [(stream.counter, dict(stream._resume)) for stream in (self.dropout_stream('D'), self.dropout_stream('DNN'))
                                if stream is not None]

    settings = Settings()
    values = dict(batch_size=BATCH, image_patch_size=SIZE, matching_loss_multiplier=1e3, contrasting_loss_multiplier=1e2,
                  gradient_penalty_multiplier=1e2, map_multiplier=1e-3, steps_to_run=10 ** 9, device_random_draws=True,
                  device_random_seed=SEED, save_step_period=0)
    if drop_rate is not None:
        values['drop_rate'] = drop_rate
    values.update(overrides)
    for key, value in values.items():
        setattr(settings, key, value)
    if load_from is not None:
        settings.load_model_path, settings.continue_existing_experiments = load_from, True
    experiment = Small(settings)
    seed_all(0)
    experiment.model_setup()
    with torch.no_grad():
        for module in experiment.D.modules():
            if isinstance(module, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                module.weight.mul_(1.5)                                # towards an active gradient penalty
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.summary_period, writer.steps_to_run = 10 ** 9, 10 ** 9
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    for optimizer in (experiment.d_optimizer, experiment.g_optimizer, experiment.dnn_optimizer):
        optimizer.count_on_device()        # every run through the device-counted Adam entry point (a captured update needs it)
    experiment.load_models()
    experiment.train_mode()
    experiment.validation_counts = []
    experiment.active_dropout = len(nn.active_dropout_layers(experiment.D)), len(nn.active_dropout_layers(experiment.DNN))
    return experiment


def batches(count):
    from test_steps_gpu import crowd_inputs
    generator = torch.Generator().manual_seed(17)
    out = []
    for _ in range(count):
        x, (heads, knn), u = crowd_inputs(generator, BATCH, SIZE)
        out.append((x.cuda(), (heads.cuda(), knn.cuda()), u.cuda()))
    return out


def snapshot(experiment):
    return {name: getattr(experiment, name)._srgan_arena.data.clone() for name in ('D', 'DNN', 'G')}


def run(experiment, steps, summaries_at=()):
    """Iterations ``steps`` (step 0 is a summary step of the writers, which only reads losses back); ``summaries_at``: steps
    after which the validation summaries run as ``end_of_step`` runs them.  Returns the losses and the weights per step."""
    from srgan_amd.tape import no_grad
    inputs = batches(max(steps) + 1)
    experiment.validation_examples = inputs[0][0]
    losses, weights = {}, {}
    for step in steps:
        x, y, u = inputs[step]
        experiment.training_iteration(x, y, u, step)
        losses[step] = {name: float(value.item()) for name, value in experiment.last_losses.items()
                        if value is not None and name in LOSSES}
        weights[step] = snapshot(experiment)
        if step in summaries_at:
            experiment.join_dnn_stream()
            experiment.eval_mode()
            with no_grad():
                experiment.validation_summaries(step)
            experiment.train_mode()
    torch.cuda.synchronize()
    return losses, weights


def assert_same_bits(a, b, steps):
    (a_losses, a_weights), (b_losses, b_weights) = a, b
    for step in steps:
        assert a_losses[step] == b_losses[step], f'step {step}: {a_losses[step]} vs {b_losses[step]}'
        for name in ('D', 'DNN', 'G'):
            x, y = a_weights[step][name], b_weights[step][name]
            assert torch.equal(x, y), (step, name, float((x - y).abs().max()))


@pytest.fixture(scope='module')
def eager_run():
    """Steps 0 .. 3 with drop_rate 0.2, eager, one stream: what the other runs are compared with."""
    experiment = small_experiment()
    assert experiment.active_dropout == (8, 8)
    result = run(experiment, range(4))
    losses = result[0]
    assert len(losses[3]) == 6 and all(np.isfinite(value) for step in losses for value in losses[step].values())
    print('[dropout] losses of the eager run:', losses)
    assert losses[3]['gradient_penalty'] > 0.0                         # the double backward carries a gradient
    for name, base in (('D', 0x10000), ('DNN', 0x20000)):
        stream = experiment.dropout_stream(name)
        assert stream.base == base and stream.state().cpu().tolist()[2] == 4                  # one advance per iteration
    # D: the stacked pass and D(fake) of the generator step in program order, the penalty's forward and the generator step's
    # D(unlabeled) in their sections; the DNN: one pass
    d, dnn = experiment.dropout_stream('D'), experiment.dropout_stream('DNN')
    assert (d.counter, d._resume, dnn.counter) == (16, {1: 0x4000 + 8, 2: 0x8000 + 8}, 8)
    assert experiment.device_draw_state().cpu().tolist()[2] == 4                              # the draws' own state, as before
    return result


@pytest.fixture(scope='module')
def rerun_and_checkpoint(tmp_path_factory):
    """The same three iterations again, saved as a checkpoint of step 2."""
    experiment = small_experiment()
    result = run(experiment, range(3))
    experiment.trial_directory = str(tmp_path_factory.mktemp('dropout_trial'))
    experiment.save_models(step=2)
    return result, experiment.trial_directory


def test_dropout_changes_the_training_and_two_runs_are_bit_identical(eager_run, rerun_and_checkpoint):
    assert_same_bits(eager_run, rerun_and_checkpoint[0], range(3))
    without = run(small_experiment(drop_rate=0.0), range(1))
    assert without[0][0] != eager_run[0][0]                            # the masks reach the losses


def test_a_resumed_run_reproduces_the_next_step(eager_run, rerun_and_checkpoint):
    resumed = small_experiment(load_from=rerun_and_checkpoint[1])
    assert resumed.starting_step == 3
    result = run(resumed, [3])
    assert resumed.dropout_stream('D').iteration == 3 and resumed.dropout_stream('D').state().cpu().tolist()[2] == 4
    assert_same_bits(eager_run, result, [3])


def test_a_replayed_graph_equals_the_eager_run(eager_run):
    experiment = small_experiment(step_graph=True, step_graph_warmup=1)
    result = run(experiment, range(4))
    captured = experiment._captured_iteration
    assert captured.eager_iterations == 1 and captured.replays == 3 and len(captured.records) == 1
    assert experiment.dropout_stream('D').state().cpu().tolist()[2] == 4
    assert experiment.dropout_stream('DNN').state().cpu().tolist()[2] == 4
    assert_same_bits(eager_run, result, range(4))


def test_a_summary_step_in_between_leaves_the_training_bits_unchanged(eager_run):
    experiment = small_experiment()
    result = run(experiment, range(3), summaries_at=(0, 1))
    assert len(experiment.validation_counts) == 4
    assert all(bool(torch.isfinite(count).all()) for count in experiment.validation_counts)
    assert_same_bits(eager_run, result, range(3))


@pytest.fixture
def single_stream_afterwards():
    from srgan_amd import fused
    saved = fused.WGRAD_STREAM
    yield
    fused.WGRAD_STREAM = saved


def test_the_side_streams_draw_the_same_masks(eager_run, single_stream_afterwards):
    """The DNN step, the penalty chain, the generator step's D(unlabeled) and the weight gradients on their side streams: the
    losses agree with the single-stream run to the tolerance the side-stream test of the dropout-free step asserts (1e-3
    relative, 1e-6 absolute below 1e-3: the penalty chain's gradients are added to the arena in another order)."""
    experiment = small_experiment(overlap_dnn_step=True, wgrad_stream=True, overlap_generator_forwards=True,
                                  overlap_gradient_penalty=True)
    losses, _ = run(experiment, range(3))
    assert experiment._penalty_stream() is not None and experiment._auxiliary_stream() is not None
    for step in range(3):
        for name, value in eager_run[0][step].items():
            print(f'[dropout side streams] step {step} {name}: {losses[step][name]:.9g} vs {value:.9g}')
            assert_close(losses[step][name], value, rtol=RTOL, atol=1e-6 if abs(value) < 1e-3 else 0.0, what=f'step {step} {name}')
    d = experiment.dropout_stream('D')
    assert (d.counter, d._resume) == (16, {1: 0x4000 + 8, 2: 0x8000 + 8})


def test_drop_rate_zero_is_the_run_without_the_setting(monkeypatch):
    import srgan_amd  # noqa: F401
    from srgan_amd import functional as F

    def refuse(*arguments, **keywords):
        raise AssertionError('dropout code ran at drop_rate 0')
    monkeypatch.setattr(F, 'dropout', refuse)
    results = []
    for drop_rate in (None, 0.0):
        experiment = small_experiment(drop_rate=drop_rate)
        assert experiment.active_dropout == (0, 0)
        results.append(run(experiment, range(3)))
        assert experiment.dropout_stream('D') is None and experiment.dropout_stream('DNN') is None
    assert_same_bits(results[0], results[1], range(3))


def test_gpu_mode_refuses_dropout_under_a_world_of_two():
    from types import SimpleNamespace
    import srgan_amd  # noqa: F401
    from srgan_amd.settings import Settings
    from srgan_amd.crowd.srgan import CrowdExperiment
    from srgan_amd.crowd.models import DCGenerator, KnnDenseNetCat

    class Small(CrowdExperiment):
        def model_setup(self):
            arguments = dict(growth_rate=4, block_config=(1, 1, 1, 1), num_init_features=8, bn_size=2, image_size=SIZE,
                             drop_rate=self.dense_drop_rate())
            self.G = DCGenerator(image_size=SIZE, conv_dim=8)
            self.D, self.DNN = KnnDenseNetCat(**arguments), KnnDenseNetCat(**arguments)
    for drop_rate, refused in ((0.2, True), (0.0, False)):
        settings = Settings()
        settings.drop_rate = drop_rate
        experiment = Small(settings)
        experiment.model_setup()
        experiment.dp = SimpleNamespace(world_size=2, rank=0, active=True)
        if refused:
            with pytest.raises(NotImplementedError, match='one device'):
                experiment.gpu_mode()
            assert getattr(experiment.D, '_srgan_arena', None) is None
        else:
            experiment.gpu_mode()
