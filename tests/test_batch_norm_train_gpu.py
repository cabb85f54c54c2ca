"""Training-mode batch normalisation (csrc/batch_norm_train.hip) on the GPU: the four C-ABI entry points against
``torch.nn.functional.batch_norm(training=True)`` and torch autograd in fp64 on the CPU, run-to-run determinism,
``nn.BatchStatNorm2d``, the refusals, the unchanged frozen ``nn.BatchNorm2d``, and whole training steps with the DCGAN
``batch_norm`` switch on against golden g16 (generated from the unmodified reference with its switch forced on) -- eager in
three schedules, replayed as a HIP graph, and on 16-bit storage.  Tolerance of the op tests: the project's op tolerance,
``assert_close_norm`` at 1e-3; of the steps: the 1e-3 of test_steps_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from helpers import load_golden, golden_state, golden_scalars, assert_close, assert_close_norm

pytestmark = pytest.mark.gpu
RTOL = 1e-3
MOMENTUM, EPS = 0.1, 1e-5

# (N, C, H, W): odd plane (scalar tail); M = 6 in one channel; N = 1; a plain float4 case; two shapes where several
# workgroups share a channel (the ordered combine); 300 workgroups of one image per channel -- and per channel group of the
# blocked twin -- so that the finishing loop of the last one wraps (parts t and t + 256); and data far from zero (offset 1000), where E[x^2] - E[x]^2 in fp32
# loses the variance (14 % off) while sums of deviations do not.
SHAPES = [(4, 5, 3, 5), (3, 1, 1, 2), (1, 4, 64, 64), (2, 3, 32, 32), (16, 64, 8, 8), (8, 8, 64, 64), (300, 5, 1, 2)]
CASES = [(shape, 0.0) for shape in SHAPES] + [((4, 5, 6, 7), 1000.0)]
SLOPES = [1.0, 0.05]


def _ids(case):
    return 'x'.join(str(v) for v in case[0]) + ('+1000' if case[1] else '')


def _call(name, *arguments):
    from srgan_amd import _lib
    _lib.check(getattr(_lib.library(), name)(*arguments), name)


def _stream():
    from srgan_amd import _lib
    return _lib.stream_handle()


@functools.lru_cache(maxsize=None)
def inputs(case):
    shape, offset = case
    generator = torch.Generator().manual_seed(sum(shape) + int(offset))
    c = shape[1]
    return dict(x=torch.randn(shape, generator=generator) + offset, gamma=torch.rand(c, generator=generator) + 0.5,
                beta=torch.randn(c, generator=generator) * 0.5, running_mean=torch.randn(c, generator=generator) * 0.1,
                running_var=torch.rand(c, generator=generator) + 0.5, cotangent=torch.randn(shape, generator=generator),
                old_gamma_grad=torch.randn(c, generator=generator), old_beta_grad=torch.randn(c, generator=generator))


@functools.lru_cache(maxsize=None)
def reference(case, slope):
    """fp64 on the CPU, computed once per (case, slope): outputs, statistics, running buffers after one and three calls, and
    the autograd gradients for a random cotangent."""
    functional = torch.nn.functional
    given = inputs(case)
    x = given['x'].double().requires_grad_()
    gamma, beta = given['gamma'].double().requires_grad_(), given['beta'].double().requires_grad_()
    running_mean, running_var = given['running_mean'].double().clone(), given['running_var'].double().clone()
    out = {}
    for call in (1, 2, 3):
        y = functional.batch_norm(x, running_mean, running_var, gamma, beta, training=True, momentum=MOMENTUM, eps=EPS)
        if call in (1, 3):
            out[f'running_mean{call}'], out[f'running_var{call}'] = running_mean.clone().numpy(), running_var.clone().numpy()
    y = functional.leaky_relu(y, slope) if slope != 1.0 else y
    gx, ggamma, gbeta = torch.autograd.grad(y, (x, gamma, beta), given['cotangent'].double())
    variance = x.detach().var(dim=(0, 2, 3), unbiased=False)
    out.update(y=y.detach().numpy(), mean=x.detach().mean(dim=(0, 2, 3)).numpy(), inv_std=(variance + EPS).rsqrt().numpy(),
               gx=gx.numpy(), ggamma=ggamma.numpy(), gbeta=gbeta.numpy())
    return out


def abi_forward(x, gamma, beta, running_mean, running_var, tracked, slope):
    n, c, h, w = x.shape
    stats, y = torch.empty(2, c, device=x.device), torch.empty_like(x)
    _call('srgan_batch_norm_train_stats', x.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), running_mean.data_ptr(),
          running_var.data_ptr(), tracked.data_ptr(), MOMENTUM, EPS, n, c, h * w, _stream())
    _call('srgan_batch_norm_train_fwd', x.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
          slope, y.data_ptr(), n, c, h * w, _stream())
    return y, stats


def abi_backward(g, x, stats, gamma, beta, slope, gamma_grad=None, beta_grad=None):
    n, c, h, w = x.shape
    sums, gx = torch.empty(2, c, device=x.device), torch.empty_like(x)
    _call('srgan_batch_norm_train_bwd_reduce', g.data_ptr(), x.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
          gamma.data_ptr(), beta.data_ptr(), slope, sums.data_ptr(), None if gamma_grad is None else gamma_grad.data_ptr(),
          None if beta_grad is None else beta_grad.data_ptr(), n, c, h * w, _stream())
    _call('srgan_batch_norm_train_bwd_apply', g.data_ptr(), x.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
          gamma.data_ptr(), beta.data_ptr(), slope, sums.data_ptr(), gx.data_ptr(), n, c, h * w, _stream())
    return gx, sums


def poison_workspace():
    """NaN in the stream's workspace: a partial that the last workgroup of a row reads before it was written shows."""
    from srgan_amd import _lib
    _lib._workspaces[(torch.cuda.current_device(), _lib.stream_handle())].fill_(float('nan'))


def on_device(case):
    return {key: value.clone().cuda() for key, value in inputs(case).items()}


@pytest.fixture(scope='module', autouse=True)
def pkg():
    import srgan_amd
    assert torch.cuda.is_available()
    return srgan_amd


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_forward_statistics_and_running_buffers(case, slope):
    want, d = reference(case, slope), on_device(case)
    tracked = torch.zeros((), dtype=torch.int64, device='cuda')
    for call in (1, 2, 3):
        poison_workspace()
        y, stats = abi_forward(d['x'], d['gamma'], d['beta'], d['running_mean'], d['running_var'], tracked, slope)
        if call in (1, 3):
            for name in ('running_mean', 'running_var'):
                got = d[name].cpu().numpy()
                print(f'{_ids(case)} slope {slope} call {call} {name}: max err {np.abs(got - want[name + str(call)]).max():.3e}')
                assert_close_norm(got, want[f'{name}{call}'], RTOL, f'{name} after {call} call(s)')
    assert int(tracked) == 3
    for name, got in (('y', y), ('mean', stats[0]), ('inv_std', stats[1])):
        got = got.cpu().numpy()
        print(f'{_ids(case)} slope {slope} {name}: max err {np.abs(got - want[name]).max():.3e} of {np.abs(want[name]).max():.3e}')
        assert_close_norm(got, want[name], RTOL, name)
    # the variance itself (what separates the two formulations on the offset case), not only its inverse root
    variance = 1.0 / stats[1].double().cpu().numpy() ** 2 - EPS
    assert_close_norm(variance, 1.0 / want['inv_std'] ** 2 - EPS, RTOL, 'batch variance')


# ------------------------------------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_backward_against_autograd(case, slope):
    want, d = reference(case, slope), on_device(case)
    tracked = torch.zeros((), dtype=torch.int64, device='cuda')
    _, stats = abi_forward(d['x'], d['gamma'], d['beta'], d['running_mean'], d['running_var'], tracked, slope)
    gamma_grad, beta_grad = d['old_gamma_grad'].clone(), d['old_beta_grad'].clone()      # a non-zero arena gradient
    gx, sums = abi_backward(d['cotangent'], d['x'], stats, d['gamma'], d['beta'], slope, gamma_grad, beta_grad)
    for name, got in (('gx', gx), ('ggamma', sums[1]), ('gbeta', sums[0])):
        got = got.cpu().numpy()
        print(f'{_ids(case)} slope {slope} {name}: max err {np.abs(got - want[name]).max():.3e} of {np.abs(want[name]).max():.3e}')
        assert_close_norm(got, want[name], RTOL, name)
    # accumulation ADDS: old + this pass's sums (fp32 addition of the very numbers returned in ``sums``)
    assert torch.equal(gamma_grad, d['old_gamma_grad'] + sums[1]) and torch.equal(beta_grad, d['old_beta_grad'] + sums[0])
    assert float((gamma_grad - d['old_gamma_grad']).abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_two_runs_are_bit_identical():
    case = ((8, 8, 64, 64), 0.0)
    runs = []
    for _ in range(2):
        d = on_device(case)
        tracked = torch.zeros((), dtype=torch.int64, device='cuda')
        y, stats = abi_forward(d['x'], d['gamma'], d['beta'], d['running_mean'], d['running_var'], tracked, 0.05)
        gx, sums = abi_backward(d['cotangent'], d['x'], stats, d['gamma'], d['beta'], 0.05)
        torch.cuda.synchronize()
        runs.append((y, stats, d['running_mean'], d['running_var'], gx, sums))
    for first, second in zip(*runs):
        assert torch.equal(first, second)


# ------------------------------------------------------------------------------------------------ 4. the module
def test_batch_stat_norm_module_trains_then_evaluates_with_refreshed_statistics():
    from srgan_amd import functional as F, nn
    from srgan_amd.tape import no_grad
    generator = torch.Generator().manual_seed(4)
    channels = 6
    ours, theirs = nn.BatchStatNorm2d(channels), torch.nn.BatchNorm2d(channels).double()
    with torch.no_grad():
        ours.weight.copy_(torch.rand(channels, generator=generator) + 0.5)
        ours.bias.copy_(torch.randn(channels, generator=generator))
    theirs.load_state_dict({key: value.double() if value.is_floating_point() else value for key, value in ours.state_dict().items()})
    assert list(ours.state_dict()) == list(theirs.state_dict())
    nn.flatten_parameters(ours, torch.device('cuda', 0))
    batches = [torch.randn(5, channels, 6, 10, generator=generator) * (1 + index) + index for index in range(4)]
    ours.eval()
    with no_grad():
        ours(F.leaf(batches[3].cuda()))                       # the cache of the eval path exists BEFORE the statistics move
    cached = [ours._inv_std_cache[1].data.data_ptr(), ours._inv_std_cache[2].data.data_ptr()]
    buffers = [ours.running_mean.data_ptr(), ours.running_var.data_ptr(), ours.num_batches_tracked.data_ptr()]
    ours.train()
    theirs.train()
    for batch in batches[:3]:
        with no_grad():
            got = ours(F.leaf(batch.cuda()), slope=0.05)
        want = torch.nn.functional.leaky_relu(theirs(batch.double()), 0.05)
        assert_close_norm(got.cpu().numpy(), want.detach().numpy(), RTOL, 'training forward')
    ours.eval()
    theirs.eval()
    with no_grad():
        got = ours(F.leaf(batches[3].cuda()))
    assert_close_norm(got.cpu().numpy(), theirs(batches[3].double()).detach().numpy(), RTOL, 'eval forward after training')
    assert int(ours.num_batches_tracked) == int(theirs.num_batches_tracked) == 3
    assert_close_norm(ours.running_var.cpu().numpy(), theirs.running_var.numpy(), RTOL, 'running_var')
    assert float((theirs.running_var - 1).abs().min()) > 0.1          # the eval output above cannot come from stale statistics
    assert cached == [ours._inv_std_cache[1].data.data_ptr(), ours._inv_std_cache[2].data.data_ptr()]
    assert buffers == [ours.running_mean.data_ptr(), ours.running_var.data_ptr(), ours.num_batches_tracked.data_ptr()]
    state = ours.state_dict()
    assert list(state) == list(theirs.state_dict()) and int(state['num_batches_tracked']) == 3


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_second_order_backward_and_single_value_channels_are_refused():
    from srgan_amd import functional as F
    from srgan_amd.tape import backward, no_grad
    d = on_device(((2, 3, 32, 32), 0.0))
    x = F.leaf(d['x'], requires_grad=True)
    gamma, beta = F.leaf(d['gamma'], requires_grad=True), F.leaf(d['beta'], requires_grad=True)
    y = F.batch_norm_train(x, gamma, beta, d['running_mean'], d['running_var'], MOMENTUM, EPS, slope=0.05)
    with pytest.raises(NotImplementedError, match='first-order'):
        backward(F.sum_all(F.square(y)), inputs=[x], create_graph=True)
    # the first-order sweep of the same op works, and agrees with the C-ABI path
    y = F.batch_norm_train(x, gamma, beta, d['running_mean'], d['running_var'], MOMENTUM, EPS, slope=0.05)
    gx, ggamma, gbeta = backward(F.sum_all(F.mul(y, F.leaf(d['cotangent']))), inputs=[x, gamma, beta])
    want = reference(((2, 3, 32, 32), 0.0), 0.05)
    for name, got in (('gx', gx), ('ggamma', ggamma), ('gbeta', gbeta)):
        assert_close_norm(got.cpu().numpy(), want[name], RTOL, name)
    with no_grad():
        assert F.batch_norm_train(x, gamma, beta, None, None, MOMENTUM, EPS).node is None       # nothing saved
    single = F.leaf(torch.randn(1, 3, 1, 1).cuda())
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        F.batch_norm_train(single, gamma, beta, d['running_mean'], d['running_var'], MOMENTUM, EPS)


# ------------------------------------------------------------------------------------------------ 6. the frozen norm
def test_frozen_batch_norm_ignores_its_training_flag():
    from srgan_amd import functional as F, nn
    from srgan_amd.tape import no_grad
    generator = torch.Generator().manual_seed(6)
    module = nn.BatchNorm2d(5)
    with torch.no_grad():
        module.weight.copy_(torch.rand(5, generator=generator) + 0.5)
        module.bias.copy_(torch.randn(5, generator=generator))
        module.running_mean.copy_(torch.randn(5, generator=generator))
        module.running_var.copy_(torch.rand(5, generator=generator) + 0.5)
    before = {key: value.clone() for key, value in module.state_dict().items()}
    nn.flatten_parameters(module, torch.device('cuda', 0))
    module.train()
    x = torch.randn(4, 5, 7, 9, generator=generator) * 3 + 2
    with no_grad():
        got = module(F.leaf(x.cuda()))
    want = torch.nn.functional.batch_norm(x.double(), before['running_mean'].double(), before['running_var'].double(),
                                          before['weight'].double(), before['bias'].double(), training=False, eps=module.eps)
    assert_close_norm(got.cpu().numpy(), want.numpy(), RTOL, 'running-statistics output in training mode')
    for key, value in module.state_dict().items():
        assert torch.equal(value.cpu(), before[key]), key


# ------------------------------------------------------------------------------------------------ 7. the step
def golden16():
    merged = {}
    for name in ('g16_tiny_dcgan_batch_norm', 'g16_tiny_dcgan_batch_norm_final', 'g16_tiny_dcgan_batch_norm_adam'):
        archive = load_golden(name)
        merged.update({key: archive[key] for key in archive.files})

    class Golden(dict):
        files = property(lambda self: list(self))
    return Golden(merged)


def dcgan_experiment(**settings):
    from test_steps_gpu import make_experiment
    from srgan_amd.age.models import Generator, Discriminator
    settings = dict(dict(batch_size=4, matching_loss_multiplier=1e2, contrasting_loss_multiplier=1e1, gradient_penalty_multiplier=1e2,
                         generator_batch_norm=True, discriminator_batch_norm=True), **settings)
    return make_experiment(lambda: (Generator(image_size=32, conv_dim=8, batch_norm=settings['generator_batch_norm']),
                                    Discriminator(32, 8, batch_norm=settings['discriminator_batch_norm']),
                                    Discriminator(32, 8, batch_norm=settings['discriminator_batch_norm'])), settings)


def assert_statistic_close(got, key, expected_state, what, after_adam_update=False):
    """A running statistic against the golden at the step tolerance of test_steps_gpu.py: rtol 1e-3, and for the running
    means (many of them near zero) that file's atol of 2e-5.  Statistics gathered AFTER an Adam update of G get one derived
    allowance on top: the bias in front of the norm has a gradient of exactly zero, Adam steps it by lr = 1e-4 in the
    direction of rounding noise (ZERO_GRADIENT_BIASES below), a sign that differs from the reference's shifts the channel
    mean by 2 lr = 2e-4, and the two momentum-0.1 updates of the step carry 0.1 + 0.09 = 0.19 of that, 3.8e-5, into the
    running mean (the norm subtracts the shift again, so nothing else moves).  The running variances get no allowance."""
    expected = expected_state[key].numpy()
    print(f'{what}: max err {np.abs(got - expected).max():.3e} of {np.abs(expected).max():.3e}')
    if key.endswith('running_mean'):
        assert_close(got, expected, rtol=RTOL, atol=2e-5 + (0.19 * 2e-4 if after_adam_update else 0.0), what=what)
    else:
        assert_close(got, expected, rtol=RTOL, atol=0.0, what=what)


# The bias of a layer that feeds a batch-statistics norm has a gradient of exactly zero (the norm subtracts the batch mean,
# so the output does not depend on it): what reaches Adam, in the reference and here, is rounding noise of either sign.
ZERO_GRADIENT_BIASES = ('layer1.0.bias', 'layer2.0.bias', 'layer3.0.bias')

SCHEDULES = {'as_written': dict(reference_schedule=True), 'shared_forwards': {},
             'four_streams': dict(overlap_dnn_step=True, wgrad_stream=True, overlap_generator_forwards=True,
                                  overlap_gradient_penalty=True)}


@pytest.mark.parametrize('schedule', list(SCHEDULES))
def test_two_steps_with_the_switch_on_match_the_reference(schedule):
    from test_steps_gpu import finish_setup, run_step, check, dev
    from srgan_amd import nn
    g = golden16()
    experiment = dcgan_experiment(**SCHEDULES[schedule])
    for module, prefix in ((experiment.G, 'init/G'), (experiment.D, 'init/D'), (experiment.DNN, 'init/DNN')):
        module.load_state_dict(golden_state(g, prefix), strict=True)
    finish_setup(experiment)
    assert sum(isinstance(m, nn.BatchStatNorm2d) and m.training for m in experiment.G.modules()) == 3
    for step in range(2):
        x, y, u = (dev(g[f's{step}/{k}']) for k in ('x', 'y', 'u'))
        result = run_step(experiment, x, y, u, step, g)
        print(schedule, step, result)
        check(result, golden_scalars(g, step), f'g16 {schedule} step {step}')
        assert_close(experiment.gradient_norm.cpu().numpy(), g[f's{step}/gradient_norm'], rtol=RTOL, what='gradient norms')
        recorded = golden_state(g, f's{step}/G_buffers')
        for key, value in recorded.items():
            got = experiment.G.state_dict()[key].cpu().numpy()
            if 'tracked' in key:
                assert int(got) == int(value) == 2 * (step + 1), key
            else:
                assert_statistic_close(got, key, recorded, f'step {step} G {key}', after_adam_update=step > 0)
    assert result['gradient_penalty'] > 1.0
    experiment.join_dnn_stream()
    torch.cuda.synchronize()
    for name in ('D', 'DNN', 'G'):
        state = getattr(experiment, name).state_dict()
        for key, value in golden_state(g, f'final/{name}').items():
            if 'tracked' in key:
                assert int(state[key]) == int(value) == (4 if name == 'G' else 0), (name, key)
            elif 'running' in key:
                assert_statistic_close(state[key].cpu().numpy(), key, golden_state(g, f'final/{name}'), f'final {name} {key}',
                                       after_adam_update=name == 'G')
            elif name == 'G' and key in ZERO_GRADIENT_BIASES:
                # Adam turns rounding noise into steps of up to lr per element and step: the criterion test_steps_gpu.py uses
                # for weights behind one such step (2.2e-4 + 1e-3 max|want|), for the two steps taken here
                got, want = state[key].cpu().numpy(), value.numpy()
                print(f'final G {key}: max err {np.abs(got - want).max():.3e}')
                assert np.abs(got - want).max() <= 2 * 2.2e-4 + 1e-3 * np.abs(want).max(), key
                assert np.abs(got - g[f'init/G/{key}']).max() <= 2 * 1.1e-4, f'{key} moved by more than two Adam steps'
            else:
                assert_close(state[key].cpu().numpy(), value.numpy(), rtol=RTOL, atol=3e-5, what=f'final {name} {key}')
    arena, optimizer = experiment.G._srgan_arena, experiment.g_optimizer
    for (pname, _), offset, size in zip(experiment.G.named_parameters(), arena.offsets, arena.sizes):
        for moment in ('exp_avg', 'exp_avg_sq'):
            expected = g[f'final_adam/G/{pname}/{moment}'].reshape(-1)
            got = getattr(optimizer, moment)[offset:offset + size].cpu().numpy()
            if pname in ZERO_GRADIENT_BIASES:
                # moments of a gradient that is exactly zero: zero at the step tolerance on the scale of the layer's own
                # weight gradient, here and in the reference
                scale = np.abs(g[f"final_adam/G/{pname.replace('bias', 'weight')}/{moment}"]).max()
                assert np.abs(got).max() <= RTOL * scale and np.abs(expected).max() <= RTOL * scale, (pname, moment)
                continue
            assert_close(got, expected, rtol=RTOL, atol=1e-4 * np.abs(expected).max(), what=f'Adam {moment} of G {pname}')
        assert float(g[f'final_adam/G/{pname}/step']) == optimizer.step_count == 2


# ------------------------------------------------------------------------------------------------ 8. replay
def _iterations(step_graph, count=3):
    from test_steps_gpu import finish_setup
    from srgan_amd.utility import seed_all
    g = golden16()
    experiment = dcgan_experiment(step_graph=step_graph, step_graph_warmup=1, steps_to_run=10 ** 9)
    for module, prefix in ((experiment.G, 'init/G'), (experiment.D, 'init/D'), (experiment.DNN, 'init/DNN')):
        module.load_state_dict(golden_state(g, prefix), strict=True)
    finish_setup(experiment)
    for optimizer in (experiment.d_optimizer, experiment.g_optimizer, experiment.dnn_optimizer):
        optimizer.count_on_device()
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.summary_period, writer.steps_to_run = 10 ** 9, 10 ** 9
    seed_all(5)
    generator = torch.Generator().manual_seed(11)
    losses = []
    for step in range(1, count + 1):
        x, u = (torch.rand(4, 3, 32, 32, generator=generator) * 2 - 1 for _ in range(2))
        y = torch.rand(4, generator=generator) * 85 + 10
        experiment.training_iteration(x.cuda(), y.cuda(), u.cuda(), step)
        losses.append({name: float(value.item()) for name, value in experiment.last_losses.items() if value is not None})
    torch.cuda.synchronize()
    return experiment, losses


def test_replayed_iterations_equal_the_eager_ones_bit_for_bit():
    eager, eager_losses = _iterations(False)
    replayed, replayed_losses = _iterations(True)
    captured = replayed._captured_iteration
    assert captured.eager_iterations == 1 and captured.replays == 2
    assert eager_losses == replayed_losses and eager_losses[-1] != eager_losses[-2]
    for name in ('D', 'DNN', 'G'):
        assert torch.equal(getattr(eager, name)._srgan_arena.data, getattr(replayed, name)._srgan_arena.data), name
        for (key, a), (_, b) in zip(getattr(eager, name).named_buffers(), getattr(replayed, name).named_buffers()):
            assert torch.equal(a, b), (name, key)
    assert int(replayed.G.layer1[1].num_batches_tracked) == 6
    for a, b in ((eager.g_optimizer, replayed.g_optimizer), (eager.d_optimizer, replayed.d_optimizer)):
        assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    # the statistics a replay wrote reach the eval path: the cache refreshes when the network leaves training mode
    from srgan_amd import functional as F
    from srgan_amd.tape import no_grad
    z = F.leaf(torch.randn(4, 256, generator=torch.Generator().manual_seed(3)).cuda())
    for experiment in (eager, replayed):
        experiment.eval_mode()
    with no_grad():
        assert torch.equal(eager.G(z).data, replayed.G(z).data)


# ------------------------------------------------------------------------------------------------ 9. 16-bit storage
def _driving_step(**overrides):
    """One step of the driving DCGAN pair on 64 x 192 frames (the configuration of the 16-bit step tests; G's planes are the
    8 x 24, 16 x 48 and 32 x 96 of the driving frames) with batch statistics in G."""
    from srgan_amd.settings import Settings
    from srgan_amd.driving.srgan import DrivingExperiment
    from srgan_amd.utility import SummaryWriter, seed_all
    size, batch = (64, 192), 8
    settings = Settings()
    settings.batch_size, settings.generator_batch_norm = batch, True
    settings.matching_loss_multiplier, settings.contrasting_loss_multiplier, settings.gradient_penalty_multiplier = 1e2, 1e1, 1e2
    for key, value in overrides.items():
        setattr(settings, key, value)
    experiment = DrivingExperiment(settings)
    experiment.image_size = size
    seed_all(0)
    experiment.model_setup()
    with torch.no_grad():
        for module in experiment.D.modules():
            if isinstance(module, torch.nn.Conv2d):
                module.weight.mul_(2.2)                     # gradient penalty active
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    experiment.train_mode()
    metas = []
    for stage in (experiment.G.layer1, experiment.G.layer2, experiment.G.layer3):
        stage[1].register_forward_hook(lambda module, args, output: metas.extend([args[0].meta, output.meta]))
    generator = torch.Generator().manual_seed(1)
    x, u = (torch.rand(batch, 3, *size, generator=generator) * 2 - 1 for _ in range(2))
    y = torch.rand(batch, generator=generator) * 2 - 1
    experiment.injected_draws = {'z_d': torch.randn(batch, 256, generator=generator), 'z_g': torch.randn(batch, 256, generator=generator),
                                 'alpha': torch.rand(batch, 1, 1, 1, generator=generator)}
    experiment.dnn_training_step(x.cuda(), y.cuda(), 0)
    experiment.gan_training_step(x.cuda(), y.cuda(), u.cuda(), 0)
    experiment.join_dnn_stream()
    torch.cuda.synchronize()
    return experiment, {k: float(v.item()) for k, v in experiment.last_losses.items() if v is not None}, metas


def test_a_step_on_bf16_storage_keeps_the_generator_on_the_fp32_graph():
    _, expected, _ = _driving_step()
    experiment, got, metas = _driving_step(compute_dtype='bf16', gradient_penalty_dtype='bf16', storage_dtype='bf16')
    assert len(metas) == 12 and all(meta is None for meta in metas)      # two forwards x three norms, fp32 in and out
    assert expected['gradient_penalty'] > 1.0
    worst = 0.0
    for key in ('labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss'):
        error = abs(got[key] - expected[key]) / max(abs(expected[key]), 1e-12)
        worst = max(worst, error)
        print(f'[bf16 storage] {key}: {got[key]:.6g}  fp32 {expected[key]:.6g}  rel {error:.2e}')
        assert error <= 5e-2, (key, got[key], expected[key])
    assert worst > 1e-7, 'results identical to fp32: the 16-bit path was not active'
    assert int(experiment.G.layer1[1].num_batches_tracked) == 2
    for parameter in experiment.G.parameters():
        assert torch.isfinite(parameter).all()
