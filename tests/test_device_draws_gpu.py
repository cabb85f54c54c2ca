"""Device random draws on the MI355X (settings.device_random_draws; csrc/random_draws.hip): ``srgan_random_fill`` against the
tests' NumPy reference of the stream (device_draws_reference.py, pinned to the Philox known answers on the CPU), the window
property behind data parallelism, the keys, the device state and its advance, a captured fills + advance chain, and training
steps of tiny experiments that draw on the device -- eager, replayed, resumed, with injected draws and on bf16 storage.

Tolerance of the normals, derived (not measured): u1, u2 and the sign are exact in fp32; logf, sqrtf and sincospif are each
within a few ulp; r <= sqrt(-2 ln 2^-24) = 5.77; rounding the angle moves it by at most about 4e-7 -- together roughly 3e-6 at
worst, and the bound is three times that."""
import numpy as np
import pytest
import torch

import device_draws_reference as R
from test_steps_gpu import make_experiment, finish_setup

pytestmark = pytest.mark.gpu
NORMAL_ATOL = 1e-5
SEED, ITERATION = 2 ** 40 + 3, 123456
LOSSES = ('dnn_loss', 'labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss')


def make_state(seed=SEED, iteration=ITERATION):
    words = np.array([seed & 0xffffffff, seed >> 32, iteration, 0], dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)).cuda()


def fill(n, first, kind, offset, draw, state, pad=8):
    """``srgan_random_fill`` into the middle of a NaN-filled buffer (``pad`` floats on either side, which must stay NaN);
    ``pad`` 8 leaves the output 16-byte aligned, 5 does not."""
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib, functional as F
    buffer = torch.full((n + 2 * pad,), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(_lib.library().srgan_random_fill(buffer.data_ptr() + 4 * pad, n, first, kind, offset, draw, state.data_ptr(),
                                                F._stream()), 'srgan_random_fill')
    host = buffer.cpu().numpy()
    assert np.isnan(host[:pad]).all() and np.isnan(host[pad + n:]).all(), (n, first, kind, pad)
    return host[pad:pad + n]


CASES = [(n, first) for n in (1, 3, 4, 5, 1027) for first in (0, 1, 2, 3, 7)] + [(4, 2 ** 34 - 2)]


@pytest.mark.parametrize('pad', [8, 5])
def test_the_kernel_against_the_reference(pad):
    state = make_state()
    worst = 0.0
    for n, first in CASES:
        uniform = fill(n, first, 0, 0.0, 1, state, pad)
        assert np.array_equal(uniform.astype(np.float64), R.expected(0, SEED, ITERATION, 1, first, n)), (n, first)   # bit for bit
        normal = fill(n, first, 1, 0.0, 0, state, pad)
        error = float(np.abs(normal.astype(np.float64) - R.expected(1, SEED, ITERATION, 0, first, n)).max())
        shifted = fill(n, first, 1, 0.5, 0, state, pad)
        error = max(error, float(np.abs(shifted.astype(np.float64) - R.expected(1, SEED, ITERATION, 0, first, n, 0.5)).max()))
        worst = max(worst, error)
        assert error <= NORMAL_ATOL, (n, first, error)
        # the offset is ONE fp32 addition of +/-offset, the sign from bit 0 of the element's own word: the rounded sum, exactly
        sign = R.signs(SEED, ITERATION, 0, first, n).astype(np.float32)
        assert np.array_equal(shifted, normal + np.float32(0.5) * sign), (n, first)
        assert np.array_equal(np.sign(shifted.astype(np.float64) - normal), sign), (n, first)
    print(f'[device draws] largest |kernel - float64 reference| of the normals over the cases (pad {pad}): {worst:.3e}')


@pytest.mark.parametrize('kind, offset', [(0, 0.0), (1, 0.0), (1, 0.5)])
def test_a_window_is_bit_identical_to_the_slice_of_one_fill_from_zero(kind, offset):
    """The data-parallel rule: whoever fills [first, first + n) gets the bits of that slice of the whole draw."""
    state = make_state()
    whole = fill(1027, 0, kind, offset, 2, state)
    assert np.array_equal(fill(20, 1001, kind, offset, 2, state), whole[1001:1021])
    assert np.array_equal(fill(20, 1001, kind, offset, 2, state, pad=5), whole[1001:1021])
    tensor = fill(60, 0, kind, offset, 0, state)                       # 6 x 10, two ranks of 3 rows
    assert np.array_equal(fill(30, 0, kind, offset, 0, state), tensor[:30])
    assert np.array_equal(fill(30, 30, kind, offset, 0, state), tensor[30:])


def test_keys():
    base = fill(64, 0, 1, 0.0, 0, make_state(1, 5))
    assert np.array_equal(base, fill(64, 0, 1, 0.0, 0, make_state(1, 5)))           # same (seed, iteration, draw): same bits
    assert not np.array_equal(base, fill(64, 0, 1, 0.0, 0, make_state(2, 5)))       # the seed
    assert not np.array_equal(base, fill(64, 0, 1, 0.0, 0, make_state(1, 6)))       # the iteration
    assert not np.array_equal(base, fill(64, 0, 1, 0.0, 1, make_state(1, 5)))       # the draw
    high = fill(64, 0, 1, 0.0, 0, make_state(2 ** 32 + 1, 5))                       # seed_hi is used
    assert not np.array_equal(base, high)
    assert np.abs(high.astype(np.float64) - R.expected(1, 2 ** 32 + 1, 5, 0, 0, 64)).max() <= NORMAL_ATOL


def test_the_state_and_its_advance():
    from srgan_amd import functional as F
    state = make_state(9, 41)
    first = fill(33, 0, 0, 0.0, 1, state)
    F.random_advance(state)
    second = fill(33, 0, 0, 0.0, 1, state)
    assert np.array_equal(first.astype(np.float64), R.expected(0, 9, 41, 1, 0, 33))
    assert np.array_equal(second.astype(np.float64), R.expected(0, 9, 42, 1, 0, 33))
    assert state.cpu().tolist() == [9, 0, 42, 0]
    state[0] = 10                                                      # a new seed in the state: nothing else is called
    assert np.array_equal(fill(33, 0, 0, 0.0, 1, state).astype(np.float64), R.expected(0, 10, 42, 1, 0, 33))
    # the functional form: a constant Var of the given shape
    z = F.random_fill((4, 10), 1, 0.5, 0, state, first=40)
    assert tuple(z.shape) == (4, 10) and not z.requires_grad
    assert np.abs(z.data.cpu().numpy().reshape(-1) - R.expected(1, 10, 42, 0, 40, 40, 0.5)).max() <= NORMAL_ATOL


def test_a_captured_chain_replays_as_consecutive_iterations():
    """The three fills + the advance on one stream (a linear chain) in a HIP graph: replay k draws iteration t + k."""
    from srgan_amd import functional as F
    state = make_state(7, 100)
    F.random_fill((4,), 0, 0.0, 1, state)                              # the library's kernels are loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z_d = F.random_fill((4, 10), 1, 0.5, 0, state)
        alpha = F.random_fill((4,), 0, 0.0, 1, state)
        z_g = F.random_fill((4, 10), 1, 0.0, 2, state)
        F.random_advance(state)
    assert state.cpu().tolist()[2] == 100                              # capturing recorded the launches, it did not run them
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        t = 100 + replay
        assert np.abs(z_d.data.cpu().numpy().reshape(-1) - R.expected(1, 7, t, 0, 0, 40, 0.5)).max() <= NORMAL_ATOL
        assert np.array_equal(alpha.data.cpu().numpy().astype(np.float64), R.expected(0, 7, t, 1, 0, 4))
        assert np.abs(z_g.data.cpu().numpy().reshape(-1) - R.expected(1, 7, t, 2, 0, 40)).max() <= NORMAL_ATOL
        assert state.cpu().tolist()[2] == t + 1


# ---- experiments ------------------------------------------------------------------------------------------------------------
def coefficient_experiment(**overrides):
    """Tiny coefficient MLPs: only the draw shapes matter, and G.input_size = 10 makes the windows ragged."""
    from srgan_amd.coefficient.models import MLP, Generator
    experiment = make_experiment(lambda: (Generator(10), MLP(10), MLP(10)),
                                 dict(batch_size=4, device_random_draws=True, device_random_seed=SEED, mean_offset=0.5,
                                      steps_to_run=10 ** 9, **overrides))
    finish_setup(experiment)
    return experiment


def coefficient_inputs(generator, batch=4):
    return (torch.randn(batch, 50, generator=generator).cuda(), torch.randn(batch, generator=generator).cuda(),
            torch.randn(batch, 50, generator=generator).cuda())


def record_samples(experiment, monkeypatch):
    """The tensors the three ``sample_*`` methods return, per call; ``draw_*`` must never be called."""
    seen = {'z_d': [], 'alpha': [], 'z_g': []}

    def refuse(*arguments, **keywords):
        raise AssertionError('a host draw was made')
    for name in ('draw_discriminator_noise', 'draw_interpolation_alpha', 'draw_generator_noise'):
        monkeypatch.setattr(experiment, name, refuse)
    def recording(key, original):
        def sample(batch):
            var = original(batch)
            seen[key].append(var)
            return var
        return sample
    for key, name in (('z_d', 'sample_discriminator_noise'), ('alpha', 'sample_interpolation_alpha'),
                      ('z_g', 'sample_generator_noise')):
        monkeypatch.setattr(experiment, name, recording(key, getattr(experiment, name)))
    return seen


def host(var):
    return var.data.cpu().numpy().astype(np.float64).reshape(-1)


def check_iteration(seen, index, iteration, batch=4, columns=10, offset=0.5, z_g_index=None):
    assert np.abs(host(seen['z_d'][index]) - R.expected(1, SEED, iteration, 0, 0, batch * columns, offset)).max() <= NORMAL_ATOL
    assert np.array_equal(host(seen['alpha'][index]), R.expected(0, SEED, iteration, 1, 0, batch))
    if z_g_index is not None:
        assert np.abs(host(seen['z_g'][z_g_index]) - R.expected(1, SEED, iteration, 2, 0, batch * columns)).max() <= NORMAL_ATOL


def test_the_three_samples_of_each_iteration_are_the_reference_draws(monkeypatch):
    experiment = coefficient_experiment()
    seen = record_samples(experiment, monkeypatch)
    generator = torch.Generator().manual_seed(3)
    for step in range(3):
        x, y, u = coefficient_inputs(generator)
        experiment.dnn_training_step(x, y, step)
        experiment.gan_training_step(x, y, u, step)
    torch.cuda.synchronize()
    assert [len(seen[key]) for key in ('z_d', 'alpha', 'z_g')] == [3, 3, 3]
    assert tuple(seen['z_d'][0].shape) == (4, 10) and tuple(seen['alpha'][0].shape) == (4,)
    for step in range(3):
        check_iteration(seen, step, experiment.starting_step + step, z_g_index=step)
    assert experiment.device_draw_state().cpu().tolist()[2] == 3


def test_a_generator_period_of_two_skips_z_g_and_keeps_the_iteration_count(monkeypatch):
    experiment = coefficient_experiment(generator_training_step_period=2)
    seen = record_samples(experiment, monkeypatch)
    generator = torch.Generator().manual_seed(3)
    for step in range(4):
        x, y, u = coefficient_inputs(generator)
        experiment.dnn_training_step(x, y, step)
        experiment.gan_training_step(x, y, u, step)
    torch.cuda.synchronize()
    assert [len(seen[key]) for key in ('z_d', 'alpha', 'z_g')] == [4, 4, 2]             # z_G is not filled on the odd steps
    for step in range(4):
        check_iteration(seen, step, step, z_g_index=step // 2 if step % 2 == 0 else None)


def test_an_injected_draw_still_takes_precedence(monkeypatch):
    experiment = coefficient_experiment()
    seen = record_samples(experiment, monkeypatch)
    generator = torch.Generator().manual_seed(3)
    x, y, u = coefficient_inputs(generator)
    injected = torch.full((4, 10), 0.25)
    experiment.injected_draws = {'z_d': injected, 'z_g': None, 'alpha': None}
    experiment.dnn_training_step(x, y, 0)
    experiment.gan_training_step(x, y, u, 0)
    torch.cuda.synchronize()
    assert np.array_equal(host(seen['z_d'][0]), injected.numpy().reshape(-1))
    assert np.array_equal(host(seen['alpha'][0]), R.expected(0, SEED, 0, 1, 0, 4))     # the others still come from the device
    assert np.abs(host(seen['z_g'][0]) - R.expected(1, SEED, 0, 2, 0, 40)).max() <= NORMAL_ATOL


def test_a_resumed_run_continues_the_stream(monkeypatch):
    fresh = coefficient_experiment()
    seen_fresh = record_samples(fresh, monkeypatch)
    generator = torch.Generator().manual_seed(3)
    for step in range(4):
        x, y, u = coefficient_inputs(generator)
        fresh.gan_training_step(x, y, u, step)
    resumed = coefficient_experiment()
    resumed.starting_step = 3
    seen_resumed = record_samples(resumed, monkeypatch)
    x, y, u = coefficient_inputs(generator)
    resumed.gan_training_step(x, y, u, 3)
    torch.cuda.synchronize()
    assert np.array_equal(host(seen_resumed['z_d'][0]), host(seen_fresh['z_d'][3]))    # its first z_D = the fourth of a run from 0
    assert not np.array_equal(host(seen_resumed['z_d'][0]), host(seen_fresh['z_d'][0]))


def dcgan_experiment(**overrides):
    """age.models at 16 x 16, conv_dim 8, batch 4: the scale of golden g16."""
    from srgan_amd.age.models import Generator, Discriminator
    settings = dict(batch_size=4, matching_loss_multiplier=1e2, contrasting_loss_multiplier=1e1, gradient_penalty_multiplier=1e2,
                    mean_offset=0.5, steps_to_run=10 ** 9)
    settings.update(overrides)
    experiment = make_experiment(lambda: (Generator(image_size=16, conv_dim=8), Discriminator(16, 8), Discriminator(16, 8)),
                                 settings)
    with torch.no_grad():
        for module in experiment.D.modules():
            if isinstance(module, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                module.weight.mul_(4.0)                                # gradient penalty active
    finish_setup(experiment)
    for optimizer in (experiment.d_optimizer, experiment.g_optimizer, experiment.dnn_optimizer):
        optimizer.count_on_device()        # every run through the device-counted Adam entry point (a captured update needs it)
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.summary_period, writer.steps_to_run = 10 ** 9, 10 ** 9
    return experiment


def dcgan_inputs(generator, batch=4, size=16):
    return (torch.rand(batch, 3, size, size, generator=generator).cuda() * 2 - 1, torch.rand(batch, generator=generator).cuda(),
            torch.rand(batch, 3, size, size, generator=generator).cuda() * 2 - 1)


def run_dcgan(iterations, draws_of=None, **overrides):
    """``iterations`` training iterations (steps 1 ..: no summary step); ``draws_of``: per iteration, the (z_d, alpha, z_g)
    to inject.  Returns the experiment, the six losses per iteration and the tensors the ``sample_*`` methods returned."""
    experiment = dcgan_experiment(**overrides)
    seen = []
    originals = {key: getattr(experiment, name) for key, name in (
        ('z_d', 'sample_discriminator_noise'), ('alpha', 'sample_interpolation_alpha'), ('z_g', 'sample_generator_noise'))}
    if draws_of is None and not overrides.get('step_graph'):
        def recording(key):
            def sample(batch):
                var = originals[key](batch)
                seen[-1][key] = var.data.clone()
                return var
            return sample
        experiment.sample_discriminator_noise = recording('z_d')
        experiment.sample_interpolation_alpha = recording('alpha')
        experiment.sample_generator_noise = recording('z_g')
    generator = torch.Generator().manual_seed(11)
    losses = []
    for step in range(1, iterations + 1):
        x, y, u = dcgan_inputs(generator)
        seen.append({})
        if draws_of is not None:
            experiment.injected_draws = dict(draws_of[step - 1])
        experiment.training_iteration(x, y, u, step)
        losses.append({name: float(value.item()) for name, value in experiment.last_losses.items()
                       if value is not None and name in LOSSES})
    torch.cuda.synchronize()
    return experiment, losses, seen


def assert_same_training(a, a_losses, b, b_losses):
    for step, (first, second) in enumerate(zip(a_losses, b_losses)):
        assert first == second, f'iteration {step}: {first} vs {second}'           # the six losses, bit for bit
    assert len(a_losses[-1]) == 6 and all(np.isfinite(value) for value in a_losses[-1].values())
    for name in ('D', 'DNN', 'G'):
        x, y = getattr(a, name)._srgan_arena.data, getattr(b, name)._srgan_arena.data
        assert torch.equal(x, y), (name, float((x - y).abs().max()))
    for x, y in ((a.d_optimizer, b.d_optimizer), (a.g_optimizer, b.g_optimizer), (a.dnn_optimizer, b.dnn_optimizer)):
        assert x.step_count == y.step_count
        assert torch.equal(x.exp_avg, y.exp_avg) and torch.equal(x.exp_avg_sq, y.exp_avg_sq)


@pytest.fixture(scope='module')
def eager_device_run():
    """Five eager iterations of the tiny DCGAN with device draws: the run the injected and the replayed runs must equal."""
    return run_dcgan(5, device_random_draws=True, device_random_seed=SEED)


def test_device_draws_equal_the_same_tensors_injected(eager_device_run):
    """Ties the new path to the one every golden test covers: the tensors the device drew, handed in through
    ``injected_draws`` with the setting off, give the same losses, weights and Adam moments, bit for bit."""
    device, device_losses, seen = eager_device_run
    assert device_losses[-1]['gradient_penalty'] > 0.0 and device_losses[-1] != device_losses[-2]
    for step, draws in enumerate(seen):
        assert np.abs(host_tensor(draws['z_d']) - R.expected(1, SEED, step, 0, 0, 4 * 256, 0.5)).max() <= NORMAL_ATOL
        assert np.array_equal(host_tensor(draws['alpha']), R.expected(0, SEED, step, 1, 0, 4))
    injected, injected_losses, _ = run_dcgan(5, draws_of=seen)
    assert injected._draw_state is None
    assert_same_training(device, device_losses, injected, injected_losses)


def host_tensor(tensor):
    return tensor.cpu().numpy().astype(np.float64).reshape(-1)


def test_replayed_iterations_with_device_draws_equal_the_eager_ones(eager_device_run, monkeypatch):
    """step_graph on one stream: the fills and the advance are captured with the step, nothing is drawn on the host."""
    from srgan_amd.srgan import Experiment
    eager, eager_losses, _ = eager_device_run

    def refuse(*arguments, **keywords):
        raise AssertionError('a host draw was made')
    for name in ('draw_discriminator_noise', 'draw_interpolation_alpha', 'draw_generator_noise'):
        monkeypatch.setattr(Experiment, name, refuse)
    replayed, replayed_losses, _ = run_dcgan(5, device_random_draws=True, device_random_seed=SEED, step_graph=True,
                                             step_graph_warmup=1)
    captured = replayed._captured_iteration
    assert captured.eager_iterations == 1 and captured.replays == 4 and len(captured.records) == 1
    assert all(record['draws'] == {} for record in captured.records.values())
    assert replayed.device_draw_state().cpu().tolist()[2] == 5
    assert_same_training(eager, eager_losses, replayed, replayed_losses)


def test_one_step_on_bf16_storage_runs_and_is_finite():
    """The draws are fp32 tensors in front of ``blocked16.pack``; nothing else changes."""
    experiment, losses, seen = run_dcgan(1, device_random_draws=True, device_random_seed=SEED, storage_dtype='bf16',
                                         compute_dtype='bf16', gradient_penalty_dtype='bf16')
    assert len(losses[0]) == 6 and all(np.isfinite(value) for value in losses[0].values())
    assert seen[0]['z_d'].dtype == torch.float32 and tuple(seen[0]['z_d'].shape) == (4, 256)
    for name in ('D', 'DNN', 'G'):
        assert bool(torch.isfinite(getattr(experiment, name)._srgan_arena.data).all())
