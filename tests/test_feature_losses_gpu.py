"""The alternative feature losses on the MI355X: ``F.acos`` / ``F.clamp`` to second order, the three composed losses and the
fused correlation loss (csrc/feature_losses.hip) against the fixture recorded from the reference (golden/g19) and the tests'
NumPy restatement (feature_losses_reference.py), the kernel's tile edges, capacity, repeatability, graph capture, null
gradient pointers, and tiny coefficient experiments that select the losses through ``settings.matching_feature_loss`` /
``settings.contrasting_feature_loss``.

Tolerances.  Correlation loss, value: an fp32 dot product of B normalised terms errs by at most about (4 B + 16) 2^-24 per
entry (Cauchy-Schwarz), so |loss - golden| <= F (F - 1) (4 B + 16) 2^-24.  Its gradients: 8 x the max-abs error of the
reference's own float32 gradients (stored in g19), floor 1e-6 max|golden| -- another summation order and the MFMA's
accumulation.  Composed losses: every quantity is a sum of at most B F fp32 terms, (B F + 64) 2^-24 relative to the largest
golden magnitude (+ 64 for the other roundings of a chain).  acos / clamp: see the tests."""
import gc

import numpy as np
import pytest
import torch

import feature_losses_reference as R
from helpers import Guarded, assert_close, golden_scalars, golden_state, load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float('nan')


@pytest.fixture(scope='module')
def g19():
    return load_golden('g19_feature_losses')


def shape_keys(g19, group='gradient_shapes'):
    return ['%dx%d' % tuple(shape) for shape in g19[group]]


def dev(array):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).cuda()


def bits(tensor):
    return tensor.detach().cpu().contiguous().view(torch.int32)


def entry_bound(batch):
    return (4 * batch + 16) * U


# ---- the raw entry points: every output in a NaN-filled, guarded buffer ---------------------------------------------------
def fused(base, other, want_base=True, want_other=True, upstream=1.0):
    """(loss, grad_base, grad_other, saved) of one _fwd + _bwd through the C ABI; a gradient that was not asked for is None."""
    from srgan_amd import _lib
    library = _lib.library()
    batch, features = base.shape
    x, y = dev(base), dev(other)
    nbytes = library.srgan_feature_corrcoef_l1_scratch_bytes(batch, features)
    assert nbytes > 0
    scratch = Guarded(nbytes // 4)
    loss, saved = Guarded(1), Guarded(6 * features)
    stream = _lib.stream_handle()
    _lib.check(library.srgan_feature_corrcoef_l1_fwd(x.data_ptr(), y.data_ptr(), loss.ptr, saved.ptr, scratch.ptr, batch, features,
                                                     stream), 'fwd')
    g = dev(np.array([upstream]))
    grads = [Guarded(batch * features) if wanted else None for wanted in (want_base, want_other)]
    _lib.check(library.srgan_feature_corrcoef_l1_bwd(x.data_ptr(), y.data_ptr(), saved.ptr, scratch.ptr, g.data_ptr(),
                                                     grads[0].ptr if want_base else None, grads[1].ptr if want_other else None,
                                                     batch, features, stream), 'bwd')
    scratch.result('scratch')
    out = [loss.result('loss').cpu().numpy().copy()[0]]
    out += [None if grad is None else grad.result('gradient', (batch, features)).cpu().numpy().copy() for grad in grads]
    return out + [saved.result('saved', (2, 3, features)).cpu().numpy().copy()]


def loss_only(base, other):
    from srgan_amd import functional as F
    return float(F.feature_corrcoef_l1(F.constant(dev(base)), F.constant(dev(other))).data.cpu()[0])


# ---- acos and clamp -------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 5003)                # 5003: five workgroups of 1024 elements and a ragged tail


@pytest.mark.parametrize('n', SIZES)
def test_acos_to_second_order(n):
    """|x| <= 0.95, so 1 - x^2 >= 0.0975: each of the ~10 fp32 operations of a chain adds at most half an ulp, amplified by at
    most 1 / (1 - x^2) <= 10.3 -- 64 x 2^-23 relative to the largest magnitude of the result (acosf itself: 2 ulp)."""
    from srgan_amd import functional as F
    from srgan_amd.tape import backward
    generator = torch.Generator().manual_seed(n)
    x_host = torch.rand(n, generator=generator) * 1.9 - 0.95
    g_host, h_host = torch.randn(n, generator=generator), torch.randn(n, generator=generator)
    x, g = F.leaf(x_host.cuda(), requires_grad=True), F.leaf(g_host.cuda(), requires_grad=True)
    y = F.acos(x)
    gx, = backward(y, grad=g, inputs=[x], create_graph=True)
    ggx, ggg = backward(gx, grad=F.constant(h_host.cuda()), inputs=[x, g])
    x64, g64 = x_host.double().requires_grad_(), g_host.double().requires_grad_()
    y64 = torch.acos(x64)
    gx64, = torch.autograd.grad(y64, x64, g64, create_graph=True)
    ggx64, ggg64 = torch.autograd.grad(gx64, [x64, g64], h_host.double())
    for name, got, want in (('acos', y, y64), ('first', gx, gx64), ('second/x', ggx, ggx64), ('second/g', ggg, ggg64)):
        want = want.detach().numpy()
        error = np.abs(got.data.cpu().numpy().astype(np.float64) - want).max()
        print(f'[acos n={n}] {name}: max error {error:.3e}, bound {64 * 2 * U * np.abs(want).max():.3e}')
        assert error <= 64 * 2 * U * np.abs(want).max(), name


@pytest.mark.parametrize('n', SIZES)
def test_clamp_to_second_order_with_inclusive_edges(n):
    """Exact: a selection, and a gradient times a 0 / 1 mask.  The elements AT low and AT high pass the gradient, as in torch."""
    from srgan_amd import functional as F
    from srgan_amd.tape import backward
    low, high = -1.0 + 1e-6, 0.75
    generator = torch.Generator().manual_seed(100 + n)
    x_host = torch.randn(n, generator=generator) * 1.2
    edges = torch.tensor([low, high, NAN], dtype=torch.float32)        # (the fp32 the kernel compares with)
    edges = torch.cat([edges, torch.nextafter(edges[:2], torch.tensor([-2.0, 2.0]))])
    x_host[:min(n, 5)] = edges[:min(n, 5)]
    g_host, h_host = torch.randn(n, generator=generator), torch.randn(n, generator=generator)
    x, g = F.leaf(x_host.cuda(), requires_grad=True), F.leaf(g_host.cuda(), requires_grad=True)
    y = F.clamp(x, low, high)
    gx, = backward(y, grad=g, inputs=[x], create_graph=True)
    ggg, = backward(gx, grad=F.constant(h_host.cuda()), inputs=[g])
    x_t, g_t = x_host.clone().requires_grad_(), g_host.clone().requires_grad_()
    y_t = torch.clamp(x_t, low, high)
    gx_t, = torch.autograd.grad(y_t, x_t, g_t, create_graph=True)
    ggg_t, = torch.autograd.grad(gx_t, g_t, h_host)
    assert torch.equal(bits(y.data), bits(y_t))                        # (bits: the NaN stays the NaN it was)
    for name, got, want in (('first', gx, gx_t), ('second', ggg, ggg_t)):
        assert torch.equal(got.data.cpu(), want.detach()), name        # (values: a masked gradient is g * 0 here, a selected 0 in torch)
    if n >= 5:
        passed = (gx.data.cpu() != 0)[:5].tolist()
        assert passed == [True, True, False, False, False]             # low, high | NaN, below low, above high


# ---- the composed losses --------------------------------------------------------------------------------------------------
def composed(name):
    from srgan_amd import srgan
    return {'angle': srgan.feature_angle_loss, 'unmeaned': srgan.feature_distance_loss_unmeaned,
            'both_unmeaned': srgan.feature_distance_loss_both_unmeaned, 'covariance': srgan.feature_covariance_loss}[name]


def tape_loss(function, base, other, gradients=True):
    from srgan_amd import functional as F
    from srgan_amd.tape import backward
    x, y = F.leaf(dev(base), requires_grad=gradients), F.leaf(dev(other), requires_grad=gradients)
    loss = function(x, y)
    assert loss.numel() == 1
    if not gradients:
        return float(loss.data.cpu().reshape(-1)[0]), None, None
    grad_base, grad_other = backward(loss, inputs=[x, y])
    return float(loss.data.cpu().reshape(-1)[0]), grad_base.data.cpu().numpy(), grad_other.data.cpu().numpy()


@pytest.mark.parametrize('name', ['angle', 'unmeaned', 'both_unmeaned'])
def test_the_composed_losses_against_the_reference(g19, name):
    checked = 0
    for key in shape_keys(g19) + shape_keys(g19, 'loss_only_shapes'):
        base, other = g19[f'{key}/base'], g19[f'{key}/other']
        with_gradients = f'{key}/{name}/grad_base' in g19
        value, grad_base, grad_other = tape_loss(composed(name), base, other, with_gradients)
        relative = (base.size + 64) * U                                # (64: the few dozen other roundings of a chain, an ulp each)
        want = float(g19[f'{key}/{name}/value'])
        print(f'[{name} {key}] value {value:.9g} vs {want:.9g}: {abs(value - want) / abs(want):.2e} of {relative:.2e}')
        assert abs(value - want) <= relative * abs(want), key
        if with_gradients:
            for side, got in (('grad_base', grad_base), ('grad_other', grad_other)):
                expected = g19[f'{key}/{name}/{side}']
                error = np.abs(got - expected).max() / np.abs(expected).max()
                print(f'[{name} {key}] {side}: {error:.2e} of {relative:.2e}')
                assert got.shape == expected.shape and error <= relative, (key, side)
            checked += 1
    assert checked >= 4


def test_parallel_means_sit_on_the_clamp_of_the_angle(g19):
    """The fp32 clamp bound is fl(1 - 1e-6) = 1 - 1.0133e-6, whose acos differs from the fp64 one by 0.7 %: the value is
    compared with the reference's own FLOAT32 run (the same bound, acosf to a few ulp); the gradients are exactly 0."""
    from srgan_amd import functional as F, srgan
    base, other = g19['parallel/base'], g19['parallel/other']
    value, grad_base, grad_other = tape_loss(srgan.feature_angle_loss, base, other)
    want = float(g19['parallel/angle/value_f32'])
    assert abs(value - want) <= 16 * U * want and not grad_base.any() and not grad_other.any()
    assert not g19['parallel/angle/grad_base'].any() and not g19['parallel/angle/grad_other'].any()
    angle = srgan.angle_between(F.constant(dev(base.mean(0))), F.constant(dev(other.mean(0))))
    assert abs(float(angle.data.cpu()[0]) - np.sqrt(want)) <= 16 * U * np.sqrt(want)
    unit = srgan.unit_vector(F.constant(dev(base[0])))
    assert_close(unit.data.cpu().numpy(), base[0].astype(np.float64) / np.linalg.norm(base[0].astype(np.float64)), rtol=1e-6, atol=1e-7)
    assert torch.equal(srgan.square(F.constant(dev(base))).data.cpu(), torch.from_numpy(base) ** 2)


def test_the_materialised_corrcoef(g19):
    """``feature_corrcoef`` / ``corrcoef`` (F.mm and elementwise tape operations) against the restatement's matrix, entry by
    entry within the dot-product bound, and differentiable through the tape."""
    from srgan_amd import functional as F, srgan
    from srgan_amd.tape import backward
    base = g19['17x70/base']
    want = R.corrcoef_rows(base, 0, 70)
    x = F.leaf(dev(base), requires_grad=True)
    matrix = srgan.feature_corrcoef(x)
    assert tuple(matrix.shape) == (70, 70)
    assert np.abs(matrix.data.cpu().numpy() - want).max() <= entry_bound(17)
    transposed = srgan.corrcoef(F.constant(dev(base.T)))
    assert np.abs(transposed.data.cpu().numpy() - want).max() <= entry_bound(17)
    gradient, = backward(F.sum_all(F.abs_(F.sub(matrix, srgan.feature_corrcoef(F.constant(dev(g19['17x70/other'])))))), inputs=[x])
    expected = g19['17x70/covariance/grad_base']
    assert np.abs(gradient.data.cpu().numpy() - expected).max() <= 1e-3 * np.abs(expected).max()


# ---- the fused correlation loss -------------------------------------------------------------------------------------------
def test_the_fixture_keeps_every_entry_away_from_a_sign_flip(g19):
    for key in shape_keys(g19):
        assert float(g19[f'{key}/min_gap']) >= 1e-5, key


@pytest.mark.parametrize('index', range(6))
def test_the_fused_loss_against_the_reference(g19, index):
    key = shape_keys(g19)[index]
    assert float(g19[f'{key}/min_gap']) >= 1e-5
    base, other = g19[f'{key}/base'], g19[f'{key}/other']
    batch, features = base.shape
    loss, grad_base, grad_other, saved = fused(base, other)
    want = float(g19[f'{key}/covariance/value'])
    bound = features * (features - 1) * entry_bound(batch)
    print(f'[fused {key}] loss {loss:.9g} vs {want:.9g}: error {abs(float(loss) - want):.3e}, bound {bound:.3e}; the reference in fp32: '
          f'{abs(float(g19[f"{key}/covariance/value_f32"]) - want):.3e}')
    assert abs(float(loss) - want) <= bound
    for side, got in (('grad_base', grad_base), ('grad_other', grad_other)):
        expected = g19[f'{key}/covariance/{side}']
        reference_error = np.abs(g19[f'{key}/covariance/{side}_f32'].astype(np.float64) - expected).max()
        tolerance = max(8.0 * reference_error, 1e-6 * np.abs(expected).max())
        error = np.abs(got.astype(np.float64) - expected).max()
        print(f'[fused {key}] {side}: max error {error:.3e} = {error / reference_error:.2f} x the reference\'s fp32 error '
              f'{reference_error:.3e} (tolerance {tolerance:.3e})')
        assert np.isfinite(got).all() and error <= tolerance, (key, side)
    means = np.stack([base.astype(np.float64).mean(0), other.astype(np.float64).mean(0)])
    assert np.abs(saved[:, 0] - means).max() <= (batch + 16) * U * max(1.0, np.abs(means).max())


@pytest.mark.parametrize('index', range(2))
def test_the_fused_loss_alone_against_the_reference(g19, index):
    key = shape_keys(g19, 'loss_only_shapes')[index]
    base, other = g19[f'{key}/base'], g19[f'{key}/other']
    batch, features = base.shape
    loss = loss_only(base, other)
    error = abs(loss - float(g19[f'{key}/covariance/value']))
    print(f'[fused {key}] loss {loss:.9g}: error {error:.3e}, bound {features * (features - 1) * entry_bound(batch):.3e}')
    assert error <= features * (features - 1) * entry_bound(batch)


@pytest.mark.parametrize('k', [0, 31, 32, 63, 64, 69])
def test_one_changed_column_reaches_only_its_row_and_column(k):
    """other = base except column k: every entry outside row and column k is exactly 0 on both sides, so the loss is twice
    the sum over row k -- an entry attributed to a wrong feature at a tile edge (waves own 32 features) shows."""
    generator = np.random.default_rng(5)
    base = generator.standard_normal((17, 70)).astype(np.float32)
    other = base.copy()
    other[:, k] = generator.standard_normal(17).astype(np.float32)
    row = np.delete(R.corrcoef_rows(base, k, k + 1)[0] - R.corrcoef_rows(other, k, k + 1)[0], k)
    loss = loss_only(base, other)
    assert abs(loss - 2.0 * np.abs(row).sum()) <= 2 * 69 * entry_bound(17)
    assert abs(2.0 * np.abs(row).sum() - R.covariance_loss(base, other, gradients=False)[0]) <= 1e-12


def test_equal_arguments_give_exactly_zero_and_swapped_ones_the_same_loss(g19):
    base, other = g19['33x130/base'], g19['33x130/other']
    assert loss_only(base, base) == 0.0 and loss_only(other, other) == 0.0
    want = R.covariance_loss(other, base, gradients=False)[0]
    assert abs(loss_only(other, base) - want) <= 130 * 129 * entry_bound(33)


def test_a_constant_column_gives_nan_and_a_duplicated_one_a_finite_loss(g19):
    base, other = g19['17x70/base'].copy(), g19['17x70/other']
    duplicated = base.copy()
    duplicated[:, 40] = duplicated[:, 3]
    loss, grad_base, grad_other, _ = fused(duplicated, other)
    assert np.isfinite(loss) and np.isfinite(grad_base).all() and np.isfinite(grad_other).all()
    assert abs(float(loss) - R.covariance_loss(duplicated, other, gradients=False)[0]) <= 70 * 69 * entry_bound(17)
    base[:, 33] = 0.5
    loss, grad_base, grad_other, _ = fused(base, other)
    assert np.isnan(loss) and np.isnan(grad_base).all() and np.isnan(grad_other).all()


def test_capacity_8192_features_against_the_blockwise_restatement():
    generator = torch.Generator().manual_seed(8192)
    base = torch.randn(16, 8192, generator=generator).numpy()
    other = (1.5 * torch.randn(16, 8192, generator=generator) + 0.3).numpy()
    want = R.covariance_loss(base, other, gradients=False, block=1024)[0]
    loss = loss_only(base, other)
    print(f'[fused 16x8192] loss {loss:.9g} vs {want:.9g}: error {abs(loss - want):.3e}, bound {8192 * 8191 * entry_bound(16):.3e}')
    assert abs(loss - want) <= 8192 * 8191 * entry_bound(16)


def test_capacity_32768_features_and_the_first_shape_beyond():
    from srgan_amd import _lib, functional as F
    generator = torch.Generator().manual_seed(32768)
    base = torch.randn(16, 32768, generator=generator).cuda()
    other = (1.5 * torch.randn(16, 32768, generator=generator) + 0.3).cuda()
    loss = float(F.feature_corrcoef_l1(F.constant(base), F.constant(other)).data.cpu()[0])
    assert np.isfinite(loss) and loss > 0.0
    assert float(F.feature_corrcoef_l1(F.constant(base), F.constant(base)).data.cpu()[0]) == 0.0
    with pytest.raises(_lib.HipLibraryError, match='capacity') as refused:
        F.feature_corrcoef_l1(F.constant(torch.zeros(8193, 10).cuda()), F.constant(torch.zeros(8193, 10).cuda()))
    assert refused.value.status == _lib.ERANGE
    with pytest.raises(_lib.HipLibraryError) as refused:
        F.feature_corrcoef_l1(F.constant(torch.zeros(1, 10).cuda()), F.constant(torch.zeros(1, 10).cuda()))
    assert refused.value.status == _lib.EINVAL


def test_two_calls_give_the_same_bits(g19):
    base, other = g19['130x40/base'], g19['130x40/other']
    first, second = fused(base, other, upstream=0.5), fused(base, other, upstream=0.5)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    generator = np.random.default_rng(3)                               # several column splits
    large, larger = (generator.standard_normal((40, 700)).astype(np.float32) for _ in range(2))
    again = [fused(large, larger) for _ in range(2)]
    for a, b in zip(*again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_only_the_requested_gradient_is_written(g19):
    """The generator's loss needs ``other`` only: the same bits as the other half of the full call, nothing for ``base``."""
    from srgan_amd import functional as F
    from srgan_amd.tape import backward
    base, other = g19['33x130/base'], g19['33x130/other']
    full = fused(base, other)
    only_other, only_base = fused(base, other, want_base=False), fused(base, other, want_other=False)
    assert only_other[1] is None and np.array_equal(only_other[2].view(np.int32), full[2].view(np.int32))
    assert only_base[2] is None and np.array_equal(only_base[1].view(np.int32), full[1].view(np.int32))
    x, y = F.constant(dev(base)), F.leaf(dev(other), requires_grad=True)
    loss = F.feature_corrcoef_l1(x, y)
    gradient, = backward(loss, inputs=[y])
    assert np.array_equal(gradient.data.cpu().numpy().view(np.int32), full[2].view(np.int32))
    assert float(loss.data.cpu()[0]) == full[0]


def test_the_backward_is_first_order_only(g19):
    from srgan_amd import functional as F
    from srgan_amd.tape import backward
    x, y = (F.leaf(dev(g19[f'5x33/{name}']), requires_grad=True) for name in ('base', 'other'))
    with pytest.raises(NotImplementedError, match='first-order'):
        backward(F.feature_corrcoef_l1(x, y), inputs=[x, y], create_graph=True)


def test_a_captured_forward_and_backward_replays_to_the_eager_bits(g19):
    from srgan_amd import functional as F
    from srgan_amd.tape import backward
    base, other = dev(g19['33x130/base']), dev(g19['33x130/other'])

    def run():
        x, y = F.leaf(base, requires_grad=True), F.leaf(other, requires_grad=True)
        loss = F.feature_corrcoef_l1(x, y)
        grad_base, grad_other = backward(loss, inputs=[x, y])
        return loss.data, grad_base.data, grad_other.data
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [tensor.clone() for tensor in run()]                   # (and the stream's workspace is registered)
        side.synchronize()
        gc.collect()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = run()
        for tensor in captured:
            tensor.fill_(NAN)
        graph.replay()
    side.synchronize()
    for got, want in zip(captured, eager):
        assert torch.equal(bits(got), bits(want))
    expected = fused(g19['33x130/base'], g19['33x130/other'])
    assert float(eager[0].cpu()[0]) == expected[0] and np.array_equal(eager[1].cpu().numpy().view(np.int32), expected[1].view(np.int32))


# ---- selecting the losses in a run ----------------------------------------------------------------------------------------
BATCH, SEED = 16, 2 ** 33 + 5


def negative_angle(base, other):
    from srgan_amd import functional as F, srgan
    return F.neg(srgan.feature_angle_loss(base, other))


def coefficient_experiment(hooks=True, direct=False, **overrides):
    """Hidden size 10, batch 16, the golden's initial weights.  ``direct``: the test calls ``dnn_training_step`` /
    ``gan_training_step`` itself, as the golden step tests do (every step logs, Adam counts on the host); otherwise the steps
    go through ``training_iteration`` (only step 0 is a summary step; the device-counted Adam a captured update needs)."""
    import srgan_amd  # noqa: F401
    from srgan_amd import srgan
    from srgan_amd.coefficient.models import MLP, Generator
    from srgan_amd.settings import Settings
    from srgan_amd.utility import SummaryWriter, seed_all

    class Small(srgan.Experiment):
        def dataset_setup(self):
            pass

        def model_setup(self):
            self.G, self.D, self.DNN = Generator(10), MLP(10), MLP(10)

        def validation_summaries(self, step):
            pass
    settings = Settings()
    values = dict(batch_size=BATCH, hidden_size=10, steps_to_run=10 ** 9, save_step_period=0)
    if hooks:
        values.update(matching_feature_loss=srgan.feature_covariance_loss, contrasting_feature_loss=negative_angle)
    values.update(overrides)
    for name, value in values.items():
        setattr(settings, name, value)
    experiment = Small(settings)
    seed_all(0)
    experiment.model_setup()
    g3 = load_golden('g3_coefficient_srgan')
    for module, prefix in ((experiment.D, 'init/D'), (experiment.DNN, 'init/DNN'), (experiment.G, 'init/G')):
        module.load_state_dict(golden_state(g3, prefix))
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    if not direct:
        for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
            writer.summary_period, writer.steps_to_run = 10 ** 9, 10 ** 9
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    if not direct:
        for optimizer in (experiment.d_optimizer, experiment.g_optimizer, experiment.dnn_optimizer):
            optimizer.count_on_device()
    experiment.train_mode()
    return experiment, g3


def rows(g3, step, name, count=BATCH):
    return np.ascontiguousarray(g3[f's{step}/{name}'][:count])


LOSS_NAMES = ('dnn_loss', 'labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss')


def run_iterations(experiment, g3, steps=3):
    """``training_iteration`` on the first 16 examples of the golden's batches, device draws; losses and weights per step."""
    losses, weights = [], []
    for step in range(steps):
        x, y, u = (dev(rows(g3, step, name)) for name in ('x', 'y', 'u'))
        experiment.training_iteration(x, y, u, step)
        losses.append({name: float(value.item()) for name, value in experiment.last_losses.items()
                       if value is not None and name in LOSS_NAMES})
        weights.append({name: getattr(experiment, name)._srgan_arena.data.clone() for name in ('D', 'DNN', 'G')})
    torch.cuda.synchronize()
    return losses, weights


@pytest.fixture(scope='module')
def hooked_run():
    experiment, g3 = coefficient_experiment(device_random_draws=True, device_random_seed=SEED)
    result = run_iterations(experiment, g3)
    print('[feature losses] losses of the hooked run:', result[0])
    assert all(np.isfinite(value) for losses in result[0] for value in losses.values()) and len(result[0][2]) == 6
    return result


def assert_same_bits(a, b):
    for step, (losses_a, losses_b) in enumerate(zip(a[0], b[0])):
        assert losses_a == losses_b, (step, losses_a, losses_b)
    for step, (weights_a, weights_b) in enumerate(zip(a[1], b[1])):
        for name in weights_a:
            assert torch.equal(weights_a[name], weights_b[name]), (step, name)


def test_two_hooked_runs_are_bit_identical_and_differ_from_the_plain_run(hooked_run):
    experiment, g3 = coefficient_experiment(device_random_draws=True, device_random_seed=SEED)
    assert_same_bits(hooked_run, run_iterations(experiment, g3))
    plain, _ = coefficient_experiment(hooks=False, device_random_draws=True, device_random_seed=SEED)
    assert run_iterations(plain, g3, steps=1)[0][0]['unlabeled_loss'] != hooked_run[0][0]['unlabeled_loss']


def test_a_replayed_graph_equals_the_eager_hooked_run(hooked_run):
    experiment, g3 = coefficient_experiment(device_random_draws=True, device_random_seed=SEED, step_graph=True, step_graph_warmup=1)
    result = run_iterations(experiment, g3)
    captured = experiment._captured_iteration
    assert captured.eager_iterations == 1 and captured.replays == 2
    assert_same_bits(hooked_run, result)


def test_the_hooked_run_on_the_four_stream_schedule(hooked_run):
    from srgan_amd import fused as fused_module
    saved = fused_module.WGRAD_STREAM
    try:
        experiment, g3 = coefficient_experiment(device_random_draws=True, device_random_seed=SEED, overlap_dnn_step=True,
                                                wgrad_stream=True, overlap_generator_forwards=True, overlap_gradient_penalty=True)
        losses, _ = run_iterations(experiment, g3)
    finally:
        fused_module.WGRAD_STREAM = saved
    for step in range(3):
        for name, value in hooked_run[0][step].items():
            assert_close(losses[step][name], value, rtol=1e-3, atol=1e-6 if abs(value) < 1e-3 else 0.0, what=f'step {step} {name}')


def test_without_the_settings_the_run_is_the_parents():
    """The golden the coefficient step tests use (batch 256), run by an experiment that never sets the two settings."""
    from test_steps_gpu import check, run_step
    experiment, g3 = coefficient_experiment(hooks=False, direct=True,
                                            batch_size=int(load_golden('g3_coefficient_srgan')['batch_size']))
    assert not any(hasattr(experiment.settings, name) for name in ('matching_feature_loss', 'contrasting_feature_loss'))
    for step in range(2):
        x, y, u = (dev(g3[f's{step}/{name}']) for name in ('x', 'y', 'u'))
        check(run_step(experiment, x, y, u, step, g3), golden_scalars(g3, step), f'g3 step {step}')


# The same step in torch autograd (fp64), with the two losses written in torch from their contracts.
def torch_correlation(x):
    xm = x - x.mean(0, keepdim=True)
    covariance = xm.t() @ xm / (x.shape[0] - 1)
    stddev = covariance.diagonal().sqrt()
    return (covariance / stddev[None, :] / stddev[:, None]).clamp(-1.0, 1.0)


def torch_covariance_loss(base, other, gaps):
    difference = torch_correlation(base) - torch_correlation(other)
    difference = difference - torch.diag(difference.diagonal())
    gaps.append(float((difference.detach().abs() + torch.eye(difference.shape[0], dtype=difference.dtype) * 9.0).min()))
    return difference.abs().sum()


def torch_negative_angle(base, other):
    def unit(vector):
        return vector / (vector.norm() + 1e-10)
    cosine = (unit(base.mean(0)) * unit(other.mean(0))).sum().clamp(-1.0 + 1e-6, 1.0 - 1e-6)
    return -(cosine.acos() - 0.0).abs().pow(2)


def test_step_zero_against_torch_autograd():
    """Losses and D's first-layer gradient of step 0 against the oracle's step in fp64 with the two losses in torch.  The step's
    tolerance (1e-3 relative, 1e-4 of the largest entry for gradients) is the one the coefficient step tests assert; the
    features keep every correlation entry 1e-4 away from a sign flip (asserted), 100 x the fp32 error of an entry."""
    from helpers import make_settings
    from oracle import models as OM
    from oracle.experiment import Draws, OracleExperiment
    experiment, g3 = coefficient_experiment(direct=True)
    gaps = []

    class Hooked(OracleExperiment):
        def _distance(self, base, other, distance=None):
            return torch_covariance_loss(base, other, gaps) if distance is None else torch_negative_angle(base, other)
    nets = OM.CoefficientMLP(10), OM.CoefficientMLP(10), OM.CoefficientGenerator(10)
    for module, prefix in zip(nets, ('init/D', 'init/DNN', 'init/G')):
        module.load_state_dict(golden_state(g3, prefix))
        module.double()
    oracle = Hooked(make_settings(batch_size=BATCH), *nets)
    x, y, u, z_d, z_g, alpha = (rows(g3, 0, name) for name in ('x', 'y', 'u', 'z_d', 'z_g', 'alpha'))
    oracle.dnn_training_step(*(torch.from_numpy(a).double() for a in (x, y)))
    expected = oracle.gan_training_step(*(torch.from_numpy(a).double() for a in (x, y, u)), 0,
                                        Draws(*(torch.from_numpy(a).double() for a in (z_d, z_g, alpha))))
    assert len(gaps) == 2 and min(gaps) >= 1e-4, gaps
    captured = {}
    original_step = experiment.d_optimizer.step

    def capturing_step():
        captured.update({name: parameter.grad.cpu().numpy().copy() for name, parameter in experiment.D.named_parameters()})
        original_step()
    experiment.d_optimizer.step = capturing_step
    experiment.injected_draws = {name: torch.from_numpy(value) for name, value in (('z_d', z_d), ('z_g', z_g), ('alpha', alpha))}
    experiment.dnn_training_step(dev(x), dev(y), 0)
    experiment.gan_training_step(dev(x), dev(y), dev(u), 0)
    torch.cuda.synchronize()
    got = {name: float(value.item()) for name, value in experiment.last_losses.items() if value is not None}
    for name in ('labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss'):
        print(f'[feature losses step 0] {name}: hip {got[name]:.9g}  torch {expected[name]:.9g}')
        assert_close(got[name], expected[name], rtol=1e-3, atol=1e-6 if abs(expected[name]) < 1e-3 else 0.0, what=name)
    want = oracle.d_grads['linear1.weight'].numpy()
    assert_close(captured['linear1.weight'], want, rtol=1e-3, atol=1e-4 * np.abs(want).max(), what='D linear1.weight gradient')


def test_gpu_mode_refuses_the_settings_under_a_world_of_two():
    from types import SimpleNamespace
    import srgan_amd  # noqa: F401
    from srgan_amd import srgan
    from srgan_amd.coefficient.models import MLP, Generator
    from srgan_amd.settings import Settings

    class Small(srgan.Experiment):
        def dataset_setup(self):
            pass

        def model_setup(self):
            self.G, self.D, self.DNN = Generator(10), MLP(10), MLP(10)

        def validation_summaries(self, step):
            pass
    for name, value, refused in (('matching_feature_loss', srgan.feature_covariance_loss, True),
                                 ('contrasting_feature_loss', negative_angle, True), ('matching_feature_loss', None, False)):
        settings = Settings()
        setattr(settings, name, value)
        experiment = Small(settings)
        experiment.model_setup()
        experiment.dp = SimpleNamespace(world_size=2, rank=0, active=True)
        if refused:
            with pytest.raises(NotImplementedError, match='one device only'):
                experiment.gpu_mode()
        else:
            experiment.gpu_mode()
