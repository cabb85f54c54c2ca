"""The frozen norm of the DCGAN discriminators on BLOCKED tensors (``srgan_h_frozen_norm_bwd``, ``blocked16.batch_norm_frozen``,
``nn.BatchNorm2d`` on blocked input, ``Discriminator(blocked_frozen_norm=True)``, ``settings.blocked_frozen_norm``) on the GPU.

1. The entry point on exact operands (the idiom of test_blocked_batch_norm_gpu.py): small integers and powers of two, so every
   result is a number of the storage type and every sum is exact in fp32 -- the kernel must reproduce torch's CPU result bit
   for bit in each of its modes; two runs of the sums are bit-identical.
2. The tape op against fp64 autograd to first order (all codes; the bounds of test_blocked_batch_norm_gpu.py) and to second
   order (code 0; 1e-3 of each tensor's scale, the project's fp32 bound); the module.
3. A discriminator with norms on blocked fp32 against the NCHW graph; golden g16 with D and DNN blocked, eager and replayed;
   the driving step on bf16 / fp16 storage."""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_close_norm, profiled
from test_blocked_batch_norm_gpu import (CODES, OP_RTOL, STORED_RTOL, _call, _compare_replay, _stream, from_blocked, integers, new_blocked,
                                         per_channel, rounded, to_blocked)

pytestmark = pytest.mark.gpu
LEAK = 0.05


@pytest.fixture(scope='module', autouse=True)
def pkg():
    import srgan_amd
    assert torch.cuda.is_available()
    return srgan_amd


def pointer(tensor):
    return None if tensor is None else tensor.data_ptr()


def abi_frozen(sb, shape, code, inv_std, gamma, xb=None, mean=None, refb=None, slope=1.0, want_gx=True, g_gamma=None, g_beta=None):
    """One ``srgan_h_frozen_norm_bwd`` call; returns the raw gx (an output buffer that started as NaN) or None."""
    n, c, h, w = shape
    gxb = new_blocked(shape, code) if want_gx else None
    _call('srgan_h_frozen_norm_bwd', sb.data_ptr(), pointer(xb), pointer(mean), inv_std.data_ptr(), gamma.data_ptr(), pointer(refb), slope,
          pointer(gxb), pointer(g_gamma), pointer(g_beta), n, c, h * w, code, _stream())
    return gxb


# ------------------------------------------------------------------------------------------------ 1. exact operands
# channel tails for g = 8 (3, 5, 12, 20) and g = 4 (3, 5), an odd plane, N = 1, M = N * H * W = 1 (legal here: nothing is divided
# by a count) and a shape with 1024 values per channel
EXACT_SHAPES = [(2, 3, 4, 8), (2, 5, 4, 8), (2, 12, 4, 8), (3, 5, 3, 5), (1, 8, 2, 2), (1, 3, 1, 1), (4, 20, 16, 16)]


def exact_operands(shape):
    """s, x, mean: integers of magnitude <= 8; gamma, inv_std: powers of two in [0.5, 4] (gamma of either sign).  |gx| <= 8 * 16
    with at most four significant bits and |sum| <= 1024 * 8 * 16 * 4 + 8: numbers of bf16 / fp16 and of fp32."""
    c = shape[1]
    pick = torch.tensor([0.5, 1.0, 2.0, 4.0])
    draw = lambda seed: pick[torch.randint(0, 4, (c,), generator=torch.Generator().manual_seed(seed))]
    sign = integers((c,), 0, 1, 13) * 2 - 1
    return dict(s=integers(shape, -8, 8, 11), x=integers(shape, -8, 8, 12), ref=integers(shape, -1, 1, 3), mean=integers((c,), -8, 8, 6),
                gamma=draw(4) * sign, inv_std=draw(7), old_gamma_grad=integers((c,), -8, 8, 9), old_beta_grad=integers((c,), -8, 8, 10))


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'ref'])
@pytest.mark.parametrize('slope', [1.0, 0.25])
@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda shape: 'x'.join(map(str, shape)))
@pytest.mark.parametrize('code', CODES)
def test_the_entry_point_is_exact_on_integers_in_every_mode(code, shape, slope, masked):
    given = exact_operands(shape)
    d = {key: value.cuda() for key, value in given.items()}
    sb, xb = to_blocked(given['s'], code), to_blocked(given['x'], code)
    refb = to_blocked(given['ref'], code) if masked else None
    s64, x64 = given['s'].double(), given['x'].double()
    want_gx = s64 * per_channel(given['gamma'] * given['inv_std']).double()
    if masked:
        want_gx = want_gx * torch.where(given['ref'] > 0, 1.0, slope).double()
    assert torch.equal(rounded(want_gx, code).double(), want_gx)                    # a number of the storage type
    want_beta = s64.sum(dim=(0, 2, 3))
    want_gamma = given['inv_std'].double() * (s64 * (x64 - per_channel(given['mean']).double())).sum(dim=(0, 2, 3))
    want_gamma_zero_mean = given['inv_std'].double() * (s64 * x64).sum(dim=(0, 2, 3))
    old_gamma, old_beta = given['old_gamma_grad'].double(), given['old_beta_grad'].double()
    for want in (want_beta, want_gamma, want_gamma_zero_mean):
        assert torch.equal(want.float().double(), want)

    # all three outputs in one pass; the sums are ADDED to what the buffers held
    gamma_grad, beta_grad = d['old_gamma_grad'].clone(), d['old_beta_grad'].clone()
    gxb = abi_frozen(sb, shape, code, d['inv_std'], d['gamma'], xb, d['mean'], refb, slope, True, gamma_grad, beta_grad)
    assert torch.equal(from_blocked(gxb, shape).cpu().double(), want_gx)            # (from_blocked: the tail channels are zero)
    assert torch.equal(gamma_grad.cpu().double(), old_gamma + want_gamma)
    assert torch.equal(beta_grad.cpu().double(), old_beta + want_beta)
    assert float(old_gamma.abs().max()) > 0 and float(old_beta.abs().max()) > 0

    # gx only (the recorded backward): x and mean are not needed, and nothing else is written
    gamma_grad, beta_grad = d['old_gamma_grad'].clone(), d['old_beta_grad'].clone()
    gxb = abi_frozen(sb, shape, code, d['inv_std'], d['gamma'], None, None, refb, slope, True, None, None)
    assert torch.equal(from_blocked(gxb, shape).cpu().double(), want_gx)
    assert torch.equal(gamma_grad, d['old_gamma_grad']) and torch.equal(beta_grad, d['old_beta_grad'])

    # the sums only, mean = NULL (the double backward's gamma gradient): no gx is written -- the call gets no such pointer
    gamma_grad, beta_grad = d['old_gamma_grad'].clone(), d['old_beta_grad'].clone()
    assert abi_frozen(sb, shape, code, d['inv_std'], d['gamma'], xb, None, refb, slope, False, gamma_grad, beta_grad) is None
    assert torch.equal(gamma_grad.cpu().double(), old_gamma + want_gamma_zero_mean)
    assert torch.equal(beta_grad.cpu().double(), old_beta + want_beta)

    # one sum at a time: the other buffer is not passed and keeps its contents; gx + g_gamma is the double backward's launch
    gamma_grad, beta_grad = d['old_gamma_grad'].clone(), d['old_beta_grad'].clone()
    gxb = abi_frozen(sb, shape, code, d['inv_std'], d['gamma'], None, None, refb, slope, True, None, beta_grad)
    assert torch.equal(from_blocked(gxb, shape).cpu().double(), want_gx)
    assert torch.equal(beta_grad.cpu().double(), old_beta + want_beta) and torch.equal(gamma_grad, d['old_gamma_grad'])
    beta_grad = d['old_beta_grad'].clone()
    abi_frozen(sb, shape, code, d['inv_std'], d['gamma'], None, None, None, 1.0, False, None, beta_grad)
    assert torch.equal(beta_grad.cpu().double(), old_beta + want_beta)
    gxb = abi_frozen(sb, shape, code, d['inv_std'], d['gamma'], xb, None, refb, slope, True, gamma_grad, None)
    assert torch.equal(from_blocked(gxb, shape).cpu().double(), want_gx)
    assert torch.equal(gamma_grad.cpu().double(), old_gamma + want_gamma_zero_mean) and torch.equal(beta_grad.cpu().double(), old_beta + want_beta)
    if shape[0] * shape[2] * shape[3] > 1:
        assert float(want_gamma.abs().max()) > 0 and float(want_gx.abs().max()) > 0
        assert not masked or slope == 1.0 or not torch.equal(want_gx, s64 * per_channel(given['gamma'] * given['inv_std']).double())


@pytest.mark.parametrize('code', CODES)
def test_two_runs_of_the_sums_are_bit_identical(code):
    """(8, 8, 64, 64): a channel group's 8 x 4096 slots are shared by several workgroups, whose partial sums meet in the stream's
    workspace.  That the launch really has more than one workgroup per channel group is read from the library's own profile
    record of the launch (kind 24: its `split` field is the number of workgroups per group)."""
    from srgan_amd import _lib
    shape = (8, 8, 64, 64)
    generator = torch.Generator().manual_seed(31)
    s, x = torch.randn(shape, generator=generator), torch.randn(shape, generator=generator) * 2 + 1
    mean, inv_std, gamma = (torch.randn(8, generator=generator).cuda(), (torch.rand(8, generator=generator) + 0.5).cuda(),
                            torch.randn(8, generator=generator).cuda())
    sb, xb = to_blocked(s, code), to_blocked(x, code)
    runs = []
    with profiled(_lib.library()) as report:
        for _ in range(2):
            gamma_grad, beta_grad = torch.zeros(8, device='cuda'), torch.zeros(8, device='cuda')
            gxb = abi_frozen(sb, shape, code, inv_std, gamma, xb, mean, None, 1.0, True, gamma_grad, beta_grad)
            torch.cuda.synchronize()
            runs.append((gamma_grad, beta_grad, gxb.float()))
    launches = [line for line in report.lines if line[3] == 24]
    assert launches and all(line[6] > 1 for line in launches), report.text
    for first, second in zip(*runs):
        assert torch.equal(first, second) and bool(torch.isfinite(first).all())
    want = (rounded(s, code).double() * (rounded(x, code).double() - per_channel(mean.cpu()).double())).sum(dim=(0, 2, 3)) * inv_std.cpu().double()
    assert_close_norm(runs[0][0].cpu().numpy(), want.numpy(), OP_RTOL, 'g_gamma')


# ------------------------------------------------------------------------------------------------ 2. tape and module
def _frozen_module(channels, seed):
    """A frozen norm with random statistics (mean != 0, variance in [0.5, 2]), gamma and beta."""
    from srgan_amd import nn
    generator = torch.Generator().manual_seed(seed)
    module = nn.BatchNorm2d(channels)
    with torch.no_grad():
        module.weight.copy_(torch.rand(channels, generator=generator) + 0.5)
        module.bias.copy_(torch.randn(channels, generator=generator))
        module.running_mean.copy_(torch.randn(channels, generator=generator) + 0.5)
        module.running_var.copy_(torch.rand(channels, generator=generator) * 1.5 + 0.5)
    return module, generator


def _reference_norm(module_state, x64, gamma64, beta64, slope, eps):
    pre = torch.nn.functional.batch_norm(x64, module_state['running_mean'].double(), module_state['running_var'].double(), gamma64, beta64,
                                         training=False, eps=eps)
    return torch.nn.functional.leaky_relu(pre, slope) if slope != 1.0 else pre


@pytest.mark.parametrize('code', CODES)
def test_the_tape_op_against_fp64_autograd(code):
    """``pack -> batch_norm_frozen(slope 0.25) -> unpack`` through a plain ``backward()``: y, the gradient of x and the gamma / beta
    gradients, added to a non-zero arena.  The inputs and the cotangent are numbers of the storage type, and so is the cotangent
    times 0.25: the pre-masked gradient the op receives is exact."""
    from srgan_amd import blocked16 as B, functional as F, nn
    from srgan_amd.tape import backward, no_grad
    shape, slope = (3, 12, 6, 10), 0.25
    module, generator = _frozen_module(shape[1], 21)
    state = {key: value.clone() for key, value in module.state_dict().items()}
    x = rounded(torch.randn(shape, generator=generator) * 2 + 1, code)
    cotangent = rounded(torch.randn(shape, generator=generator), code)
    arena = nn.flatten_parameters(module, torch.device('cuda', 0))
    old = torch.randn(arena.grad.shape, generator=generator)
    arena.grad.copy_(old)
    x64 = x.double().requires_grad_()
    gamma64, beta64 = (state[key].double().requires_grad_() for key in ('weight', 'bias'))
    want_y = _reference_norm(state, x64, gamma64, beta64, slope, module.eps)
    want = torch.autograd.grad(want_y, (x64, gamma64, beta64), cotangent.double())

    def forward(leaf):
        inv_std, mean = module._inverse_std()
        y = B.batch_norm_frozen(B.pack(leaf, code), mean, inv_std, nn.P(module.weight), nn.P(module.bias), slope=slope)
        assert y.meta.code == code and y.meta.mask_ref is y.data and y.meta.slope == slope
        return y

    leaf = F.leaf(x.cuda(), requires_grad=True)
    out = B.unpack(forward(leaf))
    print(f'code {code} y: max err {np.abs(out.cpu().numpy() - want_y.detach().numpy()).max():.3e} of {float(want_y.detach().abs().max()):.3e}')
    assert_close_norm(out.cpu().numpy(), want_y.detach().numpy(), STORED_RTOL[code], 'y')
    backward(F.sum_all(F.mul(out, F.leaf(cotangent.cuda()))))
    got_gamma = (module.weight.grad.cpu() - old[arena.offsets[0]:arena.offsets[0] + shape[1]]).numpy()
    got_beta = (module.bias.grad.cpu() - old[arena.offsets[1]:arena.offsets[1] + shape[1]]).numpy()
    for name, got, expected, bound in (('gx', leaf.grad.cpu().numpy(), want[0].numpy(), STORED_RTOL[code]),
                                       ('ggamma', got_gamma, want[1].numpy(), OP_RTOL), ('gbeta', got_beta, want[2].numpy(), OP_RTOL)):
        print(f'code {code} {name}: max err {np.abs(got - expected).max():.3e} of {np.abs(expected).max():.3e} (bound {bound:.3e} of the latter)')
        assert_close_norm(got, expected, bound, name)
    assert float(np.abs(old.numpy()).min()) > 0 and float(np.abs(want[1].numpy()).max()) > 0
    for key, value in module.state_dict().items():                  # frozen: the buffers are inputs
        assert torch.equal(value.cpu(), state[key]) or key in ('weight', 'bias'), key
    with no_grad():
        assert forward(leaf).node is None                           # no_grad records nothing
    # a recorded sweep computes no parameter gradients; one value per channel is refused (the forward entry point wants M >= 2)
    with pytest.raises(NotImplementedError, match='plain backward sweeps only'):
        backward(F.sum_all(B.unpack(forward(leaf))), inputs=[nn.P(module.weight)], create_graph=True)
    single = B.pack(F.leaf(torch.randn(1, shape[1], 1, 1).cuda()), code)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        B.batch_norm_frozen(single, *reversed(module._inverse_std()), nn.P(module.weight), nn.P(module.bias))


def test_second_order_against_fp64_on_blocked_fp32():
    """conv4x4s2 -> batch_norm_frozen(0.25) -> conv4x4s2(0.25) on a (4, 8, 16, 16) input in code 0: the penalty
    sum(grad(sum(out * c), input, create_graph=True) ** 2) through a plain ``backward``.  The gamma gradient exists only through
    the recorded backward of the norm (its double backward); both convolutions' weight gradients pass through it."""
    from srgan_amd import blocked16 as B, functional as F, nn
    from srgan_amd.tape import backward
    functional = torch.nn.functional
    generator = torch.Generator().manual_seed(8)
    shape, slope = (4, 8, 16, 16), 0.25
    first, second = nn.Conv2d(8, 12, 4, 2, 1), nn.Conv2d(12, 6, 4, 2, 1)
    norm, _ = _frozen_module(12, 17)
    network = nn.Sequential(first, norm, second)
    with torch.no_grad():
        for convolution in (first, second):
            convolution.weight.copy_(torch.randn(convolution.weight.shape, generator=generator) * 0.2)
            convolution.bias.copy_(torch.randn(convolution.bias.shape, generator=generator) * 0.5)
    state = {key: value.clone().double() for key, value in network.state_dict().items()}
    x = torch.randn(shape, generator=generator)
    c = torch.randn(4, 6, 4, 4, generator=generator)
    # fp64 torch
    parameters = {key: state[key].clone().requires_grad_() for key in ('0.weight', '0.bias', '1.weight', '1.bias', '2.weight', '2.bias')}
    x64 = x.double().requires_grad_()
    h = functional.conv2d(x64, parameters['0.weight'], parameters['0.bias'], 2, 1)
    h = functional.leaky_relu(functional.batch_norm(h, state['1.running_mean'], state['1.running_var'], parameters['1.weight'],
                                                    parameters['1.bias'], training=False, eps=norm.eps), slope)
    out64 = functional.leaky_relu(functional.conv2d(h, parameters['2.weight'], parameters['2.bias'], 2, 1), slope)
    inner, = torch.autograd.grad((out64 * c.double()).sum(), x64, create_graph=True)
    want = dict(zip(('0.weight', '1.weight', '2.weight'),
                    torch.autograd.grad((inner ** 2).sum(), [parameters[key] for key in ('0.weight', '1.weight', '2.weight')])))
    # the tape, blocked fp32
    arena = nn.flatten_parameters(network, torch.device('cuda', 0))
    arena.zero_grad()

    def penalty_graph(leaf, weights):
        with F.compute_dtype('f32'):
            h = norm(B.conv4x4s2(B.pack(leaf, 0), first), slope=slope)
            assert h.meta.code == 0 and h.meta.mask_ref is h.data
            out = B.unpack(B.conv4x4s2(h, second, slope=slope))
            return out, backward(F.sum_all(F.mul(out, weights)), inputs=[leaf], create_graph=True)[0]

    leaf = F.leaf(x.cuda(), requires_grad=True)
    out, gradient = penalty_graph(leaf, F.leaf(c.cuda()))
    assert_close_norm(out.cpu().numpy(), out64.detach().numpy(), OP_RTOL, 'out')
    assert_close_norm(gradient.cpu().numpy(), inner.detach().numpy(), OP_RTOL, 'the recorded gradient')
    with F.compute_dtype('f32'):
        backward(F.sum_all(F.square(gradient)))
    torch.cuda.synchronize()
    for key, module in (('0.weight', first), ('1.weight', norm), ('2.weight', second)):
        got, expected = module.weight.grad.cpu().numpy(), want[key].numpy()
        print(f'penalty gradient of {key}: max err {np.abs(got - expected).max():.3e} of {np.abs(expected).max():.3e}')
        assert np.abs(expected).max() > 0.0
        assert_close_norm(got, expected, OP_RTOL, key)
    # third order: a recorded sweep through the double backward of the norm (towards the cotangent weights, so that no
    # parameter gradient -- refused in every recorded sweep -- is asked for on the way)
    weights = F.leaf(c.cuda(), requires_grad=True)
    _, gradient = penalty_graph(F.leaf(x.cuda(), requires_grad=True), weights)
    with pytest.raises(NotImplementedError, match='third-order'), F.compute_dtype('f32'):
        backward(F.sum_all(F.square(gradient)), inputs=[weights], create_graph=True)


@pytest.mark.parametrize('code', CODES)
def test_frozen_norm_module_on_blocked_input_uses_the_running_statistics_in_both_modes(code):
    from srgan_amd import blocked16 as B, functional as F, nn
    from srgan_amd.tape import no_grad
    channels = 6
    module, generator = _frozen_module(channels, 4)
    other, _ = _frozen_module(channels, 40)
    nn.flatten_parameters(module, torch.device('cuda', 0))
    x = rounded(torch.randn(5, channels, 6, 10, generator=generator) * 2 + 1, code)

    def run(**arguments):
        with no_grad():
            out = module(B.pack(F.leaf(x.cuda()), code), **arguments)
            assert out.meta.code == code
            return B.unpack(out).cpu().numpy()

    def want(state, slope=1.0):
        return _reference_norm(state, x.double(), state['weight'].double(), state['bias'].double(), slope, module.eps).numpy()

    state = {key: value.cpu().clone() for key, value in module.state_dict().items()}
    for mode in (module.train, module.eval):
        mode()
        assert_close_norm(run(), want(state), STORED_RTOL[code], 'plain')
        assert_close_norm(run(slope=LEAK), want(state, LEAK), STORED_RTOL[code], 'with the leaky-ReLU')
        assert_close_norm(run(relu=True), want(state, 0.0), STORED_RTOL[code], 'with the ReLU')
        for key, value in module.state_dict().items():
            assert torch.equal(value.cpu(), state[key]), key          # buffers untouched ...
        assert int(module.num_batches_tracked) == 0                   # ... in training mode too
    cached = [module._inv_std_cache[1].data.data_ptr(), module._inv_std_cache[2].data.data_ptr()]
    module.load_state_dict(other.state_dict())
    reloaded = {key: value.cpu().clone() for key, value in other.state_dict().items()}
    assert float((reloaded['running_var'] - state['running_var']).abs().min()) > 1e-3
    assert_close_norm(run(slope=LEAK), want(reloaded, LEAK), STORED_RTOL[code], 'after load_state_dict')
    assert np.abs(want(reloaded, LEAK) - want(state, LEAK)).max() > 10 * STORED_RTOL[code] * np.abs(want(reloaded, LEAK)).max()
    assert cached == [module._inv_std_cache[1].data.data_ptr(), module._inv_std_cache[2].data.data_ptr()]


# ------------------------------------------------------------------------------------------------ 3. the discriminator
def _randomise_norms(network, seed):
    """Non-trivial statistics, gamma and beta on every norm layer of ``network`` (before it moves to the device)."""
    generator = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for module in network.modules():
            if isinstance(module, torch.nn.BatchNorm2d):
                module.weight.copy_(torch.rand(module.weight.shape, generator=generator) + 0.5)
                module.bias.copy_(torch.randn(module.bias.shape, generator=generator) * 0.3)
                module.running_mean.copy_(torch.randn(module.running_mean.shape, generator=generator) * 0.3)
                module.running_var.copy_(torch.rand(module.running_var.shape, generator=generator) * 1.5 + 0.5)


def _norms(network):
    return [stage[1] for stage in (network.layer2, network.layer3, network.layer4)]


def test_discriminator_with_norms_on_blocked_fp32_equals_the_nchw_graph():
    """Scores, features, one plain backward and one penalty-style double backward of a discriminator with frozen norms under
    ``F.storage_dtype('f32b')`` against the same weights on the plain fp32 graph: the same fp32 arithmetic in another order, 1e-3
    of each tensor's scale."""
    from srgan_amd import functional as F, nn
    from srgan_amd.age.models import Discriminator
    from srgan_amd.tape import backward
    generator = torch.Generator().manual_seed(12)
    x = torch.randn(6, 3, 32, 32, generator=generator)
    score_weights, feature_weights = torch.randn(6, generator=generator), torch.randn(6, 64 * 2 * 2, generator=generator)
    results = {}
    for blocked in (False, True):
        network = Discriminator(32, 8, batch_norm=True, blocked_frozen_norm=blocked)
        _randomise_norms(network, 5)
        with torch.no_grad():
            for module in network.modules():
                if isinstance(module, torch.nn.Conv2d):
                    module.weight.mul_(2.0)
        arena = nn.flatten_parameters(network, torch.device('cuda', 0))
        network.train()
        codes = []
        for norm in _norms(network):
            norm.register_forward_hook(lambda module, args, output: codes.append(
                (getattr(args[0].meta, 'code', None), getattr(output.meta, 'code', None))))

        def loss(leaf):
            scores = network(leaf)
            return scores, network.features, F.add(F.sum_all(F.mul(scores, F.leaf(score_weights.cuda()))),
                                                    F.sum_all(F.mul(network.features, F.leaf(feature_weights.cuda()))))

        with F.compute_dtype('f32'), F.storage_dtype('f32b' if blocked else None):
            leaf = F.leaf(x.cuda(), requires_grad=True)
            scores, features, value = loss(leaf)
            backward(value)
            torch.cuda.synchronize()
            found = dict(scores=scores.data.clone(), features=features.data.clone(), x_grad=leaf.grad.data.clone(),
                         **{f'grad {name}': parameter.grad.clone() for name, parameter in network.named_parameters()})
            arena.zero_grad()
            leaf = F.leaf(x.cuda(), requires_grad=True)
            gradient, = backward(loss(leaf)[2], inputs=[leaf], create_graph=True)
            backward(F.sum_all(F.square(gradient)))
            torch.cuda.synchronize()
            found.update({f'penalty grad {name}': parameter.grad.clone() for name, parameter in network.named_parameters()})
        assert codes == ([(0, 0)] * 6 if blocked else [(None, None)] * 6), codes      # two forwards x three norms
        assert all(int(norm.num_batches_tracked) == 0 for norm in _norms(network))
        results[blocked] = found
    assert len(results[True]) == 3 + 2 * 16
    moved = 0
    for key, want in results[False].items():
        got, want = results[True][key].cpu().numpy(), want.cpu().numpy()
        scale = np.abs(want).max()
        print(f'{key}: max err {np.abs(got - want).max():.3e} of {scale:.3e}')
        assert np.abs(got - want).max() <= OP_RTOL * scale, key
        moved += scale > 0.0
    # a piecewise-linear network: the penalty has no gradient for the biases and beta (zero on both paths); everything else moves
    assert moved == len(results[True]) - 8, moved


def _frozen_dcgan_experiment(seen):
    """``dcgan_experiment`` of test_batch_norm_train_gpu.py with all three networks built for the blocked path and blocked fp32
    on; ``seen`` collects (network, code of the input) of every norm layer of D and DNN."""
    def build(**settings):
        from test_steps_gpu import make_experiment
        from srgan_amd.age.models import Generator, Discriminator
        settings = dict(dict(batch_size=4, matching_loss_multiplier=1e2, contrasting_loss_multiplier=1e1, gradient_penalty_multiplier=1e2,
                             generator_batch_norm=True, discriminator_batch_norm=True, blocked_fp32=True, blocked_batch_norm=True,
                             blocked_frozen_norm=True), **settings)
        experiment = make_experiment(lambda: (Generator(image_size=32, conv_dim=8, batch_norm=True, blocked_batch_norm=True),
                                              Discriminator(32, 8, batch_norm=True, blocked_frozen_norm=True),
                                              Discriminator(32, 8, batch_norm=True, blocked_frozen_norm=True)), settings)
        for name in ('D', 'DNN'):
            for norm in _norms(getattr(experiment, name)):
                norm.register_forward_hook(lambda module, args, output, name=name: seen.append((name, getattr(args[0].meta, 'code', None))))
        return experiment
    return build


def test_two_steps_of_g16_with_blocked_discriminators_match_the_reference(monkeypatch):
    """Golden g16 (the unmodified reference with its batch-norm switch on: three frozen norms in D, the penalty active) with
    ``blocked_fp32``, ``blocked_batch_norm`` and ``blocked_frozen_norm``: the checks and tolerances of the NCHW step test, whose
    body runs here on an experiment whose three networks take the blocked path."""
    import test_batch_norm_train_gpu as nchw
    seen = []
    monkeypatch.setattr(nchw, 'dcgan_experiment', _frozen_dcgan_experiment(seen))
    nchw.test_two_steps_with_the_switch_on_match_the_reference('shared_forwards')
    # per step, three norms each: the DNN's one forward; D's stacked pass over [x, u, fake], D(interpolates) of the penalty,
    # D(fake) and D(u) of the generator loss -- 3 + 4 * 3 calls, two steps
    assert seen.count(('DNN', 0)) == 2 * 3 and seen.count(('D', 0)) == 2 * 12 and len(seen) == 30, seen


def test_replayed_g16_iterations_with_blocked_discriminators_equal_the_eager_ones(monkeypatch):
    import test_batch_norm_train_gpu as nchw
    seen = []
    monkeypatch.setattr(nchw, 'dcgan_experiment', _frozen_dcgan_experiment(seen))
    eager, eager_losses = nchw._iterations(False)
    assert len(seen) == 3 * 15 and {code for _, code in seen} == {0}, seen
    replayed, replayed_losses = nchw._iterations(True)
    _compare_replay(eager, eager_losses, replayed, replayed_losses)
    assert all(np.isfinite(value) for value in eager_losses[-1].values())


# ------------------------------------------------------------------------------------------------ 4. 16-bit storage
BF16 = dict(storage_dtype='bf16', compute_dtype='bf16', gradient_penalty_dtype='bf16')
# fp16 with the fp32 penalty chain; ``blocked_fp32`` keeps that chain on blocked tensors too (code 0), so that every norm of D
# sees a blocked tensor of its phase's code
FP16 = dict(storage_dtype='f16', compute_dtype='f16', gradient_penalty_dtype='f32', loss_scale=256.0, blocked_fp32=True)


def _driving_step(**overrides):
    """``_driving_step`` of test_batch_norm_train_gpu.py (the driving pair at 64 x 192, batch 8) with norm layers in all three
    networks and non-trivial statistics, gamma and beta on those of D and DNN, set before the networks move to the device.
    Returns (experiment, losses, [(network, meta of the input) of every norm call of D and DNN])."""
    from srgan_amd.settings import Settings
    from srgan_amd.driving.srgan import DrivingExperiment
    from srgan_amd.utility import SummaryWriter, seed_all
    size, batch = (64, 192), 8
    settings = Settings()
    settings.batch_size, settings.generator_batch_norm, settings.discriminator_batch_norm = batch, True, True
    settings.matching_loss_multiplier, settings.contrasting_loss_multiplier, settings.gradient_penalty_multiplier = 1e2, 1e1, 1e2
    for key, value in overrides.items():
        setattr(settings, key, value)
    experiment = DrivingExperiment(settings)
    experiment.image_size = size
    seed_all(0)
    experiment.model_setup()
    _randomise_norms(experiment.D, 5)
    _randomise_norms(experiment.DNN, 6)
    with torch.no_grad():
        for module in experiment.D.modules():
            if isinstance(module, torch.nn.Conv2d):
                module.weight.mul_(2.2)                     # gradient penalty active
    experiment.dnn_summary_writer, experiment.gan_summary_writer = SummaryWriter(), SummaryWriter()
    experiment.gpu_mode()
    experiment.prepare_optimizers()
    experiment.train_mode()
    metas = []
    for name in ('D', 'DNN'):
        for norm in _norms(getattr(experiment, name)):
            norm.register_forward_hook(lambda module, args, output, name=name: metas.append((name, args[0].meta)))
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


@functools.lru_cache(maxsize=None)
def _fp32_driving_losses():
    """The same step in fp32 on the NCHW graph, once."""
    experiment, losses, metas = _driving_step()
    assert len(metas) == 15 and all(meta is None for _, meta in metas)
    return losses


@pytest.mark.parametrize('name, overrides, code, tolerance', [('bf16', BF16, 1, 5e-2), ('fp16', FP16, 2, 2e-2)])
def test_a_driving_step_on_16_bit_storage_keeps_the_discriminators_blocked(name, overrides, code, tolerance):
    """Measured on an MI355X (relative error of each loss against the fp32 NCHW step; bounds 5e-2 / 2e-2 as in
    test_a_driving_step_on_16_bit_storage_keeps_the_generator_blocked): see profiles/blocked_frozen_norm_kernels.md."""
    from srgan_amd.blocked16 import Blocked
    expected = _fp32_driving_losses()
    experiment, got, metas = _driving_step(blocked_batch_norm=True, blocked_frozen_norm=True, **overrides)
    # three norms each: the DNN's forward; D's stacked pass, D(fake) and D(u) of the generator loss in the step's type, and
    # D(interpolates) in the penalty phase's
    penalty_code = 0 if overrides['gradient_penalty_dtype'] == 'f32' else code
    assert len(metas) == 15 and all(isinstance(meta, Blocked) for _, meta in metas), metas
    assert sorted(meta.code for network, meta in metas if network == 'DNN') == [code] * 3
    assert sorted(meta.code for network, meta in metas if network == 'D') == sorted([code] * 9 + [penalty_code] * 3)
    assert expected['gradient_penalty'] > 1.0
    worst = 0.0
    for key in ('labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss'):
        error = abs(got[key] - expected[key]) / max(abs(expected[key]), 1e-12)
        worst = max(worst, error)
        print(f'[{name} storage, blocked frozen norms] {key}: {got[key]:.6g}  fp32 {expected[key]:.6g}  rel {error:.2e}')
        assert error <= tolerance, (key, got[key], expected[key])
    assert worst > 1e-7, 'results identical to fp32: the 16-bit path was not active'
    for network in (experiment.G, experiment.D, experiment.DNN):
        for parameter in network.parameters():
            assert torch.isfinite(parameter).all()
    assert all(int(norm.num_batches_tracked) == 0 for norm in _norms(experiment.D) + _norms(experiment.DNN))
