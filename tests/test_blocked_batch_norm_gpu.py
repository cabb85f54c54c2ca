"""Training-mode batch normalisation on BLOCKED tensors (csrc/blocked16_batch_norm.hip; codes 0 = blocked fp32, 1 = bf16,
2 = fp16) on the GPU.

1. Exact operands (the idiom of test_blocked16_gpu.py): small integers and powers of two, so the fp32 result is exact and
   the kernels must reproduce it, rounded once to the storage type, bit for bit -- forward, both backward kernels, the zero
   padding channels of the layout, accumulation into the parameter gradients.
2. Statistics and random data against fp64 torch on x rounded to the storage type.  Tolerances (``assert_close_norm``: against
   the largest magnitude): the fp32 results -- mean, inv_std, variance, running buffers -- 1e-3, the project's op tolerance;
   y and gx 1e-3 for code 0 and for fp16 (unit roundoff 2^-11, doubled for the fp32 arithmetic in front of the rounding, is
   below 1e-3) and 2^-7 for bf16 (unit roundoff 2^-8, doubled likewise).
3. The tape op and ``nn.BatchStatNorm2d`` on blocked input; a generator with norm layers on blocked fp32 against the NCHW
   graph; whole steps (golden g16 in blocked fp32, the driving pair on bf16 / fp16 storage) and their HIP-graph replay."""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_close_norm
from test_batch_norm_train_gpu import CASES, EPS, MOMENTUM, _ids, inputs, poison_workspace

pytestmark = pytest.mark.gpu
CODES = [0, 1, 2]
TORCH = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
OP_RTOL = 1e-3
STORED_RTOL = {0: 1e-3, 1: 2.0 ** -7, 2: 1e-3}


@pytest.fixture(scope='module', autouse=True)
def pkg():
    import srgan_amd
    assert torch.cuda.is_available()
    return srgan_amd


def _call(name, *arguments):
    from srgan_amd import _lib
    _lib.check(getattr(_lib.library(), name)(*arguments), name)


def _stream():
    from srgan_amd import _lib
    return _lib.stream_handle()


def group(code):
    return 4 if code == 0 else 8


def to_blocked(t, code):
    """fp32 NCHW (host or device) -> the raw blocked tensor [N][C / g][H][W][g] through ``pack``."""
    from srgan_amd import blocked16 as B, functional as F
    from srgan_amd.tape import no_grad
    with no_grad():
        return B.pack(F.leaf(t.float().cuda()), code).data


def new_blocked(shape, code):
    """An output buffer full of NaN: a slot the kernel does not write shows."""
    n, c, h, w = shape
    return torch.full((n, (c + group(code) - 1) // group(code), h, w, group(code)), float('nan'), dtype=TORCH[code], device='cuda')


def all_channels(raw):
    """A raw blocked tensor as [N, groups * g, H, W] in fp32: the padding channels of the last group included."""
    n, groups, h, w, g = raw.shape
    return raw.float().permute(0, 1, 4, 2, 3).reshape(n, groups * g, h, w)


def from_blocked(raw, shape):
    """The logical channels; asserts the layout's invariant -- channels >= C of the last group are stored as zeros."""
    full = all_channels(raw)
    assert torch.equal(full[:, shape[1]:], torch.zeros_like(full[:, shape[1]:])), 'padding channels are not zero'
    return full[:, :shape[1]].contiguous()


def rounded(t, code):
    return t.float().to(TORCH[code]).float()


def integers(shape, low, high, seed):
    return torch.randint(low, high + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def per_channel(t):
    return t.view(1, -1, 1, 1)


def abi_stats(xb, shape, code, running_mean=None, running_var=None, tracked=None):
    n, c, h, w = shape
    stats = torch.full((2, c), float('nan'), device='cuda')
    pointer = lambda t: None if t is None else t.data_ptr()
    _call('srgan_h_batch_norm_stats', xb.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), pointer(running_mean),
          pointer(running_var), pointer(tracked), MOMENTUM, EPS, n, c, h * w, code, _stream())
    return stats


def abi_fwd(xb, shape, code, mean, inv_std, gamma, beta, slope):
    n, c, h, w = shape
    yb = new_blocked(shape, code)
    _call('srgan_h_batch_norm_fwd', xb.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), gamma.data_ptr(), beta.data_ptr(), slope,
          yb.data_ptr(), n, c, h * w, code, _stream())
    return yb


def abi_reduce(sb, xb, shape, code, mean, inv_std, gamma_grad=None, beta_grad=None):
    n, c, h, w = shape
    sums = torch.full((2, c), float('nan'), device='cuda')
    _call('srgan_h_batch_norm_bwd_reduce', sb.data_ptr(), xb.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), sums.data_ptr(),
          None if gamma_grad is None else gamma_grad.data_ptr(), None if beta_grad is None else beta_grad.data_ptr(), n, c, h * w,
          code, _stream())
    return sums


def abi_apply(sb, xb, shape, code, mean, inv_std, gamma, sums, refb=None, slope=1.0):
    n, c, h, w = shape
    gxb = new_blocked(shape, code)
    _call('srgan_h_batch_norm_bwd_apply', sb.data_ptr(), xb.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), gamma.data_ptr(),
          sums.data_ptr(), None if refb is None else refb.data_ptr(), slope, gxb.data_ptr(), n, c, h * w, code, _stream())
    return gxb


# ------------------------------------------------------------------------------------------------ 1. exact operands
# channel tails for g = 8 (3, 5, 12, 20) and g = 4 (3, 5); M = N * H * W a power of two (64, 1024) for the apply kernel
APPLY_SHAPES = [(2, 3, 4, 8), (2, 5, 4, 8), (2, 12, 4, 8), (4, 20, 16, 16)]
# plus an odd plane and a 2 x 2 one with N = 1 for the forward and the sums
EXACT_SHAPES = APPLY_SHAPES + [(3, 5, 3, 5), (1, 8, 2, 2)]
EXACT_SLOPES = [1.0, 0.25]


def exact_operands(shape):
    c = shape[1]
    pick = torch.tensor([0.5, 1.0, 2.0])
    return dict(x=integers(shape, -4, 4, 1), s=integers(shape, -3, 3, 2), ref=integers(shape, -1, 1, 3),
                gamma=integers((c,), -2, 2, 4), beta=integers((c,), -3, 3, 5), mean=integers((c,), -2, 2, 6),
                inv_std=pick[torch.randint(0, 3, (c,), generator=torch.Generator().manual_seed(7))],
                sums=integers((2, c), -2, 2, 8) * float(shape[0] * shape[2] * shape[3]),
                old_gamma_grad=integers((c,), -5, 5, 9), old_beta_grad=integers((c,), -5, 5, 10))


@pytest.mark.parametrize('slope', EXACT_SLOPES)
@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda shape: 'x'.join(map(str, shape)))
@pytest.mark.parametrize('code', CODES)
def test_forward_is_exact_on_integers(code, shape, slope):
    given = exact_operands(shape)
    d = {key: value.cuda() for key, value in given.items()}
    yb = abi_fwd(to_blocked(given['x'], code), shape, code, d['mean'], d['inv_std'], d['gamma'], d['beta'], slope)
    pre = (given['x'].double() - per_channel(given['mean'])) * per_channel(given['inv_std'] * given['gamma']) + per_channel(given['beta'])
    want = torch.where(pre > 0, pre, pre * slope)
    assert torch.equal(want.float().double(), want)                       # the exact result is an fp32 number
    assert torch.equal(from_blocked(yb, shape).cpu(), rounded(want, code))
    assert float(want.abs().max()) > 8.0


@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda shape: 'x'.join(map(str, shape)))
@pytest.mark.parametrize('code', CODES)
def test_backward_reduce_is_exact_and_adds_to_the_parameter_gradients(code, shape):
    given = exact_operands(shape)
    d = {key: value.cuda() for key, value in given.items()}
    gamma_grad, beta_grad = d['old_gamma_grad'].clone(), d['old_beta_grad'].clone()
    sb, xb = to_blocked(given['s'], code), to_blocked(given['x'], code)
    sums = abi_reduce(sb, xb, shape, code, d['mean'], d['inv_std'], gamma_grad, beta_grad)
    xhat = (given['x'].double() - per_channel(given['mean'])) * per_channel(given['inv_std'])
    want = torch.stack([given['s'].double().sum(dim=(0, 2, 3)), (given['s'].double() * xhat).sum(dim=(0, 2, 3))])
    assert torch.equal(sums.cpu().double(), want)
    assert torch.equal(beta_grad.cpu().double(), given['old_beta_grad'].double() + want[0])       # added to, not replaced
    assert torch.equal(gamma_grad.cpu().double(), given['old_gamma_grad'].double() + want[1])
    assert float(given['old_gamma_grad'].abs().max()) > 0 and float(want.abs().max()) > 0
    # without the gradient pointers the sums are the same and nothing else is written
    assert torch.equal(abi_reduce(sb, xb, shape, code, d['mean'], d['inv_std']), sums)


@pytest.mark.parametrize('slope', EXACT_SLOPES)
@pytest.mark.parametrize('shape', APPLY_SHAPES, ids=lambda shape: 'x'.join(map(str, shape)))
@pytest.mark.parametrize('code', CODES)
def test_backward_apply_is_exact_with_and_without_a_mask_reference(code, shape, slope):
    given = exact_operands(shape)
    d = {key: value.cuda() for key, value in given.items()}
    count = float(shape[0] * shape[2] * shape[3])
    sb, xb, refb = (to_blocked(given[key], code) for key in ('s', 'x', 'ref'))
    xhat = (given['x'].double() - per_channel(given['mean'])) * per_channel(given['inv_std'])
    want = per_channel(given['gamma'] * given['inv_std']).double() * \
        (given['s'].double() - per_channel(given['sums'][0]) / count - xhat * per_channel(given['sums'][1]) / count)
    assert torch.equal(want.float().double(), want)
    plain = abi_apply(sb, xb, shape, code, d['mean'], d['inv_std'], d['gamma'], d['sums'])
    assert torch.equal(from_blocked(plain, shape).cpu(), rounded(want, code))
    masked = abi_apply(sb, xb, shape, code, d['mean'], d['inv_std'], d['gamma'], d['sums'], refb, slope)
    want_masked = want * torch.where(given['ref'] > 0, 1.0, slope).double()
    assert torch.equal(from_blocked(masked, shape).cpu(), rounded(want_masked, code))
    assert float(want.abs().max()) > 8.0 and (slope == 1.0 or not torch.equal(want, want_masked))


# ------------------------------------------------------------------------------------------------ 2. statistics, random data
def stored_x(case, code):
    return rounded(inputs(case)['x'], code)


@functools.lru_cache(maxsize=None)
def reference(case, code, slope):
    """fp64 on the CPU, once per (case, code, slope), on x ROUNDED to the storage type: outputs, statistics, the running buffers
    after one and three calls, and the gradients of the normalisation for the PRE-MASKED cotangent ``s`` (itself rounded to
    the storage type) -- the backward kernels of this path see no activation."""
    functional = torch.nn.functional
    given = inputs(case)
    x = stored_x(case, code).double().requires_grad_()
    gamma, beta = given['gamma'].double().requires_grad_(), given['beta'].double().requires_grad_()
    running_mean, running_var = given['running_mean'].double().clone(), given['running_var'].double().clone()
    out = {}
    for call in (1, 2, 3):
        pre = functional.batch_norm(x, running_mean, running_var, gamma, beta, training=True, momentum=MOMENTUM, eps=EPS)
        if call in (1, 3):
            out[f'running_mean{call}'], out[f'running_var{call}'] = running_mean.clone().numpy(), running_var.clone().numpy()
    y = functional.leaky_relu(pre, slope) if slope != 1.0 else pre
    s = rounded(given['cotangent'], code)
    gx, ggamma, gbeta = torch.autograd.grad(pre, (x, gamma, beta), s.double())
    variance = x.detach().var(dim=(0, 2, 3), unbiased=False)
    out.update(y=y.detach().numpy(), mean=x.detach().mean(dim=(0, 2, 3)).numpy(), inv_std=(variance + EPS).rsqrt().numpy(),
               variance=variance.numpy(), gx=gx.numpy(), ggamma=ggamma.numpy(), gbeta=gbeta.numpy(), s=s)
    return out


def test_the_offset_case_separates_the_two_variance_formulas():
    """The case with data near 1000 keeps its teeth in every storage type: E[x^2] - E[x]^2 in fp32 on the values the kernels
    see misses the true variance by >= 1.1e-3 of it in every channel and by > 1e-2 in at least four of the five -- a kernel
    that used it would fail the 1e-3 checks below.  (numpy on the CPU; needs no device.)"""
    case = CASES[-1]
    assert case == ((4, 5, 6, 7), 1000.0)
    for code in CODES:
        x = stored_x(case, code).numpy()
        channels = x.transpose(1, 0, 2, 3).reshape(x.shape[1], -1)
        true = channels.astype(np.float64).var(axis=1)
        count = np.float32(channels.shape[1])
        mean = channels.sum(axis=1, dtype=np.float32) / count
        naive = (channels * channels).sum(axis=1, dtype=np.float32) / count - mean * mean
        miss = np.abs(naive.astype(np.float64) - true) / true
        print(f'code {code}: naive fp32 variance misses by {miss}')
        assert (miss >= 1.1e-3).all() and (miss > 1e-2).sum() >= 4, (code, miss)


@pytest.mark.parametrize('case', CASES, ids=_ids)
@pytest.mark.parametrize('code', CODES)
def test_statistics_forward_and_backward_against_fp64(code, case):
    shape, slope = case[0], 0.05
    want, given = reference(case, code, slope), inputs(case)
    d = {key: value.clone().cuda() for key, value in given.items()}
    xb = to_blocked(stored_x(case, code), code)
    tracked = torch.zeros((), dtype=torch.int64, device='cuda')
    label = f'code {code} {_ids(case)}'
    for call in (1, 2, 3):
        poison_workspace()
        stats = abi_stats(xb, shape, code, d['running_mean'], d['running_var'], tracked)
        if call in (1, 3):
            for name in ('running_mean', 'running_var'):
                got = d[name].cpu().numpy()
                print(f'{label} call {call} {name}: max err {np.abs(got - want[name + str(call)]).max():.3e}')
                assert_close_norm(got, want[f'{name}{call}'], OP_RTOL, f'{name} after {call} call(s)')
    assert int(tracked) == 3
    variance = 1.0 / stats[1].double().cpu().numpy() ** 2 - EPS
    for name, got in (('mean', stats[0].cpu().numpy()), ('inv_std', stats[1].cpu().numpy()), ('variance', variance)):
        print(f'{label} {name}: max err {np.abs(got - want[name]).max():.3e} of {np.abs(want[name]).max():.3e}')
        assert_close_norm(got, want[name], OP_RTOL, name)
    yb = abi_fwd(xb, shape, code, stats[0], stats[1], d['gamma'], d['beta'], slope)
    gamma_grad, beta_grad = d['old_gamma_grad'].clone(), d['old_beta_grad'].clone()
    sb = to_blocked(want['s'], code)
    sums = abi_reduce(sb, xb, shape, code, stats[0], stats[1], gamma_grad, beta_grad)
    gxb = abi_apply(sb, xb, shape, code, stats[0], stats[1], d['gamma'], sums)
    for name, got in (('ggamma', sums[1]), ('gbeta', sums[0])):
        got = got.cpu().numpy()
        print(f'{label} {name}: max err {np.abs(got - want[name]).max():.3e} of {np.abs(want[name]).max():.3e}')
        assert_close_norm(got, want[name], OP_RTOL, name)
    assert torch.equal(gamma_grad, d['old_gamma_grad'] + sums[1]) and torch.equal(beta_grad, d['old_beta_grad'] + sums[0])
    for name, got in (('y', yb), ('gx', gxb)):
        got = from_blocked(got, shape).cpu().numpy()
        print(f'{label} {name}: max err {np.abs(got - want[name]).max():.3e} of {np.abs(want[name]).max():.3e} '
              f'(bound {STORED_RTOL[code]:.3e} of the latter)')
        assert_close_norm(got, want[name], STORED_RTOL[code], name)


@pytest.mark.parametrize('code', CODES)
def test_two_runs_are_bit_identical(code):
    case = ((8, 8, 64, 64), 0.0)                   # several workgroups share a channel group
    shape = case[0]
    runs = []
    for _ in range(2):
        d = {key: value.clone().cuda() for key, value in inputs(case).items()}
        xb, sb = to_blocked(stored_x(case, code), code), to_blocked(inputs(case)['cotangent'], code)
        tracked = torch.zeros((), dtype=torch.int64, device='cuda')
        stats = abi_stats(xb, shape, code, d['running_mean'], d['running_var'], tracked)
        yb = abi_fwd(xb, shape, code, stats[0], stats[1], d['gamma'], d['beta'], 0.05)
        sums = abi_reduce(sb, xb, shape, code, stats[0], stats[1])
        gxb = abi_apply(sb, xb, shape, code, stats[0], stats[1], d['gamma'], sums, yb, 0.05)
        torch.cuda.synchronize()
        runs.append((stats, d['running_mean'], d['running_var'], all_channels(yb), sums, all_channels(gxb)))
    for first, second in zip(*runs):
        assert torch.equal(first, second) and bool(torch.isfinite(first).all())


# ------------------------------------------------------------------------------------------------ 3. tape and module
def _norm_module(channels, seed):
    from srgan_amd import nn
    generator = torch.Generator().manual_seed(seed)
    module = nn.BatchStatNorm2d(channels)
    with torch.no_grad():
        module.weight.copy_(torch.rand(channels, generator=generator) + 0.5)
        module.bias.copy_(torch.randn(channels, generator=generator))
    return module, generator


@pytest.mark.parametrize('code', CODES)
def test_the_tape_op_against_fp64_autograd(code):
    """``blocked16.batch_norm_train`` between ``pack`` and ``unpack`` through a plain ``backward()``: the gradient of x and the
    gamma / beta gradients, added to a non-zero arena.  The cotangent and its product with the slope 0.25 are numbers of the
    storage type, so the pre-masked gradient the op receives is exact."""
    from srgan_amd import blocked16 as B, functional as F, nn
    from srgan_amd.tape import backward, no_grad
    shape, slope = (3, 12, 6, 10), 0.25
    module, generator = _norm_module(shape[1], 21)
    x = rounded(torch.randn(shape, generator=generator) * 2 + 1, code)
    cotangent = rounded(torch.randn(shape, generator=generator), code)
    arena = nn.flatten_parameters(module, torch.device('cuda', 0))
    old = torch.randn(arena.grad.shape, generator=generator)
    arena.grad.copy_(old)
    x64 = x.double().requires_grad_()
    gamma64, beta64 = (p.detach().cpu().double().requires_grad_() for p in (module.weight, module.bias))
    want_y = torch.nn.functional.leaky_relu(torch.nn.functional.batch_norm(x64, None, None, gamma64, beta64, training=True, eps=EPS), slope)
    want = torch.autograd.grad(want_y, (x64, gamma64, beta64), cotangent.double())

    def forward(leaf):
        y = B.batch_norm_train(B.pack(leaf, code), nn.P(module.weight), nn.P(module.bias), module.running_mean, module.running_var,
                               MOMENTUM, EPS, slope=slope, num_batches_tracked=module.num_batches_tracked)
        assert y.meta.code == code and y.meta.mask_ref is y.data and y.meta.slope == slope
        return y

    leaf = F.leaf(x.cuda(), requires_grad=True)
    y = forward(leaf)
    out = B.unpack(y)
    assert_close_norm(out.cpu().numpy(), want_y.detach().numpy(), STORED_RTOL[code], 'y')
    backward(F.sum_all(F.mul(out, F.leaf(cotangent.cuda()))))
    got_gamma = (module.weight.grad.cpu() - old[arena.offsets[0]:arena.offsets[0] + shape[1]]).numpy()
    got_beta = (module.bias.grad.cpu() - old[arena.offsets[1]:arena.offsets[1] + shape[1]]).numpy()
    for name, got, expected, bound in (('gx', leaf.grad.cpu().numpy(), want[0].numpy(), STORED_RTOL[code]),
                                       ('ggamma', got_gamma, want[1].numpy(), OP_RTOL), ('gbeta', got_beta, want[2].numpy(), OP_RTOL)):
        print(f'code {code} {name}: max err {np.abs(got - expected).max():.3e} of {np.abs(expected).max():.3e}')
        assert_close_norm(got, expected, bound, name)
    assert int(module.num_batches_tracked) == 1
    # a recorded backward is refused; no_grad saves nothing; the refusals of the NCHW op
    with pytest.raises(NotImplementedError, match='first-order'):
        backward(F.sum_all(F.square(B.unpack(forward(leaf)))), inputs=[leaf], create_graph=True)
    with no_grad():
        assert forward(leaf).node is None
    with pytest.raises(NotImplementedError, match='momentum=None'):
        B.batch_norm_train(B.pack(leaf, code), nn.P(module.weight), nn.P(module.bias), None, None, None, EPS)
    single = B.pack(F.leaf(torch.randn(1, shape[1], 1, 1).cuda()), code)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        B.batch_norm_train(single, nn.P(module.weight), nn.P(module.bias), None, None, MOMENTUM, EPS)


@pytest.mark.parametrize('code', CODES)
def test_batch_stat_norm_module_on_blocked_input_trains_then_evaluates(code):
    from srgan_amd import blocked16 as B, functional as F, nn
    from srgan_amd.tape import backward, no_grad
    channels = 6
    ours, generator = _norm_module(channels, 4)
    theirs = torch.nn.BatchNorm2d(channels).double()
    theirs.load_state_dict({key: value.double() if value.is_floating_point() else value for key, value in ours.state_dict().items()})
    nn.flatten_parameters(ours, torch.device('cuda', 0))
    batches = [rounded(torch.randn(5, channels, 6, 10, generator=generator) * (1 + index) + index, code) for index in range(4)]

    def run(batch, **arguments):
        with no_grad():
            out = ours(B.pack(F.leaf(batch.cuda()), code), **arguments)
            assert out.meta.code == code
            return B.unpack(out).cpu().numpy()

    ours.eval()
    run(batches[3])                                          # the cache of the eval path exists BEFORE the statistics move
    cached = [ours._inv_std_cache[1].data.data_ptr(), ours._inv_std_cache[2].data.data_ptr()]
    buffers = [ours.running_mean.data_ptr(), ours.running_var.data_ptr(), ours.num_batches_tracked.data_ptr()]
    ours.train()
    theirs.train()
    for batch in batches[:3]:
        want = torch.nn.functional.leaky_relu(theirs(batch.double()), 0.05)
        assert_close_norm(run(batch, slope=0.05), want.detach().numpy(), STORED_RTOL[code], 'training forward')
    ours.eval()
    theirs.eval()
    assert_close_norm(run(batches[3]), theirs(batches[3].double()).detach().numpy(), STORED_RTOL[code], 'eval forward after training')
    want = torch.nn.functional.leaky_relu(theirs(batches[3].double()), 0.05)
    assert_close_norm(run(batches[3], slope=0.05), want.detach().numpy(), STORED_RTOL[code], 'eval forward with the activation')
    assert int(ours.num_batches_tracked) == int(theirs.num_batches_tracked) == 3
    assert_close_norm(ours.running_mean.cpu().numpy(), theirs.running_mean.numpy(), OP_RTOL, 'running_mean')
    assert_close_norm(ours.running_var.cpu().numpy(), theirs.running_var.numpy(), OP_RTOL, 'running_var')
    assert float((theirs.running_var - 1).abs().min()) > 0.1          # the eval output above cannot come from stale statistics
    assert cached == [ours._inv_std_cache[1].data.data_ptr(), ours._inv_std_cache[2].data.data_ptr()]
    assert buffers == [ours.running_mean.data_ptr(), ours.running_var.data_ptr(), ours.num_batches_tracked.data_ptr()]
    # eval mode on blocked tensors is forward only
    leaf = F.leaf(batches[3].cuda(), requires_grad=True)
    out = B.unpack(ours(B.pack(leaf, code)))
    with pytest.raises(NotImplementedError, match='forward only'):
        backward(F.sum_all(out))


# ------------------------------------------------------------------------------------------------ 4. the generator
def test_generator_with_norms_on_blocked_fp32_equals_the_nchw_graph():
    """Forward and one backward of a generator with norm layers under ``F.storage_dtype('f32b')`` against the same weights on
    the plain fp32 graph: the same fp32 arithmetic in another order, 1e-3 of each tensor's scale."""
    from srgan_amd import functional as F, nn
    from srgan_amd.age.models import Generator
    from srgan_amd.tape import backward
    from test_batch_norm_train_gpu import ZERO_GRADIENT_BIASES
    generator = torch.Generator().manual_seed(12)
    z = torch.randn(6, 32, generator=generator)
    cotangent = torch.randn(6, 3, 128, 128, generator=generator)
    results = {}
    for blocked in (False, True):
        network = Generator(32, conv_dim=16, batch_norm=True, blocked_batch_norm=blocked)
        nn.flatten_parameters(network, torch.device('cuda', 0))
        network.train()
        codes = []
        for stage in (network.layer1, network.layer2, network.layer3):
            stage[1].register_forward_hook(lambda module, args, output: codes.append(
                (getattr(args[0].meta, 'code', None), getattr(output.meta, 'code', None))))
        leaf = F.leaf(z.cuda(), requires_grad=True)
        with F.compute_dtype('f32'), F.storage_dtype('f32b' if blocked else None):
            images = network(leaf)
            backward(F.sum_all(F.mul(images, F.leaf(cotangent.cuda()))))
        torch.cuda.synchronize()
        assert codes == [(0, 0)] * 3 if blocked else codes == [(None, None)] * 3, codes
        results[blocked] = dict(images=images.data, z_grad=leaf.grad.data,
                                **{f'grad {name}': parameter.grad for name, parameter in network.named_parameters()},
                                **{name: buffer for name, buffer in network.named_buffers() if 'running' in name})
        assert all(int(buffer) == 1 for name, buffer in network.named_buffers() if 'tracked' in name)
    assert len(results[True]) == 2 + 16 + 6
    for key, want in results[False].items():
        got, want = results[True][key].cpu().numpy(), want.cpu().numpy()
        scale = np.abs(want).max()
        if key.replace('grad ', '') in ZERO_GRADIENT_BIASES:
            # exactly zero in exact arithmetic (the norm subtracts the batch mean): rounding noise on both sides, compared on
            # the scale of the layer's weight gradient
            scale = np.abs(results[False][key.replace('bias', 'weight')].cpu().numpy()).max()
        print(f'{key}: max err {np.abs(got - want).max():.3e} of {scale:.3e}')
        assert np.abs(got - want).max() <= OP_RTOL * scale, key
        assert scale > 0.0


# ------------------------------------------------------------------------------------------------ 5. steps
def _blocked_dcgan_experiment(seen):
    """``dcgan_experiment`` of test_batch_norm_train_gpu.py with the generator built for the blocked path and blocked fp32 on;
    ``seen`` collects the code of every norm layer's input."""
    def build(**settings):
        from test_steps_gpu import make_experiment
        from srgan_amd.age.models import Generator, Discriminator
        settings = dict(dict(batch_size=4, matching_loss_multiplier=1e2, contrasting_loss_multiplier=1e1, gradient_penalty_multiplier=1e2,
                             generator_batch_norm=True, discriminator_batch_norm=True, blocked_fp32=True, blocked_batch_norm=True),
                        **settings)
        experiment = make_experiment(lambda: (Generator(image_size=32, conv_dim=8, batch_norm=True, blocked_batch_norm=True),
                                              Discriminator(32, 8, batch_norm=True), Discriminator(32, 8, batch_norm=True)), settings)
        for stage in (experiment.G.layer1, experiment.G.layer2, experiment.G.layer3):
            stage[1].register_forward_hook(lambda module, args, output: seen.append(getattr(args[0].meta, 'code', None)))
        return experiment
    return build


def test_two_steps_of_g16_in_blocked_fp32_match_the_reference(monkeypatch):
    """Golden g16 (the unmodified reference with its batch-norm switch on) with ``blocked_fp32`` and ``blocked_batch_norm``: the
    checks and tolerances of the NCHW step test, whose body runs here on an experiment built for the blocked path."""
    import test_batch_norm_train_gpu as nchw
    seen = []
    monkeypatch.setattr(nchw, 'dcgan_experiment', _blocked_dcgan_experiment(seen))
    nchw.test_two_steps_with_the_switch_on_match_the_reference('shared_forwards')
    assert len(seen) == 12 and set(seen) == {0}, seen          # two steps x two generator forwards x three norms, all blocked fp32


def test_replayed_g16_iterations_in_blocked_fp32_equal_the_eager_ones(monkeypatch):
    import test_batch_norm_train_gpu as nchw
    seen = []
    monkeypatch.setattr(nchw, 'dcgan_experiment', _blocked_dcgan_experiment(seen))
    eager, eager_losses = nchw._iterations(False)
    assert len(seen) == 18 and set(seen) == {0}, seen
    replayed, replayed_losses = nchw._iterations(True)
    _compare_replay(eager, eager_losses, replayed, replayed_losses)


def _compare_replay(eager, eager_losses, replayed, replayed_losses):
    captured = replayed._captured_iteration
    assert captured.eager_iterations == 1 and captured.replays == 2
    assert eager_losses == replayed_losses and eager_losses[-1] != eager_losses[-2]
    for name in ('D', 'DNN', 'G'):
        assert torch.equal(getattr(eager, name)._srgan_arena.data, getattr(replayed, name)._srgan_arena.data), name
        for (key, a), (_, b) in zip(getattr(eager, name).named_buffers(), getattr(replayed, name).named_buffers()):
            assert torch.equal(a, b), (name, key)
    assert int(replayed.G.layer1[1].num_batches_tracked) == 6
    for a, b in ((eager.g_optimizer, replayed.g_optimizer), (eager.d_optimizer, replayed.d_optimizer),
                 (eager.dnn_optimizer, replayed.dnn_optimizer)):
        assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)


BF16 = dict(storage_dtype='bf16', compute_dtype='bf16', gradient_penalty_dtype='bf16')
FP16 = dict(storage_dtype='f16', compute_dtype='f16', gradient_penalty_dtype='f32', loss_scale=256.0)


@functools.lru_cache(maxsize=None)
def _fp32_driving_losses():
    from test_batch_norm_train_gpu import _driving_step
    return _driving_step()[1]


@pytest.mark.parametrize('name, overrides, code, tolerance', [('bf16', BF16, 1, 5e-2), ('fp16', FP16, 2, 2e-2)])
def test_a_driving_step_on_16_bit_storage_keeps_the_generator_blocked(name, overrides, code, tolerance):
    from srgan_amd.blocked16 import Blocked
    from test_batch_norm_train_gpu import _driving_step
    expected = _fp32_driving_losses()
    experiment, got, metas = _driving_step(blocked_batch_norm=True, **overrides)
    assert len(metas) == 12 and all(isinstance(meta, Blocked) and meta.code == code for meta in metas), metas
    assert expected['gradient_penalty'] > 1.0
    worst = 0.0
    for key in ('labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss'):
        error = abs(got[key] - expected[key]) / max(abs(expected[key]), 1e-12)
        worst = max(worst, error)
        print(f'[{name} storage, blocked norms] {key}: {got[key]:.6g}  fp32 {expected[key]:.6g}  rel {error:.2e}')
        assert error <= tolerance, (key, got[key], expected[key])
    assert worst > 1e-7, 'results identical to fp32: the 16-bit path was not active'
    assert int(experiment.G.layer1[1].num_batches_tracked) == 2
    for parameter in experiment.G.parameters():
        assert torch.isfinite(parameter).all()


def _driving_iterations(step_graph, count=3):
    """``_iterations`` of test_batch_norm_train_gpu.py for the driving pair on bf16 storage at 64 x 192, batch 4."""
    from srgan_amd.settings import Settings
    from srgan_amd.driving.srgan import DrivingExperiment
    from srgan_amd.utility import SummaryWriter, seed_all
    size, batch = (64, 192), 4
    settings = Settings()
    for key, value in dict(BF16, batch_size=batch, generator_batch_norm=True, blocked_batch_norm=True, matching_loss_multiplier=1e2,
                           contrasting_loss_multiplier=1e1, gradient_penalty_multiplier=1e2, step_graph=step_graph,
                           step_graph_warmup=1, steps_to_run=10 ** 9).items():
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
    for optimizer in (experiment.d_optimizer, experiment.g_optimizer, experiment.dnn_optimizer):
        optimizer.count_on_device()
    for writer in (experiment.dnn_summary_writer, experiment.gan_summary_writer):
        writer.summary_period, writer.steps_to_run = 10 ** 9, 10 ** 9
    codes = []
    for stage in (experiment.G.layer1, experiment.G.layer2, experiment.G.layer3):
        stage[1].register_forward_hook(lambda module, args, output: codes.append(getattr(args[0].meta, 'code', None)))
    seed_all(5)
    generator = torch.Generator().manual_seed(11)
    losses = []
    for step in range(1, count + 1):
        x, u = (torch.rand(batch, 3, *size, generator=generator) * 2 - 1 for _ in range(2))
        y = torch.rand(batch, generator=generator) * 2 - 1
        experiment.training_iteration(x.cuda(), y.cuda(), u.cuda(), step)
        losses.append({name: float(value.item()) for name, value in experiment.last_losses.items() if value is not None})
    torch.cuda.synchronize()
    assert codes and set(codes) == {1}, codes
    return experiment, losses


def test_replayed_driving_iterations_on_bf16_storage_equal_the_eager_ones():
    eager, eager_losses = _driving_iterations(False)
    replayed, replayed_losses = _driving_iterations(True)
    _compare_replay(eager, eager_losses, replayed, replayed_losses)
    assert all(np.isfinite(value) for value in eager_losses[-1].values())
