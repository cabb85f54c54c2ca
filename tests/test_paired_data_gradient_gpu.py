"""The 1x1 data gradients of two consecutive dense layers as strip + pair (srgan_conv2d_bwd_data_bnrelu_strip / _pair,
pointwise_ring.hip's PAIR kernel) against the per-layer launches they replace: the same bits in the gradient buffer and in
the partial-sum scratch, exact values on small-integer operands, nothing written outside the pair's rows and regions, and
fused.dense_block's backward with fused.PAIRED_DGRAD on and off.

Shapes: 16 images of 32 x 32 pixels, 128 + 32 l channels.  A pair's rows are layer B's: 192 (a partial last tile of 64
rows), 160 (of 32 rows) and, for the exact case, 224 (of 96); the strip then lies in the second row tile.  The LDS-DMA
kernel takes a layer by itself from 192 workgroups, here two row tiles: (160, 128) is no pair, and neither is (96, 64) of the
6-layer block, so those layers keep their per-layer launches inside the blocks."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
N, H, W, WIDTH, TOTAL = 16, 32, 32, 128, 256
HW = H * W
TILES = N * HW // 128


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def bits(tensor):
    return tensor.contiguous().view(torch.int32).cpu()


def same_bits(actual, expected, what):
    different = int((bits(actual) != bits(expected)).sum())
    assert different == 0, f'{what}: {different} of {actual.numel()} elements differ in their bits'


def layer_desc(lib, rows):
    return lib.ConvDesc(N, rows, H, W, WIDTH, 1, 1, 1, 1, 0, 0, H, W, TOTAL * HW, 0, 0)


def operands(rows_a, seed, exact):
    """x, the old gradient buffer, and per layer (gy, weight [128][rows], mean, inv_std, gamma, beta) on the host."""
    gen = torch.Generator().manual_seed(seed)

    def integers(shape, bound):
        return torch.randint(-bound, bound + 1, shape, generator=gen).float()

    layers = []
    if exact:
        # every product and partial sum an integer below 2^24 (a = inv_std * gamma a signed power of two): fp32 is exact
        x, old = integers((N, TOTAL, H, W), 3), integers((N, TOTAL, H, W), 8)
        for rows in (rows_a, rows_a - 32):
            gamma = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (rows,), generator=gen)]
            inv = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (rows,), generator=gen)]
            layers.append((integers((N, WIDTH, H, W), 2), integers((WIDTH, rows), 2), integers((rows,), 1), inv, gamma,
                           integers((rows,), 1)))
    else:
        x, old = torch.randn(N, TOTAL, H, W, generator=gen), torch.randn(N, TOTAL, H, W, generator=gen)
        for rows in (rows_a, rows_a - 32):
            gamma = torch.rand(rows, generator=gen) + 0.5
            gamma[torch.rand(rows, generator=gen) < 0.3] *= -1.0                       # negative gammas included
            layers.append((torch.randn(N, WIDTH, H, W, generator=gen), torch.randn(WIDTH, rows, generator=gen) / WIDTH ** 0.5,
                           torch.randn(rows, generator=gen) * 0.3, (torch.rand(rows, generator=gen) + 0.5).rsqrt(), gamma,
                           torch.randn(rows, generator=gen) * 0.3))
    return x, old, layers


class Scratch:
    """[guard | A's region | guard | B's region | guard], NaN all over before a run."""
    GUARD = 4096

    def __init__(self, rows_a):
        self.at_a = self.GUARD
        self.at_b = self.at_a + 2 * TILES * rows_a + self.GUARD
        self.end = self.at_b + 2 * TILES * (rows_a - 32)
        self.data = torch.full((self.end + self.GUARD,), float('nan'), device='cuda')

    def pointer(self, at):
        return self.data.data_ptr() + 4 * at

    def guards(self):
        return torch.cat((self.data[:self.at_a], self.data[self.at_b - self.GUARD:self.at_b], self.data[self.end:]))


def run(lib, rows_a, x, old, layers, paired, sums, poison=False):
    """Both layers' data gradients accumulated into a copy of `old`: per layer, or as strip + pair.  Returns the buffer
    and the scratch (None without sums).  `poison`: NaN over the rows above B's before the pair launch, checked after."""
    library, stream = lib.library(), lib.stream_handle()
    rows_b = rows_a - 32
    device = [[t.cuda() for t in layer] for layer in layers]
    xd, gx = x.cuda(), old.cuda()
    desc_a, desc_b = layer_desc(lib, rows_a), layer_desc(lib, rows_b)
    bn_a, bn_b = (lib.BnRelu(*(t.data_ptr() for t in layer[2:])) for layer in device)
    (gy_a, w_a), (gy_b, w_b) = ((layer[0].data_ptr(), layer[1].data_ptr()) for layer in device)
    scratch = Scratch(rows_a) if sums else None
    part_a, part_b = (scratch.pointer(scratch.at_a), scratch.pointer(scratch.at_b)) if sums else (None, None)
    if not paired:
        for desc, gy, w, bn, part in ((desc_a, gy_a, w_a, bn_a, part_a), (desc_b, gy_b, w_b, bn_b, part_b)):
            if sums:
                lib.check(library.srgan_conv2d_bwd_data_bnrelu_partials(desc, gy, w, bn, xd.data_ptr(), gx.data_ptr(), part, 1, stream),
                          'per-layer data gradient, partials form')
            else:
                lib.check(library.srgan_conv2d_bwd_data_bnrelu(desc, gy, w, bn, xd.data_ptr(), gx.data_ptr(), None, None, 1, stream),
                          'per-layer data gradient, no sums')
        return gx, scratch
    assert library.srgan_conv2d_bwd_data_bnrelu_pair_supported(desc_a, desc_b) == 1, rows_a
    lib.check(library.srgan_conv2d_bwd_data_bnrelu_strip(desc_a, desc_b, gy_a, w_a, bn_a, xd.data_ptr(), gx.data_ptr(), part_a, stream),
              'strip')
    if poison:
        kept = gx[:, rows_b:].clone()
        gx[:, rows_b:] = float('nan')
    lib.check(library.srgan_conv2d_bwd_data_bnrelu_pair(desc_a, desc_b, gy_a, w_a, bn_a, part_a, gy_b, w_b, bn_b, part_b, xd.data_ptr(),
                                                        gx.data_ptr(), stream), 'pair')
    if poison:
        assert bool(torch.isnan(gx[:, rows_b:]).all()), 'the pair wrote rows above layer B\'s'
        assert bool(torch.isfinite(gx[:, :rows_b]).all())
        gx[:, rows_b:] = kept
    return gx, scratch


@gpu
@pytest.mark.parametrize('rows_a', [224, 192])
@pytest.mark.parametrize('sums', [True, False])
def test_strip_and_pair_give_the_bits_of_the_per_layer_launches(lib, rows_a, sums):
    x, old, layers = operands(rows_a, 41 + rows_a, exact=False)
    reference, reference_scratch = run(lib, rows_a, x, old, layers, paired=False, sums=sums)
    paired, scratch = run(lib, rows_a, x, old, layers, paired=True, sums=sums)
    assert bool((reference[:, :rows_a] != old.cuda()[:, :rows_a]).any())
    same_bits(paired, reference, f'gradient buffer, rows {rows_a} / {rows_a - 32}')
    if sums:
        assert bool(torch.isfinite(reference_scratch.data[scratch.at_a:scratch.at_b - scratch.GUARD]).all())
        assert bool(torch.isfinite(reference_scratch.data[scratch.at_b:scratch.end]).all())
        same_bits(scratch.data, reference_scratch.data, f'partial-sum scratch, rows {rows_a} / {rows_a - 32}')


def restatement(x, old, layers, rows_a):
    """NumPy: per layer gx[:, :rows] += (W^T gy) * [x * a + b > 0] * a with a = inv_std * gamma, b = beta - mean * a, and
    per 128-pixel block and row the sums of the masked gradient and of masked * (x - mean), as [2][tiles][rows]."""
    gx = old.numpy().astype(np.float64).reshape(N, TOTAL, HW)
    xs = x.numpy().astype(np.float64).reshape(N, TOTAL, HW)
    regions = []
    for rows, (gy, weight, mean, inv, gamma, beta) in zip((rows_a, rows_a - 32), layers):
        a = (inv * gamma).numpy().astype(np.float64)[None, :, None]
        mu = mean.numpy().astype(np.float64)[None, :, None]
        b = beta.numpy().astype(np.float64)[None, :, None] - mu * a
        d = np.matmul(weight.numpy().astype(np.float64).T, gy.numpy().astype(np.float64).reshape(N, WIDTH, HW))
        v = np.where(xs[:, :rows] * a + b > 0.0, d, 0.0)
        gx[:, :rows] += v * a
        blocks = lambda t: t.reshape(N, rows, HW // 128, 128).sum(-1).transpose(0, 2, 1).reshape(TILES, rows)
        regions.append(np.stack((blocks(v), blocks(v * (xs[:, :rows] - mu)))))
    return gx.reshape(N, TOTAL, H, W), regions


@gpu
@pytest.mark.parametrize('rows_a', [256, 192])
def test_small_integer_operands_are_exact(lib, rows_a):
    x, old, layers = operands(rows_a, 7 + rows_a, exact=True)
    gx_ref, regions = restatement(x, old, layers, rows_a)
    assert np.abs(gx_ref).max() < 2 ** 24 and max(np.abs(r).max() for r in regions) < 2 ** 24
    assert max(np.abs(r).max() for r in regions) > 1000.0
    for paired in (False, True):
        gx, scratch = run(lib, rows_a, x, old, layers, paired=paired, sums=True, poison=paired)
        what = 'strip + pair' if paired else 'per layer'
        assert np.array_equal(gx.cpu().numpy().astype(np.float64), gx_ref), what + ': gradient buffer'
        for at, region, name in ((scratch.at_a, regions[0], 'A'), (scratch.at_b, regions[1], 'B')):
            got = scratch.data[at:at + region.size].cpu().numpy().astype(np.float64).reshape(region.shape)
            assert np.array_equal(got, region), f'{what}: partial sums of layer {name}'


@gpu
@pytest.mark.parametrize('sums', [True, False])
def test_the_pair_writes_its_own_rows_and_regions_only(lib, sums):
    rows_a = 224
    x, old, layers = operands(rows_a, 3, exact=False)
    gx, scratch = run(lib, rows_a, x, old, layers, paired=True, sums=sums, poison=True)
    same_bits(gx[:, rows_a:], old.cuda()[:, rows_a:], 'rows beyond layer A')
    if sums:
        assert bool(torch.isnan(scratch.guards()).all()), 'scratch outside the two layers\' regions'
        assert bool(torch.isfinite(scratch.data[scratch.at_a:scratch.at_b - scratch.GUARD]).all())
        assert bool(torch.isfinite(scratch.data[scratch.at_b:scratch.end]).all())


def make_block(layers, c0, seed):
    from srgan_amd.crowd.models import _DenseBlock
    torch.manual_seed(seed)
    block = _DenseBlock(num_layers=layers, num_input_features=c0, bn_size=4, growth_rate=32)
    gen = torch.Generator().manual_seed(seed + 1)
    for m in block.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=gen) + 0.5
            m.weight.data[torch.rand(m.weight.shape, generator=gen) < 0.25] *= -1.0
            m.bias.data = torch.randn(m.bias.shape, generator=gen) * 0.2
            m.running_mean.data = torch.randn(m.running_mean.shape, generator=gen) * 0.2
            m.running_var.data = torch.rand(m.running_var.shape, generator=gen) + 0.5
    return block, gen


# (layers, c0, the pairs (A, B) by layer index that run as strip + pair)
BLOCKS = [(4, 128, [(3, 2)]), (6, 64, [(5, 4)]), (5, 128, [(4, 3), (2, 1)])]


@gpu
@pytest.mark.parametrize('layers,c0,pairs', BLOCKS)
def test_dense_block_backward_with_and_without_pairs(lib, layers, c0, pairs):
    """fused.dense_block: first-order backward with trainable parameters (partials form), with frozen parameters (no
    sums), the recorded backward (no sums) and the double backward behind it -- PAIRED_DGRAD on against off, bit for bit;
    and the launches really are the expected strips and pairs."""
    from srgan_amd import functional as F, fused, nn
    from srgan_amd.tape import backward
    block, gen = make_block(layers, c0, 11 * layers)
    arena = nn.flatten_parameters(block, torch.device('cuda', 0))
    out_channels = c0 + 32 * layers
    x_host = torch.randn(N, c0, H, W, generator=gen)
    cotangent = torch.randn(N, out_channels, H, W, generator=gen)
    head = F.leaf(torch.randn(out_channels, generator=gen).cuda(), requires_grad=True)
    calls = []
    original = F._call

    def counting(name, *args):
        if name in ('srgan_conv2d_bwd_data_bnrelu_strip', 'srgan_conv2d_bwd_data_bnrelu_pair'):
            calls.append((name.rsplit('_', 1)[1], args[0].C, args[1].C))
        return original(name, *args)

    results = {}
    F._call = counting
    try:
        for on in (False, True):
            fused.PAIRED_DGRAD = on
            del calls[:]
            arena.zero_grad()
            x = F.leaf(x_host.cuda(), requires_grad=True)
            backward(block(x), grad=F.leaf(cotangent.cuda()))
            first = (x.grad.data.clone(), arena.grad.data.clone())
            arena.zero_grad()
            with nn.frozen_parameters(block):
                x = F.leaf(x_host.cuda(), requires_grad=True)
                y = block(x)
            backward(y, grad=F.leaf(cotangent.cuda()))
            frozen = x.grad.data.clone()
            arena.zero_grad()
            head.grad = None
            x = F.leaf(x_host.cuda(), requires_grad=True)
            scalar = F.sum_all(F.mul(F.chan_affine(block(x), None, head, None, None), F.leaf(cotangent.cuda())))
            (gx,) = backward(scalar, inputs=[x], create_graph=True)
            penalty = F.mean_all(F.square(F.add_scalar(F.row_norm(F.flatten2d(gx)), -1.0)))
            backward(penalty)
            results[on] = first + (frozen, gx.data.clone(), arena.grad.data.clone(), head.grad.data.clone())
            expected = [(kind, c0 + 32 * a, c0 + 32 * b) for a, b in pairs for kind in ('strip', 'pair')] if on else []
            assert calls == expected * 3, (on, calls)
    finally:
        F._call = original
        fused.PAIRED_DGRAD = True
    names = ('input gradient', 'parameter gradients', 'input gradient with frozen parameters', 'recorded input gradient',
             'parameter gradients of the penalty', 'head gradient of the penalty')
    for name, paired, per_layer in zip(names, results[True], results[False]):
        assert bool(torch.isfinite(per_layer).all()) and float(per_layer.abs().max()) > 0.0, name
        same_bits(paired, per_layer, f'{layers} layers from {c0} channels: {name}')
