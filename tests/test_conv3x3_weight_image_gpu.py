"""The fp32 3x3 convolutions of the dense layers with their weights staged from per-step packed weight images
(``srgan_conv2d_*_bnrelu_image``, ``blocked16.Conv3x3ImageShadow``): the packers against the NumPy restatement of the layout,
the packed calls BIT FOR BIT against the calls that gather from the masters (and against float64 on exact operands), the images
following in-place edits / optimizer updates / a HIP-graph replay, and one whole crowd iteration with and without
``SRGAN_NO_CONV3_IMAGE=1``.

Run as a program (``python tests/test_conv3x3_weight_image_gpu.py OUT.npz``) the file is the child of the step-level test: one
iteration of the 64 x 64 crowd configuration (the shapes of golden g7b), its losses and weight arenas written to OUT.npz."""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')

# (direction, N, reduced -> rows channels of the kernel, H, W, what the plan of conv_plan.h gives: (bm, bn = 32 * th, split))
# The first block holds the cases of the issue; `exact`: also checked against float64 on small-integer operands.  The second
# block reaches the tile variants that need 512 workgroups (TH 8 and the 64-row tiles), compared packed == gathered only.
FORWARD_CASES = [
    (2, 128, 32, 16, 16, (32, 128, 8), True),       # TW 16, K split
    (2, 128, 32, 32, 32, (32, 128, 8), True),       # TH 4, K split
    (1, 128, 32, 64, 64, (32, 128, 8), True),       # (TH 8 needs 512 workgroups: below)
    (2, 12, 40, 20, 40, (32, 128, 1), True),        # partial chunk, partial row tile, ragged plane
    (32, 16, 32, 64, 64, (32, 256, 1), False),      # <32, 8>
    (16, 16, 64, 64, 64, (64, 128, 1), False),      # <64, 4>
    (32, 16, 64, 64, 64, (64, 256, 1), False),      # <64, 8>
    (256, 16, 64, 16, 16, (64, 128, 1), False),     # <64, 4, TW 16>
]
DATA_CASES = [
    (2, 32, 128, 16, 16, (32, 128, 1), True),
    (2, 32, 128, 32, 32, (32, 128, 1), True),
    (1, 32, 128, 64, 64, (32, 128, 1), True),
    (2, 40, 12, 20, 40, (32, 128, 1), True),
    (32, 16, 32, 64, 64, (32, 256, 1), False),
    (16, 16, 64, 64, 64, (64, 128, 1), False),
    (32, 16, 64, 64, 64, (64, 256, 1), False),
    (256, 16, 64, 16, 16, (64, 128, 1), False),
]


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib.library()


def _abi():
    from srgan_amd import _lib
    return _lib


def check(status, what):
    _abi().check(status, what)


def stream():
    return _abi().stream_handle()


def desc_of(n, c, h, w, k):
    return _abi().ConvDesc(n, c, h, w, k, 3, 3, 1, 1, 1, 1, h, w, 0, 0, 0)


def nans(*shape):
    return torch.full(shape, NAN, device='cuda')


def pack_images(lib, weight):
    """(forward, transposed) images of the device weights [K][C][3][3] by the single-layer packer, over NaN-filled buffers."""
    k, c = weight.shape[:2]
    images = []
    for transposed, (rows, reduced) in enumerate(((k, c), (c, k))):
        image = nans(int(lib.srgan_conv3x3_image_floats(reduced, rows)))
        check(lib.srgan_h_pack_conv3x3_image(weight.data_ptr(), image.data_ptr(), k, c, transposed, stream()),
              'srgan_h_pack_conv3x3_image')
        images.append(image)
    return images


# ---------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize('ci,co', [(12, 32), (32, 40), (128, 32), (32, 128)])
def test_packers_write_the_restated_layout(lib, ci, co):
    """Both directions by the single-layer packer and as jobs of ``srgan_h_pack_batched``: exactly the NumPy restatement, the
    padding zeros included (the buffers start as NaN), and the two packers byte for byte."""
    from test_conv3x3_weight_image_cpu import image_reference
    generator = torch.Generator().manual_seed(ci * 1000 + co)
    weight = torch.randn(co, ci, 3, 3, generator=generator)
    device_weight = weight.cuda()
    single = pack_images(lib, device_weight)
    size = lib.srgan_h_pack_job_bytes()
    host = ctypes.create_string_buffer(2 * size)
    batched, blocks = [], 0
    for transposed, (rows, reduced) in enumerate(((co, ci), (ci, co))):
        image = nans(int(lib.srgan_conv3x3_image_floats(reduced, rows)))
        taken = lib.srgan_h_pack_job_conv3x3_image(ctypes.byref(host, transposed * size), blocks, device_weight.data_ptr(),
                                                   image.data_ptr(), co, ci, transposed)
        assert taken > 0
        blocks += taken
        batched.append(image)
    table = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).cuda()
    check(lib.srgan_h_pack_batched(table.data_ptr(), 2, blocks, stream()), 'srgan_h_pack_batched')
    torch.cuda.synchronize()
    for transposed in (0, 1):
        want = image_reference(weight.numpy(), transposed)
        got = single[transposed].cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got, want), f'{ci}->{co} transposed={transposed}: {(got != want).sum()} elements differ'
        assert single[transposed].cpu().numpy().tobytes() == batched[transposed].cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------- kernel parity
def report_rows(lib, run):
    """``run()`` inside a live-profile bracket: the conv3x3_lds rows of the shape report as (bm, bn, split, from_image)."""
    from helpers import profiled
    with profiled(lib) as report:
        run()
    rows = []
    for line in report.text.splitlines():
        fields = line.split()
        if len(fields) >= 9 and int(fields[3]) == 2:
            rows.append((int(fields[4]), int(fields[5]), int(fields[6]), int(fields[7])))
    return rows


def bn_vectors(channels, generator, exact):
    from test_exact_contractions_gpu import bn_operands
    if exact:
        return {name: value.float() for name, value in bn_operands(channels, generator).items()}
    return dict(mean=torch.randn(channels, generator=generator) * 0.3, inv=torch.rand(channels, generator=generator) + 0.5,
                gamma=torch.rand(channels, generator=generator) + 0.5, beta=torch.randn(channels, generator=generator) * 0.3)


def bn_struct(vectors):
    device = {name: value.cuda() for name, value in vectors.items()}
    return _abi().BnRelu(device['mean'].data_ptr(), device['inv'].data_ptr(), device['gamma'].data_ptr(),
                         device['beta'].data_ptr()), device


def bn_pre(x, v):
    view = lambda t: t.double().view(1, -1, 1, 1)
    return (x.double() - view(v['mean'])) * view(v['inv']) * view(v['gamma']) + view(v['beta'])


def operands(shape, generator, exact, bound=3, keep=1.0):
    if not exact:
        return torch.randn(shape, generator=generator)
    values = torch.randint(-bound, bound + 1, shape, generator=generator).float()
    if keep < 1.0:
        values *= (torch.rand(shape, generator=generator) < keep).float()
    return values


def run_forward(lib, case, exact):
    n, ci, co, h, w, plan, _ = case
    generator = torch.Generator().manual_seed(zlib.crc32(repr(('forward', n, ci, co, h, w, exact)).encode()))
    x, weight = operands((n, ci, h, w), generator, exact), operands((co, ci, 3, 3), generator, exact, 2)
    v = bn_vectors(ci, generator, exact)
    bn, keep = bn_struct(v)
    dx, dw = x.cuda(), weight.cuda()
    forward_image, _ = pack_images(lib, dw)
    desc = desc_of(n, ci, h, w, co)
    gathered, packed = nans(n, co, h, w), nans(n, co, h, w)
    check(lib.srgan_conv2d_fwd_bnrelu(desc, dx.data_ptr(), bn, dw.data_ptr(), None, gathered.data_ptr(), stream()),
          'srgan_conv2d_fwd_bnrelu')
    rows = report_rows(lib, lambda: check(lib.srgan_conv2d_fwd_bnrelu_image(
        desc, dx.data_ptr(), bn, dw.data_ptr(), forward_image.data_ptr(), None, packed.data_ptr(), stream()),
        'srgan_conv2d_fwd_bnrelu_image'))
    assert rows == [plan + (1,)], (case, rows)                      # the tile and split the table says, weights from the image
    assert not torch.isnan(packed).any()
    assert torch.equal(packed, gathered), f'forward {case}: {int((packed != gathered).sum())} elements differ'
    if exact:
        act = bn_pre(x, v).relu()
        want = TF.conv2d(act, weight.double(), None, 1, 1)
        assert float(TF.conv2d(act, weight.double().abs(), None, 1, 1).max()) < 2 ** 22      # quarter steps: sums exact in fp32
        assert torch.equal(packed.cpu().double(), want), f'forward {case} against float64'


@pytest.mark.parametrize('case', FORWARD_CASES, ids=lambda c: 'x'.join(map(str, c[:5])))
def test_forward_from_the_image_equals_the_gathered_forward(lib, case):
    run_forward(lib, case, False)
    if case[6]:
        run_forward(lib, case, True)


def run_data_gradient(lib, case, exact):
    """The kernel's reduced channels are the convolution's OUTPUT channels k (gy), its rows the input channels c (gx)."""
    n, k, c, h, w, plan, _ = case
    generator = torch.Generator().manual_seed(zlib.crc32(repr(('data', n, k, c, h, w, exact)).encode()))
    x = operands((n, c, h, w), generator, exact)
    gy = operands((n, k, h, w), generator, exact, 1, 0.25)
    weight = operands((k, c, 3, 3), generator, exact, 1)
    v = bn_vectors(c, generator, exact)
    bn, keep = bn_struct(v)
    dx, dgy, dw = x.cuda(), gy.cuda(), weight.cuda()
    _, transposed_image = pack_images(lib, dw)
    desc = desc_of(n, c, h, w, k)
    assert lib.srgan_conv2d_bnrelu_supported(desc, 1) == 1
    tiles = int(lib.srgan_conv2d_bwd_data_bnrelu_tiles(desc))
    assert tiles > 0
    gx = {name: nans(n, c, h, w) for name in ('gathered', 'packed', 'gathered_partials', 'packed_partials')}
    sums = {name: torch.zeros(2, c, device='cuda') for name in ('gathered', 'packed')}
    partials = {name: nans(2 * tiles * c) for name in ('gathered', 'packed')}
    check(lib.srgan_conv2d_bwd_data_bnrelu(desc, dgy.data_ptr(), dw.data_ptr(), bn, dx.data_ptr(), gx['gathered'].data_ptr(),
                                           sums['gathered'][0].data_ptr(), sums['gathered'][1].data_ptr(), 0, stream()),
          'srgan_conv2d_bwd_data_bnrelu')
    check(lib.srgan_conv2d_bwd_data_bnrelu_partials(desc, dgy.data_ptr(), dw.data_ptr(), bn, dx.data_ptr(),
                                                    gx['gathered_partials'].data_ptr(), partials['gathered'].data_ptr(), 0, stream()),
          'srgan_conv2d_bwd_data_bnrelu_partials')

    def packed_calls():
        check(lib.srgan_conv2d_bwd_data_bnrelu_image(desc, dgy.data_ptr(), dw.data_ptr(), transposed_image.data_ptr(), bn,
                                                     dx.data_ptr(), gx['packed'].data_ptr(), sums['packed'][0].data_ptr(),
                                                     sums['packed'][1].data_ptr(), 0, stream()), 'srgan_conv2d_bwd_data_bnrelu_image')
        check(lib.srgan_conv2d_bwd_data_bnrelu_partials_image(desc, dgy.data_ptr(), dw.data_ptr(), transposed_image.data_ptr(), bn,
                                                              dx.data_ptr(), gx['packed_partials'].data_ptr(),
                                                              partials['packed'].data_ptr(), 0, stream()),
              'srgan_conv2d_bwd_data_bnrelu_partials_image')
    rows = report_rows(lib, packed_calls)
    assert rows == [plan + (1,)], (case, rows)                      # both launches on the same row (count 2)
    for name in ('packed', 'packed_partials', 'gathered_partials'):
        assert not torch.isnan(gx[name]).any()
        assert torch.equal(gx[name], gx['gathered']), f'data gradient {case} {name}'
    assert torch.equal(sums['packed'], sums['gathered']), f'data gradient {case}: the two parameter-sum rows'
    assert not torch.isnan(partials['packed']).any()
    assert torch.equal(partials['packed'], partials['gathered']), f'data gradient {case}: the partials'
    if exact:
        pre = bn_pre(x, v)
        mask = (pre > 0).double()
        scale = (v['inv'].double() * v['gamma'].double()).view(1, -1, 1, 1)
        xhat = (x.double() - v['mean'].double().view(1, -1, 1, 1)) * v['inv'].double().view(1, -1, 1, 1)
        g_act = torch.nn.grad.conv2d_input((n, c, h, w), weight.double(), gy.double(), 1, 1) * mask
        g_abs = torch.nn.grad.conv2d_input((n, c, h, w), weight.double().abs(), gy.double().abs(), 1, 1) * mask
        largest = max(float((g_abs * scale).max()), float((g_abs * xhat.abs()).sum(dim=(0, 2, 3)).max()),
                      float(g_abs.sum(dim=(0, 2, 3)).max()))
        assert largest < 2 ** 22, f'{case}: a partial sum reaches {largest:g}: the case is broken'
        assert torch.equal(gx['packed'].cpu().double(), g_act * scale), f'data gradient {case} against float64'
        assert torch.equal(sums['packed'][0].cpu().double(), (g_act * xhat).sum(dim=(0, 2, 3))), f'{case} gamma sums'
        assert torch.equal(sums['packed'][1].cpu().double(), g_act.sum(dim=(0, 2, 3))), f'{case} beta sums'


@pytest.mark.parametrize('case', DATA_CASES, ids=lambda c: 'x'.join(map(str, c[:5])))
def test_data_gradient_from_the_image_equals_the_gathered_data_gradient(lib, case):
    run_data_gradient(lib, case, False)
    if case[6]:
        run_data_gradient(lib, case, True)


# ---------------------------------------------------------------------------------------------------------- freshness
def _dense_block():
    """A dense block whose geometry takes the in-kernel batch-norm forms (test_ops_gpu's), its parameters in an arena."""
    import srgan_amd  # noqa: F401
    from srgan_amd import nn
    from srgan_amd.crowd.models import _DenseBlock
    torch.manual_seed(5)
    block = _DenseBlock(num_layers=3, num_input_features=32, bn_size=4, growth_rate=8)
    generator = torch.Generator().manual_seed(6)
    for m in block.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=generator) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=generator) * 0.2
            m.running_mean.data = torch.randn(m.running_mean.shape, generator=generator) * 0.2
            m.running_var.data = torch.rand(m.running_var.shape, generator=generator) + 0.5
    arena = nn.flatten_parameters(block, torch.device('cuda', 0))
    x = torch.randn(2, 32, 16, 16, generator=generator).cuda()
    cotangent = torch.randn(2, 56, 16, 16, generator=generator).cuda()
    return block, arena, x, cotangent


def _block_pass(block, arena, x_data, cotangent, with_image):
    """Forward, plain backward (input and parameter gradients) and the recorded backward of the gradient penalty, with the 3x3
    weights staged from the images or gathered from the masters: (y, gx, parameter gradients, recorded gx)."""
    from srgan_amd import fused
    from srgan_amd import functional as F
    from srgan_amd.tape import backward
    fused.WEIGHT_IMAGE = with_image
    try:
        arena.zero_grad()
        x = F.leaf(x_data.clone(), requires_grad=True)
        y = block(x)
        backward(y, grad=F.leaf(cotangent.clone()))
        first = (y.data.clone(), x.grad.data.clone(), arena.grad.detach().clone())
        x = F.leaf(x_data.clone(), requires_grad=True)
        scalar = F.sum_all(F.mul(block(x), F.leaf(cotangent.clone())))
        (gx,) = backward(scalar, inputs=[x], create_graph=True)
        return first + (gx.data.clone(),)
    finally:
        fused.WEIGHT_IMAGE = True


def _assert_same(got, want, what):
    for name, a, b in zip(('output', 'input gradient', 'parameter gradients', 'recorded input gradient'), got, want):
        assert torch.equal(a, b), f'{what}: {name} differs in {int((a != b).sum())} elements'


def test_images_follow_an_edit_an_update_and_a_replay(lib):
    """A first pass, a weight edited in place, then one ``Adam.step()``: every time the pass that stages from the images equals
    the pass that gathers from the masters, bit for bit.  Then an eager and a captured, replayed block forward on one stream:
    replay equals eager."""
    from srgan_amd import blocked16, fused
    from srgan_amd import functional as F
    from srgan_amd.optim import Adam
    from srgan_amd.tape import no_grad
    block, arena, x, cotangent = _dense_block()
    first = _block_pass(block, arena, x, cotangent, True)
    images = [s for s in arena.shadows if s.kind == 'conv3x3_image']
    assert len(images) == 3, 'the block did not ask for the weight images of its three layers'
    rows = report_rows(lib, lambda: _block_pass(block, arena, x, cotangent, True))
    assert rows and all(row[3] == 1 for row in rows), rows            # every 3x3 launch of the pass staged from an image
    rows = report_rows(lib, lambda: _block_pass(block, arena, x, cotangent, False))
    assert rows and all(row[3] == 0 for row in rows), rows            # ... and with the switch off none did
    _assert_same(first, _block_pass(block, arena, x, cotangent, False), 'first pass')

    layer = [m for m in block.children()][1]
    with torch.no_grad():
        layer.conv2.weight.mul_(1.5)                                  # in place: the version key moves, the image is re-packed
    edited = _block_pass(block, arena, x, cotangent, True)
    assert not torch.equal(edited[0], first[0])
    _assert_same(edited, _block_pass(block, arena, x, cotangent, False), 'after an in-place edit')

    optimizer = Adam(arena, lr=1e-2)
    optimizer.step()                                                  # raw-pointer update; the batched refresh behind it
    assert not blocked16.stale(arena)
    updated = _block_pass(block, arena, x, cotangent, True)
    assert not torch.equal(updated[0], edited[0])
    _assert_same(updated, _block_pass(block, arena, x, cotangent, False), 'after Adam.step()')

    # capture: the images exist and are current (blocked16.prepare); the capture records launches only
    blocked16.prepare(arena)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), no_grad():
        eager = block(F.leaf(x)).data.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = block(F.leaf(x)).data
        captured.fill_(NAN)
        graph.replay()
    side.synchronize()
    assert torch.equal(captured, eager) and torch.equal(eager, updated[0])


# ---------------------------------------------------------------------------------------------------------- step level
LOSSES = ('labeled_loss', 'unlabeled_loss', 'fake_loss', 'gradient_penalty', 'generator_loss', 'dnn_loss')


def _child(path):
    """One iteration of the 64 x 64 crowd configuration at golden g7b's batch size, seeds and multipliers."""
    from helpers import load_golden
    from test_steps_gpu import make_experiment, finish_setup, crowd_inputs
    import srgan_amd  # noqa: F401
    from srgan_amd.crowd.models import DCGenerator, KnnDenseNetCat
    from srgan_amd.utility import seed_all
    golden = load_golden('g7b_crowd64')
    batch, size = int(golden['batch_size']), 64
    experiment = make_experiment(
        lambda: (DCGenerator(image_size=size), KnnDenseNetCat(image_size=size), KnnDenseNetCat(image_size=size)),
        dict(batch_size=batch, matching_loss_multiplier=1e3, contrasting_loss_multiplier=1e2, gradient_penalty_multiplier=1e2,
             map_multiplier=1e-3), crowd=True)
    finish_setup(experiment)
    seed_all(5)
    generator = torch.Generator().manual_seed(int(golden['input_seed']))
    x, labels, u = crowd_inputs(generator, batch, size)
    experiment.dnn_training_step(x.cuda(), tuple(t.cuda() for t in labels), 1)
    experiment.gan_training_step(x.cuda(), tuple(t.cuda() for t in labels), u.cuda(), 1)
    torch.cuda.synchronize()
    out = {'loss/' + name: np.float32(value.item()) for name, value in experiment.last_losses.items() if value is not None}
    for name in ('D', 'DNN', 'G'):
        out['arena/' + name] = getattr(experiment, name)._srgan_arena.data.cpu().numpy()
    out['image_shadows'] = np.int64(sum(s.kind == 'conv3x3_image' for s in experiment.D._srgan_arena.shadows))
    np.savez(path, **out)


def test_a_crowd_iteration_is_bit_identical_with_and_without_the_images(tmp_path):
    results = {}
    for switch in ('0', '1'):
        path = str(tmp_path / f'step_{switch}.npz')
        environment = dict(os.environ, SRGAN_NO_CONV3_IMAGE=switch)
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=environment, cwd=ROOT, timeout=600)
        results[switch] = np.load(path)
    with_images, without = results['0'], results['1']
    assert int(with_images['image_shadows']) > 0
    for key in ['loss/' + name for name in LOSSES]:
        assert np.isfinite(with_images[key]) and with_images[key].tobytes() == without[key].tobytes(), key
    for name in ('D', 'DNN', 'G'):
        assert with_images['arena/' + name].tobytes() == without['arena/' + name].tobytes(), name


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    _child(sys.argv[1])
