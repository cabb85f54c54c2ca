"""Every fp32 contraction kernel path (and the mixed-precision 3x3 kernels' store modes) on exact operands, bit for bit
against float64.

Operands are small integers (x, gy in [-3, 3], weights in [-2, 2], biases in [-4, 4]) or dyadic values of a few bits (the fused
batch-norm activations are quarter steps).  Every partial sum stays below 2^(24 - f) in magnitude, f = the operands' fractional
bits -- asserted per case on the |x| / |w| contraction in float64 -- so fp32 addition is exact in any order: every correct kernel,
whatever its tile, K split, finish order or fp32 atomics, reproduces the float64 result exactly, and one dropped, doubled or
misplaced term anywhere fails.  Store-mode outputs start as NaN (an element never written fails); accumulate-mode outputs start
as distinct random integers (an epilogue that reads another element's old value fails).

Each convolution case runs inside a profile bracket and asserts that the kinds its table entry (contraction_cases.py) declares
were launched.  test_the_file_again_with_fp32_atomic_combines re-runs the file with SRGAN_ATOMIC_SPLIT=1, where the K slices
meet through fp32 atomics instead of the ordered finishes and partial buffers.
"""
import ctypes
import functools
import os
import subprocess
import sys
import time
import zlib

import pytest
import torch
import torch.nn.functional as TF

from helpers import assert_exact, profiled
from contraction_cases import (B, BN_DATA_CASES, BN_FORWARD_CASES, CONV_CASES, CONVT_CASES, EXACT_LIMIT, FUSED_WGRAD_REACH,
                               GEMM_CASES, GROUPED_WGRAD_CASES, GROUPED_WGRAD_REACH, PREFILL, W, X, direct_is_cheap)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')


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


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def ints(shape, bound, generator):
    """Integers in [-bound, bound] as float64 (CPU)."""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=generator).double()


def pick(values, shape, generator):
    values = torch.tensor(values, dtype=torch.float64)
    return values[torch.randint(0, len(values), tuple(shape), generator=generator)]


def prefill(shape, generator):
    return ints(shape, PREFILL, generator)


def cuda(t):
    return t.float().cuda()


def nans(shape):
    return torch.full(tuple(shape), NAN, device='cuda')


def assert_limit(magnitude, fraction_bits, what):
    """The precondition of exactness: the largest partial sum (the contraction of the absolute operands, plus prefill / bias)
    below 2^(24 - f)."""
    limit = EXACT_LIMIT >> fraction_bits
    assert magnitude < limit, f'{what}: a partial sum reaches {magnitude:g} >= 2^{24 - fraction_bits}: the case is broken'


# ------------------------------------------------------------------------------------------------- convolutions
def desc_of(shape, x_batch_stride=0, y_batch_stride=0, compute_dtype=0):
    n, c, h, w, k, r, s, stride, pad = shape
    oh, ow = (h + 2 * pad[0] - r) // stride[0] + 1, (w + 2 * pad[1] - s) // stride[1] + 1
    return _abi().ConvDesc(n, c, h, w, k, r, s, stride[0], stride[1], pad[0], pad[1], oh, ow, x_batch_stride, y_batch_stride,
                           compute_dtype)


@functools.lru_cache(maxsize=1)
def conv_problem(shape):
    """Operands, float64 results and the precondition of one table shape (cached across the force values of a case)."""
    n, c, h, w, k, r, s, stride, pad = shape
    generator = torch.Generator().manual_seed(seed_of(shape))
    x = ints((n, c, h, w), X, generator)
    weight = ints((k, c, r, s), W, generator)
    bias_k, bias_c = ints((k,), B, generator), ints((c,), B, generator)
    y = TF.conv2d(x, weight, None, stride, pad)
    gy = ints(y.shape, X, generator)
    gx = torch.nn.grad.conv2d_input(x.shape, weight, gy, stride, pad)
    gw = torch.nn.grad.conv2d_weight(x, weight.shape, gy, stride, pad)
    # precondition: the same contractions on absolute values, plus the largest bias and prefill
    largest = max(float(TF.conv2d(x.abs(), weight.abs(), None, stride, pad).max()) + B,
                  float(torch.nn.grad.conv2d_input(x.shape, weight.abs(), gy.abs(), stride, pad).max()) + B,
                  float(torch.nn.grad.conv2d_weight(x.abs(), weight.shape, gy.abs(), stride, pad).max())) + PREFILL
    prefills = dict(old_gx=prefill(x.shape, generator), old_gw=prefill(weight.shape, generator))
    return dict(x=x, weight=weight, bias_k=bias_k, bias_c=bias_c, y=y, gy=gy, gx=gx, gw=gw, largest=largest, **prefills)


def conv_params():
    params = []
    for index, entry in enumerate(CONV_CASES):
        n, c, h, w, k, r, s, stride, pad = entry.shape
        name = f'{n}x{c}x{h}x{w}-k{k}-{r}x{s}-s{stride[0]}{stride[1]}-p{pad[0]}{pad[1]}'
        for force in (0, 1, 2):
            if force != 1 or direct_is_cheap(entry.shape):
                params.append(pytest.param(entry, force, id=f'{name}-force{force}'))
    return params


@pytest.mark.parametrize('entry,force', conv_params())
def test_convolution_passes_are_exact(lib, entry, force):
    """Forward (with and without bias), data gradient (stored with and without a bias on the input channels -- the transposed
    convolution's form -- and accumulated with and without it) and weight gradient (stored, accumulated) of one table shape."""
    shape = entry.shape
    p = conv_problem(shape)
    assert_limit(p['largest'], 0, f'{shape}')
    desc = desc_of(shape)
    x, weight, gy = cuda(p['x']), cuda(p['weight']), cuda(p['gy'])
    bias_k, bias_c = cuda(p['bias_k']), cuda(p['bias_c'])
    what = f'{shape} force={force}'
    with profiled(lib) as report:
        for bias, want in ((None, p['y']), (bias_k, p['y'] + p['bias_k'].view(1, -1, 1, 1))):
            y = nans(p['y'].shape)
            check(lib.srgan_conv2d_fwd(desc, x.data_ptr(), weight.data_ptr(), bias.data_ptr() if bias is not None else None,
                                       y.data_ptr(), force, stream()), 'srgan_conv2d_fwd')
            assert_exact(y, want, f'{what} forward bias={bias is not None}')
        for accumulate in (0, 1):
            for bias in (None, bias_c):
                start = p['old_gx'] if accumulate else torch.full(p['x'].shape, NAN, dtype=torch.float64)
                gx = cuda(start)
                check(lib.srgan_conv2d_bwd_data(desc, gy.data_ptr(), weight.data_ptr(),
                                                bias.data_ptr() if bias is not None else None, gx.data_ptr(), accumulate, force,
                                                stream()), 'srgan_conv2d_bwd_data')
                want = p['gx'] + (p['bias_c'].view(1, -1, 1, 1) if bias is not None else 0.0)
                assert_exact(gx, want + (start if accumulate else 0.0),
                             f'{what} data gradient accumulate={accumulate} bias={bias is not None}')
        for accumulate in (0, 1):
            start = p['old_gw'] if accumulate else torch.full(p['weight'].shape, NAN, dtype=torch.float64)
            gw = cuda(start)
            check(lib.srgan_conv2d_bwd_weight(desc, x.data_ptr(), gy.data_ptr(), gw.data_ptr(), accumulate, force, stream()),
                  'srgan_conv2d_bwd_weight')
            assert_exact(gw, p['gw'] + (start if accumulate else 0.0), f'{what} weight gradient accumulate={accumulate}',
                         ('k', 'c', 'r', 's'))
    if force == 0:
        report.assert_reached(entry.reach, entry.split, what)
    else:                                   # the cross-checks run the generic kernels only: direct (1) or MFMA (2)
        assert report.kinds == {0 if force == 1 else 1}, f'{what}: launched {sorted(report.kinds)}\n{report.text}'


# The two mixed-precision 3x3 kernels of conv3x3.hip (a tile of one image; whole 4 x 4 / 8 x 8 images side by side) with
# bf16 / fp16 operands, which hold the integers above exactly: (n, c, h, w, k, the data gradient's K slices).  Only the data
# gradient has an accumulate argument, and its reduction runs over k: the shapes with k <= 48 (fewer than four 16-channel
# chunks) stay unsplit -- store and accumulate --, the others split K -- ordered finish storing and accumulating here,
# fp32 atomics onto the live output in the re-run below.  Small planes: 16 chunks on 8 workgroups; a ragged image group
# (19 images, 8 per workgroup) with channel tails, split and (c and k swapped) unsplit.  Tiles: the 16-wide tile; channel
# tails on a 7-wide plane, split and unsplit.
MIXED_3X3_CASES = [(32, 256, 4, 4, 128, True), (19, 40, 4, 4, 72, True), (19, 72, 4, 4, 40, False),
                   (2, 64, 16, 16, 64, True), (1, 130, 9, 7, 70, True), (1, 130, 9, 7, 40, False)]


@pytest.mark.parametrize('dtype', [1, 2], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', MIXED_3X3_CASES, ids=lambda c: 'x'.join(map(str, c[:5])))
def test_mixed_3x3_store_modes_are_exact(lib, case, dtype):
    """Forward (stored, with bias) and data gradient (stored and accumulated, with bias) of the mixed-precision 3x3 kernels."""
    n, c, h, w, k, splits = case
    shape = (n, c, h, w, k, 3, 3, (1, 1), (1, 1))
    p = conv_problem(shape)
    assert_limit(p['largest'], 0, f'{shape}')
    desc = desc_of(shape, compute_dtype=dtype)
    x, weight, gy, bias_k, bias_c = cuda(p['x']), cuda(p['weight']), cuda(p['gy']), cuda(p['bias_k']), cuda(p['bias_c'])
    what = f'mixed 3x3 {case} dtype={dtype}'
    with profiled(lib) as forward:
        y = nans(p['y'].shape)
        check(lib.srgan_conv2d_fwd(desc, x.data_ptr(), weight.data_ptr(), bias_k.data_ptr(), y.data_ptr(), 0, stream()),
              'srgan_conv2d_fwd')
        assert_exact(y, p['y'] + p['bias_k'].view(1, -1, 1, 1), f'{what} forward')
    with profiled(lib) as backward:
        for accumulate in (0, 1):
            start = p['old_gx'] if accumulate else torch.full(p['x'].shape, NAN, dtype=torch.float64)
            gx = cuda(start)
            check(lib.srgan_conv2d_bwd_data(desc, gy.data_ptr(), weight.data_ptr(), bias_c.data_ptr(), gx.data_ptr(), accumulate, 0,
                                            stream()), 'srgan_conv2d_bwd_data')
            assert_exact(gx, p['gx'] + p['bias_c'].view(1, -1, 1, 1) + (start if accumulate else 0.0),
                         f'{what} data gradient accumulate={accumulate}')
    assert forward.kinds == {2} and backward.kinds == {2}, f'{what}: not the 3x3 kernel\n{forward.text}{backward.text}'
    assert {line[6] > 1 for line in backward.lines} == {splits}, f'{what}: K slices\n{backward.text}'


@pytest.mark.parametrize('force', [0, 2])
@pytest.mark.parametrize('case', CONVT_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_transposed_convolutions_are_exact(lib, case, force):
    """conv_transpose2d (the data gradient with a bias on its output channels) at test_conv_transpose's shapes, stored and
    accumulated."""
    cin, cout, k, s, p, hin, batch = case
    generator = torch.Generator().manual_seed(seed_of('convT', case))
    z, weight, bias = ints((batch, cin, hin, hin), X, generator), ints((cin, cout, k, k), W, generator), ints((cout,), B, generator)
    want = TF.conv_transpose2d(z, weight, bias, stride=s, padding=p)
    largest = float(TF.conv_transpose2d(z.abs(), weight.abs(), None, stride=s, padding=p).max()) + B + PREFILL
    assert_limit(largest, 0, f'convT {case}')
    hout = want.shape[2]
    desc = desc_of((batch, cout, hout, hout, cin, k, k, (s, s), (p, p)))
    assert desc.OH == hin
    old = prefill(want.shape, generator)
    dz, dw, db = cuda(z), cuda(weight), cuda(bias)
    with profiled(lib) as report:
        for accumulate in (0, 1):
            out = cuda(old) if accumulate else nans(want.shape)
            check(lib.srgan_conv2d_bwd_data(desc, dz.data_ptr(), dw.data_ptr(), db.data_ptr(), out.data_ptr(), accumulate, force,
                                            stream()), 'srgan_conv2d_bwd_data')
            assert_exact(out, want + (old if accumulate else 0.0), f'convT {case} force={force} accumulate={accumulate}')
    if force == 2:
        assert report.kinds == {1}, report.text


# ------------------------------------------------------------------------------------------------- matrix multiplies
@pytest.mark.parametrize('force', [0, 2])
@pytest.mark.parametrize('entry', GEMM_CASES, ids=lambda e: 'x'.join(map(str, e.shape)))
def test_gemm_is_exact_in_every_layout(lib, entry, force):
    """srgan_gemm at test_linear_and_mm's shapes: the five products of a linear layer's passes (x w^T, g w, g^T x, x^T g,
    w x^T), each in all four operand layouts, bias on rows and on columns, stored and accumulated."""
    batch, fin, fout = entry.shape
    problems = [(batch, fout, fin), (batch, fin, fout), (fout, fin, batch), (fin, fout, batch), (fout, batch, fin)]
    generator = torch.Generator().manual_seed(seed_of('gemm', entry.shape))
    with profiled(lib) as report:
        for (m, n, k) in problems:
            a, b = ints((m, k), X, generator), ints((k, n), W, generator)
            bias_rows, bias_cols = ints((m,), B, generator), ints((n,), B, generator)
            product = a @ b
            assert_limit(float((a.abs() @ b.abs()).max()) + B + PREFILL, 0, f'gemm {m}x{n}x{k}')
            old = prefill((m, n), generator)
            for ta in (False, True):
                for tb in (False, True):
                    da = cuda(a.t().contiguous() if ta else a)
                    db = cuda(b.t().contiguous() if tb else b)
                    sai, sak = (1, m) if ta else (k, 1)
                    sbk, sbj = (1, k) if tb else (n, 1)
                    for accumulate, bias, on_columns in ((0, None, 1), (0, bias_cols, 1), (0, bias_rows, 0),
                                                         (1, None, 1), (1, bias_cols, 1), (1, bias_rows, 0)):
                        out = cuda(old) if accumulate else nans((m, n))
                        dbias = cuda(bias) if bias is not None else None
                        check(lib.srgan_gemm(m, n, k, da.data_ptr(), sai, sak, db.data_ptr(), sbk, sbj, out.data_ptr(), n, 1,
                                             dbias.data_ptr() if dbias is not None else None, on_columns, accumulate, force, 0,
                                             stream()), 'srgan_gemm')
                        want = product.clone()
                        if bias is not None:
                            want += bias.view(1, -1) if on_columns else bias.view(-1, 1)
                        if accumulate:
                            want += old
                        assert_exact(out, want, f'gemm {m}x{n}x{k} ta={ta} tb={tb} force={force} accumulate={accumulate} '
                                                f'bias={"none" if bias is None else ("columns" if on_columns else "rows")}',
                                     ('row', 'column'))
    if force == 0:
        report.assert_reached(entry.reach, entry.split, f'gemm {entry.shape}')
    else:
        assert report.kinds == {1}, report.text


# ------------------------------------------------------------------------------------------------- fused batch norm
def bn_operands(c, generator):
    """Dyadic frozen batch-norm vectors: relu((x - mean) * inv * gamma + beta) is a quarter-step value for integer x, in any
    folding order."""
    return dict(mean=ints((c,), 1, generator), inv=pick([0.5, 1.0, 2.0], (c,), generator),
                gamma=pick([0.5, 1.0, 1.5], (c,), generator), beta=pick([-1.0, -0.5, 0.0, 0.5, 1.0], (c,), generator))


def bn_pre(x, v):
    view = lambda t: t.view(1, -1, 1, 1)
    return (x - view(v['mean'])) * view(v['inv']) * view(v['gamma']) + view(v['beta'])


def bn_struct(v):
    device = {name: cuda(t) for name, t in v.items()}
    struct = _abi().BnRelu(device['mean'].data_ptr(), device['inv'].data_ptr(), device['gamma'].data_ptr(),
                           device['beta'].data_ptr())
    return struct, device


@pytest.mark.parametrize('case', BN_FORWARD_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_fused_batch_norm_forward_and_weight_gradient_are_exact(lib, case):
    """srgan_conv2d_fwd_bnrelu (stored; _into_zeros where the forward splits K) and srgan_conv2d_bwd_weight_bnrelu (stored and
    accumulated) on a channel slice of a wider buffer, at test_fused_batch_norm_convolutions' shapes."""
    n, c, total, h, w, k, r = case
    pad = r // 2
    generator = torch.Generator().manual_seed(seed_of('bn', case))
    wide = ints((n, total, h, w), X, generator)
    v = bn_operands(c, generator)
    weight, bias = ints((k, c, r, r), W, generator), ints((k,), B, generator)
    act = bn_pre(wide[:, :c], v).relu()
    y_want = TF.conv2d(act, weight, bias, 1, pad)
    gy = ints(y_want.shape, X, generator)
    gw_want = torch.nn.grad.conv2d_weight(act, weight.shape, gy, 1, pad)
    largest = max(float(TF.conv2d(act, weight.abs(), None, 1, pad).max()) + B,
                  float(torch.nn.grad.conv2d_weight(act, weight.shape, gy.abs(), 1, pad).abs().max())) + PREFILL
    assert_limit(largest, 2, f'fused bn {case}')
    desc = desc_of((n, c, h, w, k, r, r, (1, 1), (pad, pad)), total * h * w)
    bn, keep = bn_struct(v)
    d_wide, d_weight, d_bias, d_gy = cuda(wide), cuda(weight), cuda(bias), cuda(gy)
    what = f'fused bn {c}/{total}->{k} k{r} {n}x{h}x{w}'
    y = nans(y_want.shape)
    check(lib.srgan_conv2d_fwd_bnrelu(desc, d_wide.data_ptr(), bn, d_weight.data_ptr(), d_bias.data_ptr(), y.data_ptr(), stream()),
          'srgan_conv2d_fwd_bnrelu')
    assert_exact(y, y_want, what + ' forward')
    if lib.srgan_conv2d_fwd_bnrelu_splits(desc) > 1:
        y = torch.zeros(y_want.shape, device='cuda')
        check(lib.srgan_conv2d_fwd_bnrelu_into_zeros(desc, d_wide.data_ptr(), bn, d_weight.data_ptr(), d_bias.data_ptr(),
                                                     y.data_ptr(), stream()), 'srgan_conv2d_fwd_bnrelu_into_zeros')
        assert_exact(y, y_want, what + ' forward into zeros')
    old = prefill(weight.shape, generator)
    with profiled(lib) as report:
        for accumulate in (1, 0):
            gw = cuda(old) if accumulate else nans(weight.shape)
            check(lib.srgan_conv2d_bwd_weight_bnrelu(desc, d_wide.data_ptr(), bn, d_gy.data_ptr(), gw.data_ptr(), accumulate,
                                                     stream()), 'srgan_conv2d_bwd_weight_bnrelu')
            assert_exact(gw, gw_want + (old if accumulate else 0.0), f'{what} weight gradient accumulate={accumulate}',
                         ('k', 'c', 'r', 's'))
    report.assert_reached(FUSED_WGRAD_REACH[r], False, what + ' weight gradient')


@pytest.mark.parametrize('case', BN_DATA_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_fused_batch_norm_data_gradient_is_exact(lib, case):
    """srgan_conv2d_bwd_data_bnrelu with g_gamma / g_beta, at test_fused_batch_norm_backward_in_the_data_gradient's shapes: gx a
    channel slice of a wider buffer (stored, and accumulated for 1x1), gy a channel slice for 3x3; every output starts as
    random integers.  (Narrower operands than the other tests -- gy, w in [-1, 1], gy sparse on the largest problems -- keep the
    parameter-gradient sums over up to 65536 pixels exact.)"""
    n, c, total, h, w, k, r = case
    pad = r // 2
    generator = torch.Generator().manual_seed(seed_of('bn data', case))
    wide = ints((n, total, h, w), X, generator)
    v = bn_operands(c, generator)
    weight = ints((k, c, r, r), 1, generator)
    gy_wide = ints((n, k + 8, h, w), 1, generator)
    if n * h * w >= 16384:                  # one gy element in eight nonzero: the parameter-gradient sums stay below 2^22
        gy_wide *= (torch.rand(gy_wide.shape, generator=generator) < 0.125).double()
    gy = gy_wide[:, 4:4 + k]
    pre = bn_pre(wide[:, :c], v)
    mask = (pre > 0).double()
    xhat = (wide[:, :c] - v['mean'].view(1, -1, 1, 1)) * v['inv'].view(1, -1, 1, 1)
    g_act = torch.nn.grad.conv2d_input((n, c, h, w), weight, gy, 1, pad) * mask
    gx_want = g_act * (v['inv'] * v['gamma']).view(1, -1, 1, 1)
    ggamma_want, gbeta_want = (g_act * xhat).sum(dim=(0, 2, 3)), g_act.sum(dim=(0, 2, 3))
    g_abs = torch.nn.grad.conv2d_input((n, c, h, w), weight.abs(), gy.abs(), 1, pad) * mask
    largest = max(float((g_abs * (v['inv'] * v['gamma']).view(1, -1, 1, 1)).max()),
                  float((g_abs * xhat.abs()).sum(dim=(0, 2, 3)).max()), float(g_abs.sum(dim=(0, 2, 3)).max())) + PREFILL
    assert_limit(largest, 2, f'fused bn data gradient {case}')
    if r == 1:
        desc = desc_of((n, c, h, w, k, 1, 1, (1, 1), (0, 0)), total * h * w)
        d_gy = cuda(gy.contiguous())
        gy_pointer = d_gy.data_ptr()
    else:
        desc = desc_of((n, c, h, w, k, 3, 3, (1, 1), (1, 1)), 0, (k + 8) * h * w)
        d_gy = cuda(gy_wide)
        gy_pointer = d_gy.data_ptr() + 4 * 4 * h * w
    bn, keep = bn_struct(v)
    d_wide, d_weight = cuda(wide), cuda(weight)
    assert lib.srgan_conv2d_bnrelu_supported(desc, 1) == 1
    old, old_gamma, old_beta = prefill((n, total, h, w), generator), prefill((c,), generator), prefill((c,), generator)
    for accumulate in ((0, 1) if r == 1 else (0,)):
        gx_wide, g_gamma, g_beta = cuda(old), cuda(old_gamma), cuda(old_beta)
        check(lib.srgan_conv2d_bwd_data_bnrelu(desc, gy_pointer, d_weight.data_ptr(), bn, d_wide.data_ptr(), gx_wide.data_ptr(),
                                               g_gamma.data_ptr(), g_beta.data_ptr(), accumulate, stream()),
              'srgan_conv2d_bwd_data_bnrelu')
        what = f'fused bn data gradient {k}->{c}/{total} k{r} {n}x{h}x{w} accumulate={accumulate}'
        want = old.clone()
        want[:, :c] = gx_want + (old[:, :c] if accumulate else 0.0)
        assert_exact(gx_wide, want, what + ' gx (channels beyond the view untouched)')
        assert_exact(g_gamma, old_gamma + ggamma_want, what + ' gamma gradient', ('c',))
        assert_exact(g_beta, old_beta + gbeta_want, what + ' beta gradient', ('c',))


# ------------------------------------------------------------------------------------------------- grouped weight gradients
@pytest.mark.parametrize('plane,shares', GROUPED_WGRAD_CASES)
def test_grouped_weight_gradients_are_exact(lib, plane, shares):
    """srgan_wgrad_group_plan / _run at test_grouped_weight_gradients_gpu.py's shapes: four norm -> relu -> 1x1 weight gradients
    over growing channel prefixes of one buffer in one launch, accumulated into random-integer gradients."""
    h, w = plane
    hw, n, width, cins = h * w, 3, 128, (96, 160, 288, 416)
    total = max(cins)
    generator = torch.Generator().manual_seed(seed_of('group', plane, shares))
    buffer = ints((n, total, h, w), X, generator)
    gy = ints((len(cins), n, width, h, w), X, generator)
    norms = [bn_operands(c, generator) for c in cins]
    want, olds = [], []
    for index, c in enumerate(cins):
        act = bn_pre(buffer[:, :c], norms[index]).relu()
        want.append(torch.nn.grad.conv2d_weight(act, (width, c, 1, 1), gy[index]))
        assert_limit(float(torch.nn.grad.conv2d_weight(act, (width, c, 1, 1), gy[index].abs()).max()) + PREFILL, 2, f'{c} channels')
        olds.append(prefill((width, c, 1, 1), generator))
    d_buffer, d_gy = cuda(buffer), cuda(gy)
    keep, slots = [], (ctypes.c_byte * (128 * len(cins)))()
    gws = [cuda(old) for old in olds]
    grid_x = grid_y = variants = 0
    partial_at = taps = elements = 0
    weights = sum(width * c for c in cins) if shares else 0
    for index, c in enumerate(cins):
        bn, vectors = bn_struct(norms[index])
        keep.append((bn, vectors))
        desc = desc_of((n, c, h, w, width, 1, 1, (1, 1), (0, 0)), total * hw)
        gx, gyy, variant, partial = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        check(lib.srgan_wgrad_group_plan(desc, bn, 0, index * n * width * hw, gws[index].data_ptr(), 0, len(cins), weights,
                                         partial_at, ctypes.byref(slots, 128 * index), ctypes.byref(gx), ctypes.byref(gyy),
                                         ctypes.byref(variant), ctypes.byref(partial)), 'srgan_wgrad_group_plan')
        partial_at += partial.value
        grid_x, grid_y, variants = max(grid_x, gx.value), max(grid_y, gyy.value), variants | variant.value
        taps += width * c
        elements += (c + width) * n * hw
    assert grid_y > 1                                               # the K range is split
    table = torch.frombuffer(bytearray(bytes(slots)), dtype=torch.uint8).cuda()
    with profiled(lib) as report:
        check(lib.srgan_wgrad_group_run(table.data_ptr(), len(cins), 1, grid_x, grid_y, variants, 1, d_buffer.data_ptr(),
                                        d_gy.data_ptr(), None, taps, n * hw, elements, partial_at, stream()), 'srgan_wgrad_group_run')
    report.assert_reached(GROUPED_WGRAD_REACH, True, f'grouped weight gradient on {h} x {w}')
    for index, c in enumerate(cins):
        assert_exact(gws[index], olds[index] + want[index], f'grouped weight gradient {c} input channels on {h} x {w}',
                     ('k', 'c', 'r', 's'))


# ------------------------------------------------------------------------------------------------- the atomic combines
def test_the_file_again_with_fp32_atomic_combines():
    """Every test above again in a child process with SRGAN_ATOMIC_SPLIT=1 (read once per process): the K slices of the split
    launches then meet through fp32 atomics (gg_prepare, conv3x3_wgrad, pointwise, pointwise_wgrad, stem7x7, split_finish.h)
    instead of the ordered finishes and partial buffers.  On exact operands the atomics are order-independent, so the same
    bit-exact assertions hold; the accumulate cases check that the atomics add onto a live, non-zero output."""
    environment = dict(os.environ, SRGAN_ATOMIC_SPLIT='1')
    started = time.time()
    done = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k', 'not atomic',
                           '-p', 'no:cacheprovider'], env=environment, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert done.returncode == 0, f'after {time.time() - started:.0f} s:\n' + done.stdout[-4000:] + done.stderr[-2000:]
    assert ' passed' in done.stdout and 'failed' not in done.stdout, done.stdout[-2000:]
