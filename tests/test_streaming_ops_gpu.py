"""The streaming and reduction kernels (elementwise.hip, reduce.hip, all of pool.hip) through the C ABI, per element.

Every output is a window inside a larger device buffer with GUARD floats of a fixed non-NaN bit pattern on each side, which must
be bit-unchanged after the call; store-mode windows start as NaN (an element never written fails), accumulate-mode windows as
distinct integers that the expected value includes.  Channel-slice outputs are compared as whole wide buffers: the untouched
channels are guard bands too.  The cases, the float64 references and the branch every case reaches are streaming_cases.py's
(checked on the CPU by test_streaming_cases_cpu.py).

Exact operands (integers, dyadic per-channel vectors; every partial sum below 2^(24 - f)) make every reduction, affine map and
loss piece equal float64 BIT FOR BIT in any summation order -- also where workgroups meet through fp32 atomics:
test_the_file_again_with_fp32_atomic_combines re-runs the file with SRGAN_ATOMIC_SPLIT=1 (srgan_chan_reduce with its zero-fill
in front, srgan_bn_act_bwd, srgan_crowd_map_l1_fwd, the parameter sums of the two fused pool backwards).

Pooling (pool.hip):
  - srgan_maxpool2d_fwd, srgan_pool_gather / _scatter, srgan_avgpool2d_fwd / _bwd at s = k and with overlapping windows,
    srgan_copy_channels: exact (k = 3 averages: 2 ulp, fl(1 / 9) and one product).
  - srgan_maxpool2d_bwd at the arg-max of the float64 reference: both four-pixels-per-thread kernels, the scalar gather kernel,
    and the scalar kernel again for a W % 4 == 0 plane whose gx is off a 16-byte boundary.
  - srgan_bn_relu_maxpool_fwd / _bwd and srgan_bn_relu_avgpool2_fwd / _bwd against float64 norm -> relu -> pool and its
    gradients, gamma of either sign, the mask's borderline bn(x) == 0 hit exactly: one and several workgroups per plane (the
    ragged last one), C at and beyond the ordered finish's 4096 rows (beyond: atomics in either mode), N * C = 65535, the
    parameter gradients added onto distinct integers or not asked for (the same gx, nothing else written), eight launches back
    to back through the one ticket array at 2, 6, 1, 2 partial sums per channel, the same bits on three runs of full-mantissa
    operands, and every refusal (the `_supported` limits, misaligned pointers, one parameter gradient without the other) with
    the outputs untouched.

Elementwise ops:
  - copy, neg, abs, sign, square, relu, step, leaky(0.25), add, sub, mul, max, leaky_mask_mul, div_safe's zero branch: bit-identical
    to float64 rounded to fp32, on integers and on random full-mantissa values.
  - affine, one_minus_square, axpy: the fused (one rounding) or the two-rounding result, per element.
  - sqrt, reciprocal, div: CORRECTLY ROUNDED under the committed build flags (-O3, no fast-math: hipcc keeps fp32 division and
    square root IEEE-exact); rsqrt = 1.f / sqrtf(x) is two correctly rounded operations.  Pinned bit for bit.
  - exp, log, log1p, tanh, pow, sigmoid, softplus: per element, in ulps of the float64 value, against max(2, 4 x the worst error
    of torch's CPU fp32 evaluation on the same inputs) + the formula's further roundings (sigmoid 2, softplus 2); results below
    the smallest normal against 2^-126.  Measured CPU figures -> bounds (streaming_cases.transcendental_bound, computed where the
    test runs and printed by the CPU test; they depend on the vector math library torch uses on that CPU) on two hosts:
    exp 0.50 / 0.52 -> 2.0 / 2.06, log 0.50 / 0.59 -> 2.0 / 2.34, log1p 0.50 / 0.52 -> 2.0 / 2.08, tanh 0.50 -> 2.0,
    pow(0.5) 0.46 / 0.67 -> 2.0 / 2.69, pow(1.5), pow(2) 0.47, 0.45 -> 2.0, pow(3) 0.95 -> 3.78, sigmoid 1.60 -> 8.4,
    softplus 0.92 -> 5.67 ulp.  The kernels' worst on the MI355X: exp 0.65, log 1.96 (at 1 - 2^-23), log1p 0.50, tanh 0.92,
    pow 1.06, sigmoid 1.60, softplus 1.21 ulp.  tanh is exactly +-1 from |x| = 9 on (test_tanh_is_exactly_one_from_nine).
  - Adam against the float64 update: in ulps at the magnitude of the operands of each tensor's last sum (streaming_cases.adam_expected),
    bounds max(2, 4 x the worse of two fp32 evaluation orders on the CPU): at n = 2048 * 256 + 1, p <= 29.3, m <= 3.5, v <= 14.0
    ulp; the kernels' worst there: p 8.1, m 0.86, v 2.8 ulp.
  - NaN rule (include/srgan_hip.h): relu, step, sign, leaky, leaky_mask_mul, max and srgan_row_max select with `x > 0` / fmaxf:
    a NaN becomes 0 or is dropped where torch propagates it.  Pinned here; everything else matches torch on +-0, +-inf, NaN.

Not testable here: the 64-bit index instantiations (copy_channels_kernel<int64_t>, maxpool_fwd_kernel<int64_t>, ...) need more
than 2^31 elements.
"""
import ctypes
import math
import os
import subprocess
import sys
import time

import pytest
import torch

import streaming_cases as S
from helpers import PATTERN, Guarded, assert_exact, device, ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib.library()


def check(status, what):
    from srgan_amd import _lib
    _lib.check(status, what)


def stream():
    from srgan_amd import _lib
    return _lib.stream_handle()


def tile(t, n):
    return t.repeat(-(-n // t.numel()))[:n]


def same_bits(got, want, what):
    got, want = got.cpu().reshape(-1).view(torch.int32), want.cpu().reshape(-1).view(torch.int32)
    assert got.shape == want.shape, f'{what}: {got.numel()} != {want.numel()} elements'
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, f'{what}: {len(bad)} of {got.numel()} elements differ in their bits, first at {bad[:8]}'


def assert_either(got, first, second, what):
    """Per element one of two float64 values (the fused and the two-rounding result)."""
    got64 = got.detach().cpu().double()
    assert_exact(got, torch.where(got64 == second, second, first), what, dims=('i',))


def assert_ulps(got, want, bound, what, x=None, scale=None):
    """`bound`: ulps (of `want`, or of `scale`: streaming_cases.ulp_error), one figure or one per element."""
    error = S.ulp_error(got, want, scale)
    bound = bound if torch.is_tensor(bound) else torch.full_like(error, bound)
    worst = int((error / bound).argmax())
    print(f'{what}: worst {float(error[worst]):.3f} ulp (bound {float(bound[worst]):.3f})' + (f' at x = {float(x[worst])!r}' if x is not None else ''))
    bad = (error > bound).nonzero().flatten()
    lines = [f'  [{i}]' + (f' x = {float(x[i])!r}' if x is not None else '') + f' got {float(got.cpu()[i])!r} want {float(want[i])!r} '
             f'({float(error[i]):.2f} ulp, bound {float(bound[i]):.2f})' for i in bad[:8].tolist()]
    assert bad.numel() == 0, f'{what}: {bad.numel()} of {error.numel()} elements beyond their bound\n' + '\n'.join(lines)


# ------------------------------------------------------------------------------------------------- elementwise maps
def unary_parameters(name):
    return {'affine': S.AFFINE_P, 'leaky': (S.LEAKY_SLOPE, 0.0), 'pow': (1.5, 0.0)}.get(name, (0.0, 0.0))


def unary_inputs(name):
    """Input sets (float64 values that are fp32-representable), each later tiled to the case's length."""
    if name in S.TRANSCENDENTAL:
        return [S.transcendental_inputs(name)]
    gen = S.generator('unary', name)
    sets = [S.ints((4099,), S.X, gen), S.full_mantissa(4099, gen)]
    if name in S.UNARY_IEEE:
        sets = [sets[0].abs() + 1.0, sets[1].abs() + 2.0 ** -10]
    return [t.float().double() for t in sets]


def check_unary(name, got, x, p0, p1, what):
    want = S.unary_ref(name, x, p0, p1)
    if name in S.UNARY_EXACT or name in ('sqrt', 'reciprocal'):
        assert_exact(got, S.round32(want), what, dims=('i',))
    elif name == 'rsqrt':                                        # 1.f / sqrtf(x): two correctly rounded operations
        assert_exact(got, S.round32(1.0 / S.round32(x.sqrt())), what, dims=('i',))
    elif name in S.UNARY_FMA:
        assert_either(got, S.round32(want), S.two_roundings(name, x, None, p0, p1), what)
    else:
        assert_ulps(got, want, S.transcendental_bound(name, p0)[1], what, x)


def run_unary(lib, name, x, p0, p1, in_place, offset=0, y_offset=None):
    y_offset = offset if y_offset is None else y_offset
    if in_place:
        out = Guarded(x.numel(), x, offset)
        source = out.ptr
    else:
        out, keep = Guarded(x.numel(), NAN, y_offset), device(x, offset)
        source = keep.data_ptr()
    check(lib.srgan_ew_unary(S.U[name], source, out.ptr, x.numel(), p0, p1, stream()), f'srgan_ew_unary {name}')
    return out.result(f'{name} n={x.numel()} offset={offset}/{y_offset} in_place={in_place}')


@pytest.mark.parametrize('name', S.UNARY)
def test_unary_maps_at_every_length_in_and_out_of_place(lib, name):
    p0, p1 = unary_parameters(name)
    for index, base in enumerate(unary_inputs(name)):
        for n in S.EW_LENGTHS:
            x = tile(base, n)
            for in_place in (False, True):
                got = run_unary(lib, name, x, p0, p1, in_place)
                check_unary(name, got, x, p0, p1, f'{name} set {index} n={n} in_place={in_place}')


@pytest.mark.parametrize('p0', S.POW_EXPONENTS)
def test_pow_exponents(lib, p0):
    x = S.transcendental_inputs('pow')
    got = run_unary(lib, 'pow', x, p0, 0.0, False)
    assert_ulps(got, S.unary_ref('pow', x, p0), S.transcendental_bound('pow', p0)[1], f'pow {p0}', x)


def test_regime_points_of_the_transcendental_ops(lib):
    """exp(89) = +inf, tanh(+-20) = +-1 exactly, the saturated ends of sigmoid and softplus."""
    def run(name, values):
        return run_unary(lib, name, torch.tensor(values, dtype=torch.float64), 0.0, 0.0, False).cpu().tolist()
    assert run('exp', [89.0, 128.0]) == [math.inf, math.inf]
    assert all(0.0 <= value <= S.SMALLEST_NORMAL for value in run('exp', [-89.0, -104.0]))
    assert run('tanh', [20.0, -20.0]) == [1.0, -1.0]
    assert run('sigmoid', [88.0, 104.0]) == [1.0, 1.0]
    assert all(0.0 <= value <= S.SMALLEST_NORMAL for value in run('sigmoid', [-88.0, -104.0]))
    assert run('softplus', [17.0, 88.0, 104.0]) == [17.0, 88.0, 104.0]
    assert all(0.0 <= value <= S.SMALLEST_NORMAL for value in run('softplus', [-88.0, -104.0]))


def binary_parameter(name):
    return {'leaky_mask_mul': S.LEAKY_SLOPE, 'axpy': S.AXPY_P}.get(name, 0.0)


def binary_inputs(name):
    gen = S.generator('binary', name)
    pairs = [(S.ints((4099,), S.X, gen), S.ints((4099,), S.X, gen)), (S.full_mantissa(4099, gen), S.full_mantissa(4099, gen))]
    if name == 'div':
        pairs[0] = (pairs[0][0], torch.where(pairs[0][1] == 0, torch.ones(()).double(), pairs[0][1]))
    return [(a.float().double(), b.float().double()) for a, b in pairs]


def check_binary(name, got, a, b, p0, what):
    want = S.binary_ref(name, a, b, p0)
    if name == 'axpy':
        assert_either(got, S.round32(want), S.two_roundings(name, a, b, p0), what)
    else:                                   # one correctly rounded operation (div: IEEE-exact under the committed flags)
        assert_exact(got, S.round32(want), what, dims=('i',))


def run_binary(lib, name, a, b, p0, mode, offsets=(0, 0, 0)):
    n = a.numel()
    if mode == 'y=a':
        out = Guarded(n, a, offsets[0])
        pa, keep = out.ptr, device(b, offsets[1])
        pb = keep.data_ptr()
    elif mode == 'y=b':
        out = Guarded(n, b, offsets[1])
        keep = device(a, offsets[0])
        pa, pb = keep.data_ptr(), out.ptr
    else:
        out, keep = Guarded(n, NAN, offsets[2]), (device(a, offsets[0]), device(b, offsets[1]))
        pa, pb = keep[0].data_ptr(), keep[1].data_ptr()
    check(lib.srgan_ew_binary(S.B[name], pa, pb, out.ptr, n, p0, stream()), f'srgan_ew_binary {name}')
    return out.result(f'{name} n={n} offsets={offsets} {mode}')


@pytest.mark.parametrize('name', S.BINARY)
def test_binary_maps_at_every_length_in_and_out_of_place(lib, name):
    p0 = binary_parameter(name)
    for index, (base_a, base_b) in enumerate(binary_inputs(name)):
        for n in S.EW_LENGTHS:
            a, b = tile(base_a, n), tile(base_b, n)
            for mode in ('out', 'y=a', 'y=b'):
                check_binary(name, run_binary(lib, name, a, b, p0, mode), a, b, p0, f'{name} set {index} n={n} {mode}')


def test_windows_off_16_byte_alignment_give_the_same_bits(lib):
    """srgan_ew_unary / srgan_ew_binary on views that start 1, 2 and 3 floats past a 16-byte boundary (every pointer, or only
    one of them): the single-float loops, same bits as the aligned call."""
    for name in S.UNARY:
        p0, p1 = unary_parameters(name)
        base = unary_inputs(name)[-1]
        for n in S.SMALL_LENGTHS:
            x = tile(base, n)
            aligned = run_unary(lib, name, x, p0, p1, False).clone()
            check_unary(name, aligned, x, p0, p1, f'{name} n={n}')
            for offset, y_offset in [(1, 1), (2, 2), (3, 3), (0, 1), (2, 0)]:
                same_bits(run_unary(lib, name, x, p0, p1, False, offset, y_offset), aligned, f'{name} n={n} offsets {offset}/{y_offset}')
            for offset in (1, 2, 3):
                same_bits(run_unary(lib, name, x, p0, p1, True, offset), aligned, f'{name} n={n} in place at offset {offset}')
    for name in S.BINARY:
        p0 = binary_parameter(name)
        base_a, base_b = binary_inputs(name)[-1]
        for n in S.SMALL_LENGTHS:
            a, b = tile(base_a, n), tile(base_b, n)
            aligned = run_binary(lib, name, a, b, p0, 'out').clone()
            check_binary(name, aligned, a, b, p0, f'{name} n={n}')
            for offsets in [(1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 0), (0, 2, 0), (0, 0, 3)]:
                same_bits(run_binary(lib, name, a, b, p0, 'out', offsets), aligned, f'{name} n={n} offsets {offsets}')
            for mode in ('y=a', 'y=b'):
                same_bits(run_binary(lib, name, a, b, p0, mode, (1, 3, 0)), aligned, f'{name} n={n} {mode} off alignment')


@pytest.mark.parametrize('value', [0.0, 2.5])
def test_fill_at_every_alignment(lib, value):
    for offset in S.OFFSETS:
        for n in S.SMALL_LENGTHS + [S.EW_LENGTHS[-1]]:
            out = Guarded(n, NAN, offset)
            check(lib.srgan_fill(out.ptr, n, value, stream()), 'srgan_fill')
            assert_exact(out.result(f'fill {value} n={n} offset={offset}'), torch.full((n,), value, dtype=torch.float64),
                         f'fill {value} n={n} offset={offset}', dims=('i',))


def test_special_values(lib):
    """+-0, +-inf and NaN through every op: torch's result wherever IEEE arithmetic defines it, the NaN rule of
    include/srgan_hip.h (a NaN is "not positive", fmaxf drops it) for relu / step / sign / leaky / leaky_mask_mul / max."""
    x = torch.tensor(S.SPECIALS, dtype=torch.float64)
    for name in S.UNARY:
        p0, p1 = unary_parameters(name)
        got = run_unary(lib, name, x, p0, p1, False)
        assert_ulps(got, S.unary_ref(name, x, p0, p1), 4.0, f'specials {name}', x)
        if name not in S.NAN_RULE_UNARY:
            assert_ulps(got, S.torch_unary(name, x, p0, p1).double(), 4.0, f'specials {name} against torch', x)
    nan_at = [i for i, v in enumerate(S.SPECIALS) if v != v][0]
    for name, expected in (('relu', 0.0), ('step', 0.0), ('sign', 0.0)):
        assert float(run_unary(lib, name, x, 0.0, 0.0, False)[nan_at]) == expected, f'{name}(NaN)'
    assert math.isnan(float(run_unary(lib, 'leaky', x, S.LEAKY_SLOPE, 0.0, False)[nan_at]))          # p0 * NaN
    a, b = x.repeat_interleave(len(S.SPECIALS)), x.repeat(len(S.SPECIALS))
    for name in S.BINARY:
        p0 = binary_parameter(name)
        got = run_binary(lib, name, a, b, p0, 'out')
        assert_ulps(got, S.binary_ref(name, a, b, p0), 0.5, f'specials {name}')
        if name not in S.NAN_RULE_BINARY:
            assert_ulps(got, S.torch_binary(name, a, b, p0).double(), 0.5, f'specials {name} against torch')
    one_nan = torch.tensor([NAN, 1.0], dtype=torch.float64), torch.tensor([1.0, NAN], dtype=torch.float64)
    assert run_binary(lib, 'max', one_nan[0], one_nan[1], 0.0, 'out').cpu().tolist() == [1.0, 1.0]      # torch.maximum: NaN, NaN
    assert run_binary(lib, 'leaky_mask_mul', torch.tensor([2.0]).double(), torch.tensor([NAN]).double(), 0.25, 'out').cpu().tolist() == [0.5]


# ------------------------------------------------------------------------------------------------- per-channel affine
def affine_problem(hw):
    n, c = S.AFFINE_N, S.AFFINE_C
    gen = S.generator('affine', hw)
    vectors = dict(mean=S.pick(S.QUARTERS, (c,), gen), scale_a=S.pick(S.SCALES, (c,), gen), scale_b=S.pick(S.SCALES, (c,), gen),
                   shift=S.pick(S.QUARTERS, (c,), gen))
    return dict(x=S.ints((n, c, hw), S.X, gen), mask=S.ints((n, c, hw), 1, gen), vectors=vectors, gen=gen)


@pytest.mark.parametrize('hw', S.AFFINE_HW)
def test_chan_affine(lib, hw):
    n, c = S.AFFINE_N, S.AFFINE_C
    problem = affine_problem(hw)
    x_device, mask_device = device(problem['x']), device(problem['mask'])
    on_device = {key: device(value) for key, value in problem['vectors'].items()}
    for subset, names in S.AFFINE_SUBSETS.items():
        vectors = {key: value for key, value in problem['vectors'].items() if key in names}
        x = problem['x'] if 'x' in names else None
        pointers = [ptr(x_device) if x is not None else None] + [ptr(on_device[key]) if key in names else None
                                                                 for key in ('mean', 'scale_a', 'scale_b', 'shift')]
        out = Guarded(n * c * hw)
        check(lib.srgan_chan_affine(*pointers, out.ptr, n, c, hw, stream()), 'srgan_chan_affine')
        assert_exact(out.result(f'chan_affine {subset} hw={hw}', (n, c, hw)), S.chan_affine_ref(x, vectors, None, 0, (n, c, hw)),
                     f'chan_affine {subset} hw={hw}', dims=('n', 'c', 'i'))
        for relu in (0, 1):
            for mask in (None, problem['mask']):
                what = f'chan_affine_act {subset} hw={hw} relu={relu} mask={mask is not None}'
                out = Guarded(n * c * hw)
                check(lib.srgan_chan_affine_act(*pointers, ptr(mask_device) if mask is not None else None, relu, out.ptr, n, c, hw,
                                                stream()), what)
                assert_exact(out.result(what, (n, c, hw)), S.chan_affine_ref(x, vectors, mask, relu, (n, c, hw)), what, dims=('n', 'c', 'i'))


@pytest.mark.parametrize('hw', S.AFFINE_HW)
def test_chan_affine_on_channel_slices(lib, hw):
    """x, mask and y as channel slices of wider buffers at three different batch strides, stored and accumulated; the wide
    output buffer is compared as a whole."""
    n, c = S.AFFINE_N, S.AFFINE_C
    problem = affine_problem(hw)
    gen, vectors = problem['gen'], problem['vectors']
    (cx, fx), (cm, fm), (cy, fy) = (5, 1), (4, 0), (6, 2)
    wide_x, wide_mask = S.ints((n, cx, hw), S.X, gen), S.ints((n, cm, hw), 1, gen)
    x, mask = wide_x[:, fx:fx + c], wide_mask[:, fm:fm + c]
    x_device, mask_device = device(wide_x), device(wide_mask)
    on_device = [device(vectors[key]) for key in ('mean', 'scale_a', 'scale_b', 'shift')]
    for accumulate in (0, 1):
        for use_mask in (False, True):
            for relu in (0, 1):
                what = f'chan_affine_act_strided hw={hw} accumulate={accumulate} mask={use_mask} relu={relu}'
                old = S.distinct((n, cy, hw), gen)
                start = old.clone()
                if not accumulate:
                    start[:, fy:fy + c] = NAN
                out = Guarded(n * cy * hw, start)
                check(lib.srgan_chan_affine_act_strided(x_device.data_ptr() + 4 * fx * hw, *[t.data_ptr() for t in on_device],
                                                        mask_device.data_ptr() + 4 * fm * hw if use_mask else None, relu,
                                                        out.at(fy * hw), n, c, hw, cx * hw, cm * hw, cy * hw, accumulate, stream()), what)
                value = S.chan_affine_ref(x, vectors, mask if use_mask else None, relu, (n, c, hw))
                want = old.clone()
                want[:, fy:fy + c] = value + old[:, fy:fy + c] if accumulate else value
                assert_exact(out.result(what, (n, cy, hw)), want, what, dims=('n', 'c', 'i'))


# ------------------------------------------------------------------------------------------------- reductions
def reduce_problem(n, c, hw):
    gen = S.generator('reduce', n, c, hw)
    return dict(a=S.ints((n, c, hw), S.X, gen), b=S.ints((n, c, hw), S.X, gen), mean=S.pick(S.QUARTERS, (c,), gen),
                scale=S.pick(S.SCALES, (c,), gen), old=S.distinct((c,), gen))


REDUCE_VARIANTS = [('a', False, False), ('a, b', True, False), ('a, b, mean, scale', True, True), ('a, mean, scale', False, True),
                   ('a == b, mean, scale', 'same', True)]


def run_reduce(lib, problem, shape, variant, accumulate, offsets=(0, 0)):
    n, c, hw = shape
    _, use_b, use_vectors = variant
    a = device(problem['a'], offsets[0])
    b = a if use_b == 'same' else device(problem['b'], offsets[1]) if use_b else None
    mean, scale = (device(problem['mean']), device(problem['scale'])) if use_vectors else (None, None)
    out = Guarded(c, problem['old'] if accumulate else NAN)
    check(lib.srgan_chan_reduce(ptr(a), ptr(b), ptr(mean), ptr(scale), out.ptr, n, c, hw, accumulate, stream()), 'srgan_chan_reduce')
    return out.result(f'chan_reduce {shape} [{variant[0]}] accumulate={accumulate} offsets={offsets}')


def reduce_expected(problem, variant, accumulate):
    _, use_b, use_vectors = variant
    b = problem['a'] if use_b == 'same' else problem['b'] if use_b else None
    mean, scale = (problem['mean'], problem['scale']) if use_vectors else (None, None)
    S.assert_exact_limit(S.chan_reduce_magnitude(problem['a'], b, mean, scale) + problem['old'].abs().max().item(), 3, 'chan_reduce')
    want = S.chan_reduce_ref(problem['a'], b, mean, scale)
    return want + problem['old'] if accumulate else want


@pytest.mark.parametrize('shape', [(n, c, 1) for n, c in S.REDUCE_COLS] + S.REDUCE_BLOCK + S.REDUCE_ROWS,
                         ids=lambda shape: 'x'.join(map(str, shape)))
def test_chan_reduce(lib, shape):
    problem = reduce_problem(*shape)
    for variant in REDUCE_VARIANTS:
        for accumulate in (0, 1):
            what = f'chan_reduce {shape} [{variant[0]}] accumulate={accumulate}'
            first = run_reduce(lib, problem, shape, variant, accumulate).clone()
            assert_exact(first, reduce_expected(problem, variant, accumulate), what, dims=('c',))
            same_bits(run_reduce(lib, problem, shape, variant, accumulate), first, what + ', second run')


def test_chan_reduce_rows_off_16_byte_alignment(lib):
    for shape in S.REDUCE_UNALIGNED:
        problem = reduce_problem(*shape)
        for variant in REDUCE_VARIANTS:
            want = reduce_expected(problem, variant, 0)
            for offsets in [(0, 0), (1, 1), (2, 2), (3, 3), (0, 2), (1, 0)]:
                assert_exact(run_reduce(lib, problem, shape, variant, 0, offsets), want, f'chan_reduce {shape} [{variant[0]}] offsets {offsets}',
                             dims=('c',))


# ------------------------------------------------------------------------------------------------- frozen-norm backward
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('shape', S.BN_BWD, ids=lambda shape: 'x'.join(map(str, shape)))
def test_bn_act_bwd(lib, shape, relu):
    n, c, hw = shape
    gen = S.generator('bn_act_bwd', shape)
    v = S.channel_vectors(c, gen)
    g, x = S.ints(shape, S.X, gen), S.ints(shape, S.X, gen)
    g_device, x_device = device(g), device(x)
    vectors = [device(v[key]) for key in ('mean', 'inv_std', 'gamma', 'beta')]
    old_gamma, old_beta = S.distinct((c,), gen), S.distinct((c,), gen)
    wide, first = c + 3, 2
    for unscaled in (0, 1):
        gx, g_gamma, g_beta = S.bn_act_bwd_ref(g, x, v, relu, unscaled)
        for mode in ('gx', 'parameters', 'both', 'gx into a slice'):
            what = f'bn_act_bwd {shape} relu={relu} unscaled={unscaled} [{mode}]'
            out_gx = out_gamma = out_beta = None
            gx_stride, accumulate = 0, 0
            if mode == 'gx into a slice':
                old = S.distinct((n, wide, hw), gen)
                out_gx, gx_stride, accumulate = Guarded(n * wide * hw, old), wide * hw, 1
            elif mode != 'parameters':
                out_gx = Guarded(n * c * hw)
            if mode in ('parameters', 'both'):
                out_gamma, out_beta = Guarded(c, old_gamma), Guarded(c, old_beta)
            check(lib.srgan_bn_act_bwd(g_device.data_ptr(), x_device.data_ptr(), *[t.data_ptr() for t in vectors], relu,
                                       None if out_gx is None else out_gx.at(first * hw if gx_stride else 0),
                                       None if out_gamma is None else out_gamma.ptr, None if out_beta is None else out_beta.ptr,
                                       n, c, hw, 0, 0, gx_stride, accumulate, unscaled, stream()), what)
            if mode == 'gx into a slice':
                want = old.clone()
                want[:, first:first + c] += gx
                assert_exact(out_gx.result(what, (n, wide, hw)), want, what, dims=('n', 'c', 'i'))
            elif out_gx is not None:
                assert_exact(out_gx.result(what, (n, c, hw)), gx, what, dims=('n', 'c', 'i'))
            if out_gamma is not None:
                assert_exact(out_gamma.result(what + ' g_gamma'), g_gamma + old_gamma, what + ' g_gamma', dims=('c',))
                assert_exact(out_beta.result(what + ' g_beta'), g_beta + old_beta, what + ' g_beta', dims=('c',))


# ------------------------------------------------------------------------------------------------- double-backward weight tangent
def tangent_problem(case):
    co, ci, taps = case
    gen = S.generator('tangent', case)
    problem = dict(w=S.ints((co, ci, taps), S.X, gen), q=S.ints((co, ci, taps), S.X, gen), inv_std=S.pick(S.SCALES, (ci,), gen),
                   gamma=S.pick(S.SCALES, (ci,), gen), old_w_grad=S.distinct((co, ci, taps), gen), old_gamma_grad=S.distinct((ci,), gen))
    scaled, w_grad, gamma_grad = S.tangent_ref(problem['w'], problem['q'], problem['inv_std'], problem['gamma'])
    problem.update(scaled=scaled, w_grad=w_grad + problem['old_w_grad'], gamma_grad=gamma_grad + problem['old_gamma_grad'])
    return problem


def run_tangent(lib, case, problem):
    co, ci, taps = case
    w, q, inv_std, gamma = (device(problem[key]) for key in ('w', 'q', 'inv_std', 'gamma'))
    scaled = Guarded(co * ci * taps)
    check(lib.srgan_bn_conv_tangent_weights(w.data_ptr(), None, inv_std.data_ptr(), gamma.data_ptr(), scaled.ptr, None, None, co, ci,
                                            taps, stream()), 'srgan_bn_conv_tangent_weights (w_scaled)')
    w_grad, gamma_grad = Guarded(co * ci * taps, problem['old_w_grad']), Guarded(ci, problem['old_gamma_grad'])
    check(lib.srgan_bn_conv_tangent_weights(w.data_ptr(), q.data_ptr(), inv_std.data_ptr(), gamma.data_ptr(), None, w_grad.ptr,
                                            gamma_grad.ptr, co, ci, taps, stream()), 'srgan_bn_conv_tangent_weights (gradients)')
    what = f'tangent weights {case}'
    return (scaled.result(what, (co, ci, taps)).clone(), w_grad.result(what, (co, ci, taps)).clone(), gamma_grad.result(what).clone())


@pytest.mark.parametrize('case', S.TANGENT, ids=lambda case: 'x'.join(map(str, case)))
def test_bn_conv_tangent_weights(lib, case):
    problem = tangent_problem(case)
    scaled, w_grad, gamma_grad = run_tangent(lib, case, problem)
    assert_exact(scaled, problem['scaled'], f'{case} w_scaled', dims=('co', 'ci', 'tap'))
    assert_exact(w_grad, problem['w_grad'], f'{case} w_grad', dims=('co', 'ci', 'tap'))
    assert_exact(gamma_grad, problem['gamma_grad'], f'{case} gamma_grad', dims=('ci',))


def test_bn_conv_tangent_weights_grouped_equals_the_single_calls(lib):
    problems = [tangent_problem(case) for case in S.TANGENT]
    singles = [run_tangent(lib, case, problem) for case, problem in zip(S.TANGENT, problems)]
    sizes = [co * ci * taps for co, ci, taps in S.TANGENT]
    offsets = [sum(sizes[:index]) for index in range(len(sizes))]
    slots = (ctypes.c_byte * (64 * len(S.TANGENT)))()
    keep, w_grads, gamma_grads = [], [], []
    for index, (case, problem) in enumerate(zip(S.TANGENT, problems)):
        co, ci, taps = case
        w, inv_std, gamma = (device(problem[key]) for key in ('w', 'inv_std', 'gamma'))
        w_grads.append(Guarded(sizes[index], problem['old_w_grad']))
        gamma_grads.append(Guarded(ci, problem['old_gamma_grad']))
        keep.append((w, inv_std, gamma))
        check(lib.srgan_bn_conv_tangent_weights_job(w.data_ptr(), inv_std.data_ptr(), gamma.data_ptr(), w_grads[-1].ptr, gamma_grads[-1].ptr,
                                                    offsets[index], co, ci, taps, ctypes.byref(slots, 64 * index)),
              'srgan_bn_conv_tangent_weights_job')
    table = torch.frombuffer(bytearray(bytes(slots)), dtype=torch.uint8).cuda()
    max_inner, max_co = max(ci * taps for _, ci, taps in S.TANGENT), max(co for co, _, _ in S.TANGENT)
    scaled_all = Guarded(sum(sizes))
    q_all = device(torch.cat([problem['q'].reshape(-1) for problem in problems]))
    check(lib.srgan_bn_conv_tangent_weights_grouped(table.data_ptr(), len(S.TANGENT), max_inner, max_co, scaled_all.ptr, None, stream()),
          'srgan_bn_conv_tangent_weights_grouped (w_scaled)')
    check(lib.srgan_bn_conv_tangent_weights_grouped(table.data_ptr(), len(S.TANGENT), max_inner, max_co, None, q_all.data_ptr(), stream()),
          'srgan_bn_conv_tangent_weights_grouped (gradients)')
    scaled = scaled_all.result('grouped w_scaled')
    for index, (case, problem) in enumerate(zip(S.TANGENT, problems)):
        co, ci, taps = case
        mine = scaled[offsets[index]:offsets[index] + sizes[index]].reshape(co, ci, taps)
        assert_exact(mine, problem['scaled'], f'grouped {case} w_scaled', dims=('co', 'ci', 'tap'))
        assert_exact(w_grads[index].result(f'grouped {case} w_grad', (co, ci, taps)), problem['w_grad'], f'grouped {case} w_grad',
                     dims=('co', 'ci', 'tap'))
        assert_exact(gamma_grads[index].result(f'grouped {case} gamma_grad'), problem['gamma_grad'], f'grouped {case} gamma_grad', dims=('ci',))
        same_bits(mine, singles[index][0], f'grouped {case} w_scaled against the single call')
        same_bits(w_grads[index].window, singles[index][1], f'grouped {case} w_grad against the single call')
        same_bits(gamma_grads[index].window, singles[index][2], f'grouped {case} gamma_grad against the single call')


# ------------------------------------------------------------------------------------------------- loss pieces
@pytest.mark.parametrize('f', S.GP_F)
def test_gp_interpolate(lib, f):
    gen = S.generator('gp', f)
    u, fake = S.ints((S.GP_B, f), S.X, gen), S.ints((S.GP_B, f), S.X, gen)
    alpha = torch.tensor([0.25, 0.5, 1.0], dtype=torch.float64)[torch.randperm(3, generator=gen)]      # (none symmetric: na = a would show)
    out = Guarded(S.GP_B * f)
    keep = device(u), device(fake), device(alpha)
    check(lib.srgan_gp_interpolate(*[t.data_ptr() for t in keep], out.ptr, S.GP_B, f, stream()), 'srgan_gp_interpolate')
    assert_exact(out.result(f'gp_interpolate {f}', (S.GP_B, f)), S.gp_interpolate_ref(u, fake, alpha), f'gp_interpolate {f}', dims=('b', 'f'))


def crowd_problem(cm, hw):
    gen = S.generator('crowd', cm, hw)
    maps, target, g = S.ints((S.L1_B, cm, hw), S.X, gen), S.ints((S.L1_B, hw), S.X, gen), S.ints((S.L1_B,), S.X, gen)
    g[g == 0] = 2.0
    maps[:, 0, 0] = target[:, 0]                                          # a pixel with map == target: gradient 0
    return maps, target, g


def run_crowd(lib, maps, target, g):
    b, cm, hw = maps.shape
    keep = device(maps), device(target), device(g)
    rows, g_maps = Guarded(b), Guarded(b * cm * hw)
    check(lib.srgan_crowd_map_l1_fwd(keep[0].data_ptr(), keep[1].data_ptr(), rows.ptr, b, cm, hw, stream()), 'srgan_crowd_map_l1_fwd')
    check(lib.srgan_crowd_map_l1_bwd(*[t.data_ptr() for t in keep], g_maps.ptr, b, cm, hw, stream()), 'srgan_crowd_map_l1_bwd')
    return rows.result(f'crowd_map_l1_fwd cm={cm} hw={hw}'), g_maps.result(f'crowd_map_l1_bwd cm={cm} hw={hw}', (b, cm, hw))


@pytest.mark.parametrize('hw', S.L1_HW)
@pytest.mark.parametrize('cm', S.L1_CM)
def test_crowd_map_l1(lib, cm, hw):
    maps, target, g = crowd_problem(cm, hw)
    assert bool(((maps - target.unsqueeze(1)) == 0).any())
    rows, g_maps = run_crowd(lib, maps, target, g)
    assert_exact(rows, S.crowd_l1_ref(maps, target), f'crowd_map_l1_fwd cm={cm} hw={hw}', dims=('b',))
    assert_exact(g_maps, S.crowd_l1_bwd_ref(maps, target, g), f'crowd_map_l1_bwd cm={cm} hw={hw}', dims=('b', 'c', 'i'))


def test_crowd_map_l1_with_three_maps(lib):
    """Cm = 3: the division by Cm is inexact, 2 ulp per element (the forward at one pixel per example: one element each)."""
    maps, target, g = crowd_problem(3, 255)
    _, g_maps = run_crowd(lib, maps, target, g)
    assert_ulps(g_maps.reshape(-1), S.crowd_l1_bwd_ref(maps, target, g).reshape(-1), 2.0, 'crowd_map_l1_bwd cm=3')
    maps, target, g = S.ints((3, 3, 1), S.X, S.generator('crowd3')), torch.tensor([[0.0], [1.0], [-2.0]]).double(), torch.ones(3).double()
    rows, _ = run_crowd(lib, maps, target, g)
    assert_ulps(rows, S.crowd_l1_ref(maps, target), 2.0, 'crowd_map_l1_fwd cm=3')


@pytest.mark.parametrize('shape', S.ROW_MAX, ids=lambda shape: 'x'.join(map(str, shape)))
def test_row_max(lib, shape):
    b, f = shape
    x = S.ints(shape, S.X, S.generator('row_max', shape))                 # small integers: ties in most rows
    x[0, :] = -math.inf
    if b > 1:
        x[1, f // 2] = math.inf
    if b > 2 and f > 1:
        x[2, 0], x[2, 1] = NAN, 2.0                                       # fmaxf drops the NaN (include/srgan_hip.h)
    out, keep = Guarded(b), device(x)
    check(lib.srgan_row_max(keep.data_ptr(), out.ptr, b, f, stream()), 'srgan_row_max')
    assert_exact(out.result(f'row_max {shape}'), S.row_max_ref(x), f'row_max {shape}', dims=('b',))


@pytest.mark.parametrize('k', S.BIN_K)
def test_nearest_bin_onehot(lib, k):
    bins = torch.arange(k, dtype=torch.float64) * 0.5 + 0.5
    halfway = bins[:-1] + 0.25
    gen = S.generator('bins', k)
    y = torch.cat([bins, halfway, torch.tensor([-3.0, 0.0, 99.0, bins[-1].item() + 0.125]).double(),
                   S.pick([v / 8 for v in range(0, 8 * (k + 1))], (300,), gen)])
    out, keep = Guarded(y.numel() * k), (device(y), device(bins))
    check(lib.srgan_nearest_bin_onehot(keep[0].data_ptr(), keep[1].data_ptr(), out.ptr, y.numel(), k, stream()), 'srgan_nearest_bin_onehot')
    got = out.result(f'nearest_bin_onehot {k}', (y.numel(), k))
    assert_exact(got, S.nearest_bin_ref(y, bins), f'nearest_bin_onehot {k}', dims=('b', 'k'))
    if k > 1:
        assert got[k:2 * k - 1].argmax(dim=1).tolist() == list(range(k - 1))          # halfway between two bins: the first wins


# ------------------------------------------------------------------------------------------------- pooling
def same_values(got, want, what):
    got, want = got.cpu().double(), want.double()
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} differ, first at {bad.nonzero()[:8].tolist()}'


@pytest.mark.parametrize('case', S.MAXPOOL, ids=lambda case: 'x'.join(map(str, case)))
def test_maxpool_indices_gather_and_scatter(lib, case):
    planes, h, w, k, s, p = case
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    gen = S.generator('pool', *case)
    x = S.pooling_inputs(planes, h, w, gen)
    values, index = S.maxpool_ref(x, k, s, p, oh, ow)
    y, argmax, keep = Guarded(planes * oh * ow), Guarded(planes * oh * ow, -7, dtype=torch.int32), device(x)
    check(lib.srgan_maxpool2d_fwd(keep.data_ptr(), y.ptr, argmax.ptr, planes, h, w, k, s, p, oh, ow, stream()), 'srgan_maxpool2d_fwd')
    got_index = argmax.result(f'maxpool {case} argmax', (planes, oh, ow))
    assert torch.equal(got_index.cpu().long(), index), f'maxpool {case}: arg-max differs at {(got_index.cpu().long() != index).nonzero()[:8].tolist()}'
    same_values(y.result(f'maxpool {case}', (planes, oh, ow)), values, f'maxpool {case} values')
    source, g = S.ints((planes, h * w), S.X, gen), S.ints((planes, oh * ow), S.X, gen)
    gathered, scattered = Guarded(planes * oh * ow), Guarded(planes * h * w)
    keep = device(source), device(g)
    check(lib.srgan_pool_gather(keep[0].data_ptr(), argmax.ptr, gathered.ptr, planes, h * w, oh * ow, stream()), 'srgan_pool_gather')
    check(lib.srgan_pool_scatter(keep[1].data_ptr(), argmax.ptr, scattered.ptr, planes, h * w, oh * ow, stream()), 'srgan_pool_scatter')
    assert_exact(gathered.result(f'pool_gather {case}', (planes, oh * ow)), S.pool_gather_ref(source, index), f'pool_gather {case}', dims=('plane', 'o'))
    assert_exact(scattered.result(f'pool_scatter {case}', (planes, h * w)), S.pool_scatter_ref(g, index, h * w), f'pool_scatter {case}',
                 dims=('plane', 'i'))


@pytest.mark.parametrize('case', S.AVGPOOL + S.AVGPOOL_STRIDED, ids=lambda case: 'x'.join(map(str, case)))
def test_avgpool(lib, case):
    """(planes, H, W, k) with s = k, (planes, H, W, k, s) with overlapping windows."""
    planes, h, w, k = case[:4]
    s = case[4] if len(case) > 4 else k
    oh, ow = S.pool_out(h, k, s), S.pool_out(w, k, s)
    gen = S.generator('avgpool', *case)
    x, g = S.ints((planes, h, w), S.X, gen), S.ints((planes, oh, ow), S.X, gen)
    y, gx, keep = Guarded(planes * oh * ow), Guarded(planes * h * w), (device(x), device(g))
    check(lib.srgan_avgpool2d_fwd(keep[0].data_ptr(), y.ptr, planes, h, w, k, s, oh, ow, stream()), 'srgan_avgpool2d_fwd')
    check(lib.srgan_avgpool2d_bwd(keep[1].data_ptr(), gx.ptr, planes, h, w, k, s, oh, ow, stream()), 'srgan_avgpool2d_bwd')
    got_y, got_gx = y.result(f'avgpool fwd {case}', (planes, oh, ow)), gx.result(f'avgpool bwd {case}', (planes, h, w))
    if k == 3:                      # 1 / 9 is rounded: sum * fl(1 / 9), 2 ulp per element
        assert_ulps(got_y.reshape(-1), S.avgpool_ref(x, k, s).reshape(-1), 2.0, f'avgpool fwd {case}')
        assert_ulps(got_gx.reshape(-1), S.avgpool_bwd_ref(g, k, h, w, s).reshape(-1), 2.0, f'avgpool bwd {case}')
    else:
        assert_exact(got_y, S.avgpool_ref(x, k, s), f'avgpool fwd {case}', dims=('plane', 'h', 'w'))
        assert_exact(got_gx, S.avgpool_bwd_ref(g, k, h, w, s), f'avgpool bwd {case}', dims=('plane', 'h', 'w'))


@pytest.mark.parametrize('case', S.MAXPOOL, ids=lambda case: 'x'.join(map(str, case)) + '-' + S.maxpool_bwd_path(case[2], *case[3:]))
def test_maxpool_backward_in_gather_form(lib, case):
    """srgan_maxpool2d_bwd at the arg-max of maxpool_ref (the -inf corner and the NaN of pooling_inputs included): the kernel the
    label names; where W % 4 == 0 again with gx 1, 2 and 3 floats off a 16-byte boundary -- the scalar kernel, the same result."""
    planes, h, w, k, s, p = case
    oh, ow = S.pool_out(h, k, s, p), S.pool_out(w, k, s, p)
    x = S.pooling_inputs(planes, h, w, S.generator('pool', *case))
    _, index = S.maxpool_ref(x, k, s, p, oh, ow)
    g = S.ints((planes, oh, ow), S.X, S.generator('maxpool-bwd', *case))
    want = S.maxpool_bwd_ref(g, index, h, w)
    S.assert_exact_limit(float(S.maxpool_bwd_ref(g.abs(), index, h, w).max()), 0, f'maxpool bwd {case}')
    keep = device(g), index.to(torch.int32).cuda()
    for offset in (S.OFFSETS if w % 4 == 0 else [0]):
        what = f'maxpool bwd {case} [{S.maxpool_bwd_path(w, k, s, p, offset)}] gx {offset} floats off alignment'
        gx = Guarded(planes * h * w, NAN, offset)
        check(lib.srgan_maxpool2d_bwd(keep[0].data_ptr(), keep[1].data_ptr(), gx.ptr, planes, h, w, k, s, p, oh, ow, stream()), what)
        assert_exact(gx.result(what, (planes, h, w)), want, what, dims=('plane', 'h', 'w'))


# ------------------------------------------------------------------------------------------------- fused norm -> relu -> pool
def case_id(case):
    return 'x'.join(map(str, case))


def fused_id(form, case):
    """(The re-run with the atomic combines selects with -k 'not atomic': no id may hold that word.)"""
    groups, last, finish = S.fused_pool_grid(form, *case)
    return f"{case_id(case)}-{groups}wg-last{last}-{'ordered' if finish == 'ordered' else 'unordered'}"


def fused_vectors(v):
    return [device(v[key]) for key in ('mean', 'inv_std', 'gamma', 'beta')]


def check_fused_precondition(form, case, problem):
    for name, bits in S.FUSED_POOL_FRACTION_BITS[form].items():
        S.assert_exact_limit(problem['magnitudes'][name], bits, f'fused {form} pool {case} {name}')
    assert bool((problem['v']['gamma'] < 0).any())


def test_the_default_mode_takes_the_ordered_finish(lib):
    """Once for the file: without SRGAN_ATOMIC_SPLIT the stream has a ticket row, so the ordered branches are what the tests
    below run; in the re-run with the variable set, the atomic ones."""
    assert lib.srgan_split_is_ordered(stream()) == (0 if os.environ.get('SRGAN_ATOMIC_SPLIT') is not None else 1)


def run_fused_max_forward(lib, case, problem, what):
    n, c, h, w = case[:4]
    k, s, p = problem['geometry']
    oh, ow = problem['g'].shape[2:]
    keep = [device(problem['x'])] + fused_vectors(problem['v'])
    y, argmax = Guarded(n * c * oh * ow), Guarded(n * c * oh * ow, PATTERN, dtype=torch.int32)
    check(lib.srgan_bn_relu_maxpool_fwd(*[t.data_ptr() for t in keep], y.ptr, argmax.ptr, n, c, h, w, k, s, p, oh, ow, stream()), what)
    return y.result(what, (n, c, oh, ow)), argmax.result(what + ' arg-max', (n, c, oh, ow))


def check_fused_max_forward(lib, case, problem):
    what = f'bn_relu_maxpool_fwd {case}'
    y, argmax = run_fused_max_forward(lib, case, problem, what)
    bad = (argmax.cpu().long() != problem['index']).nonzero()
    assert bad.numel() == 0, f'{what}: {bad.shape[0]} arg-max differ, first at {bad[:8].tolist()}'
    assert_exact(y, problem['y'], what, dims=('n', 'c', 'oh', 'ow'))


@pytest.mark.parametrize('case', S.FUSED_MAX_FWD, ids=case_id)
def test_fused_max_pool_forward(lib, case):
    """maxpool(relu(bn(x))) at every window geometry: the values exact, the arg-max the first maximum in row-major window order
    (zeros of the ReLU tie in most windows; a negative a = inv_std * gamma flips which pixel wins)."""
    problem = S.fused_pool_problem('max', case)
    check_fused_precondition('max', case, problem)
    check_fused_max_forward(lib, case, problem)


class FusedBackward:
    """One srgan_bn_relu_maxpool_bwd / srgan_bn_relu_avgpool2_bwd call: every buffer made first (that synchronises), `launch`
    only launches, `check` waits and compares."""

    def __init__(self, form, case, problem, parameters=True):
        n, c, h, w = case
        self.form, self.case, self.problem = form, case, problem
        self.inputs = [device(problem['g'])] + ([problem['index'].to(torch.int32).cuda()] if form == 'max' else []) + \
            [device(problem['x'])] + fused_vectors(problem['v'])
        self.gx = Guarded(n * c * h * w)
        self.g_gamma = Guarded(c, problem['old_gamma']) if parameters else None
        self.g_beta = Guarded(c, problem['old_beta']) if parameters else None
        self.what = f'bn_relu_{form}pool_bwd {case}' + ('' if parameters else ' without parameter gradients')

    def launch(self, lib):
        n, c, h, w = self.case
        outputs = [self.gx.ptr, None if self.g_gamma is None else self.g_gamma.ptr, None if self.g_beta is None else self.g_beta.ptr]
        if self.form == 'max':
            oh, ow = self.problem['g'].shape[2:]
            status = lib.srgan_bn_relu_maxpool_bwd(*[t.data_ptr() for t in self.inputs], *outputs, n, c, h, w, 3, 2, 1, oh, ow, stream())
        else:
            status = lib.srgan_bn_relu_avgpool2_bwd(*[t.data_ptr() for t in self.inputs], *outputs, n, c, h, w, stream())
        check(status, self.what)
        return self

    def check(self):
        assert_exact(self.gx.result(self.what + ' gx', self.case), self.problem['gx'], self.what + ' gx')
        self.check_parameters()

    def check_parameters(self):
        if self.g_gamma is not None:
            assert_exact(self.g_gamma.result(self.what + ' g_gamma'), self.problem['g_gamma'], self.what + ' g_gamma', dims=('c',))
            assert_exact(self.g_beta.result(self.what + ' g_beta'), self.problem['g_beta'], self.what + ' g_beta', dims=('c',))


def check_fused_backward(lib, form, case):
    """With both parameter gradients (added onto distinct integers), then with neither: the same gx, and the first call's
    parameter windows as they were."""
    problem = S.fused_pool_problem(form, case)
    check_fused_precondition(form, case, problem)
    full = FusedBackward(form, case, problem).launch(lib)
    full.check()
    bare = FusedBackward(form, case, problem, parameters=False).launch(lib)
    bare.check()
    same_bits(bare.gx.window, full.gx.window, bare.what)
    full.check_parameters()


@pytest.mark.parametrize('case', S.FUSED_MAX_BWD, ids=lambda case: fused_id('max', case))
def test_fused_max_pool_backward(lib, case):
    """srgan_bn_relu_maxpool_bwd (3 / 2 / 1) per element: gx = S * [bn(x) > 0] * inv_std * gamma, g_gamma += inv_std * sum S (x -
    mean), g_beta += sum S, from one to several workgroups per plane, C up to and beyond the ordered finish's rows, N * C at the
    grid's limit; the fused forward at the same shapes gives the arg-max this backward is handed."""
    problem = S.fused_pool_problem('max', case)
    check_fused_max_forward(lib, case, problem)
    check_fused_backward(lib, 'max', case)


@pytest.mark.parametrize('case', S.FUSED_AVG, ids=lambda case: fused_id('avg', case))
def test_fused_avg_pool_forward_and_backward(lib, case):
    """srgan_bn_relu_avgpool2_fwd / _bwd per element, S = 0.25 * gy[h / 2, w / 2]; the small cases again with y and gy 8 bytes
    (not 16) past a 16-byte boundary, which their float2 accesses allow."""
    n, c, h, w = case
    problem = S.fused_pool_problem('avg', case)
    check_fused_precondition('avg', case, problem)
    keep = [device(problem['x'])] + fused_vectors(problem['v'])
    for offset in ([0, 2] if n * c * h * w <= 4096 else [0]):
        what = f'bn_relu_avgpool2_fwd {case} y {offset} floats off alignment'
        y = Guarded(n * c * (h // 2) * (w // 2), NAN, offset)
        check(lib.srgan_bn_relu_avgpool2_fwd(*[t.data_ptr() for t in keep], y.ptr, n, c, h, w, stream()), what)
        assert_exact(y.result(what, problem['y'].shape), problem['y'], what)
    check_fused_backward(lib, 'avg', case)
    if n * c * h * w <= 4096:
        shifted = FusedBackward('avg', case, problem)
        shifted.inputs[0] = device(problem['g'], 2)
        shifted.what += ' gy 2 floats off alignment'
        shifted.launch(lib).check()


def test_fused_pool_backwards_back_to_back_on_one_stream(lib):
    """Eight launches with no synchronisation between them -- the max form at 2, 6, 1, 2 partial sums per channel with another N,
    C and plane each time, then the average form likewise -- through the one ticket array and the one workspace region: a
    ticket that is not put back, or partials indexed with the previous launch's parts, shows in a later launch's sums."""
    calls = [FusedBackward(form, case, S.fused_pool_problem(form, case))
             for form, cases in (('max', S.FUSED_MAX_SEQUENCE), ('avg', S.FUSED_AVG_SEQUENCE)) for case in cases]
    for call in calls:
        check_fused_precondition(call.form, call.case, call.problem)
    torch.cuda.synchronize()
    for call in calls:
        call.launch(lib)
    for call in calls:
        call.check()


def test_fused_pool_backwards_repeat_bit_for_bit(lib):
    """Full-mantissa operands, several workgroups per plane, three runs each: gx, g_gamma and g_beta have the same bits every
    time (the ordered finish; correctness is the exact cases').  Only in the default mode: fp32 atomics add in arrival order."""
    if os.environ.get('SRGAN_ATOMIC_SPLIT') is not None:
        return
    assert lib.srgan_split_is_ordered(stream()) == 1
    for form, cases in S.FUSED_REPEAT.items():
        for case in cases:
            problem = dict(S.fused_pool_random_problem(form, case))
            if form == 'max':
                problem['index'] = run_fused_max_forward(lib, case, problem, f'bn_relu_maxpool_fwd {case} (random)')[1].cpu().long()
            runs = []
            for _ in range(3):
                call = FusedBackward(form, case, problem).launch(lib)
                runs.append([call.gx.result(call.what).clone(), call.g_gamma.result(call.what).clone(), call.g_beta.result(call.what).clone()])
            assert bool(torch.isfinite(runs[0][0]).all()) and not bool((runs[0][1].cpu() == problem['old_gamma'].float()).any())
            for run in runs[1:]:
                for name, got, first in zip(('gx', 'g_gamma', 'g_beta'), run, runs[0]):
                    same_bits(got, first, f'{call.what} (random) {name} against the first run')


def test_fused_pools_refuse_what_they_do_not_have(lib):
    """Host side only (nothing is launched): the two `_supported` predicates across their limits; SRGAN_EUNSUPPORTED for such a
    geometry and for x / gx off 16 bytes or the average form's y / gy off 8; SRGAN_EINVAL for exactly one parameter gradient.
    Every buffer is large enough for the call had it been accepted; every output keeps its NaN / old contents and its guards."""
    from srgan_amd import _lib
    max_ok, avg_ok = lib.srgan_bn_relu_maxpool_bwd_supported, lib.srgan_bn_relu_avgpool2_supported
    max_geometries = [(2, 3, 8, 4, 3, 2, 1), (2, 3, 7, 8, 3, 2, 1), (2, 3, 8, 6, 3, 2, 1), (2, 3, 8, 5, 3, 2, 1), (1, 65535, 1, 4, 3, 2, 1),
                      (1, 65536, 1, 4, 3, 2, 1), (2, 32768, 1, 4, 3, 2, 1), (5, 13107, 1, 4, 3, 2, 1), (2, 3, 8, 4, 2, 2, 0), (2, 3, 8, 4, 3, 1, 1),
                      (2, 3, 8, 4, 3, 2, 0), (2, 3, 8, 4, 3, 3, 0), (2, 3, 8, 4, 2, 2, 1)]
    assert [max_ok(*g) for g in max_geometries] == [1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0]
    assert [int(S.fused_max_bwd_supported(*g)) for g in max_geometries] == [max_ok(*g) for g in max_geometries]
    avg_geometries = [(2, 3, 6, 8), (2, 3, 6, 6), (2, 3, 6, 7), (2, 3, 5, 8), (2, 3, 1, 8), (1, 65535, 2, 4), (1, 65536, 2, 4), (5, 13107, 2, 4),
                      (4, 16384, 2, 4)]
    assert [avg_ok(*g) for g in avg_geometries] == [1, 0, 0, 0, 0, 1, 0, 1, 0]
    assert [int(S.fused_avg_supported(*g)) for g in avg_geometries] == [avg_ok(*g) for g in avg_geometries]

    def buffers(n, c, h, w, oh, ow, x_offset=0, gx_offset=0, y_offset=0):
        zeros = torch.zeros(n * c * max(h * w, oh * ow))
        vectors = [device(torch.ones(c)) for _ in range(4)]
        return dict(x=device(zeros[:n * c * h * w], x_offset), gy=device(zeros[:n * c * oh * ow], y_offset),
                    index=torch.zeros(n * c * oh * ow, dtype=torch.int32, device='cuda'), vectors=[t.data_ptr() for t in vectors], keep=vectors,
                    gx=Guarded(n * c * h * w, NAN, gx_offset), y=Guarded(n * c * oh * ow, NAN, y_offset),
                    g_gamma=Guarded(c, 5.0), g_beta=Guarded(c, -3.0))

    def untouched(b, what):
        for name, value in (('gx', None), ('y', None), ('g_gamma', 5.0), ('g_beta', -3.0)):
            window = b[name].result(f'{what}: {name}').cpu()
            assert bool(torch.isnan(window).all() if value is None else (window == value).all()), f'{what}: {name} was written'

    def max_bwd(b, geometry, oh, ow, g_gamma=True, g_beta=True):
        return lib.srgan_bn_relu_maxpool_bwd(b['gy'].data_ptr(), b['index'].data_ptr(), b['x'].data_ptr(), *b['vectors'], b['gx'].ptr,
                                             b['g_gamma'].ptr if g_gamma else None, b['g_beta'].ptr if g_beta else None, *geometry, oh, ow, stream())

    def avg_fwd(b, geometry):
        return lib.srgan_bn_relu_avgpool2_fwd(b['x'].data_ptr(), *b['vectors'], b['y'].ptr, *geometry, stream())

    def avg_bwd(b, geometry, g_gamma=True, g_beta=True):
        return lib.srgan_bn_relu_avgpool2_bwd(b['gy'].data_ptr(), b['x'].data_ptr(), *b['vectors'], b['gx'].ptr,
                                              b['g_gamma'].ptr if g_gamma else None, b['g_beta'].ptr if g_beta else None, *geometry, stream())

    for geometry in [g for g in max_geometries if not max_ok(*g)]:
        n, c, h, w, k, s, p = geometry
        oh, ow = S.pool_out(h, k, s, p), S.pool_out(w, k, s, p)
        b = buffers(n, c, h, w, oh, ow)
        assert max_bwd(b, geometry, oh, ow) == _lib.EUNSUPPORTED, geometry
        assert max_bwd(b, geometry, oh, ow, False, False) == _lib.EUNSUPPORTED, geometry
        untouched(b, f'srgan_bn_relu_maxpool_bwd {geometry}')
    for geometry in [g for g in avg_geometries if not avg_ok(*g)]:
        n, c, h, w = geometry
        b = buffers(n, c, h, w, max(h // 2, 1), max(w // 2, 1))
        assert avg_fwd(b, geometry) == _lib.EUNSUPPORTED and avg_bwd(b, geometry) == _lib.EUNSUPPORTED, geometry
        assert avg_bwd(b, geometry, False, False) == _lib.EUNSUPPORTED, geometry
        untouched(b, f'srgan_bn_relu_avgpool2 {geometry}')
    geometry = (2, 3, 8, 4, 3, 2, 1)
    for offsets in (dict(x_offset=1), dict(gx_offset=1), dict(x_offset=2), dict(gx_offset=3)):
        b = buffers(2, 3, 8, 4, 4, 2, **offsets)
        assert max_bwd(b, geometry, 4, 2) == _lib.EUNSUPPORTED, offsets
        untouched(b, f'srgan_bn_relu_maxpool_bwd {offsets}')
    geometry = (2, 3, 6, 8)
    for offsets in (dict(x_offset=1), dict(gx_offset=1), dict(x_offset=2), dict(gx_offset=2), dict(y_offset=1), dict(y_offset=3)):
        b = buffers(2, 3, 6, 8, 3, 4, **offsets)
        if 'gx_offset' not in offsets:
            assert avg_fwd(b, geometry) == _lib.EUNSUPPORTED, offsets
        assert avg_bwd(b, geometry) == _lib.EUNSUPPORTED, offsets
        untouched(b, f'srgan_bn_relu_avgpool2 {offsets}')
    b = buffers(2, 3, 8, 4, 4, 2)
    assert max_bwd(b, (2, 3, 8, 4, 3, 2, 1), 4, 2, True, False) == _lib.EINVAL and max_bwd(b, (2, 3, 8, 4, 3, 2, 1), 4, 2, False, True) == _lib.EINVAL
    untouched(b, 'srgan_bn_relu_maxpool_bwd with one parameter gradient')
    b = buffers(2, 3, 6, 8, 3, 4)
    assert avg_bwd(b, (2, 3, 6, 8), True, False) == _lib.EINVAL and avg_bwd(b, (2, 3, 6, 8), False, True) == _lib.EINVAL
    untouched(b, 'srgan_bn_relu_avgpool2_bwd with one parameter gradient')


@pytest.mark.parametrize('case', S.COPY_CHANNELS, ids=lambda case: f"accumulate{case['accumulate']}")
def test_copy_channels(lib, case):
    n, hw, count = case['N'], case['HW'], case['count']
    (cs, fs), (cd, fd) = case['src'], case['dst']
    gen = S.generator('copy_channels', n, hw, count)
    source, old = S.distinct((n, cs, hw), gen), S.distinct((n, cd, hw), gen)
    out, keep = Guarded(n * cd * hw, old), device(source)
    check(lib.srgan_copy_channels(keep.data_ptr(), cs, fs, out.ptr, cd, fd, count, n, hw, case['accumulate'], stream()), 'srgan_copy_channels')
    want = old.clone()
    want[:, fd:fd + count] = source[:, fs:fs + count] + (old[:, fd:fd + count] if case['accumulate'] else 0)
    assert_exact(out.result(f'copy_channels {case}', (n, cd, hw)), want, f'copy_channels {case}', dims=('n', 'c', 'i'))


# ------------------------------------------------------------------------------------------------- Adam
def adam_call(lib, tensors, grad, n, decay, step=None, state=None):
    hyper = (S.ADAM['lr'], S.ADAM['beta1'], S.ADAM['beta2'], S.ADAM['eps'], decay)
    if state is None:
        check(lib.srgan_adam_step(tensors[0].ptr, grad.data_ptr(), tensors[1].ptr, tensors[2].ptr, n, *hyper, step, stream()), 'srgan_adam_step')
    else:
        check(lib.srgan_adam_step_counted(tensors[0].ptr, grad.data_ptr(), tensors[1].ptr, tensors[2].ptr, n, *hyper, state.data_ptr(),
                                          stream()), 'srgan_adam_step_counted')


@pytest.mark.parametrize('decay', S.ADAM_DECAY)
@pytest.mark.parametrize('n', S.ADAM_N)
def test_adam_both_entry_points(lib, n, decay):
    """Three consecutive steps through srgan_adam_step(step = t) and srgan_adam_step_counted from the same start: bit-identical
    p, m, v (both round the same double-precision corrections), state[0] counts up; and every step, started from torch.optim.Adam's
    fp32 state, within the bound of streaming_cases.adam_expected of the float64 update."""
    problem, steps = S.adam_problem(n, decay), S.adam_expected(n, decay)
    grads = [device(grad) for grad in problem['grads']]
    plain = [Guarded(n, problem[key]) for key in 'pmv']
    counted = [Guarded(n, problem[key]) for key in 'pmv']
    state = torch.zeros(3, dtype=torch.int32, device='cuda')
    for index in range(S.ADAM_STEPS):
        adam_call(lib, plain, grads[index], n, decay, step=index + 1)
        adam_call(lib, counted, grads[index], n, decay, state=state)
        for name, one, other in zip('pmv', plain, counted):
            what = f'adam n={n} decay={decay} step {index + 1} {name}'
            same_bits(one.result(what), other.result(what + ' (counted)'), what + ': srgan_adam_step against srgan_adam_step_counted')
        assert int(state[0]) == index + 1
    for index, entry in enumerate(steps):
        for form in ('plain', 'counted'):
            tensors = [Guarded(n, start) for start in entry['start']]
            if form == 'plain':
                adam_call(lib, tensors, grads[index], n, decay, step=index + 1)
            else:
                counter = torch.tensor([index, 0, 0], dtype=torch.int32, device='cuda')
                adam_call(lib, tensors, grads[index], n, decay, state=counter)
                assert int(counter[0]) == index + 1
            for name, tensor, want, bound, scale in zip('pmv', tensors, entry['want'], entry['bound'], entry['scale']):
                what = f'adam ({form}) n={n} decay={decay} step {index + 1} {name}'
                assert_ulps(tensor.result(what), want, bound, what, scale=scale)


def test_adam_counter_advances_without_elements(lib):
    state = torch.tensor([4, 0, 0], dtype=torch.int32, device='cuda')
    tensors = [Guarded(1, 1.0) for _ in range(3)]
    grad = device(torch.ones(1))
    adam_call(lib, tensors, grad, 0, 0.0, state=state)
    assert int(state[0]) == 5
    for tensor in tensors:
        assert tensor.result('adam n = 0').cpu().tolist() == [1.0]


def test_tanh_is_exactly_one_from_nine(lib):
    """The tanh op saturates at |x| = 9 (include/srgan_hip.h): exactly +-1 from there on, the library's tanhf below.  tanh(9) =
    0.99999996954 in float64; the fp32 neighbours are 1 - 2^-24 = 0.99999994 (0.49 ulp away, what the library's tanhf and torch's
    CPU fp32 tanh return at 9) and 1.0 (0.51 ulp away), and from 9.011 on 1.0 is the nearest anyway: the saturated value is never
    more than 0.51 ulp off, well inside the sweep's 2 ulp."""
    got = run_unary(lib, 'tanh', torch.tensor([9.0, -9.0], dtype=torch.float64), 0.0, 0.0, False).cpu().tolist()
    assert got == [1.0, -1.0], got
    below = float(torch.nextafter(torch.tensor(9.0), torch.tensor(0.0)))
    edge = torch.tensor([9.0, 9.000001, 9.005, 9.011, 12.0, 88.0, math.inf, below, 8.5], dtype=torch.float64).float().double()
    x = torch.cat([edge, -edge])
    got = run_unary(lib, 'tanh', x, 0.0, 0.0, False).cpu()
    assert_exact(got[x.abs() >= 9.0], x[x.abs() >= 9.0].sign(), 'tanh from 9 on', dims=('i',))
    assert_ulps(got, S.unary_ref('tanh', x), S.transcendental_bound('tanh')[1], 'tanh around 9', x)
    assert bool((got.abs() <= 1.0).all())
    assert math.isnan(float(run_unary(lib, 'tanh', torch.tensor([NAN], dtype=torch.float64), 0.0, 0.0, False)[0]))


# ------------------------------------------------------------------------------------------------- fp32 atomics
CHILD_TIMEOUT = 30            # seconds: the child takes 9 s on the MI355X (6.2 s of tests + start-up), 3 x that and rounded up


def test_the_file_again_with_fp32_atomic_combines():
    """Every test above again in a child process with SRGAN_ATOMIC_SPLIT=1 (read once per process): srgan_chan_reduce (with its
    zero-fill in front), srgan_bn_act_bwd and srgan_crowd_map_l1_fwd then meet through fp32 atomics instead of the ordered
    finishes.  On exact operands the atomics are order-independent, so the same bit-exact assertions hold; the accumulate cases
    check that the atomics add onto a live, non-zero output."""
    environment = dict(os.environ, SRGAN_ATOMIC_SPLIT='1')
    started = time.time()
    done = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k', 'not atomic',
                           '-p', 'no:cacheprovider'], env=environment, capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
    assert done.returncode == 0, f'after {time.time() - started:.0f} s:\n' + done.stdout[-4000:] + done.stderr[-2000:]
    assert ' passed' in done.stdout and 'failed' not in done.stdout, done.stdout[-2000:]
    assert ' 1 deselected' in done.stdout, done.stdout[-2000:]          # this test alone: no other id may hold the word `atomic`
