"""The kernels that create and move the blocked layout and the weight shadows, through the C ABI, per element and bit for bit:
srgan_h_pack / _unpack / _add / _channel_sums, srgan_h_maxpool2 / _bwd, srgan_h_pack_conv_weights, srgan_h_pack_k4s2_weights,
srgan_h_pack_matrix (both bodies), the bias rows and srgan_h_pack_batched.

Every output is a window between guard bands (helpers.Guarded), prefilled with NaN bits of its type -- an element never written
fails, the padding lanes of a slot included, which must come out as +0 -- or, for the accumulating srgan_h_channel_sums, with
distinct integers that the expected value includes.  Outputs are compared as bits; a NaN compares as "is NaN".  Blocked inputs of
srgan_h_unpack and srgan_h_channel_sums carry NaN bits in their padding lanes, which must not reach a result.  The cases, the
references and the branch every case reaches are blocked_cases.py's (checked on the CPU by test_blocked_cases_cpu.py).

Bit-exactness is the criterion everywhere but in test_channel_sums_of_inexact_values (L * 2^-24 * sum |x|, L from the kernels;
on the MI355X, L = 31: worst error 0.022 / 0.0023 / 0.0018 of the bound for dtype 0 / 1 / 2, and L = 24 with the two-launch finish).
The rules asserted here are the "Rounding" and "NaN and mask rule" paragraphs of include/srgan_hip.h.  Found on the MI355X:
the 16-bit stores equal torch's CPU conversion on every entry of the rounding table, fp32-subnormal inputs and 16-bit subnormal
results included (nothing is flushed to zero), and srgan_h_add equals one fp32 addition and one rounding on sums of subnormals.

srgan_h_pack_conv_weights has no case of 257 slots: its slot count is even (two halves per chunk); 258 stands in (CONV_258).
"""
import ctypes
import os
import subprocess
import sys
import time

import pytest
import torch

import blocked_cases as B
from helpers import Guarded, assert_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1
ATOMIC = os.environ.get('SRGAN_ATOMIC_SPLIT') is not None
CHILD_TIMEOUT = 60            # seconds


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


def dev(t):
    t = t.contiguous().cuda()
    assert t.data_ptr() % 16 == 0
    return t


def slots_window(slots, dtype):
    """An output of `slots` 16-byte slots, every element a NaN of the type."""
    return Guarded(4 * max(int(slots), 1), B.NAN_FILL[dtype], dtype=torch.int32)


def stored(out, dtype, what, shape):
    """The window's bits after the call (guards checked): int32 for dtype 0, int16 halves for the 16-bit types."""
    out.result(what)
    return (out.window if dtype == 0 else out.halves()).cpu().reshape(shape)


def float_bits(out, what, shape):
    return out.result(what).view(torch.int32).cpu().reshape(shape)


def same(got, want, dtype, what, inputs=None):
    assert got.shape == want.shape and got.dtype == want.dtype, f'{what}: {tuple(got.shape)} {got.dtype} != {tuple(want.shape)} {want.dtype}'
    fine = (got == want) | (B.is_nan(got, dtype) & B.is_nan(want, dtype))
    if bool(fine.all()):
        return
    bad = (~fine).nonzero()
    mask = 0xFFFFFFFF if got.dtype == torch.int32 else 0xFFFF
    lines = [f'{what}: {bad.shape[0]} of {got.numel()} elements differ in their bits (shape {tuple(got.shape)})']
    for index in bad[:12].tolist():
        at = tuple(index)
        lines.append(f'  {index}: got {int(got[at]) & mask:#x} want {int(want[at]) & mask:#x}' + (f' from {inputs(at)}' if inputs else ''))
    raise AssertionError('\n'.join(lines))


def untouched(out, dtype, what):
    out.result(what)
    assert bool((out.window.cpu() == B.NAN_FILL[dtype]).all()), f'{what}: the output window was written'


# ----------------------------------------------------------------------------------------------------- pack / unpack
def run_pack(lib, x, dtype, ref_bits=None, slope=1.0):
    n, c, hw = x.shape
    out = slots_window(B.pack_slots(n, c, hw, dtype), dtype)
    source, ref = dev(x), None if ref_bits is None else dev(ref_bits)
    check(lib.srgan_h_pack(source.data_ptr(), out.ptr, None if ref is None else ref.data_ptr(), slope, n, c, hw, dtype, stream()), 'srgan_h_pack')
    return stored(out, dtype, f'pack {tuple(x.shape)} dtype {dtype}', (n, B.groups(c, dtype), hw, B.GROUP[dtype]))


def run_unpack(lib, bits, c, dtype):
    n, _, hw, _ = bits.shape
    out = Guarded(n * c * hw)
    source = dev(bits)
    check(lib.srgan_h_unpack(source.data_ptr(), out.ptr, n, c, hw, dtype, stream()), 'srgan_h_unpack')
    return float_bits(out, f'unpack {tuple(bits.shape)} C={c} dtype {dtype}', (n, c, hw))


def pack_and_unpack(lib, n, c, hw, dtype):
    x = B.distinct_values(n * c * hw, dtype, 'pack', n, c, hw).reshape(n, c, hw)
    want = B.pack_ref(x, dtype)
    same(run_pack(lib, x, dtype), want, dtype, f'pack N={n} C={c} HW={hw} dtype {dtype}')
    poisoned = B.poison_padding(want, c, dtype)
    same(run_unpack(lib, poisoned, c, dtype), x.view(torch.int32), 0, f'unpack N={n} C={c} HW={hw} dtype {dtype}')


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_pack_and_unpack_at_every_shape(lib, dtype):
    """Distinct values: a misplaced element shows.  Padding lanes: +0 out of pack, NaN bits into unpack."""
    for n in B.PACK_N:
        for c in B.PACK_C:
            for hw in B.PACK_HW:
                pack_and_unpack(lib, n, c, hw, dtype)


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_pack_and_unpack_on_the_second_grid_stride_trip(lib, dtype):
    pack_and_unpack(lib, *B.PACK_SECOND_TRIP[dtype], dtype)


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_pack_and_unpack_of_no_images_write_nothing(lib, dtype):
    out, source = slots_window(4, dtype), torch.zeros(64, device='cuda')
    assert lib.srgan_h_pack(source.data_ptr(), out.ptr, None, 1.0, 0, 5, 7, dtype, stream()) == OK
    untouched(out, dtype, 'pack N=0')
    assert lib.srgan_h_unpack(source.data_ptr(), out.ptr, 0, 5, 7, dtype, stream()) == OK
    untouched(out, dtype, 'unpack N=0')


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_pack_rounds_to_nearest_even(lib, dtype):
    """The rounding table against torch's CPU conversion: ties of both parities and signs, the overflow boundaries, 16-bit and
    fp32 subnormals (nothing is flushed), +-0, +-inf, NaN.  dtype 0 copies the bits."""
    table = B.rounding_table(dtype if dtype else 1)
    x = table.reshape(1, -1, 1)
    words = table.view(torch.int32)
    got = run_pack(lib, x, dtype)
    same(got, B.pack_ref(x, dtype), dtype, f'rounding table dtype {dtype}',
         inputs=lambda at: f'{int(words[at[1] * B.GROUP[dtype] + at[3]]) & 0xFFFFFFFF:#010x}' if at[1] * B.GROUP[dtype] + at[3] < words.numel() else 'padding')
    if dtype:
        for word, low in B.rounding_ties(dtype):                     # said again without torch: a tie goes to the even neighbour
            index = int((words == B.wrap32([word])).nonzero()[0])
            result = int(got[0, index // 8, 0, index % 8]) & 0xFFFF
            assert result in (low, low + 1) and result % 2 == 0, (hex(word), hex(low), hex(result))


@pytest.mark.parametrize('slope', B.SLOPES)
@pytest.mark.parametrize('dtype', B.DTYPES)
def test_pack_masks_by_reference(lib, dtype, slope):
    """x * (1 if ref > 0 else slope) in fp32, rounded once; ref > 0 per the header's rule: the stored bits for the 16-bit types
    (a NaN with a clear sign is positive), the float comparison for dtype 0 (a NaN never is)."""
    n, c, hw = 2, 13, 27
    x = B.distinct_values(n * c * hw, dtype, 'mask', moderate=True).reshape(n, c, hw)
    refs = B.mask_ref_bits(dtype)
    count = B.pack_slots(n, c, hw, dtype) * B.GROUP[dtype]
    ref_bits = refs.repeat(-(-count // refs.numel()))[:count].reshape(n, B.groups(c, dtype), hw, B.GROUP[dtype])      # 9 and G are coprime
    got = run_pack(lib, x, dtype, ref_bits, slope)
    same(got, B.pack_ref(x, dtype, ref_bits, slope), dtype, f'mask dtype {dtype} slope {slope}',
         inputs=lambda at: f'ref {int(ref_bits[at]) & 0xFFFFFFFF:#x}')
    # said again from the table of the rule: the factor of every reference kind
    values, factors = B.from_bits(got, dtype), B.blocked(x, dtype)
    for kind, is_positive in enumerate(B.MASK_POSITIVE[dtype]):
        chosen = (ref_bits == refs[kind]) & (factors != 0)
        want = B.from_bits(B.to_bits(factors[chosen] * (1.0 if is_positive else slope), dtype), dtype)
        assert chosen.any() and torch.equal(values[chosen], want), (dtype, slope, kind)


@pytest.mark.parametrize('dtype', B.HALVES)
def test_unpack_and_pack_of_every_bit_pattern(lib, dtype):
    """All 65536 patterns: unpack is torch's reinterpretation, and packing the result gives every non-NaN pattern back."""
    n, c, hw = B.ALL_PATTERNS
    bits = B.wrap16(torch.arange(65536)).reshape(n, 1, hw, c)
    unpacked = run_unpack(lib, bits, c, dtype)
    same(unpacked, B.unpack_ref(bits, c, dtype).view(torch.int32), 0, f'unpack of every pattern, dtype {dtype}')
    again = run_pack(lib, unpacked.view(torch.float32), dtype)
    same(again, bits, dtype, f'pack of every unpacked pattern, dtype {dtype}')
    nan = B.is_nan(bits, dtype)
    assert torch.equal(again[~nan], bits[~nan]) and int(nan.sum()) == (254 if dtype == 1 else 2046)


# ----------------------------------------------------------------------------------------------------- add
ADD_PAIRS = {
    2: [(2048.0, 1.0), (2050.0, 1.0), (2048.0, 1.0 + 2.0 ** -10), (2050.0, 1.0 - 2.0 ** -11), (-2048.0, -1.0), (-2050.0, -1.0),
        (65504.0, 16.0), (65504.0, 15.9921875), (-65504.0, -16.0), (65504.0, 65504.0), (2.0 ** -24, 2.0 ** -24), (2.0 ** -14, -2.0 ** -24),
        (float('inf'), float('-inf')), (float('inf'), 1.0), (0.0, -0.0), (-0.0, -0.0), (3.0, 4.0), (1.5, -1.5)],
    1: [(256.0, 1.0), (258.0, 1.0), (256.0, 1.0078125), (258.0, 0.99609375), (-256.0, -1.0), (-258.0, -1.0),
        (3.3895313892515355e38, 2.0 ** 119), (3.3895313892515355e38, 2.0 ** 118), (-3.3895313892515355e38, -2.0 ** 119),
        (3.3895313892515355e38, 3.3895313892515355e38), (2.0 ** -133, 2.0 ** -133), (2.0 ** -126, -2.0 ** -133),
        (float('inf'), float('-inf')), (float('inf'), 1.0), (0.0, -0.0), (-0.0, -0.0), (3.0, 4.0), (1.5, -1.5)],
    0: [(1.0 + 2.0 ** -23, 2.0 ** -24), (1.0, 2.0 ** -24), (1.0 + 2.0 ** -22, -2.0 ** -24), (3.4028234663852886e38, 3.4028234663852886e38),
        (3.4028234663852886e38, 2.0 ** 103), (2.0 ** -149, 2.0 ** -149), (2.0 ** -126, -2.0 ** -149),
        (float('inf'), float('-inf')), (float('inf'), 1.0), (0.0, -0.0), (-0.0, -0.0), (3.0, 4.0), (1.5, -1.5)]}


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_add_at_every_length(lib, dtype):
    """One fp32 addition and one rounding per element: exact operands, ties of both parities, overflow to inf, inf - inf, sums of
    subnormals, then distinct moderate values."""
    g = B.GROUP[dtype]
    pairs = torch.tensor(ADD_PAIRS[dtype], dtype=torch.float32)
    assert torch.equal(B.from_bits(B.to_bits(pairs, dtype), dtype).nan_to_num(), pairs.nan_to_num())          # all representable
    for slots in B.ADD_SLOTS:
        count = slots * g
        a = torch.cat([pairs[:, 0], B.distinct_values(count, dtype, 'add a', moderate=True)])[:count]
        b = torch.cat([pairs[:, 1], B.distinct_values(count, dtype, 'add b', moderate=True)])[:count]
        a_bits, b_bits = B.to_bits(a, dtype).reshape(slots, g), B.to_bits(b, dtype).reshape(slots, g)
        out = slots_window(slots, dtype)
        first, second = dev(a_bits) if slots else torch.zeros(8, device='cuda'), dev(b_bits) if slots else torch.zeros(8, device='cuda')
        assert lib.srgan_h_add(first.data_ptr(), second.data_ptr(), out.ptr, slots, dtype, stream()) == OK
        if slots == 0:
            untouched(out, dtype, 'add of no slots')
            continue
        same(stored(out, dtype, f'add {slots} slots dtype {dtype}', (slots, g)), B.add_ref(a_bits, b_bits, dtype), dtype,
             f'add {slots} slots dtype {dtype}', inputs=lambda at: f'{float(a[at[0] * g + at[1]])!r} + {float(b[at[0] * g + at[1]])!r}')


# ----------------------------------------------------------------------------------------------------- channel sums
def prefill(c):
    return (torch.arange(c) % 61 - 30).float() * 4 + 1               # distinct-ish integers of either sign, |.| <= 4 * 30 + 1


def launch_sums(lib, source, out, n, c, hw, dtype):
    check(lib.srgan_h_channel_sums(source.data_ptr(), out.ptr, n, c, hw, dtype, stream()), 'srgan_h_channel_sums')


def integer_case(n, c, hw, dtype):
    x = B.integers((n, c, hw), B.generator('sums', n, c, hw, dtype))
    B.assert_sums_exact(n, hw, 4 * 30 + 1)
    return B.poison_padding(B.pack_ref(x, dtype), c, dtype)


def check_sums(out, bits, c, dtype, what):
    got = out.result(what)
    assert_exact(got, prefill(c).double() + B.channel_sums_ref(bits, c, dtype), what, dims=('c',))
    return got.cpu().view(torch.int32)


def test_channel_sums_finish_mode(lib):
    assert lib.srgan_split_is_ordered(stream()) == (0 if ATOMIC else 1)


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_channel_sums_of_integers_at_every_parts_choice(lib, dtype):
    """parts 1, 2, 3 and the cap of 256, CG beyond the ordered finish's rows; C no multiple of G; NaN bits in the padding lanes;
    accumulated onto distinct integers in a window of exactly C floats."""
    for n, c, hw in B.SUMS_SMALL + [B.SUMS_CAP, B.sums_many_groups(dtype)]:
        bits = integer_case(n, c, hw, dtype)
        source, out = dev(bits), Guarded(c, prefill(c))
        launch_sums(lib, source, out, n, c, hw, dtype)
        first = check_sums(out, bits, c, dtype, f'channel sums N={n} C={c} HW={hw} dtype {dtype} parts {B.sums_parts(n, c, hw, dtype)}')
        again = Guarded(c, prefill(c))
        launch_sums(lib, source, again, n, c, hw, dtype)
        assert torch.equal(again.result('again').cpu().view(torch.int32), first)


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_channel_sums_where_the_parts_are_halved(lib, dtype):
    """parts * CG > 4096: 2049 groups of 4097 pixels, generated on the device, against a device int64 sum."""
    n, c, hw = B.sums_halved(dtype)
    g, cg = B.GROUP[dtype], B.groups(c, dtype)
    assert B.sums_parts(n, c, hw, dtype) == (1, 'halved')
    gen = torch.Generator(device='cuda').manual_seed(5)
    integers = torch.randint(-B.X, B.X + 1, (n, cg, hw, g), device='cuda', dtype=torch.int16, generator=gen)
    want = integers.sum(dim=(0, 2), dtype=torch.int64).reshape(-1)[:c].cpu()
    bits = integers.to(B.TORCH[dtype]).view(B.BITS[dtype])
    del integers
    bits[:, -1, :, g - (cg * g - c):] = B.NAN_BITS[dtype]            # the padding lane
    out = Guarded(c, prefill(c))
    launch_sums(lib, bits, out, n, c, hw, dtype)
    assert_exact(out.result('halved parts'), prefill(c).double() + want.double(), f'channel sums, halved parts, dtype {dtype}', dims=('c',))


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_channel_sums_back_to_back_reuse_the_tickets(lib, dtype):
    """Launches with another CG and another number of parts each time, enqueued without a wait in between."""
    runs = []
    for n, c, hw in B.SUMS_SEQUENCE:
        bits = integer_case(n, c, hw, dtype)
        runs.append((bits, dev(bits), Guarded(c, prefill(c)), n, c, hw))
    for _, source, out, n, c, hw in runs:
        launch_sums(lib, source, out, n, c, hw, dtype)
    for bits, _, out, n, c, hw in runs:
        check_sums(out, bits, c, dtype, f'back to back N={n} C={c} HW={hw} dtype {dtype}')


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_channel_sums_of_inexact_values(lib, dtype):
    """Full-mantissa values against float64: |error| <= L * 2^-24 * (|out before| + sum |x|) per channel, L = the longest chain of
    dependent fp32 additions (blocked_cases.sums_chain_length); the same bits on a second run."""
    n, c, hw = B.SUMS_INEXACT
    x = B.distinct_values(n * c * hw, dtype, 'inexact', moderate=True).reshape(n, c, hw)
    if dtype == 0:
        x = x / 7
    bits = B.poison_padding(B.pack_ref(x, dtype), c, dtype)
    stored_x = B.unpack_ref(bits, c, dtype).double()
    source, out, again = dev(bits), Guarded(c, prefill(c)), Guarded(c, prefill(c))
    launch_sums(lib, source, out, n, c, hw, dtype)
    launch_sums(lib, source, again, n, c, hw, dtype)
    got = out.result('inexact sums').cpu()
    chain = B.sums_chain_length(n, c, hw, dtype, ATOMIC)
    error = (got.double() - (prefill(c).double() + stored_x.sum(dim=(0, 2)))).abs()
    bound = chain * 2.0 ** -24 * (prefill(c).double().abs() + stored_x.abs().sum(dim=(0, 2)))
    worst = int((error / bound).argmax())
    print(f'channel sums of inexact values, dtype {dtype}: L = {chain}, worst |error| {float(error[worst]):.3e} against the bound '
          f'{float(bound[worst]):.3e} ({float(error[worst] / bound[worst]):.4f} of it), channel {worst}')
    assert bool((error <= bound).all()), (error / bound).tolist()
    assert torch.equal(again.result('inexact sums again').cpu().view(torch.int32), got.view(torch.int32))


def test_the_channel_sums_again_with_the_two_launch_finish():
    """Every channel-sums test above in a child process with SRGAN_ATOMIC_SPLIT=1 (read once per process): no ordered finish, so
    h_channel_sums_finish_kernel adds the parts in a second launch at every shape."""
    environment = dict(os.environ, SRGAN_ATOMIC_SPLIT='1')
    started = time.time()
    done = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k', 'test_channel_sums',
                           '-p', 'no:cacheprovider'], env=environment, capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
    assert done.returncode == 0, f'after {time.time() - started:.0f} s:\n' + done.stdout[-4000:] + done.stderr[-2000:]
    assert ' passed' in done.stdout and 'failed' not in done.stdout and 'skipped' not in done.stdout, done.stdout[-2000:]


# ----------------------------------------------------------------------------------------------------- pool
def run_pool(lib, x_bits, dtype, mode, g_bits=None):
    planes, h, w, _ = x_bits.shape
    out = slots_window(planes * (h // 2) * (w // 2), dtype)
    source, other = dev(x_bits), None if g_bits is None else dev(g_bits)
    check(lib.srgan_h_maxpool2(source.data_ptr(), None if other is None else other.data_ptr(), out.ptr, planes, h, w, mode, dtype, stream()),
          'srgan_h_maxpool2')
    return stored(out, dtype, f'pool mode {mode} {tuple(x_bits.shape)}', (planes, h // 2, w // 2, 8))


def run_pool_bwd(lib, x_bits, gp_bits, dtype, masked, slope):
    planes, h, w, _ = x_bits.shape
    out = slots_window(planes * h * w, dtype)
    source, other = dev(x_bits), dev(gp_bits)
    check(lib.srgan_h_maxpool2_bwd(source.data_ptr(), other.data_ptr(), out.ptr, planes, h, w, masked, slope, dtype, stream()), 'srgan_h_maxpool2_bwd')
    return stored(out, dtype, f'pool backward {tuple(x_bits.shape)} masked {masked} slope {slope}', (planes, h, w, 8))


def check_pool(lib, x_bits, dtype, what, backwards=None):
    planes, h, w, _ = x_bits.shape
    pooled, at = B.pool_ref(x_bits, dtype)
    same(run_pool(lib, x_bits, dtype, 0), pooled, dtype, f'{what}: pool')
    g_bits = B.to_bits(B.distinct_values(x_bits.numel(), dtype, 'g', moderate=True).reshape(x_bits.shape), dtype)
    same(run_pool(lib, x_bits, dtype, 2, g_bits), B.pool_gather_ref(g_bits, at), dtype, f'{what}: gather')
    gp_bits = B.to_bits(B.distinct_values(pooled.numel(), dtype, 'gp', moderate=True).reshape(pooled.shape), dtype)
    for masked, slope in backwards if backwards is not None else [(0, 0.0)] + [(1, slope) for slope in B.POOL_SLOPES]:
        got = run_pool_bwd(lib, x_bits, gp_bits, dtype, masked, slope)
        same(got, B.pool_bwd_ref(x_bits, gp_bits, dtype, masked, slope), dtype, f'{what}: backward masked {masked} slope {slope}')
        if not masked:                          # all four positions written, three of them with +0, the fourth with gp's bits
            assert int((got == 0).sum()) == 3 * gp_bits.numel() and torch.equal(B.pool_gather_ref(got, at), gp_bits)


@pytest.mark.parametrize('dtype', B.HALVES)
def test_pool_takes_the_first_maximum_of_every_tie_pattern(lib, dtype):
    x_bits, _ = B.tie_windows(dtype)
    check_pool(lib, x_bits, dtype, f'81 tie patterns, dtype {dtype}')


@pytest.mark.parametrize('dtype', B.HALVES)
def test_pool_on_zeros_infinities_and_nan(lib, dtype):
    """Every window over -inf, -0, +0, the smallest subnormal, 1, +inf, NaN, -NaN: +0 and -0 tie (the first wins), a NaN is kept
    at position (0,0) only, and the masked backward takes `pooled > 0` from the bits (a NaN with a clear sign is positive)."""
    check_pool(lib, B.special_windows(dtype), dtype, f'special windows, dtype {dtype}')
    nan, one, two = B.NAN_BITS[dtype], int(B.to_bits(torch.tensor([1.0]), dtype)), int(B.to_bits(torch.tensor([2.0]), dtype))
    for position in range(4):                   # the header's NaN rule, said without the reference
        window = [one, two, one, one]
        window[position] = nan
        got = run_pool(lib, B.wrap16(window).reshape(1, 2, 2, 1).expand(1, 2, 2, 8).contiguous(), dtype, 0)
        assert (B.is_nan(got, dtype).all() if position == 0 else (got == (one if position == 1 else two)).all()), (dtype, position)


@pytest.mark.parametrize('dtype', B.HALVES)
def test_pool_at_every_shape(lib, dtype):
    for planes, h, w in B.POOL_SHAPES:
        x = B.integers((planes, h, w, 8), B.generator('pool', planes, h, w), limit=2)
        check_pool(lib, B.to_bits(x, dtype), dtype, f'pool {planes} x {h} x {w}, dtype {dtype}')


@pytest.mark.parametrize('dtype', B.HALVES)
def test_pool_past_the_grid_stride_cap(lib, dtype):
    planes, h, w = B.POOL_PAST_CAP
    x = B.integers((planes, h, w, 8), B.generator('pool past the cap'), limit=2)
    check_pool(lib, B.to_bits(x, dtype), dtype, f'pool of {planes} windows, dtype {dtype}', backwards=[(1, 0.125)])


@pytest.mark.parametrize('dtype', B.HALVES)
def test_pool_of_no_planes_writes_nothing(lib, dtype):
    out, source = slots_window(4, dtype), torch.zeros(64, device='cuda')
    assert lib.srgan_h_maxpool2(source.data_ptr(), None, out.ptr, 0, 4, 4, 0, dtype, stream()) == OK
    assert lib.srgan_h_maxpool2(source.data_ptr(), source.data_ptr(), out.ptr, 0, 4, 4, 2, dtype, stream()) == OK
    assert lib.srgan_h_maxpool2_bwd(source.data_ptr(), source.data_ptr(), out.ptr, 0, 4, 4, 1, 0.125, dtype, stream()) == OK
    untouched(out, dtype, 'pool of no planes')


# ----------------------------------------------------------------------------------------------------- weight-shadow packers
def conv_weights(k, c, r, s, dtype):
    return B.distinct_values(k * c * r * s, dtype, 'conv weights', k, c, r, s).reshape(k, c, r, s)


def run_conv_weights(lib, w, transposed, dtype):
    k, c, r, s = w.shape
    rows, reduced = (c, k) if transposed else (k, c)
    slots = lib.srgan_h_conv_weight_slots(rows, reduced, r, s)
    assert slots == B.conv_weight_slots(rows, reduced, r, s)
    out, source = slots_window(slots, dtype), dev(w)
    check(lib.srgan_h_pack_conv_weights(source.data_ptr(), out.ptr, k, c, r, s, transposed, dtype, stream()), 'srgan_h_pack_conv_weights')
    return stored(out, dtype, f'conv weights {tuple(w.shape)} transposed {transposed}', (slots, 8))


@pytest.mark.parametrize('transposed', [0, 1])
@pytest.mark.parametrize('dtype', B.HALVES)
def test_conv_weight_shadows(lib, dtype, transposed):
    """Distinct representable weights: every slot at its place, zeros (+0) beyond the reduced extent, nothing unwritten."""
    cases = [(k, c, r, s) for k in B.CONV_K for c in B.CONV_C for r, s in B.CONV_TAPS] + [B.CONV_256, B.CONV_258]
    for k, c, r, s in cases:
        w = conv_weights(k, c, r, s, dtype)
        same(run_conv_weights(lib, w, transposed, dtype), B.to_bits(B.conv_weights_ref(w, transposed), dtype), dtype,
             f'conv weights K={k} C={c} {r}x{s} transposed {transposed} dtype {dtype}')


def k4s2_weights(a_, b_, dtype):
    return B.distinct_values(a_ * b_ * 16, dtype, 'k4s2', a_, b_).reshape(a_, b_, 4, 4)


def run_k4s2_weights(lib, w, direction, dtype):
    a_, b_ = w.shape[:2]
    slots = lib.srgan_h_k4s2_weight_slots(a_, b_, direction, dtype)
    assert slots == B.k4s2_slots(a_, b_, direction, dtype)
    out, source = slots_window(slots, dtype), dev(w)
    check(lib.srgan_h_pack_k4s2_weights(source.data_ptr(), out.ptr, a_, b_, direction, dtype, stream()), 'srgan_h_pack_k4s2_weights')
    return stored(out, dtype, f'k4s2 weights {tuple(w.shape)} direction {direction}', (slots, B.GROUP[dtype]))


@pytest.mark.parametrize('direction', [0, 1])
@pytest.mark.parametrize('dtype', B.DTYPES)
def test_k4s2_weight_shadows(lib, dtype, direction):
    """Direction 0 and the four parity classes of direction 1, group counts that are no multiple of the chunk."""
    for a_, b_ in B.K4_SHAPES:
        w = k4s2_weights(a_, b_, dtype)
        same(run_k4s2_weights(lib, w, direction, dtype), B.to_bits(B.k4s2_weights_ref(w, direction, dtype), dtype), dtype,
             f'k4s2 weights A={a_} B={b_} direction {direction} dtype {dtype}')


def matrix_source(case, dtype):
    return B.distinct_values(B.matrix_source_size(*case), dtype, 'matrix', *case)


def run_matrix(lib, src, case, dtype):
    rows, cols = case[:2]
    slots = rows * -(-cols // 8)
    out, source = slots_window(slots, dtype), dev(src)
    check(lib.srgan_h_pack_matrix(source.data_ptr(), out.ptr, *case, dtype, stream()), 'srgan_h_pack_matrix')
    return stored(out, dtype, f'matrix {case}', (slots, 8))


def tile_cases():
    cases = [(rows, cols, rows, cols, 1, rows + 3, 1, 1) for rows in B.TILE_ROWS for cols in B.TILE_COLS]
    cases += [(130, 200, 97, 181, 1, 131, 1, 1), (65, 72, 64, 65, 1, 64, 1, 1)]                  # rows_real < rows, cols_real < cols
    return cases


@pytest.mark.parametrize('dtype', B.HALVES)
def test_matrix_shadows_through_both_bodies(lib, dtype):
    """The one-thread-per-slot body (ragged rows and columns, rows_real / cols_real inside), the transposing tile body
    (row_stride 1), and the arguments the linear and linear_t shadows pass, plane maps included."""
    recorded = [tuple(call[:8]) for call in B.recorded_matrix_calls()]
    assert {B.matrix_body(case[4], case[5]) for case in recorded} == {'slot', 'tile'}
    for case in B.MATRIX_SLOT + tile_cases() + recorded:
        src = matrix_source(case, dtype)
        same(run_matrix(lib, src, case, dtype), B.to_bits(B.matrix_ref(src, *case), dtype), dtype,
             f'matrix {case} ({B.matrix_body(case[4], case[5])} body) dtype {dtype}')


class Jobs:
    """A host array of srgan_h_pack_batched jobs and the outputs they write."""

    def __init__(self, lib, capacity=16):
        self.lib, self.bytes = lib, lib.srgan_h_pack_job_bytes()
        self.host = ctypes.create_string_buffer(capacity * self.bytes)
        self.count, self.blocks, self.keep, self.outputs = 0, 0, [], []

    def at(self):
        return ctypes.addressof(self.host) + self.count * self.bytes

    def added(self, blocks, jobs, out, check_result):
        assert blocks > 0, blocks
        self.count, self.blocks = self.count + jobs, self.blocks + blocks
        self.outputs.append((out, check_result, blocks))

    def conv(self, w, transposed, dtype):
        k, c, r, s = w.shape
        rows, reduced = (c, k) if transposed else (k, c)
        slots = B.conv_weight_slots(rows, reduced, r, s)
        out, source = slots_window(slots, dtype), dev(w)
        self.keep.append(source)
        blocks = self.lib.srgan_h_pack_job_conv_weights(self.at(), self.blocks, source.data_ptr(), out.ptr, k, c, r, s, transposed, dtype)
        want = B.to_bits(B.conv_weights_ref(w, transposed), dtype)
        single = run_conv_weights(self.lib, w, transposed, dtype)
        self.added(blocks, 1, out, lambda: (same(stored(out, dtype, 'conv job', (slots, 8)), want, dtype, 'conv job'),
                                             same(stored(out, dtype, 'conv job', (slots, 8)), single, dtype, 'conv job against the single call')))

    def k4s2(self, w, direction, dtype):
        a_, b_ = w.shape[:2]
        slots, g = B.k4s2_slots(a_, b_, direction, dtype), B.GROUP[dtype]
        out, source, written = slots_window(slots, dtype), dev(w), ctypes.c_int32(0)
        self.keep.append(source)
        blocks = self.lib.srgan_h_pack_job_k4s2_weights(self.at(), self.blocks, source.data_ptr(), out.ptr, a_, b_, direction, dtype, ctypes.byref(written))
        assert written.value == (4 if direction else 1)
        want = B.to_bits(B.k4s2_weights_ref(w, direction, dtype), dtype)
        single = run_k4s2_weights(self.lib, w, direction, dtype)
        self.added(blocks, written.value, out, lambda: (same(stored(out, dtype, 'k4s2 job', (slots, g)), want, dtype, 'k4s2 job'),
                                                        same(stored(out, dtype, 'k4s2 job', (slots, g)), single, dtype, 'k4s2 job against the single call')))

    def matrix(self, case, dtype):
        src = matrix_source(case, dtype)
        slots = case[0] * -(-case[1] // 8)
        out, source = slots_window(slots, dtype), dev(src)
        self.keep.append(source)
        blocks = self.lib.srgan_h_pack_job_matrix(self.at(), self.blocks, source.data_ptr(), out.ptr, *case, dtype)
        want = B.to_bits(B.matrix_ref(src, *case), dtype)
        single = run_matrix(self.lib, src, case, dtype)
        self.added(blocks, 1, out, lambda: (same(stored(out, dtype, 'matrix job', (slots, 8)), want, dtype, f'matrix job {case}'),
                                             same(stored(out, dtype, 'matrix job', (slots, 8)), single, dtype, 'matrix job against the single call')))

    def bias_rows(self, channels, plane):
        bias = B.distinct_values(channels, 0, 'bias', channels, plane)
        floats = -(-channels // 8) * plane * 8
        out, source = Guarded(floats), dev(bias)
        self.keep.append(source)
        blocks = self.lib.srgan_h_pack_job_bias_rows(self.at(), self.blocks, source.data_ptr(), out.ptr, channels, plane)
        want = B.bias_rows_ref(bias, plane).view(torch.int32)
        self.added(blocks, 1, out, lambda: same(float_bits(out, 'bias rows', (floats,)), want, 0, f'bias rows of {channels} channels, plane {plane}'))

    def image(self, w, transposed):
        k, c = w.shape[:2]
        rows, reduced = (c, k) if transposed else (k, c)
        floats = self.lib.srgan_conv3x3_image_floats(reduced, rows)
        out, single, source = Guarded(floats), Guarded(floats), dev(w)
        self.keep.append(source)
        blocks = self.lib.srgan_h_pack_job_conv3x3_image(self.at(), self.blocks, source.data_ptr(), out.ptr, k, c, transposed)
        check(self.lib.srgan_h_pack_conv3x3_image(source.data_ptr(), single.ptr, k, c, transposed, stream()), 'srgan_h_pack_conv3x3_image')
        alone = float_bits(single, 'image', (floats,))
        self.added(blocks, 1, out, lambda: same(float_bits(out, 'image job', (floats,)), alone, 0, 'image job against the single call'))

    def launch(self):
        table = torch.frombuffer(self.host, dtype=torch.uint8)[:self.count * self.bytes].clone().cuda()
        check(self.lib.srgan_h_pack_batched(table.data_ptr(), self.count, self.blocks, stream()), 'srgan_h_pack_batched')
        for _, check_result, _ in self.outputs:
            check_result()


def test_bias_rows_as_single_jobs(lib):
    """count = 1: the bisection has nothing to search."""
    for channels in B.BIAS_CHANNELS:
        for plane in B.BIAS_PLANES:
            jobs = Jobs(lib)
            jobs.bias_rows(channels, plane)
            assert jobs.count == 1
            jobs.launch()


@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('dtype', B.HALVES)
def test_batched_jobs_of_every_kind(lib, dtype, reverse):
    """Seven jobs, one of every kind and a second convolution, one-block and many-block jobs in the first and in the last place
    (the bisection hits its first and its last job); every output bit-equal to the reference and to the single call."""
    makers = [lambda j: j.bias_rows(9, 3),                                               # one workgroup
              lambda j: j.k4s2(k4s2_weights(3, 5, dtype), 0, dtype),
              lambda j: j.matrix(B.MATRIX_SLOT[1], dtype),
              lambda j: j.matrix((130, 200, 97, 181, 1, 131, 1, 1), dtype),            # 12 tiles
              lambda j: j.image(conv_weights(5, 3, 3, 3, 0), 1),
              lambda j: j.conv(conv_weights(5, 3, 3, 3, dtype), 1, dtype),
              lambda j: j.conv(conv_weights(72, 40, 3, 3, dtype), 0, dtype)]          # 3888 slots: 16 workgroups
    jobs = Jobs(lib)
    for make in (makers[::-1] if reverse else makers):
        make(jobs)
    assert jobs.count == 7
    first, last = jobs.outputs[0][2], jobs.outputs[-1][2]
    assert (first, last) == ((16, 1) if reverse else (1, 16))
    jobs.launch()


@pytest.mark.parametrize('dtype', B.DTYPES)
def test_batched_k4s2_up_jobs(lib, dtype):
    """The four parity classes of direction 1 as four jobs, behind a convolution job where the type has one."""
    jobs = Jobs(lib)
    if dtype:
        jobs.conv(conv_weights(5, 17, 2, 3, dtype), 0, dtype)
    jobs.k4s2(k4s2_weights(17, 33, dtype), 1, dtype)
    jobs.k4s2(k4s2_weights(3, 5, dtype), 0, dtype)
    jobs.launch()


# ----------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_outputs_untouched(lib):
    big = 1 << 31
    for dtype in B.DTYPES:
        out, source = slots_window(64, dtype), torch.zeros(1024, device='cuda')
        s, x, o = stream(), source.data_ptr(), out.ptr
        calls = {
            'pack C=0': lambda: lib.srgan_h_pack(x, o, None, 1.0, 1, 0, 4, dtype, s),
            'pack HW=0': lambda: lib.srgan_h_pack(x, o, None, 1.0, 1, 4, 0, dtype, s),
            'pack HW=2^31': lambda: lib.srgan_h_pack(x, o, None, 1.0, 1, 4, big, dtype, s),
            'pack N<0': lambda: lib.srgan_h_pack(x, o, None, 1.0, -1, 4, 4, dtype, s),
            'pack x=NULL': lambda: lib.srgan_h_pack(None, o, None, 1.0, 1, 4, 4, dtype, s),
            'pack out=NULL': lambda: lib.srgan_h_pack(x, None, None, 1.0, 1, 4, 4, dtype, s),
            'unpack C=0': lambda: lib.srgan_h_unpack(x, o, 1, 0, 4, dtype, s),
            'unpack HW=0': lambda: lib.srgan_h_unpack(x, o, 1, 4, 0, dtype, s),
            'unpack HW=2^31': lambda: lib.srgan_h_unpack(x, o, 1, 4, big, dtype, s),
            'unpack N<0': lambda: lib.srgan_h_unpack(x, o, -1, 4, 4, dtype, s),
            'unpack x=NULL': lambda: lib.srgan_h_unpack(None, o, 1, 4, 4, dtype, s),
            'unpack out=NULL': lambda: lib.srgan_h_unpack(x, None, 1, 4, 4, dtype, s),
            'add slots<0': lambda: lib.srgan_h_add(x, x, o, -1, dtype, s),
            'add a=NULL': lambda: lib.srgan_h_add(None, x, o, 4, dtype, s),
            'add b=NULL': lambda: lib.srgan_h_add(x, None, o, 4, dtype, s),
            'add out=NULL': lambda: lib.srgan_h_add(x, x, None, 4, dtype, s),
            'sums C=0': lambda: lib.srgan_h_channel_sums(x, o, 1, 0, 4, dtype, s),
            'sums HW=0': lambda: lib.srgan_h_channel_sums(x, o, 1, 4, 0, dtype, s),
            'sums HW=2^31': lambda: lib.srgan_h_channel_sums(x, o, 1, 4, big, dtype, s),
            'sums N=0': lambda: lib.srgan_h_channel_sums(x, o, 0, 4, 4, dtype, s),
            'sums N<0': lambda: lib.srgan_h_channel_sums(x, o, -1, 4, 4, dtype, s),
            'sums x=NULL': lambda: lib.srgan_h_channel_sums(None, o, 1, 4, 4, dtype, s),
            'sums out=NULL': lambda: lib.srgan_h_channel_sums(x, None, 1, 4, 4, dtype, s),
        }
        if dtype:
            for h, w in ((3, 4), (4, 3), (0, 4), (4, 0), (1, 2), (2, 1), (-2, 4)):
                calls[f'pool {h}x{w}'] = lambda h=h, w=w: lib.srgan_h_maxpool2(x, None, o, 1, h, w, 0, dtype, s)
                calls[f'pool backward {h}x{w}'] = lambda h=h, w=w: lib.srgan_h_maxpool2_bwd(x, x, o, 1, h, w, 0, 0.0, dtype, s)
            calls.update({
                'pool mode 1': lambda: lib.srgan_h_maxpool2(x, x, o, 1, 4, 4, 1, dtype, s),
                'pool mode 3': lambda: lib.srgan_h_maxpool2(x, x, o, 1, 4, 4, 3, dtype, s),
                'pool mode 2 without g': lambda: lib.srgan_h_maxpool2(x, None, o, 1, 4, 4, 2, dtype, s),
                'pool planes<0': lambda: lib.srgan_h_maxpool2(x, None, o, -1, 4, 4, 0, dtype, s),
                'pool x=NULL': lambda: lib.srgan_h_maxpool2(None, None, o, 1, 4, 4, 0, dtype, s),
                'pool out=NULL': lambda: lib.srgan_h_maxpool2(x, None, None, 1, 4, 4, 0, dtype, s),
                'pool backward planes<0': lambda: lib.srgan_h_maxpool2_bwd(x, x, o, -1, 4, 4, 0, 0.0, dtype, s),
                'pool backward x=NULL': lambda: lib.srgan_h_maxpool2_bwd(None, x, o, 1, 4, 4, 0, 0.0, dtype, s),
                'pool backward gp=NULL': lambda: lib.srgan_h_maxpool2_bwd(x, None, o, 1, 4, 4, 0, 0.0, dtype, s),
                'pool backward gx=NULL': lambda: lib.srgan_h_maxpool2_bwd(x, x, None, 1, 4, 4, 0, 0.0, dtype, s),
            })
        for name, call in calls.items():
            assert call() == EINVAL, f'{name}, dtype {dtype}'
        untouched(out, dtype, f'argument errors, dtype {dtype}')
