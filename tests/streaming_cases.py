"""The cases of the streaming-kernel tests (elementwise.hip, reduce.hip, all of pool.hip), shared by
test_streaming_cases_cpu.py (no library needed) and test_streaming_ops_gpu.py (the C ABI, bit for bit): the case tables, a
float64 reference of every operation written from the formulas of include/srgan_hip.h, the branch each table entry exists to
reach -- re-derived here from the hosts' constants, so that a changed constant fails the CPU test instead of un-covering a
kernel -- and the precondition of exactness.

Exact operands: tensors and cotangents are integers in [-X, X]; per-channel mean / beta are quarters, inv_std / gamma / scale
are in {0.5, 1, 2}, alpha in {0, 0.25, 0.5, 1}.  Every partial sum of absolute values stays below 2^(24 - f), f = the
fractional bits of the terms (assert_exact_limit), so every fp32 sum is exact in any order, fma(x, a, b) is exact (the
recomputed ReLU mask has no borderline element), and a correct kernel equals float64 bit for bit.

The fused pools (srgan_bn_relu_maxpool_*, srgan_bn_relu_avgpool2_*) take the same operands with gamma of EITHER SIGN
(fused_pool_vectors: at least one negative channel per case -- a = inv_std * gamma < 0 flips the order of the activated window
-- and one channel whose norm is exactly 0 at x = mean, so `> 0` against `>= 0` shows).  a is then a multiple of 1/4, b = beta -
mean * a and fma(x, a, b) multiples of 1/16 below 32; the pooled gradient per pixel S is an integer (max form) or a multiple of
1/4 (average form: the 0.25 adds two fractional bits), S * a, S * (x - mean) and the sum times inv_std follow with the bits
FUSED_POOL_FRACTION_BITS lists.
"""
import functools
import math

import numpy as np
import torch

# ---- the hosts' constants (elementwise.hip, reduce.hip, common.h) ---------------------------------------------------------
THREADS = 256
STREAM_BLOCKS = 2048            # stream_grid's cap
AFF_SEG = 4096                  # chan_affine_rows_kernel / gp_interpolate_kernel: elements of a row per workgroup
RED_SEG = 4096                  # row_run_sum / crowd_map_l1_kernel: smallest run of a row per workgroup
ROWS_MIN_HW = 256               # chan_affine_launch: rows kernel from this plane size on, flat kernel below
BLOCK_MIN_C, BLOCK_MAX_NHW = 256, 8192      # srgan_chan_reduce: one workgroup per channel
REDUCE_MIN_WGS, REDUCE_SEG_CAP = 256, 65536
TANGENT_ROWS = 16
POOL_BWD_QUADS = 1024           # pool.hip: thread items (float4s of x; pairs of them in the average form) of one plane per workgroup
ROW_FINISH_ROWS = 4096          # split_finish.h: channels per launch that can use the ordered finish; above: fp32 atomics
POOL_MAX_PLANES = 65535         # the fused backwards and the fused average forward put N * C into the grid's y

X, PREFILL = 3, 64
EXACT_LIMIT = 2 ** 24
QUARTERS = [v / 4 for v in range(-8, 9)]
SCALES = [0.5, 1.0, 2.0]
ALPHAS = [0.0, 0.25, 0.5, 1.0]

UNARY = ['copy', 'neg', 'abs', 'sign', 'sqrt', 'exp', 'log', 'log1p', 'square', 'reciprocal', 'tanh', 'relu', 'step', 'affine',
         'pow', 'leaky', 'sigmoid', 'softplus', 'one_minus_square', 'rsqrt']
BINARY = ['add', 'sub', 'mul', 'div', 'div_safe', 'max', 'leaky_mask_mul', 'axpy']
U = {name: code for code, name in enumerate(UNARY)}
B = {name: code for code, name in enumerate(BINARY)}
# one correctly rounded operation, or exact on the integer inputs: bit-identical to float64 rounded to fp32
UNARY_EXACT = ['copy', 'neg', 'abs', 'sign', 'square', 'relu', 'step', 'leaky']
BINARY_EXACT = ['add', 'sub', 'mul', 'max', 'leaky_mask_mul', 'div_safe']
UNARY_FMA = ['affine', 'one_minus_square']          # the compiler may contract these (and axpy) into one fma
UNARY_IEEE = ['sqrt', 'reciprocal', 'rsqrt']        # hardware paths that are IEEE-exact unless the build relaxes them
TRANSCENDENTAL = ['exp', 'log', 'log1p', 'tanh', 'pow', 'sigmoid', 'softplus']
EXTRA_ROUNDINGS = {'sigmoid': 2, 'softplus': 2}     # further roundings of the op's formula in elementwise.hip
NAN_RULE_UNARY = ['relu', 'step', 'sign', 'leaky']  # `x > 0` / fmaxf: a NaN is "not positive" (include/srgan_hip.h)
NAN_RULE_BINARY = ['max', 'leaky_mask_mul']
LEAKY_SLOPE = 0.25
AFFINE_P = (2.5, -1.0)
AXPY_P = 0.75

EW_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4 * STREAM_BLOCKS * THREADS + 5]
SMALL_LENGTHS = list(range(1, 10)) + [1025]          # the fill cases and the unaligned windows
OFFSETS = [0, 1, 2, 3]                               # floats past a 16-byte boundary

AFFINE_HW = [1, 255, 256, 257, 4095, 4096, 4097]     # N = 2, C = 3
AFFINE_N, AFFINE_C = 2, 3
AFFINE_SUBSETS = {'all': ('x', 'mean', 'scale_a', 'scale_b', 'shift'), 'none': (), 'mean+scale_a': ('x', 'mean', 'scale_a'),
                  'shift': ('x', 'shift')}

REDUCE_COLS = [(1, 1), (9, 33), (8, 32), (17, 65)]                              # (N, C), HW = 1
REDUCE_BLOCK = [(2, 256, 9), (3, 257, 300)]
REDUCE_ROWS = [(2, 3, 4097), (1, 2, 8199), (3, 5, 4096), (2, 3, 1000)]
REDUCE_UNALIGNED = [(1, 2, hw) for hw in SMALL_LENGTHS]        # rows path (hw > 1), windows 0..3 floats off alignment

BN_BWD = [(5, 512, 4), (5, 512, 9), (3, 5, 42), (2, 4, 1600), (1, 7, 1)]
TANGENT = [(1, 1, 1), (17, 7, 9), (16, 8, 9), (5, 70, 1), (33, 15, 9)]          # (CO, CI, taps)

GP_B, GP_F = 3, [1, 255, 4096, 4097, 8193]
L1_B, L1_CM, L1_HW = 3, [1, 2, 4], [1, 255, 4096, 4097, 8193]
ROW_MAX = [(b, f) for b in (1, 256, 257) for f in (1, 2, 10)]
BIN_K = [1, 2, 10]
# (planes, H, W, k, s, p): test_pooling_and_layout's geometries
MAXPOOL = [(10, 13, 11, 3, 2, 1), (10, 13, 11, 2, 2, 0)] + \
    [(12, h, w, k, s, p) for (k, s, p, h, w) in [(2, 2, 0, 12, 10), (3, 1, 1, 9, 7), (3, 2, 1, 16, 16), (3, 3, 0, 10, 11), (2, 1, 0, 5, 6),
                                                  (2, 2, 0, 12, 8), (3, 2, 1, 15, 20), (3, 2, 1, 8, 4)]]
AVGPOOL = [(6, 8, 8, 2), (3, 8, 6, 2), (2, 8, 8, 4), (3, 12, 10, 4), (4, 9, 12, 3), (5, 9, 6, 3)]   # (planes, H, W, k), s = k
AVGPOOL_STRIDED = [(6, 12, 12, 3, 1), (6, 10, 10, 3, 2), (4, 5, 6, 2, 1), (3, 9, 12, 3, 2)]         # (planes, H, W, k, s), s != k
# the fused pools, (N, C, H, W[, k, s, p]); C divides nothing, so c = plane % C is tested
FUSED_MAX_FWD = [(2, 3, 13, 11, 3, 2, 1), (2, 3, 13, 11, 2, 2, 0), (1, 5, 9, 7, 3, 1, 1), (2, 3, 10, 11, 3, 3, 0)]
FUSED_MAX_BWD = [(1, 1, 1, 4), (2, 3, 8, 4), (3, 5, 15, 20), (2, 3, 32, 128), (2, 3, 41, 100), (3, 2, 80, 64), (1, 4096, 2, 4),
                 (1, 4097, 2, 4), (1, 65535, 1, 4)]                                              # 3 / 2 / 1 windows
FUSED_AVG = [(1, 1, 2, 4), (2, 3, 6, 8), (3, 5, 10, 12), (2, 3, 64, 128), (2, 3, 50, 164), (3, 2, 80, 128), (1, 4096, 2, 4),
             (1, 4097, 2, 4)]
# back-to-back launches on one stream, parts (= N x workgroups per plane) 2, 6, 1, 2 with another C each time
FUSED_MAX_SEQUENCE = [(2, 3, 8, 4), (3, 2, 41, 100), (1, 5, 15, 20), (1, 4, 80, 64)]
FUSED_AVG_SEQUENCE = [(2, 3, 6, 8), (3, 2, 50, 164), (1, 5, 10, 12), (1, 4, 80, 128)]
FUSED_REPEAT = dict(max=[(2, 3, 41, 100), (3, 2, 80, 64)], avg=[(2, 3, 50, 164), (3, 2, 80, 128)])     # several workgroups per plane
COPY_CHANNELS = [dict(N=3, HW=35, src=(7, 2), dst=(5, 1), count=3, accumulate=0),      # (channels, first channel)
                 dict(N=2, HW=1025, src=(4, 1), dst=(6, 3), count=2, accumulate=1)]
ADAM_N = [1, 3, 255, 257, STREAM_BLOCKS * THREADS + 1]
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_DECAY = [0.0, 0.1]
ADAM_STEPS = 3


# ---- the branch every entry is there for --------------------------------------------------------------------------------
def stream_grid(items, per_block=THREADS):
    return max(1, min(STREAM_BLOCKS, -(-items // per_block)))


def ew_trips(n):
    """(grid-stride trips of the float4 body, tail elements) of unary_kernel / binary_kernel at length n."""
    quads = n // 4
    return -(-quads // (stream_grid(-(-n // 4)) * THREADS)), n % 4


def stream_trips(n):
    """Grid-stride trips of a one-element-per-thread kernel (fill, Adam) at length n."""
    return -(-n // (stream_grid(n) * THREADS))


def affine_path(hw):
    return ('rows', -(-hw // AFF_SEG)) if hw >= ROWS_MIN_HW else ('flat', 1)


def reduce_path(n, c, hw):
    """('cols' | 'block' | 'rows', run length, runs per row) as srgan_chan_reduce chooses."""
    if hw == 1:
        return 'cols', 1, 1
    if c >= BLOCK_MIN_C and n * hw <= BLOCK_MAX_NHW:
        return 'block', hw, 1
    seg = RED_SEG
    while seg < REDUCE_SEG_CAP and n * c * (-(-hw // (2 * seg))) >= REDUCE_MIN_WGS:
        seg *= 2
    return 'rows', seg, -(-hw // seg)


def rows_run_shape(hw, seg, part, base):
    """Of run `part` of a row starting at element `base`: (aligned start, trips of the four-in-flight loop, quads left to the
    single loop, scalar tail) as row_run_sum walks it."""
    beg, end = part * seg, min(hw, (part + 1) * seg)
    aligned = (base | beg) & 3 == 0
    quads = (end - beg) // 4
    four = len(range(0, max(0, quads - 768), 1024)) if aligned else 0          # thread 0's trips: i + 768 < n4
    return aligned, four, quads, (end - beg) - 4 * quads if aligned else end - beg


def bn_bwd_images_per_block(n, c, hw):
    per = 1
    while per < n and (c * (-(-n // per)) > 2048 or per * hw < 4096) and c * (-(-n // (2 * per))) >= 1024:
        per *= 2
    return per


def tangent_span(taps):
    return 64 - 64 % taps


def fused_pool_grid(form, n, c, h, w):
    """(workgroups per plane, thread items in the last one, 'ordered' | 'atomic' parameter sums in the default mode) of the
    fused backwards and the fused average forward; form 'max': one item = a float4 of x, 'avg': two rows' float4s."""
    items = h * (w // 4) if form == 'max' else (h // 2) * (w // 4)
    groups = -(-items // POOL_BWD_QUADS)
    return groups, items - (groups - 1) * POOL_BWD_QUADS, 'ordered' if c <= ROW_FINISH_ROWS else 'atomic'


def fused_pool_parts(form, n, c, h, w):
    """The partial sums per channel that meet in ordered_row_finish: images x workgroups per plane."""
    return n * fused_pool_grid(form, n, c, h, w)[0]


def fused_max_bwd_supported(n, c, h, w, k, s, p):
    return (k, s, p) == (3, 2, 1) and w % 4 == 0 and n * c <= POOL_MAX_PLANES and n * c * h * w < 2 ** 31


def fused_avg_supported(n, c, h, w):
    return (n > 0 and c > 0 and h >= 2 and w >= 4 and h % 2 == 0 and w % 4 == 0 and n * c <= POOL_MAX_PLANES
            and n * c * h * w < 2 ** 31)


def maxpool_bwd_path(w, k, s, p, offset=0):
    """The kernel srgan_maxpool2d_bwd takes for rows of w floats with gx `offset` floats past a 16-byte boundary."""
    if w % 4 == 0 and offset % 4 == 0 and (k, s, p) in ((3, 2, 1), (2, 2, 0)):
        return 'quad321' if k == 3 else 'quad220'
    return 'scalar'


def pool_out(size, k, s, p=0):
    return (size + 2 * p - k) // s + 1


# ---- operands -------------------------------------------------------------------------------------------------------------
def generator(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(shape, bound, gen):
    return torch.randint(-bound, bound + 1, tuple(shape), generator=gen).double()


def pick(values, shape, gen):
    values = torch.tensor(values, dtype=torch.float64)
    return values[torch.randint(0, len(values), tuple(shape), generator=gen)]


def distinct(shape, gen):
    """Distinct integers (an accumulate-mode output's old contents), shuffled."""
    count = int(np.prod(shape))
    return (torch.randperm(count, generator=gen).double() - count // 2).reshape(tuple(shape))


def assert_exact_limit(magnitude, fraction_bits, what):
    limit = EXACT_LIMIT >> fraction_bits
    assert magnitude < limit, f'{what}: a partial sum reaches {magnitude:g} >= 2^{24 - fraction_bits}: the case is broken'


def full_mantissa(n, gen):
    """Random fp32 values with full mantissas, both signs, magnitudes 2^-8 .. 2^8 (as float64)."""
    return (torch.randn(n, generator=gen).float() * torch.exp2(torch.randint(-8, 9, (n,), generator=gen).float())).double()


def channel_vectors(c, gen):
    return dict(mean=pick(QUARTERS, (c,), gen), inv_std=pick(SCALES, (c,), gen), gamma=pick(SCALES, (c,), gen),
                beta=pick(QUARTERS, (c,), gen))


def fused_pool_vectors(c, gen):
    """channel_vectors with gamma of either sign -- at least one channel negative -- and one channel whose norm is exactly zero
    at x = mean (mean = +-1, beta = 0): the recomputed mask meets its borderline, exactly."""
    v = channel_vectors(c, gen)
    sign = pick([-1.0, 1.0], (c,), gen)
    sign[int(torch.randint(0, c, (1,), generator=gen))] = -1.0
    v['gamma'] = v['gamma'] * sign
    zero = int(torch.randint(0, c, (1,), generator=gen))
    v['mean'][zero] = float(pick([-1.0, 1.0], (1,), gen))
    v['beta'][zero] = 0.0
    return v


# ---- float64 references ---------------------------------------------------------------------------------------------------
def unary_ref(name, x, p0=0.0, p1=0.0):
    """The op in float64 (NaN rule of include/srgan_hip.h: `x > 0` is false for a NaN)."""
    x = x.double()
    zero, one = torch.zeros_like(x), torch.ones_like(x)
    table = {
        'copy': lambda: x.clone(), 'neg': lambda: -x, 'abs': lambda: x.abs(),
        'sign': lambda: torch.where(x > 0, one, torch.where(x < 0, -one, zero)),
        'sqrt': lambda: x.sqrt(), 'exp': lambda: x.exp(), 'log': lambda: x.log(), 'log1p': lambda: x.log1p(),
        'square': lambda: x * x, 'reciprocal': lambda: 1.0 / x, 'tanh': lambda: x.tanh(),
        'relu': lambda: torch.where(x > 0, x, zero), 'step': lambda: torch.where(x > 0, one, zero),
        'affine': lambda: p0 * x + p1, 'pow': lambda: x.pow(p0), 'leaky': lambda: torch.where(x > 0, x, p0 * x),
        'sigmoid': lambda: 1.0 / (1.0 + (-x).exp()),
        'softplus': lambda: torch.where(x > 0, x, zero) + (-x.abs()).exp().log1p() + torch.where(x != x, x, zero),
        'one_minus_square': lambda: 1.0 - x * x, 'rsqrt': lambda: 1.0 / x.sqrt()}
    return table[name]()


def binary_ref(name, a, b, p0=0.0):
    a, b = a.double(), b.double()
    table = {'add': lambda: a + b, 'sub': lambda: a - b, 'mul': lambda: a * b, 'div': lambda: a / b,
             'div_safe': lambda: torch.where(b == 0, torch.zeros_like(a), a / b),
             'max': lambda: torch.from_numpy(np.fmax(a.numpy(), b.numpy())),       # fmaxf: a NaN operand is dropped
             'leaky_mask_mul': lambda: torch.where(b > 0, a, p0 * a), 'axpy': lambda: a + p0 * b}
    return table[name]()


def torch_unary(name, x, p0=0.0, p1=0.0):
    """torch's own fp32 op (CPU)."""
    import torch.nn.functional as TF
    x = x.float()
    table = {'copy': lambda: x.clone(), 'neg': lambda: -x, 'abs': x.abs, 'sign': x.sign, 'sqrt': x.sqrt, 'exp': x.exp, 'log': x.log,
             'log1p': x.log1p, 'square': x.square, 'reciprocal': x.reciprocal, 'tanh': x.tanh, 'relu': x.relu,
             'step': lambda: (x > 0).float(), 'affine': lambda: p0 * x + p1, 'pow': lambda: x.pow(p0),
             'leaky': lambda: TF.leaky_relu(x, p0), 'sigmoid': x.sigmoid, 'softplus': lambda: TF.softplus(x),
             'one_minus_square': lambda: 1 - x * x, 'rsqrt': x.rsqrt}
    return table[name]()


def torch_binary(name, a, b, p0=0.0):
    a, b = a.float(), b.float()
    table = {'add': lambda: a + b, 'sub': lambda: a - b, 'mul': lambda: a * b, 'div': lambda: a / b,
             'div_safe': lambda: torch.where(b == 0, torch.zeros_like(a), a / b), 'max': lambda: torch.fmax(a, b),
             'leaky_mask_mul': lambda: torch.where(b > 0, a, p0 * a), 'axpy': lambda: a + p0 * b}
    return table[name]()


def round32(t):
    """float64 -> the nearest fp32, as float64."""
    return t.double().float().double()


def two_roundings(name, x, b=None, p0=0.0, p1=0.0):
    """affine / one_minus_square / axpy with the product rounded to fp32 before the add (no fma), as float64."""
    x = x.double()
    if name == 'affine':
        return round32(round32(p0 * x) + p1)
    if name == 'one_minus_square':
        return round32(1.0 - round32(x * x))
    return round32(x + round32(p0 * b.double()))            # axpy: a + p0 * b


def ulp32(value):
    """The fp32 unit in the last place at the magnitude of a float64 tensor (2^-149 below the smallest normal)."""
    _, exponent = np.frexp(np.abs(value.double().numpy()))
    return torch.from_numpy(np.ldexp(1.0, np.maximum(exponent - 1, -126) - 23))


SMALLEST_NORMAL = 2.0 ** -126


def ulp_error(got, want, scale=None):
    """Per element: |got - want| in fp32 ulps of the float64 `want` (of `scale` where given: the magnitude of the operands of a
    sum that may cancel); results below the smallest normal are measured against 2^-126 instead (1.0 = at the absolute bound);
    an inf / NaN `want` needs the same inf / a NaN (error 0, else inf)."""
    got, want = got.double().cpu(), want.double()
    want = torch.where(want.abs() >= 2.0 ** 128 - 2.0 ** 103, want.sign() * math.inf, want)       # rounds to an fp32 infinity
    finite = torch.isfinite(want)
    error = torch.where(finite, (got - want).abs() / ulp32(want if scale is None else scale), torch.zeros_like(want))
    tiny = finite & (want.abs() < SMALLEST_NORMAL)
    error = torch.where(tiny, (got - want).abs() / SMALLEST_NORMAL, error)
    special_ok = torch.where(torch.isnan(want), torch.isnan(got), got == want)
    error = torch.where(~finite & ~special_ok, torch.full_like(want, math.inf), error)
    return torch.where(torch.isnan(error), torch.full_like(want, math.inf), error)


def sweep(positive_only=False):
    """Log-spaced magnitudes 2^-30 .. 2^6 (8 per octave, off the powers of two as well as on them), both signs."""
    magnitudes = torch.exp2(torch.arange(-30 * 8, 6 * 8 + 1, dtype=torch.float64) / 8).float().double()
    return magnitudes if positive_only else torch.cat([magnitudes, -magnitudes])


POW_EXPONENTS = [0.5, 1.5, 2.0, 3.0]


def transcendental_inputs(name):
    """The sweep plus the points where the op's formula changes regime (fp32-representable, as float64)."""
    extra = {'exp': [87.0, -87.0, 89.0, -89.0, -104.0], 'tanh': [9.0, -9.0, 20.0, -20.0],
             'sigmoid': [17.0, -17.0, 88.0, -88.0, 104.0, -104.0], 'softplus': [17.0, -17.0, 88.0, -88.0, 104.0, -104.0],
             'log1p': [2.0 ** -24, -2.0 ** -24], 'log': [1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23, 1.0], 'pow': []}[name]
    base = sweep(positive_only=name in ('log', 'pow'))
    return torch.cat([base, torch.tensor(extra, dtype=torch.float64)]).float().double()


@functools.lru_cache(maxsize=None)
def transcendental_bound(name, p0=0.0):
    """(worst error of torch's CPU fp32 evaluation on transcendental_inputs against float64, in ulps; the bound for the
    kernel: max(2, 4 x that) + the further roundings of the op's formula)."""
    x = transcendental_inputs(name)
    measured = float(ulp_error(torch_unary(name, x, p0), unary_ref(name, x, p0)).max())
    return measured, max(2.0, 4.0 * measured) + EXTRA_ROUNDINGS.get(name, 0)


SPECIALS = [0.0, -0.0, math.inf, -math.inf, math.nan, 1.0, -1.0, 2.5]


def chan_affine_ref(x, vectors, mask, relu, shape):
    """((x ? x : 1) - mean) * scale_a * scale_b + shift as the kernel forms it: a = scale_a * scale_b, b = shift - mean * a,
    fma(x, a, b); then max(., 0) and 0 where mask <= 0."""
    n, c, hw = shape
    one = torch.ones(c, dtype=torch.float64)
    a = vectors.get('scale_a', one) * vectors.get('scale_b', one)
    b = vectors.get('shift', 0 * one) - vectors.get('mean', 0 * one) * a
    value = (x if x is not None else torch.ones(n, c, hw, dtype=torch.float64)) * a.view(1, c, 1) + b.view(1, c, 1)
    if relu:
        value = value.clamp_min(0.0)
    if mask is not None:
        value = torch.where(mask > 0, value, torch.zeros_like(value))
    return value


def chan_reduce_ref(a, b, mean, scale):
    """out[c] = scale[c] * sum_{n, i} a * ((b ? b : 1) - mean[c]) over [N, C, HW]."""
    c = a.shape[1]
    other = b if b is not None else torch.ones_like(a)
    if mean is not None:
        other = other - mean.view(1, c, 1)
    total = (a * other).sum(dim=(0, 2))
    return total * scale if scale is not None else total


def chan_reduce_magnitude(a, b, mean, scale):
    other = (b.abs() if b is not None else torch.ones_like(a)) + (mean.abs().view(1, -1, 1) if mean is not None else 0)
    total = (a.abs() * other).sum(dim=(0, 2))
    return float((total * scale if scale is not None else total).max())


def bn_act_bwd_ref(g, x, v, relu, unscaled):
    """(gx, g_gamma, g_beta) of the frozen norm (+ReLU): mask = fma(x, a, b) > 0 with a = inv_std * gamma, b = beta - mean * a."""
    c = x.shape[1]
    a = v['inv_std'] * v['gamma']
    b = v['beta'] - v['mean'] * a
    y = x * a.view(1, c, 1) + b.view(1, c, 1)
    masked = torch.where(y > 0, g, torch.zeros_like(g)) if relu else g
    gx = masked if unscaled else masked * a.view(1, c, 1)
    g_gamma = v['inv_std'] * (masked * (x - v['mean'].view(1, c, 1))).sum(dim=(0, 2))
    return gx, g_gamma, masked.sum(dim=(0, 2))


def tangent_ref(w, q, inv_std, gamma):
    """(w_scaled, w_grad increment, gamma_grad increment) for w, q [CO][CI][taps]."""
    a = (inv_std * gamma).view(1, -1, 1)
    return w * a, q * a, inv_std * (w * q).sum(dim=(0, 2))


def gp_interpolate_ref(u, fake, alpha):
    return alpha.view(-1, 1) * u + (1.0 - alpha.view(-1, 1)) * fake


def crowd_l1_ref(maps, target):
    """rows[b] = sum_hw (1 / Cm) sum_c |maps[b, c, hw] - target[b, hw]|."""
    return ((maps - target.unsqueeze(1)).abs().sum(dim=1) / maps.shape[1]).sum(dim=1)


def crowd_l1_bwd_ref(maps, target, g):
    d = maps - target.unsqueeze(1)
    sign = torch.where(d > 0, 1.0, 0.0) - torch.where(d < 0, 1.0, 0.0)
    return g.view(-1, 1, 1) * sign / maps.shape[1]


def row_max_ref(x):
    """fmaxf over the row: NaNs dropped."""
    return torch.from_numpy(np.fmax.reduce(x.double().numpy(), axis=1))


def nearest_bin_ref(y, bins):
    """One-hot of the FIRST k minimising |y[b] - bins[k]| (distances in fp32, as the kernel's)."""
    d = (y.float().view(-1, 1) - bins.float().view(1, -1)).abs().numpy()
    onehot = np.zeros(d.shape)
    onehot[np.arange(d.shape[0]), d.argmin(axis=1)] = 1.0            # numpy's argmin: the first minimum
    return torch.from_numpy(onehot)


def maxpool_ref(x, k, s, p, oh, ow):
    """(values, flat in-plane arg-max) over [planes, H, W]: the window scanned row-major, a later element replaces the best
    only when greater -- or NaN; padding is skipped (a window of -inf keeps its first element)."""
    x = x.double().numpy()
    planes, h, w = x.shape
    best = np.full((planes, oh, ow), -np.inf)
    best_i = np.full((planes, oh, ow), -1, dtype=np.int64)
    rows, cols = np.arange(oh) * s - p, np.arange(ow) * s - p
    for r in range(k):
        for c in range(k):
            hh, ww = rows + r, cols + c
            valid = ((hh >= 0) & (hh < h))[:, None] & ((ww >= 0) & (ww < w))[None, :]
            value = x[:, np.clip(hh, 0, h - 1)[:, None], np.clip(ww, 0, w - 1)[None, :]]
            flat = (np.clip(hh, 0, h - 1)[:, None] * w + np.clip(ww, 0, w - 1)[None, :])[None]
            with np.errstate(invalid='ignore'):
                take = valid[None] & ((value > best) | (best_i < 0) | np.isnan(value))
            best = np.where(take, value, best)
            best_i = np.where(take, flat, best_i)
    return torch.from_numpy(best), torch.from_numpy(best_i)


def pooling_inputs(planes, h, w, gen):
    """Integer planes (many ties), one plane's corner windows all -inf, one NaN."""
    x = ints((planes, h, w), X, gen)
    x[0, :4, :4] = -math.inf
    x[-1, h // 2, w // 2] = math.nan
    return x


def pool_gather_ref(src, index):
    """out[plane, o] = src[plane, index[plane, o]] (flat planes)."""
    return torch.gather(src.reshape(src.shape[0], -1), 1, index.reshape(index.shape[0], -1))


def pool_scatter_ref(g, index, in_plane):
    out = torch.zeros(g.shape[0], in_plane, dtype=torch.float64)
    return out.index_put_((torch.arange(g.shape[0]).view(-1, 1).expand(-1, index[0].numel()).reshape(-1), index.reshape(-1)),
                          g.reshape(-1).double(), accumulate=True)


def maxpool_bwd_ref(g, index, h, w):
    """gx [planes, H, W]: every g added at its window's arg-max (pool_scatter_ref, reshaped)."""
    return pool_scatter_ref(g.reshape(g.shape[0], -1), index.reshape(index.shape[0], -1), h * w).reshape(g.shape[0], h, w)


def avgpool_ref(x, k, s=None):
    """Windows of k x k at stride s (default k), no padding: the mean of each."""
    planes, h, w = x.shape
    if s is None or s == k:
        oh, ow = h // k, w // k
        return x[:, :oh * k, :ow * k].reshape(planes, oh, k, ow, k).sum(dim=(2, 4)) / (k * k)
    return x.unfold(1, k, s).unfold(2, k, s).sum(dim=(3, 4)) / (k * k)


def avgpool_bwd_ref(g, k, h, w, s=None):
    """gx[h, w] = (1 / k^2) x the sum of g over the windows that contain (h, w)."""
    planes, oh, ow = g.shape
    gx = torch.zeros(planes, h, w, dtype=torch.float64)
    if s is None or s == k:
        gx[:, :oh * k, :ow * k] = (g / (k * k)).repeat_interleave(k, dim=1).repeat_interleave(k, dim=2)
        return gx
    for r in range(k):
        for c in range(k):
            gx[:, r:r + s * oh:s, c:c + s * ow:s] += g
    return gx / (k * k)


def batch_norm_eval_ref(x, v):
    """(x - mean) * inv_std * gamma + beta per channel of [N, C, H, W] (include/srgan_hip.h)."""
    shape = (1, -1, 1, 1)
    return (x - v['mean'].view(shape)) * v['inv_std'].view(shape) * v['gamma'].view(shape) + v['beta'].view(shape)


def bn_relu_maxpool_ref(x, v, k, s, p):
    """maxpool(relu(bn(x))): (values, flat in-plane arg-max) [N, C, OH, OW] -- the first maximum in row-major window order,
    padding skipped (maxpool_ref)."""
    n, c, h, w = x.shape
    oh, ow = pool_out(h, k, s, p), pool_out(w, k, s, p)
    values, index = maxpool_ref(batch_norm_eval_ref(x, v).clamp_min(0.0).reshape(n * c, h, w), k, s, p, oh, ow)
    return values.reshape(n, c, oh, ow), index.reshape(n, c, oh, ow)


def fused_pool_bwd_from(pooled, x, v):
    """From S, the pooled gradient per input pixel: (masked S, gx = S * inv_std * gamma, g_gamma = sum S * (x - mean) * inv_std,
    g_beta = sum S), S masked by [bn(x) > 0]."""
    shape = (1, -1, 1, 1)
    masked = torch.where(batch_norm_eval_ref(x, v) > 0, pooled, torch.zeros_like(pooled))
    gx = masked * v['inv_std'].view(shape) * v['gamma'].view(shape)
    g_gamma = (masked * (x - v['mean'].view(shape)) * v['inv_std'].view(shape)).sum(dim=(0, 2, 3))
    return masked, gx, g_gamma, masked.sum(dim=(0, 2, 3))


def bn_relu_maxpool_bwd_ref(g, index, x, v):
    """(gx, g_gamma, g_beta): g scattered through the arg-max, times [bn(x) > 0]."""
    n, c, h, w = x.shape
    pooled = maxpool_bwd_ref(g.reshape(n * c, *g.shape[2:]), index.reshape(n * c, *index.shape[2:]), h, w).reshape(n, c, h, w)
    return fused_pool_bwd_from(pooled, x, v)[1:]


def bn_relu_avgpool2_ref(x, v):
    n, c, h, w = x.shape
    return avgpool_ref(batch_norm_eval_ref(x, v).clamp_min(0.0).reshape(n * c, h, w), 2).reshape(n, c, h // 2, w // 2)


def bn_relu_avgpool2_bwd_ref(g, x, v):
    """The same with S = 0.25 * g[h / 2, w / 2]."""
    pooled = (0.25 * g).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return fused_pool_bwd_from(pooled, x, v)[1:]


# fractional bits of every exact output of the fused pools (a: 2, b and fma(x, a, b): 4, x - mean: 2, inv_std: 1)
FUSED_POOL_FRACTION_BITS = {'max': dict(y=4, gx=2, g_gamma=3, g_beta=0), 'avg': dict(y=6, gx=4, g_gamma=5, g_beta=2)}


def fused_pool_magnitudes(form, g, index, x, v, old_gamma, old_beta):
    """Per output, the largest sum of ABSOLUTE values any order of adding its terms can reach (the old contents included)."""
    n, c, h, w = x.shape
    shape = (1, -1, 1, 1)
    if form == 'max':
        pooled = maxpool_bwd_ref(g.abs().reshape(n * c, *g.shape[2:]), index.reshape(n * c, *index.shape[2:]), h, w).reshape(n, c, h, w)
    else:
        pooled = (0.25 * g.abs()).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    a = (v['inv_std'] * v['gamma']).abs().view(shape)
    activated = x.abs() * a + (v['beta'].abs() + v['mean'].abs() * a.view(-1)).view(shape)
    centred = pooled * (x.abs() + v['mean'].abs().view(shape)) * v['inv_std'].view(shape)
    return dict(y=float(activated.max()) * (1 if form == 'max' else 4), gx=float((pooled * a).max()),
                g_gamma=float((centred.sum(dim=(0, 2, 3)) + old_gamma.abs()).max()),
                g_beta=float((pooled.sum(dim=(0, 2, 3)) + old_beta.abs()).max()))


@functools.lru_cache(maxsize=None)
def fused_pool_problem(form, case):
    """Operands and float64 results of one fused-pool case, computed once and shared (do not modify): x, g, v, old_gamma,
    old_beta, y, (index), gx, g_gamma, g_beta (the last two WITH the old contents), magnitudes."""
    n, c, h, w = case[:4]
    k, s, p = case[4:] if len(case) > 4 else (3, 2, 1) if form == 'max' else (2, 2, 0)
    gen = generator('fused-pool', form, case)
    v = fused_pool_vectors(c, gen)
    x = ints((n, c, h, w), X, gen)
    g = ints((n, c, pool_out(h, k, s, p), pool_out(w, k, s, p)), X, gen)
    old = distinct((2, c), gen)
    problem = dict(x=x, g=g, v=v, old_gamma=old[0], old_beta=old[1], geometry=(k, s, p))
    if form == 'max':
        problem['y'], problem['index'] = bn_relu_maxpool_ref(x, v, k, s, p)
        gx, g_gamma, g_beta = bn_relu_maxpool_bwd_ref(g, problem['index'], x, v)
    else:
        problem['y'], problem['index'] = bn_relu_avgpool2_ref(x, v), None
        gx, g_gamma, g_beta = bn_relu_avgpool2_bwd_ref(g, x, v)
    problem.update(gx=gx, g_gamma=g_gamma + old[0], g_beta=g_beta + old[1],
                   magnitudes=fused_pool_magnitudes(form, g, problem['index'], x, v, old[0], old[1]))
    return problem


def fused_pool_random_problem(form, case):
    """Full-mantissa operands (randn) for the repeatability test: no result is exact, only its bits from run to run matter
    (the arg-max of the max form is the fused forward's own, taken on the device)."""
    n, c, h, w = case
    gen = generator('fused-pool-random', form, case)
    k, s, p = (3, 2, 1) if form == 'max' else (2, 2, 0)
    v = dict(mean=torch.randn(c, generator=gen) * 0.3, inv_std=(torch.rand(c, generator=gen) + 0.5).rsqrt(),
             gamma=torch.randn(c, generator=gen), beta=torch.randn(c, generator=gen) * 0.3)
    x = torch.randn(n, c, h, w, generator=gen)
    g = torch.randn(n, c, pool_out(h, k, s, p), pool_out(w, k, s, p), generator=gen)
    return dict(x=x.double(), g=g.double(), v={key: value.double() for key, value in v.items()}, geometry=(k, s, p),
                old_gamma=torch.randn(c, generator=gen).double(), old_beta=torch.randn(c, generator=gen).double())


def adam_ref(p, g, m, v, step, weight_decay, dtype=torch.float64, lr=ADAM['lr'], beta1=ADAM['beta1'], beta2=ADAM['beta2'],
             eps=ADAM['eps']):
    """One step in the order of elementwise.hip's adam_kernel (torch.optim.Adam's single-tensor path), in `dtype`, with the
    two corrections computed in double and rounded to fp32 as both entry points do."""
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    f = (lambda value: float(np.float32(value)))
    lr, beta1, beta2, eps, weight_decay = f(lr), f(beta1), f(beta2), f(eps), f(weight_decay)
    bc1 = f(1.0 - beta1 ** step)
    bc2_sqrt = f(math.sqrt(1.0 - beta2 ** step))
    if dtype == torch.float32:
        one_minus_b1, one_minus_b2, step_size = f(np.float32(1) - np.float32(beta1)), f(np.float32(1) - np.float32(beta2)), f(np.float32(lr) / np.float32(bc1))
    else:
        one_minus_b1, one_minus_b2, step_size = 1.0 - beta1, 1.0 - beta2, lr / bc1
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (g - m) * one_minus_b1
    v = v * beta2 + one_minus_b2 * g * g
    p = p - step_size * (m / (v.sqrt() / bc2_sqrt + eps))
    return p, m, v


def adam_problem(n, weight_decay):
    gen = generator('adam', n, weight_decay)
    return dict(p=torch.randn(n, generator=gen).float(), m=torch.zeros(n), v=torch.zeros(n),
                grads=[torch.randn(n, generator=gen).float() * 0.1 for _ in range(ADAM_STEPS)])


@functools.lru_cache(maxsize=None)
def adam_expected(n, weight_decay):
    """Three steps: the float64 update from torch.optim.Adam's fp32 state (`want`, from `start`), torch's own fp32 result, and
    per step and tensor the bound in ulps: max(2, 4 x measured), measured = the worst error against float64, FROM THE SAME
    fp32 STATE, of the update evaluated in fp32 in two orders -- torch's (fused multiply-adds where its vector code has them)
    and the plain one-rounding-per-operation order of the formula: what reordering the update's fp32 operations costs on
    these inputs.  The unit (`scale`): an fp32 ulp at the magnitude of the OPERANDS of the tensor's last sum, not of its
    result -- p - step * m / denom and g + decay * p cancel on some elements, and a sum's rounding error is relative to what
    goes in: ulps of a cancelled result would measure the conditioning of the element, not the arithmetic."""
    problem = adam_problem(n, weight_decay)
    parameter = torch.nn.Parameter(problem['p'].clone())
    as32 = (lambda value: float(np.float32(value)))          # the ABI takes fp32 hyper-parameters: torch gets the same values
    optimizer = torch.optim.Adam([parameter], lr=as32(ADAM['lr']), betas=(as32(ADAM['beta1']), as32(ADAM['beta2'])),
                                 eps=as32(ADAM['eps']), weight_decay=as32(weight_decay), foreach=False)
    steps = []
    p, m, v = problem['p'], problem['m'], problem['v']
    for index, grad in enumerate(problem['grads']):
        want = adam_ref(p, grad, m, v, index + 1, weight_decay)
        parameter.grad = grad.clone()
        optimizer.step()
        state = optimizer.state[parameter]
        torch_now = (parameter.detach().clone(), state['exp_avg'].clone(), state['exp_avg_sq'].clone())
        decay32 = float(np.float32(weight_decay))
        terms = torch.maximum(grad.double().abs(), (decay32 * p.double()).abs())        # the operands of g + decay * p
        scale = (torch.maximum(p.double().abs(), want[0].abs()),
                 torch.maximum(torch.maximum(m.double().abs(), want[1].abs()), terms),
                 torch.maximum(want[2].abs(), (1.0 - float(np.float32(ADAM['beta2']))) * terms * terms))      # (g * g inherits g's error)
        steps.append(dict(start=(p, m, v), want=want, torch=torch_now, scale=scale,
                          plain=adam_ref(p, grad, m, v, index + 1, weight_decay, torch.float32)))
        p, m, v = torch_now                                   # the next step starts from torch's fp32 state
    for entry in steps:
        entry['measured'] = [max(float(ulp_error(t, w, s).max()), float(ulp_error(o, w, s).max()))
                             for t, o, w, s in zip(entry['torch'], entry['plain'], entry['want'], entry['scale'])]
        entry['bound'] = [max(2.0, 4.0 * value) for value in entry['measured']]
    return steps
