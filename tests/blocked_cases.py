"""The cases of the blocked layout and weight-shadow kernel tests (srgan_h_pack / _unpack / _add / _channel_sums,
srgan_h_maxpool2 / _bwd, the weight-shadow packers and srgan_h_pack_batched), shared by test_blocked_cases_cpu.py (no library
needed) and test_blocked_streaming_gpu.py (the C ABI, bit for bit): the case tables, a reference of every operation written from
the formulas of include/srgan_hip.h and the layout comments of blocked16.h, the branch each table entry exists to reach --
re-derived here from the hosts' constants, so that a changed constant fails the CPU test instead of un-covering a branch -- and
the precondition of exactness.

A blocked tensor is carried as its BITS: an int16 (dtype 1 bf16, 2 fp16) or int32 (dtype 0, fp32) tensor [N][CG][HW][G], G = 8
or 4.  The one rounding of a 16-bit store is torch's CPU conversion `.to(torch.bfloat16 / torch.float16)`.
"""
import torch

# ---- the hosts' constants (common.h, split_finish.h, weight_shadows.h, blocked16_streaming.hip, blocked16_shadows.hip) -------
THREADS = 256
STREAM_BLOCKS = 2048            # stream_grid's cap
ROW_FINISH_ROWS = 4096          # split_finish.h: channel groups per launch that can use the ordered finish; above: two launches
SUMS_PER_PART = 4096            # srgan_h_channel_sums: (n, pixel) pairs per workgroup of a group ...
SUMS_MAX_PARTS = 256            # ... at most this many workgroups per group ...
SUMS_MAX_BLOCKS = 4096          # ... halved while parts * CG is above this
K4_CK, K4_TAPS = 4, 4           # weight_shadows.h: k-slots per chunk and taps of the 4x4 / stride 2 operands
TILE = 64                       # h_pack_matrix_tile: rows x columns of one workgroup

GROUP = {0: 4, 1: 8, 2: 8}      # channels per 16-byte slot
TORCH = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
BITS = {0: torch.int32, 1: torch.int16, 2: torch.int16}
DTYPES = [0, 1, 2]
HALVES = [1, 2]
NAN_BITS = {0: 0x7FC00000, 1: 0x7FC0, 2: 0x7FC0}     # 0x7FC0 is a NaN of bf16 AND of fp16
NAN_FILL = {0: 0x7FC00000, 1: 0x7FC07FC0, 2: 0x7FC07FC0}      # the 32-bit word an output window is prefilled with

X = 3                           # exact channel sums: integers in [-X, X]
EXACT_LIMIT = 2 ** 24
SLOPES = [0.0, 0.125, 1.0]


# ---- bits and layout ------------------------------------------------------------------------------------------------------
def to_bits(x, dtype):
    """fp32 values -> the stored bits: ONE round to nearest even (torch's CPU conversion); dtype 0: the float's own bits."""
    return x.float().to(TORCH[dtype]).contiguous().view(BITS[dtype])


def from_bits(bits, dtype):
    """The stored bits -> fp32, exactly."""
    return bits.contiguous().view(TORCH[dtype]).float()


def wrap16(patterns):
    """Patterns 0 .. 65535 as int16 bits."""
    patterns = torch.as_tensor(patterns, dtype=torch.int64)
    return (patterns - 65536 * (patterns >= 32768)).to(torch.int16)


def wrap32(patterns):
    patterns = torch.as_tensor(patterns, dtype=torch.int64)
    return (patterns - (1 << 32) * (patterns >= (1 << 31))).to(torch.int32)


def float_of_words(words):
    """fp32 values given as 32-bit patterns."""
    return wrap32(words).view(torch.float32)


def is_nan(bits, dtype):
    return from_bits(bits, dtype).isnan()


def groups(c, dtype):
    return -(-c // GROUP[dtype])


def blocked(x, dtype):
    """fp32 [N, C, HW] -> fp32 [N][ceil(C / G)][HW][G] with +0 in the lanes beyond C."""
    n, c, hw = x.shape
    g, cg = GROUP[dtype], groups(c, dtype)
    padded = torch.zeros(n, cg * g, hw, dtype=torch.float32)
    padded[:, :c] = x
    return padded.reshape(n, cg, g, hw).permute(0, 1, 3, 2).contiguous()


def unblocked(v, c):
    """[N][CG][HW][G] -> [N, C, HW]: the lanes beyond C are dropped."""
    n, cg, hw, g = v.shape
    return v.permute(0, 1, 3, 2).reshape(n, cg * g, hw)[:, :c].contiguous()


def positive(bits, dtype):
    """`ref > 0` of the mask by reference (include/srgan_hip.h, NaN and mask rule): the 16-bit forms test the stored bits (sign
    clear, not zero: a NaN with a clear sign counts), dtype 0 compares the float (a NaN never counts)."""
    return from_bits(bits, 0) > 0 if dtype == 0 else bits > 0


def mask_factor(ref_bits, dtype, slope):
    return torch.where(positive(ref_bits, dtype), torch.tensor(1.0), torch.tensor(slope, dtype=torch.float32))


def pack_ref(x, dtype, ref_bits=None, slope=1.0):
    """srgan_h_pack: x fp32 [N, C, HW] (times 1 where ref > 0 else slope, in fp32) rounded once, as blocked bits."""
    v = blocked(x, dtype)
    if ref_bits is not None:
        v = v * mask_factor(ref_bits, dtype, slope)
    return to_bits(v, dtype)


def unpack_ref(bits, c, dtype):
    """srgan_h_unpack: blocked bits -> fp32 [N, C, HW]."""
    return unblocked(from_bits(bits, dtype), c)


def add_ref(a_bits, b_bits, dtype):
    """srgan_h_add: ONE fp32 addition, then one rounding (not a float64 sum rounded once: that is another function)."""
    return to_bits(from_bits(a_bits, dtype) + from_bits(b_bits, dtype), dtype)


def channel_sums_ref(bits, c, dtype):
    """float64 sums over n and pixels of the channels below C."""
    return unpack_ref(bits, c, dtype).double().sum(dim=(0, 2))


def poison_padding(bits, c, dtype, pattern=None):
    """A copy with garbage (NaN bits by default) in the lanes beyond C of the last group."""
    g = GROUP[dtype]
    out = bits.clone()
    spare = groups(c, dtype) * g - c
    if spare:
        out[:, -1, :, g - spare:] = NAN_BITS[dtype] if pattern is None else pattern
    return out


# ---- operands ---------------------------------------------------------------------------------------------------------------
def generator(*key):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate('/'.join(str(k) for k in key))) % (2 ** 31))


def normal_patterns(dtype, moderate=False):
    """Every finite, normal pattern of a 16-bit type (moderate: magnitudes in [2^-8, 2^9) only)."""
    patterns = torch.arange(65536, dtype=torch.int64)
    shift, bias, top = (7, 127, 255) if dtype == 1 else (10, 15, 31)
    exponent = (patterns >> shift) & top
    keep = (exponent >= bias - 8) & (exponent <= bias + 8) if moderate else (exponent > 0) & (exponent < top)
    return patterns[keep]


def distinct_values(count, dtype, *key, moderate=False):
    """`count` fp32 values that the type holds exactly and that differ from each other: a random permutation of the finite normal
    16-bit patterns (repeated from its start when `count` is larger); dtype 0: distinct non-zero integers of either sign."""
    gen = generator('distinct', dtype, count, *key)
    if dtype == 0:
        magnitude = (torch.randperm(count, generator=gen) + 1).float()
        assert count < EXACT_LIMIT
        return torch.where(torch.arange(count) % 3 == 0, -magnitude, magnitude)
    patterns = normal_patterns(dtype, moderate)
    patterns = patterns[torch.randperm(patterns.numel(), generator=gen)]
    return from_bits(wrap16(patterns.repeat(-(-count // patterns.numel()))[:count]), dtype)


def integers(shape, gen, limit=X):
    return torch.randint(-limit, limit + 1, shape, generator=gen).float()


# The lower 16-bit neighbours of the rounding table's ties (both parities of the last bit), without the sign.
TIE_LOWS = {1: [0x3F80, 0x3F81, 0x4000, 0x4001, 0x7F7E, 0x7F7F, 0x0001, 0x0002, 0x007F, 0x0080],
            2: [0x3C00, 0x3C01, 0x4000, 0x4001, 0x7BFE, 0x7BFF, 0x0000, 0x0001, 0x0002, 0x03FF, 0x0400]}
FP32_SUBNORMAL_WORDS = [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007FFFFF]
SPECIAL_WORDS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000]
SIGN = 0x80000000


def rounding_ties(dtype):
    """[(fp32 word of the value halfway between two neighbouring 16-bit values, the lower neighbour's 16-bit pattern)] for both
    signs ("lower" in magnitude).  Beyond the largest finite value the upper neighbour is the next power of two (-> inf)."""
    ties = []
    for sign16 in (0, 0x8000):
        for low in TIE_LOWS[dtype]:
            if dtype == 1:
                word = (low << 16) | 0x8000
            else:
                value = from_bits(wrap16([low]), 2).double()
                upper = from_bits(wrap16([low + 1]), 2).double() if low != 0x7BFF else torch.tensor([65536.0], dtype=torch.float64)
                halfway = ((value + upper) / 2).float()
                assert halfway.double() == (value + upper) / 2
                word = int(halfway.view(torch.int32)) & 0x7FFFFFFF
            ties.append((word | (SIGN if sign16 else 0), low | sign16))
    return ties


def rounding_table(dtype):
    """fp32 values at and next to the halfway points between neighbouring 16-bit values, the 16-bit values themselves, the
    overflow boundaries, fp32 subnormals, +-0, +-inf, NaN."""
    words = []
    for word, low in rounding_ties(dtype):
        exact = int(from_bits(wrap16([low]), dtype).view(torch.int32)) & 0xFFFFFFFF
        words += [word - 1, word, word + 1, exact]
    boundary = [0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF]                 # the largest finite bf16 and above
    boundary += [int(torch.tensor(v, dtype=torch.float32).view(torch.int32)) for v in (65504.0, 65519.99, 65520.0, 65536.0, 2.0 ** -25, 2.0 ** -24)]
    for word in boundary + FP32_SUBNORMAL_WORDS:
        words += [word, word | SIGN]
    return float_of_words(words + SPECIAL_WORDS)


# mask references: positive normal, smallest positive subnormal, +0, -0, negative, +inf, -inf, NaN with the sign clear / set
MASK_REFS = {1: [0x3F80, 0x0001, 0x0000, 0x8000, 0xBF80, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0],
             2: [0x3C00, 0x0001, 0x0000, 0x8000, 0xBC00, 0x7C00, 0xFC00, 0x7E00, 0xFE00],
             0: [0x3F800000, 0x00000001, 0x00000000, 0x80000000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000]}
MASK_POSITIVE = {1: [1, 1, 0, 0, 0, 1, 0, 1, 0], 2: [1, 1, 0, 0, 0, 1, 0, 1, 0], 0: [1, 1, 0, 0, 0, 1, 0, 0, 0]}


def mask_ref_bits(dtype):
    return (wrap32 if dtype == 0 else wrap16)(MASK_REFS[dtype])


# ---- pack / unpack / add tables ------------------------------------------------------------------------------------------
PACK_C = [1, 3, 4, 5, 7, 8, 9, 13, 16, 17]
PACK_HW = [1, 2, 60, 255, 256, 257]
PACK_N = [1, 3]
PACK_SECOND_TRIP = {0: (1, 13, 131073), 1: (1, 27, 131073), 2: (1, 27, 131073)}     # (N, C, HW): cap * 256 + 4 slots
ADD_SLOTS = [0, 1, 255, 256, 257, STREAM_BLOCKS * THREADS + 1]
ALL_PATTERNS = (1, 8, 8192)             # (N, C, HW): 65536 elements of a 16-bit type


def stream_grid(items, per_block=THREADS):
    return max(1, min(STREAM_BLOCKS, -(-items // per_block)))


def stream_trips(slots):
    """Grid-stride trips of a one-slot-per-thread kernel (0: the host returns before the launch)."""
    return 0 if slots == 0 else -(-slots // (stream_grid(slots) * THREADS))


def pack_slots(n, c, hw, dtype):
    return n * groups(c, dtype) * hw


# ---- channel sums -------------------------------------------------------------------------------------------------------------
def sums_parts(n, c, hw, dtype):
    """(parts, 'first' | 'cap' | 'halved'): workgroups per channel group as srgan_h_channel_sums chooses them."""
    cg = groups(c, dtype)
    parts, how = -(-(n * hw) // SUMS_PER_PART), 'first'
    if parts > SUMS_MAX_PARTS:
        parts, how = SUMS_MAX_PARTS, 'cap'
    parts = max(parts, 1)
    while parts > 1 and parts * cg > SUMS_MAX_BLOCKS:
        parts, how = parts >> 1, 'halved'
    return parts, how


def sums_finish(c, dtype, atomic_split=False):
    """'ordered' (one launch, the group's last workgroup adds the parts) | 'two launches' (h_channel_sums_finish_kernel)."""
    return 'two launches' if atomic_split or groups(c, dtype) > ROW_FINISH_ROWS else 'ordered'


def sums_chain_length(n, c, hw, dtype, atomic_split=False):
    """L: the longest chain of dependent fp32 additions between an element and out[c], as the kernels are built.  A thread adds
    its ceil(N * HW / (parts * 256)) elements one after the other; wave_sum is a butterfly of 6 levels; the four waves meet in
    (w0 + w1) + (w2 + w3): 2.  Ordered finish with parts > 1 (split_finish.h, ordered_row_finish): a thread adds its
    ceil(parts / 256) parts, then block_sum_256 = 6 levels + 3 additions over the waves in a row.  Two launches: one thread adds
    the `parts` parts one after the other onto 0.  Last: out[c] += total."""
    parts, _ = sums_parts(n, c, hw, dtype)
    per_thread = -(-(n * hw) // (parts * THREADS))
    chain = per_thread + 6 + 2
    if sums_finish(c, dtype, atomic_split) == 'ordered':
        chain += (-(-parts // THREADS) + 6 + 3) if parts > 1 else 0
    else:
        chain += parts
    return chain + 1


# (N, C, HW) per dtype group size; C is no multiple of G where the shape allows it
SUMS_SMALL = [(1, 1, 1), (3, 13, 5), (1, 13, 4096), (1, 13, 4097), (3, 7, 2731), (2, 18, 2048), (1, 5, 8193)]
SUMS_CAP = (1, 3, SUMS_MAX_PARTS * SUMS_PER_PART + 1)


def sums_halved(dtype):
    return (1, 2049 * GROUP[dtype] - 1, SUMS_PER_PART + 1)


def sums_many_groups(dtype):
    return (1, GROUP[dtype] * ROW_FINISH_ROWS + GROUP[dtype], 1)


SUMS_SEQUENCE = [(1, 13, 4097), (2, 41, 6000), (3, 5, 7), (1, 13, 4097)]      # back to back on one stream: another CG and parts each time
SUMS_INEXACT = (3, 13, 3001)


def assert_sums_exact(n, hw, prefill_limit, limit=X):
    """Every partial sum of integers in [-limit, limit] (and the prefilled output) is an integer below 2^24: exact in any order."""
    assert n * hw * limit + prefill_limit < EXACT_LIMIT, (n, hw, limit, prefill_limit)


# ---- pool -------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 2, 2), (3, 2, 6), (5, 8, 12), (2, 16, 16)]          # (planes, H, W)
POOL_PAST_CAP = (STREAM_BLOCKS * THREADS + 1, 2, 2)
POOL_SLOPES = [0.0, 0.125]
POOL_SPECIAL_VALUES = {1: [0xFF80, 0x8000, 0x0000, 0x0001, 0x3F80, 0x7F80, 0x7FC0, 0xFFC0],
                       2: [0xFC00, 0x8000, 0x0000, 0x0001, 0x3C00, 0x7C00, 0x7E00, 0xFE00]}    # -inf -0 +0 tiny 1 +inf NaN -NaN


def pool_ref(x_bits, dtype):
    """x bits [planes][H][W][8] -> (pooled bits [planes][H/2][W/2][8], position 0..3 of the maximum): a loop over the four window
    positions in scan order (0,0), (0,1), (1,0), (1,1), the FIRST maximum under `>` (a NaN is never greater and never beaten)."""
    x = from_bits(x_bits, dtype)
    window = [(x[:, dy::2, dx::2], x_bits[:, dy::2, dx::2]) for dy in (0, 1) for dx in (0, 1)]
    best, best_bits = window[0][0].clone(), window[0][1].clone()
    at = torch.zeros(best.shape, dtype=torch.int64)
    for q in (1, 2, 3):
        greater = window[q][0] > best
        best = torch.where(greater, window[q][0], best)
        best_bits = torch.where(greater, window[q][1], best_bits)
        at = torch.where(greater, torch.tensor(q), at)
    return best_bits, at


def pool_gather_ref(g_bits, at):
    """mode 2: g (input shape) at the arg-max of x."""
    window = torch.stack([g_bits[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)])
    return torch.gather(window, 0, at[None])[0]


def pool_bwd_ref(x_bits, gp_bits, dtype, masked, slope):
    """gx (input shape) = gp at the arg-max, +0 at the other three positions, times mask(pooled value, slope) when masked."""
    pooled, at = pool_ref(x_bits, dtype)
    g = from_bits(gp_bits, dtype)
    if masked:
        g = g * mask_factor(pooled, dtype, slope)
    g = to_bits(g, dtype)
    gx = torch.full(x_bits.shape, -1, dtype=x_bits.dtype)
    for q, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        gx[:, dy::2, dx::2] = torch.where(at == q, g, torch.zeros((), dtype=g.dtype))
    return gx


def tie_windows(dtype):
    """x bits [1][2 * 9][2 * 9][8]: all 81 windows over {0, 1, 2}^4, a different one in every channel lane of a slot."""
    window = torch.arange(81).reshape(9, 9, 1)
    pattern = (window * 8 + torch.arange(8) * 11) % 81                                      # [9][9][8]
    digits = torch.stack([(pattern // 3 ** q) % 3 for q in range(4)], dim=-1).float()       # [9][9][8][4]
    x = torch.zeros(1, 18, 18, 8)
    for q, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        x[0, dy::2, dx::2] = digits[..., q]
    return to_bits(x, dtype), pattern


def special_windows(dtype):
    """x bits [1][2 * 16][2 * 32][8]: all 8^4 windows over -inf, -0, +0, the smallest subnormal, 1, +inf, NaN, -NaN."""
    values = wrap16(POOL_SPECIAL_VALUES[dtype])
    index = torch.arange(4096).reshape(16, 32, 8)
    x = torch.zeros(1, 32, 64, 8, dtype=torch.int16)
    for q, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        x[0, dy::2, dx::2] = values[(index // 8 ** q) % 8]
    return x


# ---- weight-shadow packers (fp32 [slots][8 or G] before the one rounding) ----------------------------------------------------
CONV_K, CONV_C = [1, 5, 64, 72], [1, 3, 8, 15, 16, 17, 40]
CONV_TAPS = [(3, 3), (1, 1), (2, 3)]
CONV_256 = (16, 16, 2, 4)           # (K, C, R, S): ceil(16 / 16) * 8 * 2 * 16 = 256 slots exactly
CONV_258 = (129, 3, 1, 1)           # 258 slots: the slot count is even (two halves per chunk), so 257 does not exist -- the first
                                    # count past one workgroup, two slots in the second
K4_SHAPES = [(1, 1), (3, 5), (4, 4), (8, 16), (17, 33), (24, 20)]
TILE_ROWS, TILE_COLS = [1, 63, 64, 65, 130], [1, 8, 60, 64, 72, 200]
BIAS_CHANNELS, BIAS_PLANES = [1, 8, 9, 20], [1, 16, 48]
# (rows, cols, rows_real, cols_real, row_stride, col_stride, row_plane, col_plane) for the one-thread-per-slot body
MATRIX_SLOT = [(3, 20, 3, 20, 20, 1, 1, 1), (5, 13, 4, 11, 17, 1, 1, 1), (7, 30, 7, 27, 1, 1, 1, 1), (9, 24, 6, 24, 2, 31, 1, 1),
               (16, 64, 10, 40, 40, 1, 1, 4)]


def conv_weight_slots(rows, reduced, r, s):
    return -(-reduced // 16) * r * s * 2 * rows


def conv_weights_ref(w, transposed):
    """w [K][C][R][S] -> [chunk][tap][half][row][8]: the 8 reduced channels chunk * 16 + half * 8 .. + 7 of row `row` at `tap`
    (zero beyond the reduced extent).  transposed: rows = C, reduced over K, taps mirrored."""
    if transposed:
        w = w.flip(2, 3).transpose(0, 1)
    rows, reduced, r, s = w.shape
    chunks = -(-reduced // 16)
    padded = torch.zeros(rows, chunks * 16, r * s)
    padded[:, :reduced] = w.reshape(rows, reduced, r * s)
    return padded.reshape(rows, chunks, 2, 8, r * s).permute(1, 4, 2, 0, 3).reshape(-1, 8).contiguous()


def conv_weights_unpack(packed, k, c, r, s, transposed):
    rows, reduced = (c, k) if transposed else (k, c)
    chunks = -(-reduced // 16)
    w = packed.reshape(chunks, r * s, 2, rows, 8).permute(3, 0, 2, 4, 1).reshape(rows, chunks * 16, r, s)[:, :reduced]
    return w.transpose(0, 1).flip(2, 3).contiguous() if transposed else w.contiguous()


def k4s2_slots(a, b, direction, dtype):
    if direction == 0:
        return groups(b, dtype) * K4_TAPS * K4_CK * a
    return 4 * -(-groups(a, dtype) // K4_CK) * K4_TAPS * K4_CK * b


def k4s2_up_taps(r):
    """Kernel rows (columns) of output parity r at tap a = 0, 1."""
    return [3, 1] if r == 0 else [2, 0]


def k4s2_weights_ref(w, direction, dtype):
    """w [A][B][4][4] -> [slots][G].  direction 0: slot (chunk, tap = 2a + b, j = 2 qy + qx, o) = the G reduced channels G * chunk ..
    of w[o][.][2a + qy][2b + qx].  direction 1: class 2 ry + rx after class, slot (chunk, tap, j, o) = the G reduced channels
    G * (4 chunk + j) .. of w[.][o][kh(ry, a)][kw(rx, b)]."""
    a_, b_ = w.shape[:2]
    g = GROUP[dtype]
    if direction == 0:
        cg = groups(b_, dtype)
        padded = torch.zeros(a_, cg * g, 4, 4)
        padded[:, :b_] = w
        # [o][chunk][lane][a][qy][b][qx] -> [chunk][a][b][qy][qx][o][lane]
        return padded.reshape(a_, cg, g, 2, 2, 2, 2).permute(1, 3, 5, 4, 6, 0, 2).reshape(-1, g).contiguous()
    chunks = -(-groups(a_, dtype) // K4_CK)
    padded = torch.zeros(chunks * K4_CK * g, b_, 4, 4)
    padded[:a_] = w
    classes = []
    for ry in (0, 1):
        for rx in (0, 1):
            taps = padded[:, :, k4s2_up_taps(ry)][:, :, :, k4s2_up_taps(rx)]                # [reduced][o][a][b]
            classes.append(taps.reshape(chunks, K4_CK, g, b_, 2, 2).permute(0, 4, 5, 1, 3, 2).reshape(-1, g))
    return torch.cat(classes).contiguous()


def k4s2_weights_unpack(packed, a_, b_, direction, dtype):
    g = GROUP[dtype]
    if direction == 0:
        cg = groups(b_, dtype)
        return packed.reshape(cg, 2, 2, 2, 2, a_, g).permute(5, 0, 6, 1, 3, 2, 4).reshape(a_, cg * g, 4, 4)[:, :b_].contiguous()
    chunks = -(-groups(a_, dtype) // K4_CK)
    w = torch.zeros(chunks * K4_CK * g, b_, 4, 4)
    per_class = packed.reshape(4, chunks, 2, 2, K4_CK, b_, g)
    for ry in (0, 1):
        for rx in (0, 1):
            taps = per_class[2 * ry + rx].permute(0, 3, 5, 4, 1, 2).reshape(chunks * K4_CK * g, b_, 2, 2)
            for a in (0, 1):
                for b in (0, 1):
                    w[:, :, k4s2_up_taps(ry)[a], k4s2_up_taps(rx)[b]] = taps[:, :, a, b]
    return w[:a_].contiguous()


def plane_index(i, plane):
    """Index of element i of a flattened BLOCKED plane tensor ([C / 8][P][8]) in the flattened NCHW order ([C][P])."""
    if plane <= 1:
        return i
    slot = i >> 3
    return ((slot // plane) * 8 + (i & 7)) * plane + slot % plane


def matrix_source_size(rows, cols, rows_real, cols_real, rs, cs, row_plane, col_plane):
    return (rows_real - 1) * rs + (cols_real - 1) * cs + 1


def matrix_ref(src, rows, cols, rows_real, cols_real, rs, cs, row_plane, col_plane):
    """out[r][c], c < 8 * ceil(cols / 8): src[map(r, row_plane) * rs + map(c, col_plane) * cs] inside rows_real x cols_real, else 0."""
    width = -(-cols // 8) * 8
    rr = plane_index(torch.arange(rows), row_plane)[:, None]
    cc = plane_index(torch.arange(width), col_plane)[None, :]
    inside = (rr < rows_real) & (cc < cols_real)
    index = torch.where(inside, rr * rs + cc * cs, torch.zeros((), dtype=torch.int64))
    return torch.where(inside, src[index], torch.zeros(())).reshape(-1, 8).contiguous()


def matrix_body(rs, cs):
    """'tile' (the transposing 64 x 64 workgroup body) | 'slot' (one thread per slot), as both hosts switch."""
    return 'tile' if rs == 1 and cs != 1 else 'slot'


def matrix_tiles(rows, cols):
    return -(-rows // TILE) * -(-(-(-cols // 8) * 8) // TILE)


def bias_rows_ref(bias, plane):
    """fp32 rows[(g * plane + p) * 8 + j] = bias[8 g + j], 0 from the channel count on."""
    channels = bias.numel()
    padded = torch.zeros(-(-channels // 8) * 8)
    padded[:channels] = bias
    return padded.reshape(-1, 1, 8).expand(-1, plane, 8).reshape(-1).contiguous()


def recorded_matrix_calls():
    """The srgan_h_pack_matrix arguments the `linear` and `linear_t` shadows really pass (tests/golden/blocked16_calls.json):
    (rows, cols, rows_real, cols_real, row_stride, col_stride, row_plane, col_plane, dtype)."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'blocked16_calls.json')
    calls = []
    for name, case in sorted(json.load(open(path))['cases'].items()):
        for call in case.get('repack', []):
            if call[0] == 'srgan_h_pack_matrix':
                calls.append(tuple(call[3:12]))
    return calls
