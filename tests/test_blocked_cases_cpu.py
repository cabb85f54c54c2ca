"""blocked_cases.py checked on the CPU, without the library: every table reaches the branches it is there for, the vectorised
packer references equal element-by-element loops written from the layout comments, packing round-trips, the pool reference
follows torch's tie rule, the rounding table holds ties of both parities, and the constants mirror the kernel sources."""
import itertools
import os
import re

import torch

import blocked_cases as B

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sr-gan_amd', 'csrc')


def test_constants_mirror_the_kernel_sources():
    """A changed host constant fails here (and then, with the mirror updated, in the branch tests below) instead of silently
    un-covering a branch."""
    text = {name: open(os.path.join(CSRC, name)).read() for name in os.listdir(CSRC) if name.endswith(('.h', '.hip'))}
    everything = ''.join(text.values())
    assert f'if (blocks > {B.STREAM_BLOCKS}) blocks = {B.STREAM_BLOCKS};' in text['common.h']
    assert f'constexpr int ROW_FINISH_ROWS = {B.ROW_FINISH_ROWS};' in text['split_finish.h']
    assert 'if (split_atomics_forced() || rows > ROW_FINISH_ROWS || parts < 1) return nullptr;' in text['split_finish.h']
    host = text['blocked16_streaming.hip']
    assert f'int parts = (int)((per_group + {B.SUMS_PER_PART - 1}) / {B.SUMS_PER_PART});' in host
    assert f'if (parts > {B.SUMS_MAX_PARTS}) parts = {B.SUMS_MAX_PARTS};' in host
    assert f'while (parts > 1 && (int64_t)parts * CG > {B.SUMS_MAX_BLOCKS}) parts >>= 1;' in host
    assert 'float* part = row_finish_workspace(CG, parts, 8, g_h_sum_tickets, s, &tickets);' in host
    assert f'i += (int64_t)parts * {B.THREADS})' in host
    layouts, shadows = text['weight_shadows.h'], text['blocked16_shadows.hip']
    assert f'constexpr int K4_CK = {B.K4_CK};' in layouts and f'constexpr int K4_TAPS = {B.K4_TAPS};' in layouts
    # the 64 x 64 tile: the LDS array (of the single-layer kernel and of the batched one), the tile origin and the hosts' tile count
    assert f'float (*tile)[{B.TILE + 1}]' in layouts and shadows.count(f'__shared__ float tile[{B.TILE}][{B.TILE + 1}];') == 2
    assert f'r0 = (int64_t)(tile_index % tiles_r) * {B.TILE}, c0 = (int64_t)(tile_index / tiles_r) * {B.TILE};' in layouts
    tile_count = f'tiles_r = (rows + {B.TILE - 1}) / {B.TILE}, tiles = tiles_r * ((row_slots * 8 + {B.TILE - 1}) / {B.TILE});'
    assert tile_count in shadows and everything.count(tile_count) == 1 and everything.count(f'(rows + {B.TILE - 1}) / {B.TILE}') == 1
    # the switch between the two matrix bodies: one rule for the single call and the job
    assert 'return row_stride == 1 && col_stride != 1;' in shadows and everything.count('row_stride == 1') == 1
    # four channels per slot for dtype 0, eight for the 16-bit types
    found = re.search(r'slot_channels\(int \w+\) \{ return \w+ == 0 \? (\d+) : (\d+); \}', text['precision_dispatch.h'])
    assert found and (int(found.group(1)), int(found.group(2))) == (B.GROUP[0], B.GROUP[1]) and B.GROUP[2] == B.GROUP[1]
    # the rules the references restate
    assert 'return (int16_t)(uint16_t)bits16 > 0;' in text['blocked16.h']
    assert 'if constexpr (PREC == 0) return __uint_as_float(s.v[j]) > 0.f;' in text['blocked16.h']
    assert 'if (v[q][j] > m[j]) { m[j] = v[q][j]; at[j] = q; }' in host


def test_pack_unpack_and_add_tables_reach_every_host_branch():
    """Grid-stride trips 0 (the host returns), 1 and 2; one workgroup and several; a ragged last group for both group sizes."""
    for dtype in B.DTYPES:
        trips = {B.stream_trips(B.pack_slots(n, c, hw, dtype)) for n in B.PACK_N for c in B.PACK_C for hw in B.PACK_HW}
        assert trips == {1}
        assert B.pack_slots(*B.PACK_SECOND_TRIP[dtype], dtype) == B.STREAM_BLOCKS * B.THREADS + 4
        assert B.stream_trips(B.pack_slots(*B.PACK_SECOND_TRIP[dtype], dtype)) == 2
        assert B.PACK_SECOND_TRIP[dtype][1] % B.GROUP[dtype] != 0
        assert B.stream_trips(B.pack_slots(0, 5, 7, dtype)) == 0
        blocks = {B.stream_grid(B.pack_slots(n, c, hw, dtype)) for n in B.PACK_N for c in B.PACK_C for hw in B.PACK_HW}
        assert 1 in blocks and max(blocks) > 1
        assert {c % B.GROUP[dtype] for c in B.PACK_C} >= {0, 1, B.GROUP[dtype] - 1}
        assert {B.groups(c, dtype) for c in B.PACK_C} >= {1, 2, 3}
    assert 1 in B.PACK_HW                                                                  # HW = 1: a matrix
    assert [B.stream_trips(slots) for slots in B.ADD_SLOTS] == [0, 1, 1, 1, 1, 2]
    assert [B.stream_grid(slots) for slots in B.ADD_SLOTS[1:5]] == [1, 1, 1, 2]
    n, c, hw = B.ALL_PATTERNS
    assert n * c * hw == 65536 and c == B.GROUP[1]


def test_channel_sums_shapes_reach_every_parts_choice_and_both_finishes():
    for dtype in B.DTYPES:
        parts = {case: B.sums_parts(*case, dtype) for case in B.SUMS_SMALL}
        assert parts[(1, 13, 4096)] == (1, 'first') and parts[(1, 13, 4097)] == (2, 'first') and parts[(3, 7, 2731)] == (3, 'first')
        assert parts[(2, 18, 2048)] == (1, 'first') and parts[(1, 5, 8193)] == (3, 'first') and parts[(1, 1, 1)] == (1, 'first')
        assert B.sums_parts(*B.SUMS_CAP, dtype) == (B.SUMS_MAX_PARTS, 'cap')
        assert B.sums_parts(B.SUMS_CAP[0], B.SUMS_CAP[1], B.SUMS_CAP[2] - 1, dtype) == (B.SUMS_MAX_PARTS, 'first')      # the smallest
        halved = B.sums_halved(dtype)
        assert B.sums_parts(*halved, dtype) == (1, 'halved') and B.groups(halved[1], dtype) == 2049
        assert B.sums_parts(halved[0], halved[1] - B.GROUP[dtype], halved[2], dtype) == (2, 'first')     # one group fewer: not halved
        assert halved[1] % B.GROUP[dtype] != 0
        many = B.sums_many_groups(dtype)
        assert B.groups(many[1], dtype) == B.ROW_FINISH_ROWS + 1 and B.sums_finish(many[1], dtype) == 'two launches'
        assert B.sums_finish(many[1] - B.GROUP[dtype], dtype) == 'ordered'
        assert all(B.sums_finish(c, dtype) == 'ordered' and B.sums_finish(c, dtype, True) == 'two launches' for _, c, _ in B.SUMS_SMALL)
        assert any(c % B.GROUP[dtype] for _, c, _ in B.SUMS_SMALL)
        sequence = [(B.groups(c, dtype), B.sums_parts(n, c, hw, dtype)[0]) for n, c, hw in B.SUMS_SEQUENCE]
        assert all(a[0] != b[0] and a[1] != b[1] for a, b in zip(sequence, sequence[1:])), sequence
        assert max(p for _, p in sequence) >= 3 and min(p for _, p in sequence) == 1
        for n, c, hw in B.SUMS_SMALL + B.SUMS_SEQUENCE + [B.SUMS_CAP, halved, many]:
            B.assert_sums_exact(n, hw, 4 * c + 64)
        # the chain of the non-exact case: 3 * 3001 = 9003 elements in 3 parts: 12 per thread + 6 + 2, the finish 1 + 9, out += 1
        assert B.sums_parts(*B.SUMS_INEXACT, dtype) == (3, 'first')
        assert B.sums_chain_length(*B.SUMS_INEXACT, dtype) == 12 + 8 + 10 + 1
        assert B.sums_chain_length(*B.SUMS_INEXACT, dtype, atomic_split=True) == 12 + 8 + 3 + 1
    # unreached: `parts < 1` (N, HW > 0 make parts >= 1) and a halving that ends above 1 (CG in (1024, 2048] with parts >= 4
    # needs 1025 * 12289 slots = 200 MB, beyond the largest buffer this suite allows itself)


def test_pool_shapes_and_operands():
    outputs = [p * (h // 2) * (w // 2) for p, h, w in B.POOL_SHAPES]
    assert min(outputs) == 1 and len(set(outputs)) == 4 and B.stream_grid(B.POOL_PAST_CAP[0]) == B.STREAM_BLOCKS
    assert B.stream_trips(B.POOL_PAST_CAP[0]) == 2 and B.POOL_PAST_CAP[0] == B.STREAM_BLOCKS * B.THREADS + 1
    for dtype in B.HALVES:
        bits, pattern = B.tie_windows(dtype)
        assert sorted(pattern.flatten().tolist()) == sorted(list(range(81)) * 8)
        assert all(len(set(slot)) == 8 for slot in pattern.reshape(81, 8).tolist())          # a different window per lane
        special = B.special_windows(dtype)
        windows = {tuple(special[0, 2 * y:2 * y + 2, 2 * x:2 * x + 2, j].flatten().tolist()) for y in range(16) for x in range(32) for j in range(8)}
        assert len(windows) == 8 ** 4
        values = B.from_bits(B.wrap16(B.POOL_SPECIAL_VALUES[dtype]), dtype)
        assert values[:6].tolist()[:3] == [float('-inf'), -0.0, 0.0] and values[4] == 1 and values[5] == float('inf')
        assert 0 < values[3] < 1e-6 and values[6:].isnan().all()
        assert torch.signbit(values[1]) and not torch.signbit(values[2])


def torch_pool(x):
    """torch's values and window positions for x [planes][H][W] (no NaN)."""
    values, index = torch.nn.functional.max_pool2d(x[None], 2, 2, return_indices=True)
    w = x.shape[-1]
    row, column = index[0] // w, index[0] % w
    return values[0], (row % 2) * 2 + column % 2


def test_pool_reference_follows_torchs_tie_rule():
    """All 81 windows over {0, 1, 2}^4, and every window over -inf, -0, +0, the smallest subnormal, 1, +inf: values (bit for bit:
    +0 against -0) and positions equal torch.nn.functional.max_pool2d's."""
    for dtype in B.HALVES:
        tie, _ = B.tie_windows(dtype)
        special = B.special_windows(dtype)
        for bits in (tie, special):
            nan_free = ~B.is_nan(bits, dtype).reshape(1, bits.shape[1] // 2, 2, bits.shape[2] // 2, 2, 8).any(dim=4).any(dim=2)
            pooled, at = B.pool_ref(bits, dtype)
            x = B.from_bits(bits, dtype)[0].permute(2, 0, 1)                                # lanes as planes
            values, position = torch_pool(torch.nan_to_num(x, nan=0.0))
            values, position = values.permute(1, 2, 0)[None], position.permute(1, 2, 0)[None]
            assert nan_free.sum() >= 81 * 8
            assert torch.equal(B.to_bits(values, dtype)[nan_free], pooled[nan_free])
            assert torch.equal(position[nan_free], at[nan_free])
    # the NaN rule: kept at position 0 only
    for dtype in B.HALVES:
        nan, one, two = B.NAN_BITS[dtype], int(B.to_bits(torch.tensor([1.0]), dtype)), int(B.to_bits(torch.tensor([2.0]), dtype))
        for position in range(4):
            window = [one, two, one, one]
            window[position] = nan
            bits = B.wrap16(window).reshape(1, 2, 2, 1).expand(1, 2, 2, 8).contiguous()
            pooled, at = B.pool_ref(bits, dtype)
            if position == 0:
                assert B.is_nan(pooled, dtype).all() and (at == 0).all()
            else:
                assert (pooled == (one if position == 1 else two)).all() and (at == (0 if position == 1 else 1)).all()


def test_pool_gather_and_backward_follow_from_the_forward():
    for dtype in B.HALVES:
        bits, _ = B.tie_windows(dtype)
        pooled, at = B.pool_ref(bits, dtype)
        assert torch.equal(B.pool_gather_ref(bits, at), pooled)                              # gathering x itself gives the pool
        gp = B.to_bits(B.distinct_values(pooled.numel(), dtype, 'gp', moderate=True).reshape(pooled.shape), dtype)
        gx = B.pool_bwd_ref(bits, gp, dtype, 0, 0.0)
        assert torch.equal(B.pool_gather_ref(gx, at), gp)
        assert int((gx != 0).sum()) == gp.numel() and int((gx == 0).sum()) == 3 * gp.numel()
        masked = B.pool_bwd_ref(bits, gp, dtype, 1, 0.0)
        zero_windows = pooled == 0
        assert (B.from_bits(B.pool_gather_ref(masked, at), dtype)[zero_windows] == 0).all() and torch.equal(B.pool_gather_ref(masked, at)[~zero_windows], gp[~zero_windows])


def test_layout_reference_round_trips_and_pads_with_plus_zero():
    for dtype in B.DTYPES:
        for n, c, hw in [(1, 1, 1), (3, 13, 5), (2, 17, 60), (1, 8, 2)]:
            x = B.distinct_values(n * c * hw, dtype, 'layout').reshape(n, c, hw)
            bits = B.pack_ref(x, dtype)
            g = B.GROUP[dtype]
            assert bits.shape == (n, B.groups(c, dtype), hw, g)
            assert torch.equal(B.unpack_ref(bits, c, dtype), x)                              # identity on representable values
            for channel in range(c):                                                         # element by element: [N][c / G][HW][c % G]
                assert torch.equal(B.from_bits(bits[:, channel // g, :, channel % g], dtype), x[:, channel])
            spare = B.groups(c, dtype) * g - c
            if spare:
                assert (bits[:, -1, :, g - spare:] == 0).all()                               # +0: all bits clear
                poisoned = B.poison_padding(bits, c, dtype)
                assert B.is_nan(poisoned[:, -1, :, g - spare:], dtype).all()
                assert torch.equal(B.unpack_ref(poisoned, c, dtype), x)
                assert torch.equal(B.channel_sums_ref(poisoned, c, dtype), x.double().sum(dim=(0, 2)))
    # every pattern of the 16-bit types: unpack is torch's reinterpretation, pack gives the bits back (NaN stays NaN)
    for dtype in B.HALVES:
        patterns = B.wrap16(torch.arange(65536))
        values = B.from_bits(patterns, dtype)
        again = B.to_bits(values, dtype)
        nan = values.isnan()
        assert torch.equal(again[~nan], patterns[~nan]) and B.is_nan(again[nan], dtype).all()
        assert int(nan.sum()) == (254 if dtype == 1 else 2046)


def test_distinct_values_are_distinct_exact_and_normal():
    for dtype in B.DTYPES:
        for moderate in (False, True):
            values = B.distinct_values(4000, dtype, 'check', moderate=moderate)
            assert values.unique().numel() == 4000 and values.isfinite().all() and (values != 0).all()
            assert torch.equal(B.from_bits(B.to_bits(values, dtype), dtype), values)
            assert (values.abs() >= 2.0 ** -126).all() and (values < 0).any() and (values > 0).any()
            if moderate and dtype:
                assert (values.abs() >= 2.0 ** -8).all() and (values.abs() < 2.0 ** 9).all()
    assert B.normal_patterns(1).numel() == 254 * 128 * 2 and B.normal_patterns(2).numel() == 30 * 1024 * 2


def test_rounding_table_holds_ties_of_both_parities_and_torch_rounds_them_to_even():
    for dtype in B.HALVES:
        table = B.rounding_table(dtype)
        words = set((table.view(torch.int32).long() & 0xFFFFFFFF).tolist())
        seen = set()
        for word, low in B.rounding_ties(dtype):
            assert {word - 1, word, word + 1} <= words
            value = B.float_of_words([word])
            lower = B.from_bits(B.wrap16([low]), dtype).double()
            rounded = int(B.to_bits(value, dtype)) & 0xFFFF
            upper = rounded if rounded != low else low + 1
            upper_value = B.from_bits(B.wrap16([low + 1]), dtype).double()
            if upper_value.isfinite():
                assert (value.double() - lower == upper_value - value.double()).all(), (hex(word), hex(low))     # exactly halfway
            assert rounded in (low, low + 1) and rounded % 2 == 0, (hex(word), hex(low), hex(rounded))
            below, above = int(B.to_bits(B.float_of_words([word - 1]), dtype)) & 0xFFFF, int(B.to_bits(B.float_of_words([word + 1]), dtype)) & 0xFFFF
            assert (below, above) == (low, low + 1), (hex(word), hex(low))
            seen.add((low >> 15, low & 1, upper == rounded))
        assert {(s, p) for s, p, _ in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        # the overflow boundaries and the specials
        top = 0x7F7F if dtype == 1 else 0x7BFF
        assert any(low & 0x7FFF == top for _, low in B.rounding_ties(dtype))
        for word in B.SPECIAL_WORDS + B.FP32_SUBNORMAL_WORDS:
            assert word in words and (word | B.SIGN) in words
        if dtype == 2:
            for value, want in ((65504.0, 0x7BFF), (65519.99, 0x7BFF), (65520.0, 0x7C00), (2.0 ** -25, 0x0000)):
                assert int(torch.tensor(value, dtype=torch.float32).view(torch.int32)) in words
                assert int(B.to_bits(torch.tensor([value]), 2)) & 0xFFFF == want
        else:
            assert int(B.to_bits(B.float_of_words([0x7F7F7FFF]), 1)) & 0xFFFF == 0x7F7F
            assert int(B.to_bits(B.float_of_words([0x7F7F8000]), 1)) & 0xFFFF == 0x7F80
            assert int(B.to_bits(B.float_of_words([0x00008000]), 1)) & 0xFFFF == 0x0000     # fp32 subnormal ties: to even, not flushed
            assert int(B.to_bits(B.float_of_words([0x00018000]), 1)) & 0xFFFF == 0x0002
            assert int(B.to_bits(B.float_of_words([0x00400000]), 1)) & 0xFFFF == 0x0040


def test_mask_operands_and_rule():
    for dtype in B.DTYPES:
        bits = B.mask_ref_bits(dtype)
        values = B.from_bits(bits, dtype)
        assert values[0] == 1 and 0 < values[1] < 1e-6 and values[4] == -1 and values[5] == float('inf') and values[6] == float('-inf')
        assert values[2] == 0 and values[3] == 0 and torch.signbit(values[3]) and not torch.signbit(values[2]) and values[7:].isnan().all()
        assert B.positive(bits, dtype).long().tolist() == B.MASK_POSITIVE[dtype]
        assert B.positive(bits, dtype)[:7].tolist() == (values[:7] > 0).tolist()          # without a NaN: `> 0`
    x = torch.tensor([3.0, -5.0]).reshape(1, 2, 1)
    ref = B.pack_ref(torch.tensor([1.0, -1.0]).reshape(1, 2, 1), 1)
    assert B.from_bits(B.pack_ref(x, 1, ref, 0.125), 1)[0, 0, 0, :2].tolist() == [3.0, -0.625]


def test_add_reference_is_one_fp32_addition_and_one_rounding():
    for dtype in B.HALVES:
        a = B.to_bits(torch.tensor([2048.0, 65504.0, float('inf'), 1.0, 3.0e38]), dtype)
        b = B.to_bits(torch.tensor([1.0, 65504.0, float('-inf'), 2.0 ** -24, 3.0e38]), dtype)
        got = B.from_bits(B.add_ref(a, b, dtype), dtype)
        assert got[2].isnan() and got[3] == 1.0
        assert got[1] == (float('inf') if dtype == 2 else 131072.0) and got[4] == float('inf')
        assert got[0] == 2048.0                                        # 2049 is halfway in fp16 (-> even 2048); bf16 holds 2048, 2064
    a, b = B.wrap32([0x3F800001]), B.wrap32([0x33800000])             # 1 + 2^-23 and 2^-24: the fp32 tie goes to even
    assert int(B.add_ref(a, b, 0)) == 0x3F800002


# ---- the packers: loops written from the layout comments --------------------------------------------------------------------
def conv_weights_loop(w, transposed):
    """packed[((chunk * T + tap) * 2 + group) * CO + o] = the 8 channels chunk * 16 + group * 8 .. + 7 of tap `tap` of output channel
    o (zero beyond CI); the data gradient's shadow: channel roles swapped, taps mirrored."""
    k, c, r, s = w.shape
    rows, reduced = (c, k) if transposed else (k, c)
    taps = r * s
    out = torch.full((B.conv_weight_slots(rows, reduced, r, s), 8), float('nan'))
    for chunk in range(-(-reduced // 16)):
        for tap in range(taps):
            kh, kw = tap // s, tap % s
            for group in range(2):
                for o in range(rows):
                    for j in range(8):
                        channel = chunk * 16 + group * 8 + j
                        if channel >= reduced:
                            value = 0.0
                        elif transposed:
                            value = w[channel, o, r - 1 - kh, s - 1 - kw]
                        else:
                            value = w[o, channel, kh, kw]
                        out[((chunk * taps + tap) * 2 + group) * rows + o, j] = value
    return out


def k4s2_loop(w, direction, dtype):
    a_, b_ = w.shape[:2]
    g = B.GROUP[dtype]
    out = torch.full((B.k4s2_slots(a_, b_, direction, dtype), g), float('nan'))
    if direction == 0:
        for chunk in range(B.groups(b_, dtype)):
            for a, b, qy, qx, o, lane in itertools.product(range(2), range(2), range(2), range(2), range(a_), range(g)):
                slot = ((chunk * B.K4_TAPS + 2 * a + b) * B.K4_CK + 2 * qy + qx) * a_ + o
                channel = g * chunk + lane
                out[slot, lane] = w[o, channel, 2 * a + qy, 2 * b + qx] if channel < b_ else 0.0
        return out
    chunks = -(-B.groups(a_, dtype) // B.K4_CK)
    per_class = chunks * B.K4_TAPS * B.K4_CK * b_
    for ry, rx, chunk, a, b, j, o, lane in itertools.product(range(2), range(2), range(chunks), range(2), range(2), range(B.K4_CK),
                                                             range(b_), range(g)):
        kh = (3 - 2 * a) if ry == 0 else (2 - 2 * a)
        kw = (3 - 2 * b) if rx == 0 else (2 - 2 * b)
        slot = (2 * ry + rx) * per_class + ((chunk * B.K4_TAPS + 2 * a + b) * B.K4_CK + j) * b_ + o
        channel = g * (B.K4_CK * chunk + j) + lane
        out[slot, lane] = w[channel, o, kh, kw] if channel < a_ else 0.0
    return out


def matrix_loop(src, rows, cols, rows_real, cols_real, rs, cs, row_plane, col_plane):
    width = -(-cols // 8) * 8
    out = torch.full((rows, width), float('nan'))
    for r in range(rows):
        for c in range(width):
            rr, cc = B.plane_index(r, row_plane), B.plane_index(c, col_plane)
            out[r, c] = src[rr * rs + cc * cs] if rr < rows_real and cc < cols_real else 0.0
    return out.reshape(-1, 8)


def test_packer_references_equal_loops_written_from_the_comments_and_round_trip():
    for k, c, r, s in [(1, 1, 1, 1), (5, 3, 3, 3), (3, 17, 2, 3), (2, 16, 1, 1)]:
        w = B.distinct_values(k * c * r * s, 1, 'conv', k, c).reshape(k, c, r, s)
        for transposed in (0, 1):
            ref = B.conv_weights_ref(w, transposed)
            assert torch.equal(ref, conv_weights_loop(w, transposed)), (k, c, r, s, transposed)
            assert torch.equal(B.conv_weights_unpack(ref, k, c, r, s, transposed), w)
    for k in B.CONV_K:
        for c in B.CONV_C:
            w = B.distinct_values(k * c * 9, 2, 'conv', k, c).reshape(k, c, 3, 3)
            for transposed in (0, 1):
                assert torch.equal(B.conv_weights_unpack(B.conv_weights_ref(w, transposed), k, c, 3, 3, transposed), w)
    for a_, b_ in B.K4_SHAPES:
        for dtype in B.DTYPES:
            w = B.distinct_values(a_ * b_ * 16, dtype, 'k4', a_, b_).reshape(a_, b_, 4, 4)
            for direction in (0, 1):
                ref = B.k4s2_weights_ref(w, direction, dtype)
                assert ref.shape == (B.k4s2_slots(a_, b_, direction, dtype), B.GROUP[dtype])
                assert torch.equal(B.k4s2_weights_unpack(ref, a_, b_, direction, dtype), w), (a_, b_, direction, dtype)
                if a_ * b_ <= 24:
                    assert torch.equal(ref, k4s2_loop(w, direction, dtype)), (a_, b_, direction, dtype)
    for case in B.MATRIX_SLOT[:4] + [(3, 9, 2, 9, 1, 5, 1, 1)] + [tuple(call[:8]) for call in B.recorded_matrix_calls()]:
        src = B.distinct_values(B.matrix_source_size(*case), 1, 'matrix', *case)
        assert torch.equal(B.matrix_ref(src, *case), matrix_loop(src, *case)), case
    assert torch.equal(B.plane_index(torch.arange(48), 3), torch.tensor([B.plane_index(i, 3) for i in range(48)]))
    assert sorted(B.plane_index(torch.arange(48), 3).tolist()) == list(range(48))
    bias = B.distinct_values(9, 0, 'bias')
    rows = B.bias_rows_ref(bias, 3)
    assert rows.shape == (2 * 3 * 8,) and all(rows[(g * 3 + p) * 8 + j] == (bias[8 * g + j] if 8 * g + j < 9 else 0)
                                              for g in range(2) for p in range(3) for j in range(8))


def test_packer_tables_reach_both_matrix_bodies_and_the_ragged_chunks():
    assert B.conv_weight_slots(B.CONV_256[0], B.CONV_256[1], *B.CONV_256[2:]) == 256
    assert B.conv_weight_slots(B.CONV_258[0], B.CONV_258[1], *B.CONV_258[2:]) == 258
    assert all(B.conv_weight_slots(k, c, r, s) % 2 == 0 for k in range(1, 9) for c in range(1, 40) for r, s in B.CONV_TAPS)      # never 257
    assert {-(-c // 16) for c in B.CONV_C} == {1, 2, 3} and {c % 16 for c in B.CONV_C} >= {0, 1, 15} and {c % 8 for c in B.CONV_C} >= {0, 1, 7}
    for dtype in B.DTYPES:
        ragged = [B.groups(a_, dtype) % B.K4_CK for a_, _ in B.K4_SHAPES]
        assert any(ragged)                                                # channel_groups(A) no multiple of K4_CK
        assert any(b_ % B.GROUP[dtype] for _, b_ in B.K4_SHAPES) and any(a_ % B.GROUP[dtype] for a_, _ in B.K4_SHAPES)
        assert max(B.k4s2_slots(a_, b_, 1, dtype) // 4 for a_, b_ in B.K4_SHAPES) > B.THREADS
    assert all(B.matrix_body(case[4], case[5]) == 'slot' for case in B.MATRIX_SLOT)
    assert B.matrix_body(1, 40) == 'tile' and B.matrix_body(1, 1) == 'slot' and B.matrix_body(40, 1) == 'slot'
    assert {B.matrix_body(call[4], call[5]) for call in B.recorded_matrix_calls()} == {'slot', 'tile'}
    assert {call[6:8] for call in B.recorded_matrix_calls()} >= {(1, 1), (1, 4), (4, 1), (6, 1), (1, 6)}
    assert any(case[2] < case[0] for case in B.MATRIX_SLOT) and any(case[3] < case[1] for case in B.MATRIX_SLOT)
    assert any(case[1] % 8 for case in B.MATRIX_SLOT)
    tiles = {B.matrix_tiles(rows, cols) for rows in B.TILE_ROWS for cols in B.TILE_COLS}
    assert 1 in tiles and max(tiles) == 3 * 4 and {rows % B.TILE for rows in B.TILE_ROWS} >= {0, 1, 63}
