"""The calls behind tests/golden/conv_routes.json: what every convolution / GEMM entry point launches, recorded through the
public ABI only (srgan_profile_begin / _end / _report and the query entry points), so that the same list runs on any commit.

``replay(lib)`` makes every call once on torch tensors filled with ones (the routes depend on shapes, strides, alignment and
the stream's workspace, never on values) and returns ``{group: {case: {call: [status, report line, ...]}}}``.  A report line is
``M N K kind bm bn split akf bkf count bytes``: srgan_profile_report's line without its ``ms`` column.  Query entry points are
stored as ``[return value]``.  tests/golden/make_conv_route_goldens.py writes the result, test_conv_routes_gpu.py compares it.
"""
import ctypes

import torch

from contraction_cases import BN_DATA_CASES, BN_FORWARD_CASES, CONV_CASES, GEMM_CASES, GROUPED_WGRAD_CASES, W, X, output_plane

# One forward call whose output is a channel slice of a wider buffer, on the generic MFMA kernel with a K split of 3
# (M = 20, N = 2 * 7 * 7, K = 288): with the stream's workspace the slices meet in the ordered finish; on a stream without one
# they are added with fp32 atomics into an output that is zeroed row by row (one row per image: the other channels stay).
# (contraction_cases' (2, 32, 16, 16, 20, 16, 16) splits K 128 ways onto 40 outputs, which goes through the partial-sum
# workspace on every stream and is an error on a stream without one, so it cannot show the atomic route.)
SLICE_SHAPE = (2, 32, 16, 16, 20, 3, 3, (2, 2), (0, 0))
SLICE_CHANNELS = 24
SLICE_FILL = 7.0


def _abi():
    from srgan_amd import _lib
    return _lib


def stream():
    return _abi().stream_handle()


def ones(*shape):
    return torch.ones(shape, device='cuda')


def pointer(t):
    return None if t is None else t.data_ptr()


def conv_name(shape):
    n, c, h, w, k, r, s, stride, pad = shape
    return f'{n}x{c}x{h}x{w}-k{k}-{r}x{s}-s{stride[0]}{stride[1]}-p{pad[0]}{pad[1]}'


def desc_of(shape, x_batch_stride=0, y_batch_stride=0, dtype=0):
    n, c, h, w, k, r, s, stride, pad = shape
    oh, ow = output_plane(shape)
    return _abi().ConvDesc(n, c, h, w, k, r, s, stride[0], stride[1], pad[0], pad[1], oh, ow, x_batch_stride, y_batch_stride, dtype)


def routed(lib, call):
    """[status, report lines without the ms column] of one call inside a profile bracket."""
    lib.srgan_profile_begin()
    status = call()
    lib.srgan_profile_end(None, None, None, None)
    size = int(lib.srgan_profile_report(None, 0))
    buffer = ctypes.create_string_buffer(size + 1)
    lib.srgan_profile_report(buffer, size + 1)
    lines = []
    for line in buffer.value.decode().splitlines():
        fields = line.split()
        if len(fields) == 12:
            lines.append(' '.join(fields[:10] + fields[11:]))
    return [int(status)] + lines


# ------------------------------------------------------------------------------------------------- convolutions
def conv_routes(lib):
    out = {}
    for entry in CONV_CASES:
        shape = entry.shape
        n, c, h, w, k, r, s, stride, pad = shape
        oh, ow = output_plane(shape)
        x, gy, weight, bias = ones(n, c, h, w), ones(n, k, oh, ow), ones(k, c, r, s), ones(max(k, c))
        y, gx, gw = ones(n, k, oh, ow), ones(n, c, h, w), ones(k, c, r, s)
        calls = out[conv_name(shape)] = {}
        for dtype in (0, 1, 2):
            desc = desc_of(shape, dtype=dtype)
            for force in ((0, 2) if dtype == 0 else (0,)):
                tag = f'dtype{dtype}/force{force}'
                for b in (None, bias):
                    calls[f'fwd/{tag}/bias{int(b is not None)}'] = routed(lib, lambda: lib.srgan_conv2d_fwd(
                        desc, x.data_ptr(), weight.data_ptr(), pointer(b), y.data_ptr(), force, stream()))
                    for accumulate in (0, 1):
                        calls[f'bwd_data/{tag}/bias{int(b is not None)}/accumulate{accumulate}'] = routed(
                            lib, lambda: lib.srgan_conv2d_bwd_data(desc, gy.data_ptr(), weight.data_ptr(), pointer(b), gx.data_ptr(),
                                                                   accumulate, force, stream()))
                for accumulate in (0, 1):
                    calls[f'bwd_weight/{tag}/accumulate{accumulate}'] = routed(lib, lambda: lib.srgan_conv2d_bwd_weight(
                        desc, x.data_ptr(), gy.data_ptr(), gw.data_ptr(), accumulate, force, stream()))
    return out


# ------------------------------------------------------------------------------------------------- matrix multiplies
def gemm_routes(lib):
    """The five products of a linear layer's passes per shape, in all four operand layouts, and once into a column-major C."""
    out = {}
    for entry in GEMM_CASES:
        batch, fin, fout = entry.shape
        calls = out['x'.join(map(str, entry.shape))] = {}
        for (m, n, k) in [(batch, fout, fin), (batch, fin, fout), (fout, fin, batch), (fin, fout, batch), (fout, batch, fin)]:
            a, b, c = ones(m * k), ones(k * n), ones(m * n)
            for dtype in (0, 1, 2):
                for ta in (0, 1):
                    for tb in (0, 1):
                        sai, sak = (1, m) if ta else (k, 1)
                        sbk, sbj = (1, k) if tb else (n, 1)
                        calls[f'{m}x{n}x{k}/dtype{dtype}/ta{ta}/tb{tb}'] = routed(lib, lambda: lib.srgan_gemm(
                            m, n, k, a.data_ptr(), sai, sak, b.data_ptr(), sbk, sbj, c.data_ptr(), n, 1, None, 1, 0, 0, dtype, stream()))
                calls[f'{m}x{n}x{k}/dtype{dtype}/column_major_c'] = routed(lib, lambda: lib.srgan_gemm(
                    m, n, k, a.data_ptr(), k, 1, b.data_ptr(), n, 1, c.data_ptr(), 1, m, None, 1, 0, 0, dtype, stream()))
    return out


# ------------------------------------------------------------------------------------------------- fused batch norm
def bn_cases():
    """(name, case, input batch stride in channels, gy channels): the forward list reads a channel slice of a wider buffer; the
    data list writes gx into one (1x1) or reads gy from one (3x3), as test_exact_contractions_gpu.py does."""
    for case in BN_FORWARD_CASES:
        yield 'forward-' + 'x'.join(map(str, case)), case, case[2], case[5]
    for case in BN_DATA_CASES:
        n, c, total, h, w, k, r = case
        yield 'data-' + 'x'.join(map(str, case)), case, (total if r == 1 else c), (k if r == 1 else k + 8)


def bn_routes(lib, images):
    """images False: the seven fused entry points and the three queries per case; True: the _image forms of the 3x3 cases."""
    out = {}
    for name, case, x_channels, gy_channels in bn_cases():
        n, c, total, h, w, k, r = case
        if images and r != 3:
            continue
        shape = (n, c, h, w, k, r, r, (1, 1), (r // 2, r // 2))
        desc = desc_of(shape, x_channels * h * w if x_channels != c else 0, gy_channels * h * w if gy_channels != k else 0)
        x, gx = ones(n, x_channels, h, w), ones(n, x_channels, h, w)
        y, gy = ones(n, gy_channels, h, w), ones(n, gy_channels, h, w)
        weight, gw, bias = ones(k, c, r, r), ones(k, c, r, r), ones(k)
        vectors = [ones(c) for _ in range(4)]
        bn = _abi().BnRelu(*(v.data_ptr() for v in vectors))
        g_gamma, g_beta = ones(c), ones(c)
        tiles = int(lib.srgan_conv2d_bwd_data_bnrelu_tiles(desc))
        partials = ones(max(1, 2 * tiles * c))
        calls = out[name] = {}
        if images:
            forward = ones(int(lib.srgan_conv3x3_image_floats(c, k)))
            transposed = ones(int(lib.srgan_conv3x3_image_floats(k, c)))
            _abi().check(lib.srgan_h_pack_conv3x3_image(weight.data_ptr(), forward.data_ptr(), k, c, 0, stream()), 'forward image')
            _abi().check(lib.srgan_h_pack_conv3x3_image(weight.data_ptr(), transposed.data_ptr(), k, c, 1, stream()), 'transposed image')
            calls['fwd_bnrelu_image'] = routed(lib, lambda: lib.srgan_conv2d_fwd_bnrelu_image(
                desc, x.data_ptr(), bn, weight.data_ptr(), forward.data_ptr(), bias.data_ptr(), y.data_ptr(), stream()))
            calls['bwd_data_bnrelu_image'] = routed(lib, lambda: lib.srgan_conv2d_bwd_data_bnrelu_image(
                desc, gy.data_ptr(), weight.data_ptr(), transposed.data_ptr(), bn, x.data_ptr(), gx.data_ptr(), g_gamma.data_ptr(),
                g_beta.data_ptr(), 0, stream()))
            calls['bwd_data_bnrelu_partials_image'] = routed(lib, lambda: lib.srgan_conv2d_bwd_data_bnrelu_partials_image(
                desc, gy.data_ptr(), weight.data_ptr(), transposed.data_ptr(), bn, x.data_ptr(), gx.data_ptr(), partials.data_ptr(), 0,
                stream()))
            continue
        for which in (0, 1, 2):
            calls[f'supported/pass{which}'] = [int(lib.srgan_conv2d_bnrelu_supported(desc, which))]
        calls['fwd_bnrelu_splits'] = [int(lib.srgan_conv2d_fwd_bnrelu_splits(desc))]
        calls['bwd_data_bnrelu_tiles'] = [tiles]
        calls['fwd_bnrelu'] = routed(lib, lambda: lib.srgan_conv2d_fwd_bnrelu(
            desc, x.data_ptr(), bn, weight.data_ptr(), bias.data_ptr(), y.data_ptr(), stream()))
        y.zero_()
        calls['fwd_bnrelu_into_zeros'] = routed(lib, lambda: lib.srgan_conv2d_fwd_bnrelu_into_zeros(
            desc, x.data_ptr(), bn, weight.data_ptr(), bias.data_ptr(), y.data_ptr(), stream()))
        for accumulate in (0, 1):
            calls[f'bwd_data_bnrelu/accumulate{accumulate}'] = routed(lib, lambda: lib.srgan_conv2d_bwd_data_bnrelu(
                desc, gy.data_ptr(), weight.data_ptr(), bn, x.data_ptr(), gx.data_ptr(), g_gamma.data_ptr(), g_beta.data_ptr(),
                accumulate, stream()))
            calls[f'bwd_data_bnrelu_partials/accumulate{accumulate}'] = routed(lib, lambda: lib.srgan_conv2d_bwd_data_bnrelu_partials(
                desc, gy.data_ptr(), weight.data_ptr(), bn, x.data_ptr(), gx.data_ptr(), partials.data_ptr(), accumulate, stream()))
            calls[f'bwd_weight_bnrelu/accumulate{accumulate}'] = routed(lib, lambda: lib.srgan_conv2d_bwd_weight_bnrelu(
                desc, x.data_ptr(), bn, gy.data_ptr(), gw.data_ptr(), accumulate, stream()))
    return out


# ------------------------------------------------------------------------------------------------- grouped weight gradients
def group_plan_routes(lib):
    """srgan_wgrad_group_plan's outputs at test_grouped_weight_gradients_gpu.py's shapes: four 1x1 weight gradients over growing
    channel prefixes of one buffer, and the same prefixes as 3x3 convolutions."""
    out = {}
    n, width, cins = 3, 128, (96, 160, 288, 416)
    for (h, w), shares in GROUPED_WGRAD_CASES:
        for r in (1, 3):
            calls = out[f'{h}x{w}-shares{int(shares)}-k{r}'] = {}
            weights = sum(width * c * r * r for c in cins) if shares else 0
            slots = (ctypes.c_byte * (128 * len(cins)))()
            partial_at = 0
            for index, c in enumerate(cins):
                vectors = [ones(c) for _ in range(4)]
                bn = _abi().BnRelu(*(v.data_ptr() for v in vectors))
                gw = ones(width, c, r, r)
                desc = desc_of((n, c, h, w, width, r, r, (1, 1), (r // 2, r // 2)), max(cins) * h * w)
                grid_x, grid_y, ragged, partial = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
                status = lib.srgan_wgrad_group_plan(desc, bn, 0, index * n * width * h * w, gw.data_ptr(), 0, len(cins), weights,
                                                    partial_at, ctypes.byref(slots, 128 * index), ctypes.byref(grid_x),
                                                    ctypes.byref(grid_y), ctypes.byref(ragged), ctypes.byref(partial))
                calls[f'{c}'] = [int(status), grid_x.value, grid_y.value, ragged.value, partial.value]
                partial_at += max(0, partial.value)
    return out


# ------------------------------------------------------------------------------------------------- channel-slice output
def slice_operands():
    """The exact integer operands of contraction_cases.py (x in [-X, X], weights in [-W, W]) for SLICE_SHAPE, on the CPU."""
    n, c, h, w, k, r, s, stride, pad = SLICE_SHAPE
    generator = torch.Generator().manual_seed(20)
    x = torch.randint(-X, X + 1, (n, c, h, w), generator=generator).double()
    weight = torch.randint(-W, W + 1, (k, c, r, s), generator=generator).double()
    return x, weight


def slice_routes(lib):
    """({call: [status, lines]}, {call: the 24-channel output buffer}) of the forward into a channel slice: on the default stream
    (workspace registered) and on a second stream whose workspace was unregistered with srgan_set_workspace(NULL, 0, stream)."""
    n, c, h, w, k, r, s, stride, pad = SLICE_SHAPE
    oh, ow = output_plane(SLICE_SHAPE)
    desc = desc_of(SLICE_SHAPE, 0, SLICE_CHANNELS * oh * ow)
    x, weight = slice_operands()
    dx, dw = x.float().cuda(), weight.float().cuda()
    calls, outputs = {}, {}
    y = torch.full((n, SLICE_CHANNELS, oh, ow), SLICE_FILL, device='cuda')
    calls['default_stream'] = routed(lib, lambda: lib.srgan_conv2d_fwd(desc, dx.data_ptr(), dw.data_ptr(), None, y.data_ptr(), 0, stream()))
    calls['default_stream/split_is_ordered'] = [int(lib.srgan_split_is_ordered(stream()))]
    outputs['default_stream'] = y
    side = torch.cuda.Stream()
    handle = side.cuda_stream
    _abi().check(lib.srgan_set_workspace(None, 0, handle), 'srgan_set_workspace(NULL)')
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y2 = torch.full((n, SLICE_CHANNELS, oh, ow), SLICE_FILL, device='cuda')
        calls['unregistered_stream'] = routed(lib, lambda: lib.srgan_conv2d_fwd(desc, dx.data_ptr(), dw.data_ptr(), None, y2.data_ptr(),
                                                                                0, handle))
        calls['unregistered_stream/split_is_ordered'] = [int(lib.srgan_split_is_ordered(handle))]
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    outputs['unregistered_stream'] = y2
    return calls, outputs


GROUPS = ('conv', 'gemm', 'bn', 'image', 'group_plan', 'slice')


def replay(lib):
    """Every group's routes, and the slice call's two output buffers."""
    assert torch.cuda.is_available()
    stream()                                        # registers the default stream's workspace
    calls, outputs = slice_routes(lib)
    routes = {'conv': conv_routes(lib), 'gemm': gemm_routes(lib), 'bn': bn_routes(lib, False), 'image': bn_routes(lib, True),
              'group_plan': group_plan_routes(lib), 'slice': {conv_name(SLICE_SHAPE): calls}}
    torch.cuda.synchronize()
    return routes, outputs
