"""The fp32 3x3 weight image on the host (no GPU): its size, its layout as the batched refresh's job states it, the slices the
kernel variants stage from it, and the bindings of the new entry points.

``image_reference`` is the NumPy restatement of the layout of include/srgan_hip.h
(``image[(ci * 9 + tap) * CO_pad + o]``, CO_pad = CO rounded up to 64, ci padded with zero rows to a multiple of 8); the GPU
tests compare the packers against it."""
import ctypes
import struct

import numpy as np
import pytest

from test_abi_cpu import c_class, ctypes_class, header_prototypes


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    return _lib


def padded(ci, co):
    return (ci + 7) // 8 * 8, (co + 63) // 64 * 64


def image_reference(weight, transposed):
    """The weight image of conv2d weights ``weight`` [K][C][3][3] as a flat float32 array: the forward operand (rows o = K,
    reduced ci = C) or the data gradient's (rows o = C, reduced ci = K, taps mirrored)."""
    k, c = weight.shape[:2]
    rows, reduced = (c, k) if transposed else (k, c)
    ci_pad, co_pad = padded(reduced, rows)
    image = np.zeros((ci_pad * 9, co_pad), dtype=np.float32)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        # forward: image[ci * 9 + tap][o] = w[o][ci][kh][kw]; transposed: image[k * 9 + tap][c] = w[k][c][2 - kh][2 - kw]
        block = weight[:, :, 2 - kh, 2 - kw] if transposed else weight[:, :, kh, kw].T
        image[tap:reduced * 9:9, :rows] = block
    return image.reshape(-1)


def test_image_floats_over_every_small_shape(lib):
    floats = lib.library().srgan_conv3x3_image_floats
    for ci in range(1, 131):
        for co in range(1, 131):
            ci_pad, co_pad = padded(ci, co)
            assert floats(ci, co) == ci_pad * 9 * co_pad, (ci, co)
            assert floats(ci, co) % 4 == 0                     # whole 16-byte transfers
    assert floats(0, 8) == 0 and floats(8, -1) == 0


def _job(lib, k, c, transposed, first_block=5):
    """The job ``srgan_h_pack_job_conv3x3_image`` writes, decoded: (slots, first_block, kind, prec, p[0..9], workgroups)."""
    library = lib.library()
    size = library.srgan_h_pack_job_bytes()
    host = ctypes.create_string_buffer(size)
    taken = library.srgan_h_pack_job_conv3x3_image(host, first_block, 4096, 8192, k, c, transposed)
    w, packed, slots, first, kind, prec = struct.unpack_from('<QQqqii', host.raw, 0)
    p = struct.unpack_from('<10i', host.raw, 40)
    assert (w, packed, first) == (4096, 8192, first_block)
    return slots, kind, prec, p, taken


@pytest.mark.parametrize('k,c', [(32, 12), (40, 32), (32, 128), (128, 32), (1, 1), (65, 9), (130, 129)])
@pytest.mark.parametrize('transposed', [0, 1])
def test_the_job_addresses_the_elements_of_the_restated_layout(lib, k, c, transposed):
    """The packer's body is ``image[e] = (o < CO && ci < CI) ? w[base + o * so + ci * si + kh * skh + kw * skw] : 0`` with the
    job's integers: evaluated here over the flat weights, it must give the restated image, zeros included."""
    generator = np.random.default_rng(k * 1000 + c * 2 + transposed)
    weight = generator.standard_normal((k, c, 3, 3)).astype(np.float32)
    slots, kind, prec, p, taken = _job(lib, k, c, transposed)
    rows, reduced = (c, k) if transposed else (k, c)
    assert (kind, prec) == (5, 0) and (p[0], p[1]) == (rows, reduced)
    assert slots == lib.library().srgan_conv3x3_image_floats(reduced, rows) and taken == (slots + 255) // 256
    base, so, si, skh, skw = p[2:7]
    ci_pad, co_pad = padded(reduced, rows)
    element = np.arange(slots)
    o, row = element % co_pad, element // co_pad
    ci, tap = row // 9, row % 9
    kh, kw = tap // 3, tap % 3
    valid = (o < rows) & (ci < reduced)
    index = np.where(valid, base + o * so + ci * si + kh * skh + kw * skw, 0)
    assert index.min() >= 0 and index.max() < weight.size
    image = np.where(valid, weight.reshape(-1)[index], np.float32(0))
    assert np.array_equal(image, image_reference(weight, transposed))


@pytest.mark.parametrize('ci,co', [(1, 1), (7, 33), (12, 40), (32, 128), (128, 32), (129, 65), (130, 130)])
def test_every_chunk_slice_lies_inside_the_image_and_holds_the_staged_operand(lib, ci, co):
    """A chunk's slice for a kernel variant (CI_T input channels from c0, BM rows from m0) is CI_T * 9 runs of BM contiguous
    floats at ``((c0 * 9 + r) * CO_pad + m0)``: inside the image for every tile the plans can ask for, and equal to the
    operand the kernel otherwise gathers -- w(m0 + o, c0 + r / 9, tap r % 9), zero where the row or the channel does not exist."""
    generator = np.random.default_rng(ci * 131 + co)
    weight = generator.standard_normal((co, ci, 3, 3)).astype(np.float32)      # forward: K = co, C = ci
    image = image_reference(weight, 0)
    floats = lib.library().srgan_conv3x3_image_floats(ci, co)
    assert image.size == floats
    ci_pad, co_pad = padded(ci, co)
    for ci_t, bm in ((8, 32), (4, 64)):
        for m0 in range(0, co, bm):
            for c0 in range(0, ci, ci_t):
                last = ((c0 + ci_t) * 9 - 1) * co_pad + m0 + bm - 1
                assert last < floats, (ci_t, bm, m0, c0)
                rows = (c0 * 9 + np.arange(ci_t * 9))[:, None] * co_pad + m0 + np.arange(bm)[None, :]
                want = np.zeros((ci_t * 9, bm), dtype=np.float32)
                channels, outputs = min(ci_t, ci - c0), min(bm, co - m0)
                want[:channels * 9, :outputs] = weight[m0:m0 + outputs, c0:c0 + channels].reshape(outputs, channels * 9).T
                assert np.array_equal(image[rows], want), (ci_t, bm, m0, c0)


def test_the_job_filler_and_the_packer_refuse_bad_arguments(lib):
    library = lib.library()
    size = library.srgan_h_pack_job_bytes()
    host = ctypes.create_string_buffer(size)
    fill = library.srgan_h_pack_job_conv3x3_image
    assert fill(host, 0, 4096, 8192, 32, 128, 0) == (128 * 9 * 64 + 255) // 256
    assert fill(host, 0, 4096, 8192, 32, 128, 1) == (32 * 9 * 128 + 255) // 256
    assert fill(None, 0, 4096, 8192, 32, 128, 0) == lib.EINVAL
    assert fill(host, -1, 4096, 8192, 32, 128, 0) == lib.EINVAL
    assert fill(host, 0, None, 8192, 32, 128, 0) == lib.EINVAL
    assert fill(host, 0, 4096, 8196, 32, 128, 0) == lib.EINVAL              # the image is not 16-byte aligned
    assert fill(host, 0, 4096, 8192, 0, 128, 0) == lib.EINVAL
    assert fill(host, 0, 4096, 8192, 32, 128, 2) == lib.EINVAL
    assert library.srgan_h_pack_conv3x3_image(None, 8192, 32, 128, 0, None) == lib.EINVAL
    assert library.srgan_h_pack_conv3x3_image(4096, 8196, 32, 128, 0, None) == lib.EINVAL


NEW_ENTRY_POINTS = ('srgan_conv3x3_image_floats', 'srgan_h_pack_conv3x3_image', 'srgan_h_pack_job_conv3x3_image',
                    'srgan_conv2d_fwd_bnrelu_image', 'srgan_conv2d_bwd_data_bnrelu_image',
                    'srgan_conv2d_bwd_data_bnrelu_partials_image')


def test_the_new_entry_points_are_bound_as_the_header_declares_them(lib):
    prototypes = header_prototypes()
    for name in NEW_ENTRY_POINTS:
        assert name in lib.SIGNATURES and getattr(lib.library(), name) is not None
        argtypes, restype = lib.SIGNATURES[name]
        c_return, c_arguments = prototypes[name]
        assert [ctypes_class(t) for t in argtypes] == [c_class(a) for a in c_arguments], name
        assert ctypes_class(restype) == c_class(c_return), name
    # the packed calls take the image right behind w and otherwise the arguments of the calls they stand in for
    for packed, plain in (('srgan_conv2d_fwd_bnrelu_image', 'srgan_conv2d_fwd_bnrelu'),
                          ('srgan_conv2d_bwd_data_bnrelu_image', 'srgan_conv2d_bwd_data_bnrelu'),
                          ('srgan_conv2d_bwd_data_bnrelu_partials_image', 'srgan_conv2d_bwd_data_bnrelu_partials')):
        assert len(prototypes[packed][1]) == len(prototypes[plain][1]) + 1
        assert sorted(prototypes[packed][1]) == sorted(prototypes[plain][1] + ['const float*'])
    assert lib.capabilities().features & 0x2000                        # SRGAN_FEATURE_CONV3X3_WEIGHT_IMAGE


def test_the_shadow_kind_states_both_forms(lib):
    """``blocked16.Conv3x3ImageShadow``: the forms of the batched refresh, from the layer's shape alone (no device needed)."""
    import torch
    from srgan_amd import blocked16
    assert blocked16.SHADOW_KINDS['conv3x3_image'] is blocked16.Conv3x3ImageShadow
    assert 'conv3x3_image' in blocked16.BATCHED_KINDS
    module = torch.nn.Conv2d(128, 32, 3, padding=1, bias=False)
    shadow = blocked16.Conv3x3ImageShadow(module, 0)
    forms = list(shadow.forms())
    assert [(f.name, f.packer, f.tail, f.dtype) for f in forms] == [
        ('forward', 'conv3x3_image', (32, 128, 0), torch.float32), ('transposed', 'conv3x3_image', (32, 128, 1), torch.float32)]
    assert [f.slots * 4 for f in forms] == [128 * 9 * 64, 32 * 9 * 128]
