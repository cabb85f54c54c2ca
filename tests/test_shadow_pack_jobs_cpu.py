"""The job fillers of the batched weight-shadow refresh for the matrix shadows and the seed layer's bias rows
(``srgan_h_pack_job_matrix`` / ``srgan_h_pack_job_bias_rows``, SRGAN_FEATURE_BATCHED_SHADOWS) on the CPU: they are exported and
bound, write the job the batched kernel expects into host memory, return its workgroup count, and reject bad arguments.  The
fillers never dereference the weight / buffer pointers, so arbitrary non-null addresses stand in for device memory.  The
conv-weight and 4x4 / stride 2 fillers' jobs are decoded too, and each kind that has a single-layer call rejects what its filler
rejects."""
import ctypes
import struct

import pytest

FEATURE_BATCHED_SHADOWS = 0x10
SRC, OUT = 0x10000, 0x20000          # stand-ins for device addresses (not dereferenced)


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    return _lib


def _job(buffer, index=0):
    """(w, packed, slots, first_block, kind, prec, p[10]) of the job at ``index`` (the 80-byte HPackJob of csrc/weight_shadows.h)."""
    fields = struct.unpack_from('<QQqqii10i', buffer.raw, 80 * index)
    return fields[:6] + (list(fields[6:]),)


def test_exported_bound_and_advertised(lib):
    library = lib.library()
    for name in ('srgan_h_pack_job_matrix', 'srgan_h_pack_job_bias_rows'):
        assert name in lib.SIGNATURES and getattr(library, name) is not None
    assert library.srgan_h_pack_job_bytes() == 80
    assert lib.capabilities().features & FEATURE_BATCHED_SHADOWS
    assert library.srgan_version() == 110


@pytest.mark.parametrize('rows, cols, row_stride, col_stride, want_kind, want_blocks', [
    (10, 24, 24, 1, 2, 1),               # forward form of a small linear layer: 10 x 3 slots
    (4096, 25088, 25088, 1, 2, 50176),   # VGG-16's first classifier layer: 4096 x 3136 slots / 256
    (25088, 4096, 1, 25088, 3, 392 * 64),  # its transposed form: 64 x 64 tiles, one workgroup each
    (100, 30, 1, 10, 3, 2),              # a ragged transposed form: 2 x 1 tiles
])
def test_matrix_jobs(lib, rows, cols, row_stride, col_stride, want_kind, want_blocks):
    library = lib.library()
    jobs = ctypes.create_string_buffer(80)
    taken = library.srgan_h_pack_job_matrix(jobs, 7, SRC, OUT, rows, cols, rows, cols, row_stride, col_stride, 1, 1, 1)
    assert taken == want_blocks
    w, packed, slots, first_block, kind, prec, p = _job(jobs)
    assert (w, packed, first_block, kind, prec) == (SRC, OUT, 7, want_kind, 1)
    row_slots = (cols + 7) // 8
    if want_kind == 2:
        assert slots == rows * row_slots and p[:7] == [row_slots, rows, cols, row_stride, col_stride, 1, 1]
    else:
        assert slots == 256 * want_blocks and p[:8] == [rows, row_slots, rows, cols, col_stride, 1, 1, (rows + 63) // 64]


@pytest.mark.parametrize('channels, plane, want_blocks', [(20, 16, 1), (512, 16, 4), (1024, 16, 8), (3, 1, 1)])
def test_bias_rows_jobs(lib, channels, plane, want_blocks):
    jobs = ctypes.create_string_buffer(80)
    taken = lib.library().srgan_h_pack_job_bias_rows(jobs, 3, SRC, OUT, channels, plane)
    assert taken == want_blocks
    w, packed, slots, first_block, kind, prec, p = _job(jobs)
    assert (w, packed, slots, first_block, kind) == (SRC, OUT, (channels + 7) // 8 * plane, 3, 4)
    assert p[:2] == [channels, plane]


@pytest.mark.parametrize('dtype', [1, 2])
def test_conv_weight_jobs(lib, dtype):
    """Both operands of w[K][C][3][3]: the forward's (rows K) and the data gradient's (rows C, taps mirrored: base at the last
    tap, negative tap strides)."""
    K, C = 20, 12
    want = {0: [K, C, 3, 3, 0, C * 9, 9, 3, 1], 1: [C, K, 3, 3, 8, 9, C * 9, -3, -1]}
    for transposed in (0, 1):
        jobs = ctypes.create_string_buffer(80)
        taken = lib.library().srgan_h_pack_job_conv_weights(jobs, 5, SRC, OUT, K, C, 3, 3, transposed, dtype)
        w, packed, slots, first_block, kind, prec, p = _job(jobs)
        rows, reduced = want[transposed][:2]
        assert slots == (reduced + 15) // 16 * 9 * 2 * rows == lib.library().srgan_h_conv_weight_slots(rows, reduced, 3, 3)
        assert taken == (slots + 255) // 256
        assert (w, packed, first_block, kind, prec) == (SRC, OUT, 5, 0, dtype)
        assert p == want[transposed] + [0]


@pytest.mark.parametrize('dtype', [0, 1])
def test_k4s2_weight_jobs(lib, dtype):
    """w[A][B][4][4]: one job "down" (rows A, mode 0), four "up" (rows B, modes 1 .. 4 = the output parity classes, class-major in
    the target), each class with workgroups of its own."""
    library = lib.library()
    A, B, group = 40, 24, (4 if dtype == 0 else 8)
    written = ctypes.c_int32(-1)
    jobs = ctypes.create_string_buffer(4 * 80)
    taken = library.srgan_h_pack_job_k4s2_weights(jobs, 9, SRC, OUT, A, B, 0, dtype, ctypes.byref(written))
    slots = -(-B // group) * 4 * 4 * A
    assert slots == library.srgan_h_k4s2_weight_slots(A, B, 0, dtype)
    assert written.value == 1 and taken == (slots + 255) // 256
    assert _job(jobs) == (SRC, OUT, slots, 9, 1, dtype, [A, B, B * 16, 16, 0] + [0] * 5)
    written = ctypes.c_int32(-1)
    taken = library.srgan_h_pack_job_k4s2_weights(jobs, 9, SRC, OUT, A, B, 1, dtype, ctypes.byref(written))
    slots = -(-(-(-A // group)) // 4) * 4 * 4 * B                        # per class: ceil(groups(A) / 4) chunks
    assert 4 * slots == library.srgan_h_k4s2_weight_slots(A, B, 1, dtype)
    blocks = (slots + 255) // 256
    assert blocks > 1 and written.value == 4 and taken == 4 * blocks
    for cls in range(4):
        assert _job(jobs, cls) == (SRC, OUT + 16 * cls * slots, slots, 9 + cls * blocks, 1, dtype,
                                   [B, A, 16, B * 16, 1 + cls] + [0] * 5)


def _bad_argument_table(lib):
    """(kind, single-layer call, job filler, good shared arguments, [(argument index, bad value)]): the single call ends in a
    stream, the filler begins with (jobs, first_block) and the k4s2 one ends in its jobs_written."""
    library = lib.library()
    jobs, written = ctypes.create_string_buffer(4 * 80), ctypes.c_int32(0)
    conv = ('conv weights', lambda *a: library.srgan_h_pack_conv_weights(*a, None),
            lambda *a: library.srgan_h_pack_job_conv_weights(jobs, 0, *a),
            [SRC, OUT, 20, 12, 3, 3, 0, 1],                              # w, packed, K, C, R, S, transposed, dtype
            [(0, None), (1, None), (2, 0), (2, -1), (3, 0), (3, -4), (4, 0), (4, -1), (5, 0), (5, -1), (7, 0), (7, 3), (7, -1)])
    k4s2 = ('k4s2 weights', lambda *a: library.srgan_h_pack_k4s2_weights(*a, None),
            lambda *a: library.srgan_h_pack_job_k4s2_weights(jobs, 0, *a, ctypes.byref(written)),
            [SRC, OUT, 40, 24, 1, 0],                                    # w, packed, A, B, direction, dtype
            [(0, None), (1, None), (2, 0), (2, -1), (3, 0), (3, -1), (4, 2), (4, -1), (5, 3), (5, -1)])
    image = ('3x3 image', lambda *a: library.srgan_h_pack_conv3x3_image(*a, None),
             lambda *a: library.srgan_h_pack_job_conv3x3_image(jobs, 0, *a),
             [SRC, OUT, 20, 12, 1],                                      # w, image, K, C, transposed (fp32 only: no dtype)
             [(0, None), (1, None), (1, OUT + 4), (2, 0), (2, -1), (3, 0), (3, -1), (4, 2), (4, -1)])
    return [conv, k4s2, image]


def test_a_kinds_single_call_and_job_filler_reject_the_same_arguments(lib):
    """NULL source or target, a non-positive extent, a dtype outside the kind's list and a direction / transposed outside
    {0, 1} (where the kind checks it: the conv-weight packer reads `transposed` as a truth value): the same status from both.
    Invalid arguments return before any launch, so the single-layer calls run here without a device."""
    cases = 0
    for kind, single, filler, good, bad in _bad_argument_table(lib):
        for index, value in bad:
            arguments = list(good)
            arguments[index] = value
            got = single(*arguments), filler(*arguments)
            assert got == (lib.EINVAL, lib.EINVAL), (kind, index, value, got)
            cases += 1
    assert cases == 13 + 10 + 9


def test_bad_arguments_are_rejected(lib):
    library = lib.library()
    jobs = ctypes.create_string_buffer(80)
    matrix = library.srgan_h_pack_job_matrix
    assert matrix(jobs, 0, SRC, OUT, 8, 8, 8, 8, 8, 1, 1, 1, 0) == lib.EINVAL          # fp32: the matrix shadows are 16-bit
    assert matrix(jobs, 0, SRC, OUT, 8, 8, 8, 8, 8, 1, 1, 1, 3) == lib.EINVAL
    assert matrix(None, 0, SRC, OUT, 8, 8, 8, 8, 8, 1, 1, 1, 1) == lib.EINVAL
    assert matrix(jobs, 0, None, OUT, 8, 8, 8, 8, 8, 1, 1, 1, 1) == lib.EINVAL
    assert matrix(jobs, 0, SRC, None, 8, 8, 8, 8, 8, 1, 1, 1, 1) == lib.EINVAL
    assert matrix(jobs, -1, SRC, OUT, 8, 8, 8, 8, 8, 1, 1, 1, 1) == lib.EINVAL
    assert matrix(jobs, 0, SRC, OUT, 0, 8, 8, 8, 8, 1, 1, 1, 2) == lib.EINVAL
    assert matrix(jobs, 0, SRC, OUT, 8, 8, 8, 8, 1 << 31, 1, 1, 1, 2) == lib.EINVAL    # strides kept in 32 bits
    assert matrix(jobs, 0, SRC, OUT, 1 << 31, 8, 8, 8, 8, 1, 1, 1, 2) == lib.EINVAL
    bias_rows = library.srgan_h_pack_job_bias_rows
    assert bias_rows(jobs, 0, SRC, OUT, 0, 16) == lib.EINVAL
    assert bias_rows(jobs, 0, SRC, OUT, 16, 0) == lib.EINVAL
    assert bias_rows(jobs, 0, None, OUT, 16, 16) == lib.EINVAL
    assert bias_rows(jobs, 0, SRC, None, 16, 16) == lib.EINVAL
    assert bias_rows(None, 0, SRC, OUT, 16, 16) == lib.EINVAL
