"""The job fillers of the batched weight-shadow refresh for the matrix shadows and the seed layer's bias rows
(``srgan_h_pack_job_matrix`` / ``srgan_h_pack_job_bias_rows``, SRGAN_FEATURE_BATCHED_SHADOWS) on the CPU: they are exported and
bound, write the job the batched kernel expects into host memory, return its workgroup count, and reject bad arguments.  The
fillers never dereference the weight / buffer pointers, so arbitrary non-null addresses stand in for device memory."""
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
    """(w, packed, slots, first_block, kind, prec, p[10]) of the job at ``index`` (the 80-byte HPackJob of csrc/blocked16.h)."""
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
