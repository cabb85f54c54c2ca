"""Which precision codes the blocked entry points take (include/srgan_hip.h: dtype 0 = fp32 in slots of four channels, 1 = bf16,
2 = fp16): every entry point with a ``dtype`` argument is called on 1 x 8 x 2 x 2 tensors (weights 8 x 8 with the family's kernel
size) with arguments that are valid but for the code.  A code the family has no kernels for -- -1 and 3 everywhere, 0 where only
1 and 2 exist -- is reported as the library's invalid-argument status before anything is enqueued: the NaN-prefilled outputs
(for the job fillers the host job array) are untouched.  Every code the family does list succeeds with the same arguments, so a
rejection can only come from the code.

Every device buffer is 64 KB, far more than the fp32 blocked form of any tensor here needs (128 bytes for the activations, 8 KB
for the largest weight operand): no reading of a code can leave a buffer.  ``srgan_h_k4s2_weight_slots`` also takes a dtype but
returns a size, not a status, and is not covered."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

FLOATS = 16384
N, C, H, W = 1, 8, 2, 2
HW = H * W
ANY, HALF = (0, 1, 2), (1, 2)
BAD = (-1, 3)


@pytest.fixture(scope='module', autouse=True)
def pkg():
    import srgan_amd
    assert torch.cuda.is_available()
    return srgan_amd


class Buffers:
    """Device buffers of one call: inputs are zeros, everything the call may write starts as NaN."""

    def __init__(self):
        self.inputs, self.outputs = [], []

    def i(self):
        self.inputs.append(torch.zeros(FLOATS, device='cuda'))
        return self.inputs[-1].data_ptr()

    def o(self):
        self.outputs.append(torch.full((FLOATS,), float('nan'), device='cuda'))
        return self.outputs[-1].data_ptr()

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(buffer).all()) for buffer in self.outputs)


# name -> (codes the family has, arguments(b, dtype, stream)); NULL for every optional pointer
DEVICE_CALLS = {
    'srgan_h_pack': (ANY, lambda b, d, s: (b.i(), b.o(), None, 1.0, N, C, HW, d, s)),
    'srgan_h_unpack': (ANY, lambda b, d, s: (b.i(), b.o(), N, C, HW, d, s)),
    'srgan_h_add': (ANY, lambda b, d, s: (b.i(), b.i(), b.o(), N * 2 * HW, d, s)),
    'srgan_h_channel_sums': (ANY, lambda b, d, s: (b.i(), b.o(), N, C, HW, d, s)),
    'srgan_h_maxpool2': (HALF, lambda b, d, s: (b.i(), None, b.o(), N * 2, H, W, 0, d, s)),
    'srgan_h_maxpool2_bwd': (HALF, lambda b, d, s: (b.i(), b.i(), b.o(), N * 2, H, W, 0, 0.0, d, s)),
    'srgan_h_pack_conv_weights': (HALF, lambda b, d, s: (b.i(), b.o(), C, C, 3, 3, 0, d, s)),
    'srgan_h_conv3x3': (HALF, lambda b, d, s: (b.i(), b.i(), None, None, 1.0, 0, b.o(), N, C, C, C, H, W, d, s)),
    'srgan_h_conv3x3_wgrad': (HALF, lambda b, d, s: (b.i(), b.i(), b.o(), N, C, C, H, W, d, s)),
    'srgan_h_pack_matrix': (HALF, lambda b, d, s: (b.i(), b.o(), C, C, C, C, C, 1, 1, 1, d, s)),
    'srgan_h_pack_matrix (transposed)': (HALF, lambda b, d, s: (b.i(), b.o(), C, C, C, C, 1, C, 1, 1, d, s)),
    'srgan_h_gemm': (HALF, lambda b, d, s: (b.i(), b.i(), None, None, 1.0, 0, b.o(), C, HW, C, C, C, d, s)),
    'srgan_h_linear_wgrad': (HALF, lambda b, d, s: (b.i(), b.i(), b.o(), HW, C, C, C, C, C, 1, 1, 1, d, s)),
    'srgan_h_pack_k4s2_weights (down)': (ANY, lambda b, d, s: (b.i(), b.o(), C, C, 0, d, s)),
    'srgan_h_pack_k4s2_weights (up)': (ANY, lambda b, d, s: (b.i(), b.o(), C, C, 1, d, s)),
    'srgan_h_conv4x4s2': (ANY, lambda b, d, s: (b.i(), b.i(), None, None, 1.0, 0, b.o(), N, C, C, H, W, d, s)),
    'srgan_h_conv_transpose4x4s2': (ANY, lambda b, d, s: (b.i(), b.i(), None, None, 1.0, 0, b.o(), N, C, C, H, W, d, s)),
    'srgan_h_k4s2_wgrad': (ANY, lambda b, d, s: (b.i(), b.i(), b.o(), N, C, C, H, W, 1, d, s)),
    'srgan_h_batch_norm_stats': (ANY, lambda b, d, s: (b.i(), b.o(), b.o(), None, None, None, 0.1, 1e-5, N, C, HW, d, s)),
    'srgan_h_batch_norm_fwd': (ANY, lambda b, d, s: (b.i(), b.i(), b.i(), b.i(), b.i(), 1.0, b.o(), N, C, HW, d, s)),
    'srgan_h_batch_norm_bwd_reduce': (ANY, lambda b, d, s: (b.i(), b.i(), b.i(), b.i(), b.o(), b.o(), b.o(), N, C, HW, d, s)),
    'srgan_h_batch_norm_bwd_apply': (ANY, lambda b, d, s: (b.i(), b.i(), b.i(), b.i(), b.i(), b.i(), None, 1.0, b.o(), N, C, HW, d, s)),
    'srgan_h_frozen_norm_bwd': (ANY, lambda b, d, s: (b.i(), b.i(), b.i(), b.i(), b.i(), None, 1.0, b.o(), b.o(), b.o(), N, C, HW, d, s)),
}

# the job fillers write HOST memory (`jobs`, and the count of the 4x4 family) and return workgroups, < 0 for an error
HOST_CALLS = {
    'srgan_h_pack_job_conv_weights': (HALF, lambda jobs, b, d, written: (jobs, 0, b.i(), b.o(), C, C, 3, 3, 0, d)),
    'srgan_h_pack_job_k4s2_weights (down)': (ANY, lambda jobs, b, d, written: (jobs, 0, b.i(), b.o(), C, C, 0, d, written)),
    'srgan_h_pack_job_k4s2_weights (up)': (ANY, lambda jobs, b, d, written: (jobs, 0, b.i(), b.o(), C, C, 1, d, written)),
    'srgan_h_pack_job_matrix': (HALF, lambda jobs, b, d, written: (jobs, 0, b.i(), b.o(), C, C, C, C, C, 1, 1, 1, d)),
}


def entry(name):
    from srgan_amd import _lib
    return getattr(_lib.library(), name.split(' ')[0])


def rejected_codes(codes):
    return BAD + tuple(code for code in ANY if code not in codes)


def test_every_blocked_entry_point_with_a_dtype_is_covered():
    """The table above against the C ABI's signature list: whatever is named srgan_h_* and takes the code is called here."""
    import re
    from srgan_amd import _build
    header = open(_build.PUBLIC_HEADER).read()
    declared = set(re.findall(r'\b(srgan_h_\w+)\([^;]*?\bdtype\b[^;]*?\);', header))
    covered = {name.split(' ')[0] for name in list(DEVICE_CALLS) + list(HOST_CALLS)}
    assert declared - {'srgan_h_k4s2_weight_slots'} == covered


@pytest.mark.parametrize('name', list(DEVICE_CALLS))
def test_a_device_entry_point_takes_its_codes_and_rejects_the_others_before_any_launch(name):
    from srgan_amd import _lib
    codes, arguments = DEVICE_CALLS[name]
    stream = _lib.stream_handle()
    for code in codes:
        buffers = Buffers()
        assert entry(name)(*arguments(buffers, code, stream)) == 0, (name, code, _lib.library().srgan_last_error())
    torch.cuda.synchronize()
    for code in rejected_codes(codes):
        buffers = Buffers()
        status = entry(name)(*arguments(buffers, code, stream))
        assert status == _lib.EINVAL, (name, code, status)
        assert _lib.library().srgan_last_error(), (name, code)
        assert buffers.untouched(), (name, code)


@pytest.mark.parametrize('name', list(HOST_CALLS))
def test_a_job_filler_takes_its_codes_and_rejects_the_others_without_writing_a_job(name):
    from srgan_amd import _lib
    codes, arguments = HOST_CALLS[name]
    job_bytes = 4 * _lib.library().srgan_h_pack_job_bytes()         # the "up" direction writes four jobs
    for code in codes + rejected_codes(codes):
        buffers = Buffers()
        jobs = ctypes.create_string_buffer(b'\xa5' * job_bytes, job_bytes)
        written = ctypes.c_int32(-7)
        result = entry(name)(*arguments(ctypes.addressof(jobs), buffers, code, ctypes.addressof(written)))
        if code in codes:
            assert result > 0 and jobs.raw != b'\xa5' * job_bytes, (name, code, result)
        else:
            assert result == _lib.EINVAL, (name, code, result)
            assert _lib.library().srgan_last_error(), (name, code)
            assert jobs.raw == b'\xa5' * job_bytes and written.value == -7, (name, code)
        assert buffers.untouched(), (name, code)                    # a job filler never touches device memory
