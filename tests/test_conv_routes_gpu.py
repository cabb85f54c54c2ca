"""Every convolution / GEMM entry point launches what tests/golden/conv_routes.json recorded: the same kernels (kind), tiles,
K splits, staging flags, launch counts and algorithmic bytes, and the same answers from the query entry points.  The calls are
the list of conv_route_cases.py, replayed once per module; golden/make_conv_route_goldens.py recorded them at the commit before
the routing code moved into conv_dispatch.hip."""
import json
import os

import pytest
import torch
import torch.nn.functional as TF

import conv_route_cases
from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def replayed():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return conv_route_cases.replay(_lib.library())


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN_DIR, 'conv_routes.json')) as handle:
        return json.load(handle)


def test_the_golden_has_every_group(golden):
    assert sorted(golden) == sorted(conv_route_cases.GROUPS)


@pytest.mark.parametrize('group', conv_route_cases.GROUPS)
def test_every_call_routes_as_recorded(replayed, golden, group):
    routes, _ = replayed
    got, want = routes[group], golden[group]
    assert sorted(got) == sorted(want), f'{group}: the cases differ'
    wrong = []
    for case in sorted(want):
        assert sorted(got[case]) == sorted(want[case]), f'{group} {case}: the calls differ'
        for call in sorted(want[case]):
            if got[case][call] != want[case][call]:
                wrong.append(f'{group} {case} {call}:\n    recorded {want[case][call]}\n    now      {got[case][call]}')
    assert not wrong, (f'{len(wrong)} calls route differently ([status, "M N K kind bm bn split akf bkf count bytes", ...]):\n'
                       + '\n'.join(wrong[:20]))


def test_the_slice_call_takes_both_combines(golden):
    """The recorded pair is what the case is for: an ordered K split with the workspace, the same split with fp32 atomics (the
    row-wise zero fill in front) without."""
    calls = golden['slice'][conv_route_cases.conv_name(conv_route_cases.SLICE_SHAPE)]
    for name, ordered in (('default_stream', 1), ('unregistered_stream', 0)):
        status, *lines = calls[name]
        assert status == 0 and len(lines) == 1, calls[name]
        fields = lines[0].split()
        assert int(fields[3]) == 1 and int(fields[6]) > 1, f'{name}: not a K split of the generic MFMA kernel: {lines[0]}'
        assert calls[name + '/split_is_ordered'] == [ordered]


def test_the_slice_outputs_are_exact_on_both_streams(replayed):
    """The forward into 20 channels of a 24-channel buffer on exact integer operands: the stream without a workspace (atomics into
    rows zeroed one image at a time) gives the bits of the default stream, both give float64's, and the four channels beyond the
    view keep their fill."""
    _, outputs = replayed
    x, weight = conv_route_cases.slice_operands()
    n, c, h, w, k, r, s, stride, pad = conv_route_cases.SLICE_SHAPE
    want = torch.full(outputs['default_stream'].shape, conv_route_cases.SLICE_FILL, dtype=torch.float64)
    want[:, :k] = TF.conv2d(x, weight, None, stride, pad)
    assert float(TF.conv2d(x.abs(), weight.abs(), None, stride, pad).max()) < 2 ** 24
    ordered, atomic = outputs['default_stream'].cpu(), outputs['unregistered_stream'].cpu()
    assert torch.equal(atomic, ordered), f'{int((atomic != ordered).sum())} elements differ between the streams'
    assert torch.equal(ordered.double(), want), f'{int((ordered.double() != want).sum())} elements differ from float64'
