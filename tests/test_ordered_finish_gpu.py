"""The ORDER in which the workgroups of a row meet (csrc/split_finish.h), pinned bit for bit against a NumPy fp32 restatement that
never calls the library: thread t of the last workgroup adds the parts t, t + 256, ... starting from 0, the 64 lanes of a wave
meet in the xor butterfly with offsets 32 ... 1, and the four waves in a tree --

    ordered_row_finish   ((w0 + w1) + w2) + w3     the tree of block_sum_256    srgan_chan_reduce
    ordered_lane_finish  (w0 + w1) + (w2 + w3)                                  srgan_h_frozen_norm_bwd, the sums

The inputs make every workgroup's OWN partial exact, so that only the cross-workgroup order decides the bits: one non-zero value
per image and channel (``randn * 2 ** randint(-8, 8)``, rounded to the storage type), every image in a workgroup of its own.  One
exception the grid rules make: the frozen kernel at C = 5 in blocked fp32 (two channel groups) takes TWO images per workgroup from
N = 255 on; its two values sit in two lanes of one wave and meet in a single fp32 addition, which no order can change, and the
restatement adds them likewise.  For the frozen kernel x = 1 at that pixel, ``mean`` is NULL and inv_std = gamma = 1: no multiply can
contract into an add.  The stream's workspace is full of NaN in front of every launch.

N = 2 and 5 (one wave), 256 (every thread one part), 257 and 300 (the ``s += 256`` wrap of the finishing loop).  That the test can
tell the orders apart is checked on the CPU: from N = 256 on the two trees and a sum in float64, rounded once, give three different
results for the seeds used (``draw`` steps a seed for which they agree; with two images per workgroup only two waves hold parts
and the trees coincide).  (The statistics kernels multiply inside Chan's merge, where contraction to fma is the compiler's choice:
their 300-part cases are held to fp64 in test_blocked_batch_norm_gpu.py and test_batch_norm_train_gpu.py instead.)"""
import numpy as np
import pytest
import torch

from helpers import profiled
from test_blocked_batch_norm_gpu import CODES, TORCH, _call, _stream, group, to_blocked

BATCHES = [2, 5, 256, 257, 300]
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
def lane_tree(w):
    return f32(f32(w[0] + w[1]) + f32(w[2] + w[3]))


def legacy_tree(w):
    return f32(f32(f32(w[0] + w[1]) + w[2]) + w[3])


def finish(partials, tree):
    """The total of one value: ``partials`` [parts] in fp32, in the order of the last workgroup's 256 threads."""
    partials = np.asarray(partials, dtype=f32)
    threads = np.zeros(256, dtype=f32)
    for t in range(min(256, len(partials))):
        for s in range(t, len(partials), 256):
            threads[t] = f32(threads[t] + partials[s])
    waves = []
    for wave in threads.reshape(4, 64):
        lanes = wave.copy()
        for offset in (32, 16, 8, 4, 2, 1):
            lanes = (lanes + lanes[np.arange(64) ^ offset]).astype(f32)
        waves.append(lanes[0])
    return tree(waves)


def workgroup_partials(values, per):
    """[N, C] values -> [parts, C]: a workgroup of ``per`` <= 2 images adds its two values in one fp32 addition."""
    assert per in (1, 2)
    if per == 1:
        return values
    padded = np.concatenate([values, np.zeros((len(values) % 2, values.shape[1]), dtype=f32)])
    return (padded[0::2] + padded[1::2]).astype(f32)


def totals(values, per, tree):
    partials = workgroup_partials(values, per)
    return np.array([finish(partials[:, c], tree) for c in range(values.shape[1])], dtype=f32)


def rounded_once(values):
    return values.astype(np.float64).sum(axis=0).astype(f32)


def told_apart(values, per):
    """The two trees and a float64 sum rounded once give different results (the trees: where all four waves hold parts)."""
    legacy, lane, once = (bits(r).tobytes() for r in (totals(values, per, legacy_tree), totals(values, per, lane_tree), rounded_once(values)))
    parts = (len(values) + per - 1) // per
    return legacy != once and lane != once and (legacy != lane or parts <= 192)


def draw(n, c, dtype, seed, per=1):
    """[N, C] values of the storage type, and the generator for the pixel of each.  From N = 256 on the seed is stepped until the
    restatement tells the orders apart (decided by the restatement alone)."""
    while True:
        generator = torch.Generator().manual_seed(seed)
        values = torch.randn(n, c, generator=generator) * 2.0 ** torch.randint(-8, 9, (n, c), generator=generator).float()
        values = values.to(dtype).float()
        if n < 256 or told_apart(values.numpy(), per):
            return values, generator
        seed += 7919


def frozen_images_per_workgroup(n, c, hw, code):
    """The host's rule at these sizes (blocked16_batch_norm.hip): one image, doubled while that leaves 256 workgroups."""
    groups, per = (c + group(code) - 1) // group(code), 1
    assert groups * n < 1024 and hw < 4096
    while per < n and groups * ((n + 2 * per - 1) // (2 * per)) >= 256:
        per *= 2
    return per


def bits(a):
    return np.asarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ on the CPU
def test_the_restatement_tells_the_orders_apart():
    """From N = 256 on (all four waves hold parts) the two trees and the float64 sum differ for the values the device tests use."""
    for n in (256, 257, 300):
        cases = [(draw(n, 2, torch.float32, 100 + n)[0], 1)]
        for code in CODES:
            for c in (3, 5):
                per = frozen_images_per_workgroup(n, c, 4, code)
                cases.append((draw(n, c, TORCH[code], 1000 * code + 10 * n + c, per)[0], per))
        for values, per in cases:
            assert told_apart(values.numpy(), per), (n, values.shape, per)
        assert sum(per == 1 for _, per in cases) >= 6              # the four-wave trees are told apart in all but C = 5, code 0
    assert frozen_images_per_workgroup(300, 5, 4, 0) == 2 and frozen_images_per_workgroup(300, 5, 4, 1) == 1
    assert frozen_images_per_workgroup(254, 5, 4, 0) == 1 and frozen_images_per_workgroup(300, 3, 4, 0) == 1


# ------------------------------------------------------------------------------------------------ on the device
@pytest.fixture(scope='module')
def workspace():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    assert torch.cuda.is_available()
    return _lib._workspaces[(torch.cuda.current_device(), _lib.stream_handle())]


@pytest.mark.gpu
@pytest.mark.parametrize('n', BATCHES)
def test_chan_reduce_meets_in_part_order_and_the_legacy_tree(workspace, n):
    """``srgan_chan_reduce`` at C = 2, HW = 8: N workgroups per channel (one run of the row each)."""
    c, hw = 2, 8
    values, generator = draw(n, c, torch.float32, 100 + n)
    pixel = torch.randint(0, hw, (n, c), generator=generator)
    a = torch.zeros(n, c, hw).scatter_(2, pixel.unsqueeze(2), values.unsqueeze(2)).cuda()
    out = torch.full((c,), float('nan'), device='cuda')
    workspace.fill_(float('nan'))
    _call('srgan_chan_reduce', a.data_ptr(), None, None, None, out.data_ptr(), n, c, hw, 0, _stream())
    want = totals(values.numpy(), 1, legacy_tree)
    print(f'chan_reduce N {n}: got {out.cpu().numpy()} want {want}')
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize('n', BATCHES)
@pytest.mark.parametrize('c', [3, 5])
@pytest.mark.parametrize('code', CODES)
def test_frozen_norm_sums_meet_in_part_order_and_the_lane_tree(workspace, code, c, n):
    """``srgan_h_frozen_norm_bwd``, sums only: g_beta alone (V = g values) and g_gamma + g_beta (V = 2 g) at HW = 4.  The number
    of workgroups per channel group is read from the launch's profile record (kind 24: its `split` field)."""
    from srgan_amd import _lib
    shape = (n, c, 2, 2)
    per = frozen_images_per_workgroup(n, c, 4, code)
    values, generator = draw(n, c, TORCH[code], 1000 * code + 10 * n + c, per)
    pixel = torch.randint(0, 4, (n, c), generator=generator)
    s = torch.zeros(n, c, 4).scatter_(2, pixel.unsqueeze(2), values.unsqueeze(2)).view(shape)
    x = torch.zeros(n, c, 4).scatter_(2, pixel.unsqueeze(2), torch.ones(n, c, 1)).view(shape)
    sb, xb = to_blocked(s, code), to_blocked(x, code)
    ones = torch.ones(c, device='cuda')
    want = totals(values.numpy(), per, lane_tree)
    for with_gamma in (False, True):
        gamma_grad, beta_grad = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
        workspace.fill_(float('nan'))
        with profiled(_lib.library()) as report:
            _call('srgan_h_frozen_norm_bwd', sb.data_ptr(), xb.data_ptr() if with_gamma else None, None, ones.data_ptr(), ones.data_ptr(),
                  None, 1.0, None, gamma_grad.data_ptr() if with_gamma else None, beta_grad.data_ptr(), n, c, 4, code, _stream())
            torch.cuda.synchronize()
        launches = [line for line in report.lines if line[3] == 24]
        assert [line[6] for line in launches] == [(n + per - 1) // per], report.text
        print(f'frozen code {code} C {c} N {n} gamma {with_gamma}: got {beta_grad.cpu().numpy()} want {want}')
        assert np.array_equal(bits(beta_grad.cpu().numpy()), bits(want))
        if with_gamma:
            assert np.array_equal(bits(gamma_grad.cpu().numpy()), bits(want))
