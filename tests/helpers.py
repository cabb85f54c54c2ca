"""Shared helpers for the test-suite (golden loading, tolerances, the contraction profile report)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name + '.npz'))


def golden_state(golden, prefix):
    """The state dict stored under ``prefix/`` as torch tensors."""
    prefix = prefix.rstrip('/') + '/'
    return {k[len(prefix):]: torch.from_numpy(np.array(golden[k])) for k in golden.files if k.startswith(prefix)}


def golden_scalars(golden, step):
    prefix = f's{step}/'
    return {k[len(prefix):]: float(golden[k]) for k in golden.files
            if k.startswith(prefix) and golden[k].ndim == 0}


def make_settings(**overrides):
    """A bare settings object with the reference's defaults for the attributes the step reads
    (reference settings.py:14-67)."""
    from oracle import functional as OF
    values = dict(batch_size=1000, learning_rate=1e-4, weight_decay=0, labeled_loss_multiplier=1.0,
                  matching_loss_multiplier=1.0, contrasting_loss_multiplier=1.0, srgan_loss_multiplier=1.0,
                  gradient_penalty_multiplier=1e1, mean_offset=0, labeled_loss_order=2,
                  generator_training_step_period=1, normalize_feature_norm=False,
                  contrasting_distance_function=OF.abs_plus_one_sqrt_mean_neg,
                  matching_distance_function=OF.abs_mean, map_multiplier=1e-6, hidden_size=10, number_of_bins=10)
    values.update(overrides)
    return SimpleNamespace(**values)


def checksum(t):
    t64 = t.detach().double().reshape(-1).cpu()
    return np.array([t64.sum().item(), t64.abs().sum().item(), t64[0].item(), t64[-1].item()])


def assert_close(actual, expected, rtol=1e-3, atol=0.0, what=''):
    actual = np.asarray(actual, dtype=np.float64)
    expected = np.asarray(expected, dtype=np.float64)
    assert actual.shape == expected.shape, f'{what}: shape {actual.shape} != {expected.shape}'
    scale = np.maximum(np.abs(expected), 1e-30)
    err = np.abs(actual - expected)
    bad = err > (atol + rtol * scale)
    assert not bad.any(), (f'{what}: {bad.sum()} of {bad.size} outside rtol={rtol} atol={atol}; '
                           f'max abs err {err.max():.3e}, max |expected| {np.abs(expected).max():.3e}')


def assert_close_norm(actual, expected, rtol=1e-3, what=''):
    """Relative error measured against the tensor's max magnitude (for tensors with near-zero entries)."""
    actual = np.asarray(actual, dtype=np.float64)
    expected = np.asarray(expected, dtype=np.float64)
    assert actual.shape == expected.shape, f'{what}: shape {actual.shape} != {expected.shape}'
    denom = max(np.abs(expected).max(), 1e-30)
    err = np.abs(actual - expected).max() / denom
    assert err <= rtol, f'{what}: max err / max|expected| = {err:.3e} > {rtol}'


def assert_exact(got, want, what, dims=('n', 'c', 'h', 'w')):
    """got (device fp32) == want (float64) exactly; on a mismatch: how many, the first eight with got / want, and which
    indices of every dimension (channels, rows, pixels) the mismatches fall in."""
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} != {tuple(want.shape)}'
    bad = ~(got == want)
    if not bool(bad.any()):
        return
    where = bad.nonzero()
    lines = [f'{what}: {where.shape[0]} of {got.numel()} elements differ (shape {tuple(got.shape)})']
    for index in where[:8].tolist():
        lines.append(f'  {dict(zip(dims, index))}: got {got[tuple(index)].item()!r} want {want[tuple(index)].item()!r}')
    for axis, name in enumerate(dims[:got.dim()]):
        values = torch.unique(where[:, axis]).tolist()
        shown = values[:24]
        lines.append(f'  {name}: {len(values)} of {got.shape[axis]} distinct {shown}{" ..." if len(values) > len(shown) else ""}')
    raise AssertionError('\n'.join(lines))


def _check(status, what):
    from srgan_amd import _lib
    _lib.check(status, what)


class profiled:
    """srgan_profile_begin ... srgan_profile_end around a block; .lines = the report's (M, N, K, kind, bm, bn, split) rows."""

    def __init__(self, lib):
        self.lib, self.lines, self.text = lib, [], ''

    def __enter__(self):
        _check(self.lib.srgan_profile_begin(), 'srgan_profile_begin')
        return self

    def __exit__(self, kind, *rest):
        ms, flops, mfma, launches = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _check(self.lib.srgan_profile_end(ctypes.byref(ms), ctypes.byref(flops), ctypes.byref(mfma), ctypes.byref(launches)),
               'srgan_profile_end')
        size = self.lib.srgan_profile_report(None, 0)
        buffer = ctypes.create_string_buffer(int(size) + 1)
        self.lib.srgan_profile_report(buffer, size + 1)
        self.text = buffer.value.decode()
        for line in self.text.splitlines():
            fields = line.split()
            if len(fields) >= 7 and not line.startswith('#'):
                self.lines.append(tuple(int(v) for v in fields[:7]))
        return False

    @property
    def kinds(self):
        return {line[3] for line in self.lines}

    def assert_reached(self, reach, split, what):
        from contraction_cases import KINDS, KINDS16
        names = {**KINDS, **KINDS16}
        missing = sorted(set(reach) - self.kinds)
        assert not missing, (f'{what}: declared kinds {[names[k] for k in missing]} not launched; launched '
                             f'{ {k: names.get(k, str(k)) for k in self.kinds} }\n'
                             f'M N K kind bm bn split ...\n{self.text}')
        if split:
            assert any(line[3] in reach and line[6] > 1 for line in self.lines), \
                f'{what}: no launch of {sorted(reach)} with split > 1\nM N K kind bm bn split ...\n{self.text}'


# ---- device buffers of the per-element kernel tests (test_streaming_ops_gpu.py, test_blocked_streaming_gpu.py) -------------
GUARD = 64
PATTERN = 0x4B3C2D1E            # the guard floats' bits (a finite fp32, 12332318.0)


class Guarded:
    """`n` elements `offset` floats past a 16-byte boundary inside a device buffer, GUARD pattern words on each side."""

    def __init__(self, n, init=float('nan'), offset=0, dtype=torch.float32):
        self.n, self.lo = int(n), GUARD + offset
        self.buffer = torch.full((self.lo + self.n + GUARD,), PATTERN, dtype=torch.int32, device='cuda')
        assert self.buffer.data_ptr() % 16 == 0
        self.window = self.buffer.view(dtype)[self.lo:self.lo + self.n]
        if torch.is_tensor(init):
            self.window.copy_(init.reshape(-1).to(dtype))
        else:
            self.window.fill_(init)

    @property
    def ptr(self):
        return self.window.data_ptr()

    def at(self, element):
        return self.window.data_ptr() + 4 * int(element)

    def halves(self):
        """The window as 16-bit words (two per element): a window of blocked bf16 / fp16 slots."""
        return self.window.view(torch.int16)

    def result(self, what, shape=None):
        """The window after the call; the guards must be bit-unchanged."""
        torch.cuda.synchronize()
        bits = self.buffer.cpu()
        for name, band in (('below', bits[:self.lo]), ('above', bits[self.lo + self.n:])):
            touched = (band != PATTERN).nonzero().flatten().tolist()
            assert not touched, f'{what}: {len(touched)} guard words {name} the window were written, first at {touched[:8]}'
        return self.window.reshape(shape) if shape is not None else self.window


def device(t, offset=0):
    """A device copy (fp32) that starts `offset` floats past a 16-byte boundary; None stays None."""
    if t is None:
        return None
    holder = torch.empty(t.numel() + 4, device='cuda')
    assert holder.data_ptr() % 16 == 0
    view = holder[offset:offset + t.numel()]
    view.copy_(t.reshape(-1).float())
    return view


def ptr(t):
    return None if t is None else t.data_ptr()
