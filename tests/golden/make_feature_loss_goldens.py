"""Generate tests/golden/g19_feature_losses.npz by calling the UNMODIFIED upstream reference's alternative feature losses on CPU.

Test infrastructure only, like make_goldens.py: it needs the reference checkout and never travels to the GPU box; the emitted
fixture holds data only.  For every shape (B, F) the inputs are drawn in fp32 from ``torch.Generator().manual_seed(seed)`` --
``base = randn(B, F)``, ``other = 1.5 * randn(B, F) + 0.3`` -- and stored as fp32, so that the device gets bit for bit what the
reference got; the reference then runs on their fp64 copies (recorded as float64) and once more in float32 (``*_f32``).
Recorded per shape under ``<B>x<F>/``: ``seed``, ``base``, ``other``, ``min_gap`` (the smallest off-diagonal
``|Cb_ij - Co_ij|`` in fp64) and per loss ``<loss>/value``, ``<loss>/value_f32``, and -- where gradients are recorded --
``<loss>/grad_base``, ``<loss>/grad_other`` from ``loss.backward()`` plus, for the correlation loss, ``*_f32`` of both.

Shapes.  The fused kernel works on 32 features per wave, 128 per workgroup, 16 batch elements per MFMA step, a batch padded to
32, and 128 examples per workgroup of the backward; the gradient shapes cross each of these from below:
(3, 5), (5, 33), (17, 70), (130, 40), (8, 300), (33, 130); loss only: (2, 3), (70, 259).  The composed losses' gradients are
recorded where B * F <= 2500 (the file stays under the repository's size limit); their values everywhere.

The sign matrix makes the correlation loss's gradient discontinuous, so for every gradient shape the seeds 0, 1, ... are searched
for the first one whose ``min_gap`` is >= 1e-5 (64 tries, else an error): the reference's fp32 per-entry error is a few 1e-7.

``parallel/``: (5, 33) with ``other = 2 * base``: the two batch means are parallel and ``angle_between`` sits on its clamp.
Usage::

    python tests/golden/make_feature_loss_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstubs  # noqa: E402

_refstubs.install()

import torch  # noqa: E402

import make_goldens  # noqa: E402  (its save())
import srgan as ref_srgan  # noqa: E402

GRADIENT_SHAPES = ((3, 5), (5, 33), (17, 70), (130, 40), (8, 300), (33, 130))
LOSS_ONLY_SHAPES = ((2, 3), (70, 259))
MIN_GAP, SEEDS, COMPOSED_GRADIENT_ELEMENTS = 1e-5, 64, 2500
LOSSES = {'angle': ref_srgan.feature_angle_loss, 'unmeaned': ref_srgan.feature_distance_loss_unmeaned,
          'both_unmeaned': ref_srgan.feature_distance_loss_both_unmeaned, 'covariance': ref_srgan.feature_covariance_loss}


def draw(seed, b, f):
    generator = torch.Generator().manual_seed(seed)
    base = torch.randn(b, f, generator=generator)
    other = 1.5 * torch.randn(b, f, generator=generator) + 0.3
    return base, other


def min_gap(base, other):
    difference = (ref_srgan.feature_corrcoef(base.double()) - ref_srgan.feature_corrcoef(other.double())).abs()
    difference.fill_diagonal_(float('inf'))
    return float(difference.min())


def evaluate(function, base, other, dtype, gradients):
    base, other = (t.detach().to(dtype).clone().requires_grad_(gradients) for t in (base, other))
    loss = function(base, other)
    if gradients:
        loss.backward()
    return (loss.detach().numpy(), base.grad.numpy() if gradients else None, other.grad.numpy() if gradients else None)


def record(out, key, base, other, gradients, skip=()):
    out[f'{key}/base'], out[f'{key}/other'] = base.numpy(), other.numpy()
    out[f'{key}/min_gap'] = np.array(min_gap(base, other))
    for name, function in LOSSES.items():
        if name in skip:
            continue
        with_grads = gradients and (name == 'covariance' or base.numel() <= COMPOSED_GRADIENT_ELEMENTS)
        value, grad_base, grad_other = evaluate(function, base, other, torch.float64, with_grads)
        value32, grad_base32, grad_other32 = evaluate(function, base, other, torch.float32, with_grads)
        out[f'{key}/{name}/value'], out[f'{key}/{name}/value_f32'] = value, value32
        if with_grads:
            out[f'{key}/{name}/grad_base'], out[f'{key}/{name}/grad_other'] = grad_base, grad_other
            if name == 'covariance':
                out[f'{key}/{name}/grad_base_f32'], out[f'{key}/{name}/grad_other_f32'] = grad_base32, grad_other32


def main():
    out = {'gradient_shapes': np.array(GRADIENT_SHAPES), 'loss_only_shapes': np.array(LOSS_ONLY_SHAPES)}
    for b, f in GRADIENT_SHAPES:
        for seed in range(SEEDS):
            base, other = draw(seed, b, f)
            if min_gap(base, other) >= MIN_GAP:
                break
        else:
            raise SystemExit(f'no seed below {SEEDS} keeps every entry of ({b}, {f}) {MIN_GAP} away from a sign flip')
        out[f'{b}x{f}/seed'] = np.array(seed)
        record(out, f'{b}x{f}', base, other, gradients=True)
        print(f'({b}, {f}): seed {seed}, min gap {float(out[f"{b}x{f}/min_gap"]):.3e}')
    for b, f in LOSS_ONLY_SHAPES:
        out[f'{b}x{f}/seed'] = np.array(0)
        record(out, f'{b}x{f}', *draw(0, b, f), gradients=False)
    base, _ = draw(0, 5, 33)
    out['parallel/seed'] = np.array(0)
    record(out, 'parallel', base, 2.0 * base, gradients=True, skip=('covariance',))   # (equal matrices: every sign is noise)
    make_goldens.save('g19_feature_losses', **out)


if __name__ == '__main__':
    main()
