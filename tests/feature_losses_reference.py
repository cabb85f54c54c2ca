"""NumPy fp64 restatement of the alternative feature losses (srgan_amd.srgan: feature_angle_loss,
feature_distance_loss_unmeaned, feature_distance_loss_both_unmeaned, feature_covariance_loss), value and both input gradients,
written from their contracts.  test_feature_losses_cpu.py pins it to the fixture recorded from the reference
(golden/g19_feature_losses.npz); the GPU tests use it where the fixture has no case (one changed column, swapped arguments,
F = 8192).  The correlation loss works on blocks of rows of the F x F matrices: nothing of that size is ever allocated.

Rules of the correlation loss (include/srgan_hip.h, srgan_feature_corrcoef_l1_fwd): the diagonal contributes exactly 0; an
entry whose unclamped value lies strictly outside [-1, 1] is clamped and passes no gradient on its side; a feature without
variance makes the loss and the gradients NaN.
"""
import numpy as np

ANGLE_EPSILON, UNIT_EPSILON = 1e-6, 1e-10


def _f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float64) for a in arrays)


def _unit(vector):
    norm = np.sqrt((vector * vector).sum())
    return vector / (norm + UNIT_EPSILON), norm


def _unit_backward(vector, norm, g_unit):
    """Gradient of vector / (|vector| + eps) applied to ``g_unit``."""
    return g_unit / (norm + UNIT_EPSILON) - vector * (vector @ g_unit) / (norm * (norm + UNIT_EPSILON) ** 2)


def angle_between(vector0, vector1):
    vector0, vector1 = _f64(vector0, vector1)
    cosine = _unit(vector0)[0] @ _unit(vector1)[0]
    return np.arccos(np.clip(cosine, -1.0 + ANGLE_EPSILON, 1.0 - ANGLE_EPSILON))


def angle_loss(base, other, target=0.0):
    """(loss, grad_base, grad_other) of |angle(mean_b base, mean_b other) - target|^2."""
    base, other = _f64(base, other)
    mean_b, mean_o = base.mean(0), other.mean(0)
    (unit_b, norm_b), (unit_o, norm_o) = _unit(mean_b), _unit(mean_o)
    cosine = unit_b @ unit_o
    low, high = -1.0 + ANGLE_EPSILON, 1.0 - ANGLE_EPSILON
    clamped = min(max(cosine, low), high)
    angle = np.arccos(clamped)
    g_cosine = 2.0 * (angle - target) * (-1.0 / np.sqrt(1.0 - clamped * clamped)) * (1.0 if low <= cosine <= high else 0.0)
    g_mean_b = _unit_backward(mean_b, norm_b, g_cosine * unit_o)
    g_mean_o = _unit_backward(mean_o, norm_o, g_cosine * unit_b)
    rows = base.shape[0]
    return (angle - target) ** 2, np.tile(g_mean_b / rows, (rows, 1)), np.tile(g_mean_o / other.shape[0], (other.shape[0], 1))


def unmeaned_loss(base, other):
    """mean((mean_b base - other)^2): (loss, grad_base, grad_other)."""
    base, other = _f64(base, other)
    difference = base.mean(0, keepdims=True) - other
    g_difference = 2.0 * difference / difference.size
    return (difference ** 2).mean(), np.tile(g_difference.sum(0) / base.shape[0], (base.shape[0], 1)), -g_difference


def both_unmeaned_loss(base, other):
    """mean_b sum_f (base - other)^2: (loss, grad_base, grad_other)."""
    base, other = _f64(base, other)
    difference = base - other
    g_difference = 2.0 * difference / base.shape[0]
    return (difference ** 2).sum(1).mean(), g_difference, -g_difference


class _Side:
    def __init__(self, x):
        self.n = x.shape[0]
        self.xm = x - x.mean(0, keepdims=True)
        self.variance = (self.xm * self.xm).sum(0) / (self.n - 1)
        with np.errstate(invalid='ignore', divide='ignore'):
            self.stddev = np.sqrt(self.variance)

    def rows(self, first, last):
        """(unclamped, clamped) rows [first, last) of the correlation matrix."""
        with np.errstate(invalid='ignore', divide='ignore'):
            raw = self.xm[:, first:last].T @ self.xm / (self.n - 1)
            raw = raw / self.stddev[None, :] / self.stddev[first:last, None]
        return raw, np.where(raw > 1.0, 1.0, np.where(raw < -1.0, -1.0, raw))


def corrcoef_rows(x, first, last):
    """Rows [first, last) of the clamped correlation matrix of the columns of x [B, F]."""
    return _Side(_f64(x)[0]).rows(first, last)[1]


def covariance_loss(base, other, gradients=True, block=256):
    """sum_{i != j} |Cb_ij - Co_ij|: (loss, grad_base, grad_other), the gradients None without ``gradients``."""
    base, other = _f64(base, other)
    sides = (_Side(base), _Side(other))
    features = base.shape[1]
    loss = 0.0
    grads = [np.zeros_like(base), np.zeros_like(other)] if gradients else [None, None]
    for first in range(0, features, block):
        last = min(features, first + block)
        (raw_b, clamped_b), (raw_o, clamped_o) = sides[0].rows(first, last), sides[1].rows(first, last)
        difference = clamped_b - clamped_o
        diagonal = (np.arange(first, last) - first, np.arange(first, last))
        difference[diagonal] = 0.0
        loss += np.abs(difference).sum()
        if not gradients:
            continue
        sign = np.sign(difference)                                   # (NaN stays NaN)
        for side, raw, clamped, factor in ((sides[0], raw_b, clamped_b, 1.0), (sides[1], raw_o, clamped_o, -1.0)):
            with np.errstate(invalid='ignore', divide='ignore'):
                g = factor * sign * np.where(np.abs(raw) > 1.0, 0.0, 1.0)
                g[diagonal] = 0.0
                r = (g * clamped).sum(1)
                weights = g / side.stddev[None, :] / side.stddev[first:last, None]
                d_xm = (2.0 / (side.n - 1)) * (weights @ side.xm.T - (r / side.variance[first:last])[:, None] * side.xm[:, first:last].T)
            grads[0 if factor > 0 else 1][:, first:last] = (d_xm - d_xm.mean(1, keepdims=True)).T
    return loss, grads[0], grads[1]


LOSSES = {'angle': angle_loss, 'unmeaned': unmeaned_loss, 'both_unmeaned': both_unmeaned_loss, 'covariance': covariance_loss}
