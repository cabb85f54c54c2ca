"""NumPy float64 restatement of ``srgan_regression_evaluation_sums`` (include/srgan_hip.h) and of the scalars
``Experiment.regression_validation_summaries`` logs from an epoch's record -- written from the contract, for the tests of
test_regression_validation_cpu.py / test_regression_validation_gpu.py.  Shared helper module, no tests of its own."""
import numpy as np

EMPTY_RECORD = (0.0, 0.0, 0.0, 0.0, np.inf, -np.inf, 0.0, 0.0)          # an epoch's eight doubles before its first batch


def row_predictions(predictions, row_stride, K, bins):
    """The fp32 prediction of every row of the flat ``predictions`` (row b starts at ``b * row_stride``): the row's value
    (``bins`` None, K == 1) or the bin of the LOWEST index of the row's maximum."""
    flat = np.asarray(predictions, dtype=np.float32).reshape(-1)
    if K < 1 or row_stride < K or (bins is None and K != 1):
        raise ValueError('K >= 1, row_stride >= K, and K > 1 needs the bins')
    rows = 0 if flat.size == 0 else (flat.size - K) // row_stride + 1
    table = np.stack([flat[b * row_stride:b * row_stride + K] for b in range(rows)]) if rows else np.zeros((0, K), np.float32)
    if bins is None:
        return table[:, 0]
    return np.asarray(bins, dtype=np.float32).reshape(-1)[np.argmax(table, axis=1)]        # np.argmax: the first occurrence


def evaluation_sums(predictions, row_stride, K, bins, labels, sums=None):
    """The eight doubles after one call: ``sums`` (default ``EMPTY_RECORD``) updated with the batch's terms; ``sums[6:]`` are
    passed through.  ``labels [B]`` fixes the number of rows read from ``predictions``."""
    out = np.array(EMPTY_RECORD if sums is None else sums, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.float32).reshape(-1)
    if labels.size == 0:
        return out
    predicted = row_predictions(predictions, row_stride, K, bins)[:labels.size]
    assert predicted.size == labels.size
    difference = predicted.astype(np.float64) - labels.astype(np.float64)
    out[0] += difference.sum()
    out[1] += np.abs(difference).sum()
    out[2] += (difference * difference).sum()
    out[3] += labels.size
    out[4] = min(out[4], float(labels.min()))
    out[5] = max(out[5], float(labels.max()))
    return out


def evaluation_scalars(sums, comparison_value=None, normalized=False):
    """``[(tag suffix, value)]`` in logging order from a record; NMAE with ``normalized``, the ratio with a comparison."""
    sums = np.asarray(sums, dtype=np.float64)
    mae = float(sums[1] / sums[3])
    scalars = [('MAE', mae)]
    if normalized:
        scalars.append(('NMAE', mae / float(sums[5] - sums[4])))
    scalars.append(('MSE', float(sums[2] / sums[3])))
    if comparison_value is not None:
        scalars.append(('Ratio MAE GAN DNN', mae / comparison_value))
    return scalars


def order_bounds(predictions, row_stride, K, bins, labels):
    """Per sum, how far two fp64 evaluations that add the same terms in different orders can lie apart: ``n * 2^-53 * sum
    |terms|`` with ``n = B`` terms (Higham, Accuracy and Stability, (4.4), as ``order_bounds`` of crowd_validation_reference.py
    argues it).  Every term -- d_b, |d_b|, fl(d_b * d_b) -- is identical in both evaluations: d_b is ONE exactly rounded fp64
    subtraction of two fp32 values, the square one rounded product.  The count, the minimum and the maximum are exact."""
    labels = np.asarray(labels, dtype=np.float32).reshape(-1)
    predicted = row_predictions(predictions, row_stride, K, bins)[:labels.size]
    difference = predicted.astype(np.float64) - labels.astype(np.float64)
    u, n = 2.0 ** -53, labels.size
    bounds = np.zeros(8, dtype=np.float64)
    bounds[0] = bounds[1] = n * u * np.abs(difference).sum()
    bounds[2] = n * u * (difference * difference).sum()
    return bounds
