"""NumPy float64 restatement of ``srgan_crowd_evaluation_sums`` (include/srgan_hip.h) and of the six scalars
``CrowdExperiment.evaluation_epoch_device`` logs from its sums -- written from the contract, for the tests of
test_crowd_validation_cpu.py / test_crowd_validation_gpu.py.  Shared helper module, no tests of its own."""
import numpy as np

TAGS = ('ME', 'MAE', 'kNN MAE', 'MSE', 'kNN MSE')          # the order evaluation_epoch logs them in


def evaluation_sums(predicted_counts, labels, predicted_maps=None, maps=None, sums=None):
    """The eight doubles after one call: ``sums`` (default zeros) plus the batch's terms; ``sums[7]`` is passed through.
    predicted_counts [B], labels [B, HW], predicted_maps [B, M, HW] and maps [B, HW] (both or neither)."""
    out = np.zeros(8, dtype=np.float64) if sums is None else np.array(sums, dtype=np.float64)
    if (predicted_maps is None) != (maps is None):
        raise ValueError('predicted_maps and maps are given together or not at all')
    labels = np.asarray(labels, dtype=np.float64)
    if labels.shape[0] == 0 or labels[0].size == 0:
        return out
    difference = np.asarray(predicted_counts, dtype=np.float64).reshape(-1) - labels.reshape(labels.shape[0], -1).sum(axis=1)
    out[0] += difference.sum()
    out[1] += np.abs(difference).sum()
    out[2] += (difference * difference).sum()
    out[3] += labels.shape[0]
    if maps is not None:
        error = np.asarray(predicted_maps, dtype=np.float64) - np.asarray(maps, dtype=np.float64)[:, None]
        out[4] += np.abs(error).sum()
        out[5] += (error * error).sum()
        out[6] += error.size
    return out


def evaluation_scalars(sums, comparison_value=None):
    """``[(tag suffix, value)]`` in logging order from the eight sums; the ratio is appended when a comparison is given."""
    sums = np.asarray(sums, dtype=np.float64)
    mae = sums[1] / sums[3]
    scalars = [('ME', sums[0] / sums[3]), ('MAE', mae), ('kNN MAE', sums[4] / sums[6]), ('MSE', sums[2] / sums[3]),
               ('kNN MSE', sums[5] / sums[6])]
    if comparison_value is not None:
        scalars.append(('Ratio MAE GAN DNN', mae / comparison_value))
    return scalars


def contraction_case(a, plane=1, batch=17, channels=2):
    """A batch on which a square rounded BEFORE it is added and a fused multiply-add give different bits, and what each
    gives.  x = a * 2^-30 (a odd, below 2^24: exact in fp32); two errors e1 = 1 - x and e2 = 1.5 - x carry 30 significant
    bits, so their squares are not exact in fp64.  Example 0 has predicted maps (1, 1.5) against the map value x at element 0,
    and the count 1 against a label patch that sums to x; example ``batch - 1`` has the count 1.5 against x; everything else
    is zero, so every other addition is exact and the order of the additions cannot matter.  With ``batch`` = 17 both count
    differences meet in the same thread of the finish kernel, as the two map errors do in thread 0 of the partials kernel.
    Returns ``(inputs, unfused, fused)``: ``unfused = fl(fl(e1 * e1) + fl(e2 * e2))`` is what sums[2] and sums[5] must be,
    ``fused = fl(fl(e1 * e1) + e2 * e2)`` what a contracted ``sum += e * e`` would leave."""
    from fractions import Fraction
    x = np.float32(a * 2.0 ** -30)
    assert float(x) == a * 2.0 ** -30
    e1, e2 = 1.0 - float(x), 1.5 - float(x)
    unfused = e1 * e1 + e2 * e2
    fused = float(Fraction(e1 * e1) + Fraction(e2) * Fraction(e2))           # one rounding, of the exact value
    counts = np.zeros(batch, dtype=np.float32)
    labels = np.zeros((batch, plane), dtype=np.float32)
    maps = np.zeros((batch, plane), dtype=np.float32)
    predicted = np.zeros((batch, channels, plane), dtype=np.float32)
    counts[0], counts[-1] = 1.0, 1.5
    labels[0, 0] = labels[-1, 0] = maps[0, 0] = x
    predicted[0, 0, 0], predicted[0, 1, 0] = 1.0, 1.5
    return (counts, labels, predicted, maps), unfused, fused


def contraction_cases(count=4, plane=1):
    """The first ``count`` odd ``a`` from 3 on whose case tells the two forms apart, as ``contraction_case`` results."""
    cases = []
    a = 3
    while len(cases) < count:
        case = contraction_case(a, plane)
        if case[1] != case[2]:
            cases.append(case)
        a += 2
    return cases


def order_bounds(predicted_counts, labels, predicted_maps=None, maps=None):
    """Per sum, how far two fp64 evaluations that add the same terms in different orders can lie apart:
    ``n * 2^-53 * sum |terms|`` with ``n`` the number of terms of that sum (Higham, Accuracy and Stability, (4.4): any
    order's error is at most (n - 1) u sum |terms| to first order, u = 2^-53 -- so two orders differ by at most twice
    that; ``n`` instead of ``n - 1`` and the bound taken against the restatement's own pairwise sums, whose error is
    O(log n) u, cover the factor with a margin that grows with n).

    sums[0], sums[1]: the nested sums over every label element and every predicted count, n = B * (HW + 1) terms
    (|sum_b |d_b|| moves by at most sum_b |delta d_b|).  sums[2]: d_b moves by at most delta_b = (HW + 1) u (|c_b| + sum
    |labels_b|), so d_b * d_b by 2 |d_b| delta_b (+ one rounding of the product's sum): sum_b 2 |d_b| delta_b + B u sum
    d_b^2.  (This is NOT the literal ``n * 2^-53 * sum |terms|`` with the n = B terms d_b^2: the d_b themselves depend on the
    order in which their label patches were added, so that literal bound is not guaranteed for any implementation; the bound
    here carries the label sums' own order bound through the square and is wider by about HW.  The exact-input cases, which
    demand equal bits, carry the weight for sums[2].)  sums[4], sums[5]: n = B * M * HW terms |e| and e * e, each term itself identical in both evaluations."""
    u = 2.0 ** -53
    labels = np.asarray(labels, dtype=np.float64).reshape(len(labels), -1)
    counts = np.asarray(predicted_counts, dtype=np.float64).reshape(-1)
    batch, plane = labels.shape
    magnitude = np.abs(counts) + np.abs(labels).sum(axis=1)
    difference = counts - labels.sum(axis=1)
    bounds = np.zeros(8, dtype=np.float64)
    bounds[0] = bounds[1] = batch * (plane + 1) * u * magnitude.sum()
    bounds[2] = (2 * np.abs(difference) * (plane + 1) * u * magnitude).sum() + batch * u * (difference * difference).sum()
    if maps is not None:
        error = np.asarray(predicted_maps, dtype=np.float64) - np.asarray(maps, dtype=np.float64)[:, None]
        bounds[4] = error.size * u * np.abs(error).sum()
        bounds[5] = error.size * u * (error * error).sum()
    return bounds
