"""The tests' own reference of the resident image loaders' device draws (``srgan_epoch_order`` /
``srgan_epoch_batch_indices``, include/srgan_hip.h): the keys from the Philox words of device_draws_reference.py, the order by
NumPy's stable argsort, the step -> (epoch, batch) arithmetic and the table slice in Python integers.  Shared by
test_epoch_order_cpu.py and test_epoch_order_gpu.py; no tests of its own."""
import numpy as np

from device_draws_reference import block_words

LABELED_DRAW, UNLABELED_DRAW = 0x30002, 0x30003
EPOCH_ORDER_MAX = 2 ** 20


def epoch_keys(seed, epoch, draw, n):
    """uint64 ``[n]``: frame ``i`` owns ``(w1 << 32) | w0`` of block ``i`` of ``draw``, the EPOCH in the iteration word."""
    words, skip = block_words(seed, epoch, draw, 0, 4 * int(n))
    assert skip == 0 and words.shape == (n, 4)
    return (words[:, 1].astype(np.uint64) << np.uint64(32)) | words[:, 0].astype(np.uint64)


def stable_argsort(keys):
    return np.argsort(np.asarray(keys, dtype=np.uint64), kind='stable')


def epoch_order(seed, epoch, draw, n):
    """int64 ``[n]``: ``order[p]`` is the frame at sorted position ``p``; a tie goes to the lower frame."""
    return stable_argsort(epoch_keys(seed, epoch, draw, n))


def epoch_and_batch(step, n, global_batch):
    """``(epoch, batch, batches)`` of training step ``step`` (drop-last: ``batches = n // global_batch``)."""
    batches = int(n) // int(global_batch)
    assert batches >= 1
    return int(step) // batches, int(step) % batches, batches


def batch_table(seed, step, draw, n, global_batch, first_row=0, rows=None):
    """The frames of rows ``[first_row, first_row + rows)`` of the global batch of step ``step``, as a list of ints."""
    rows = global_batch - first_row if rows is None else rows
    assert 0 <= first_row and 0 <= rows and first_row + rows <= global_batch
    epoch, batch, _ = epoch_and_batch(step, n, global_batch)
    order = epoch_order(seed, epoch, draw, n).tolist()
    start = batch * global_batch + first_row
    return order[start:start + rows]
