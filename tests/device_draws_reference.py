"""The tests' own reference of the device draws (``srgan_random_fill``, include/srgan_hip.h): the stream written out in NumPy,
integer steps in uint64, everything after the words in float64.  Shared by test_device_draws_cpu.py (which pins it to the
published Philox4x32-10 known answers and checks the distributions it produces) and test_device_draws_gpu.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything that broadcasts) of 32-bit words -> uint32 [..., 4]."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def block_words(seed, iteration, draw, first, n):
    """uint32 [blocks, 4]: the output words of every Philox block that intersects elements [first, first + n), and the
    position of element ``first`` inside the first of them."""
    first, n, seed = int(first), int(n), int(seed)
    blocks = np.arange(first >> 2, ((first + n - 1) >> 2) + 1, dtype=np.uint64)
    counter = np.stack([blocks & MASK, blocks >> np.uint64(32), np.full_like(blocks, draw), np.full_like(blocks, iteration)], axis=-1)
    return philox4x32_10(counter, np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint64)), first & 3


def own_words(seed, iteration, draw, first, n):
    """uint32 [n]: the word each element owns (``w[e & 3]`` of block ``e >> 2``)."""
    words, skip = block_words(seed, iteration, draw, first, n)
    return words.reshape(-1)[skip:skip + n]


def signs(seed, iteration, draw, first, n):
    """float64 [n] of +1 / -1: bit 0 of the element's own word picks the mixture component."""
    return np.where(own_words(seed, iteration, draw, first, n) & 1, 1.0, -1.0)


def expected(kind, seed, iteration, draw, first, n, offset=0.0):
    """float64 [n]: elements [first, first + n) of a draw.  kind 0: U[0, 1); kind 1: N(0, 1) + (+/-)offset."""
    words, skip = block_words(seed, iteration, draw, first, n)
    unit = (words >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    if kind == 0:
        values = unit
    else:
        u1, u2 = 1.0 - unit[:, 0::2], unit[:, 1::2]                # word pairs (w0, w1) and (w2, w3)
        r = np.sqrt(-2.0 * np.log(u1))
        values = np.empty_like(unit)
        values[:, 0::2] = r * np.cos(2.0 * np.pi * u2)
        values[:, 1::2] = r * np.sin(2.0 * np.pi * u2)
        if offset != 0.0:
            values = values + np.where(words & 1, offset, -offset)
    return values.reshape(-1)[skip:skip + int(n)]
