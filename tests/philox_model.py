"""Philox4x32-10 in vectorised numpy (test infrastructure): the host model of csrc/maze_common.h philox4x32_10 and of
the two draw kernels of csrc/env.hip.

Layout, as philox4x32_10(seed, index, stream, out) packs it: counter = (index lo, index hi, stream lo, stream hi),
key = (seed lo, seed hi); ten rounds, the key bumped by the Weyl constants after each.  Pinned to the Random123
known-answer vectors by test_replay_edges_cpu.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10_raw(counter, key):
    """counter: four uint32 words (scalars or equal-shaped arrays), key: two uint32 words -> [4, ...] uint64 array
    holding the four 32-bit output words."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = M0 * c[0]                      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return np.stack(c)


def philox4x32_10(seed, index, stream):
    """The device function's packing: 64-bit seed, index (array) and stream."""
    index = np.asarray(index, dtype=np.uint64)
    seed, stream = int(seed), int(stream)
    return philox4x32_10_raw((index & MASK, index >> S32, stream & 0xFFFFFFFF, (stream >> 32) & 0xFFFFFFFF),
                             (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def draw_index(n, row_len=None, row_stride=None, col0=0):
    """Element i of a draw of n is element (i // row_len) * row_stride + col0 + i % row_len of the stream."""
    row_len = n if row_len is None else row_len
    row_stride = row_len if row_stride is None else row_stride
    i = np.arange(n, dtype=np.uint64)
    return (i // np.uint64(row_len)) * np.uint64(row_stride) + np.uint64(col0) + i % np.uint64(row_len)


def uniform(seed, stream, n, row_len=None, row_stride=None, col0=0):
    """53-bit uniforms in [0, 1): ((r0 >> 5) * 2**26 + (r1 >> 6)) / 2**53, exact in fp64."""
    r = philox4x32_10(seed, draw_index(n, row_len, row_stride, col0), stream)
    return ((r[0] >> np.uint64(5)) * np.uint64(1 << 26) + (r[1] >> np.uint64(6))).astype(np.float64) / 2.0 ** 53


def randint(seed, stream, high, n, row_len=None, row_stride=None, col0=0):
    """(r0 * high) >> 32 for 0 < high < 2**31."""
    r = philox4x32_10(seed, draw_index(n, row_len, row_stride, col0), stream)
    return ((r[0] * np.uint64(high)) >> S32).astype(np.int32)
