"""Host model of the exploration bonus (csrc/explore.hip) in numpy integers: the frame code (average-pool ->
quantise -> multilinear hash), which rollout rows earn, the count table and the bonus.  Everything up to the bonus is
int64 / uint64 arithmetic reduced mod 2^32 where the kernel's uint32 wraps, so the device is held to it bit for bit; the
bonus is fp64 (the kernel: fp32 sqrt and divide)."""
import numpy as np

try:
    import philox_model as PH
except ImportError:            # imported as tests.<module>
    from tests import philox_model as PH

STREAM = 0x4558504C            # "EXPL": counter word 2 of the multiplier draws
GOLDEN = 0x9E3779B1
MAX_FEATURES = 1323
M32 = (1 << 32) - 1


def n_features(H, W, cell):
    assert cell >= 2 and H % cell == 0 and W % cell == 0, (H, W, cell)
    F = (H // cell) * (W // cell) * 3
    assert F <= MAX_FEATURES, F
    return F


def multipliers(F, seed):
    """m_f = word 0 of philox4x32_10(seed, f, STREAM) | 1 -> uint64 [F] (values below 2^32)."""
    return PH.philox4x32_10(seed, np.arange(F, dtype=np.uint64), STREAM)[0] | np.uint64(1)


def cell_sums(frames, cell, vmax):
    """frames uint8 [n, H, W, 3] -> S int64 [n, F], f = ((y / cell) (W / cell) + x / cell) 3 + c."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    n_features(H, W, cell)
    clamped = np.minimum(frames.astype(np.int64), int(vmax))
    return clamped.reshape(n, H // cell, cell, W // cell, cell, 3).sum(axis=(2, 4)).reshape(n, -1)


def levels_of(frames, cell, levels, vmax):
    """-> int64 [n, F] in 0 .. levels - 1."""
    assert 2 <= levels <= 64 and 1 <= vmax <= 255
    return cell_sums(frames, cell, vmax) * int(levels) // (int(vmax) * cell * cell + 1)


def hash_of(level, mult):
    """h = sum_f level_f m_f mod 2^32 -> int64 [n].  (level < 64, m < 2^32, F <= 1323: the sum stays below 2^49.)"""
    return (np.asarray(level, dtype=np.uint64) * mult[None, :]).sum(axis=1).astype(np.int64) & M32


def codes_of(frames, cell, levels, vmax, bits, mult):
    """-> int64 [n] codes in [0, 2^bits)."""
    assert 10 <= bits <= 26
    h = hash_of(levels_of(frames, cell, levels, vmax), mult).astype(np.uint64)       # (h GOLDEN < 2^64: uint64 holds it)
    return (((h * np.uint64(GOLDEN)) & np.uint64(M32)) >> np.uint64(32 - bits)).astype(np.int64)


def earning(active_log, n_steps, terminal_end):
    """active_log [T, B], n_steps [B], terminal_end [B] -> bool [T, B]: the row took a step that did not end an episode."""
    active_log = np.asarray(active_log)
    T, B = active_log.shape
    t = np.arange(T)[:, None]
    last = (np.asarray(terminal_end)[None, :] != 0) & (t == np.asarray(n_steps)[None, :] - 1)
    return (active_log != 0) & ~last


def count_add(table, codes):
    """table[code] += 1 for every code >= 0 (in place; int64 or int32 table) -> table."""
    codes = np.asarray(codes).reshape(-1)
    ok = (codes >= 0) & (codes < len(table))
    np.add.at(table, codes[ok], 1)
    return table


def bonus_of(table, codes, beta):
    """beta / sqrt(table[code]) in fp64 for every code >= 0 (the kernel's beta is the fp32 one), 0 elsewhere; also
    -> (earning rows, rows whose count is 1)."""
    codes = np.asarray(codes)
    ok = (codes >= 0) & (codes < len(table))
    n = np.where(ok, table[np.where(ok, codes, 0)], 1).astype(np.float64)
    bonus = np.where(ok, float(np.float32(beta)) / np.sqrt(n), 0.0)
    return bonus, int(ok.sum()), int((ok & (n == 1)).sum())
