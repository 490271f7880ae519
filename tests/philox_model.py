"""Host model of the off-policy collectors' in-kernel random draws (csrc/scg_wide.h: `normal4` and
`uniform_action_kernel`, one definition for the SAC and the DDPG library), in float64 on top of oracle/rng.py's Philox4x32-10.

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (*d_counter, row, stream, 0x5ac1)          stream 3: the collector's N(0, 1) draws, 4: the uniform warm-up action
    normal4 : r0 = sqrt(-2 ln u(w.x)), r1 = sqrt(-2 ln u(w.z));  columns (r0 cos 2 pi u(w.y), r0 sin .., r1 cos 2 pi u(w.w), r1 sin ..)
    uniform : column j = low_j + (high_j - low_j) u(w_j)

The kernels evaluate Box-Muller with __logf / __sincosf in float32; this model is the exact value they approximate."""
import numpy as np

from oracle.rng import philox4x32_10, u01_from_word

TAG = 0x5AC1
STREAM_NORMAL, STREAM_UNIFORM = 3, 4


def words(seed, counter, rows, stream):
    """Philox block of each row: (len(rows), 4) uint32."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1)
    ctr = np.empty((rows.shape[0], 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.uint32(counter), rows, np.uint32(stream), np.uint32(TAG)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), (rows.shape[0], 2))
    return philox4x32_10(ctr, key)


def normal4(seed, counter, rows):
    """The four N(0, 1) draws of each row (stream 3), float64: (len(rows), 4)."""
    u = u01_from_word(words(seed, counter, rows, STREAM_NORMAL))
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t0, t1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1)


def uniform01(seed, counter, rows):
    """The warm-up action's four U(0, 1) words of each row (stream 4), float64 (each exact in float32): (len(rows), 4)."""
    return u01_from_word(words(seed, counter, rows, STREAM_UNIFORM))
