"""Host model of the off-policy collectors' in-kernel random draws (csrc/scg_wide.h: `normal4` and
`uniform_action_kernel`, one definition for the SAC and the DDPG library), in float64 on top of oracle/rng.py's Philox4x32-10.

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (*d_counter, row, stream, 0x5ac1)          stream 3: the collector's N(0, 1) draws, 4: the uniform warm-up action
    normal4 : r0 = sqrt(-2 ln u(w.x)), r1 = sqrt(-2 ln u(w.z));  columns (r0 cos 2 pi u(w.y), r0 sin .., r1 cos 2 pi u(w.w), r1 sin ..)
    uniform : column j = low_j + (high_j - low_j) u(w_j)

The kernels evaluate Box-Muller with __logf / __sincosf in float32; this model is the exact value they approximate.

The env stream of csrc/scg_rng.h (what the fused on-policy rollouts draw their action noise from) is addressed differently:

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (global env id, episode, step in episode, tag),   tag = (channel << 16) | (item << 8) | block
    channel 5: the policy's N(0, 1) draws (scg_rollout_policy / _adversarial / _cbf / _safe), 6: the adversary's
    env_normal4 : normal4's columns of that block

`follow` gives the (episode, step) a K-step launch draws with, `eps_tol` the allowed |eps_kernel - eps64| of those kernels' float32
Box-Muller (logf, sqrtf, a degree-9 cosine):  D_EPS (1 + |eps64|) + D_LOG / r,  r the column's pair radius.  D_LOG: u01<float> is
NOT exact in float32 for words >= 2^31 ((float)(w >> 8) + 0.5f needs 25 bits there and rounds), the error of u is <= 2^-25 at
u >= 0.5, so |d ln u| <= 2^-25 / 0.5 ~ 6e-8, and an absolute error dL of ln u moves r = sqrt(-2 ln u) by dL / r.  D_EPS: logf,
sqrtf, the cosine polynomial (absolute error < 2e-7) and the products.  tests/test_onpolicy_noise_model_cpu.py holds a float32
NumPy restatement of the kernels' text to this bound."""
import numpy as np

from oracle.rng import make_tag, philox4x32_10, u01_from_word

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


# ---------------------------------------------------------------------------------------------------------------- env streams
CH_RESET, CH_RANDOM_ACTION, CH_POLICY, CH_ADVERSARY = 0, 4, 5, 6
D_EPS, D_LOG = 4e-6, 6e-8


def _u32(v):
    return (np.asarray(v).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def env_words(seed, gid, episode, step, channel, item=0, block=0):
    """Philox block at counter (gid, episode, step, tag(channel, item, block)); gid / episode / step broadcast: (..., 4) uint32."""
    g, e, s = np.broadcast_arrays(_u32(gid), _u32(episode), _u32(step))
    ctr = np.stack([g, e, s, np.full(g.shape, make_tag(channel, item, block), dtype=np.uint32)], axis=-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), g.shape + (2,))
    return philox4x32_10(ctr, key)


def box_muller4(w):
    """float64 (columns (r0 cos t0, r0 sin t0, r1 cos t1, r1 sin t1), each column's pair radius) of Philox blocks (..., 4):
    r0 <- w.x, t0 <- w.y, r1 <- w.z, t1 <- w.w."""
    u = u01_from_word(w)
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    t0, t1 = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
    eps = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1)
    return eps, np.stack([r0, r0, r1, r1], axis=-1)


def env_normal4(seed, gid, episode, step, channel, item=0, block=0):
    """(eps64 (..., 4), r (..., 4)): the four N(0, 1) draws of each env-stream block and the Box-Muller radius of each column's pair."""
    return box_muller4(env_words(seed, gid, episode, step, channel, item, block))


def follow(step0, episode0, done):
    """(episode [K, n], step [K, n]) a K-step launch draws with, from the counters at entry and its done [K, n] output: step t draws
    at the counters BEFORE its env step; where done[t] the env auto-resets (episode += 1 modulo 2^32, step = 0)."""
    done = np.asarray(done).astype(bool)
    ep, st = np.asarray(episode0).astype(np.int64) & 0xFFFFFFFF, np.asarray(step0).astype(np.int64).copy()
    eps, sts = np.empty(done.shape, np.int64), np.empty(done.shape, np.int64)
    for t in range(done.shape[0]):
        eps[t], sts[t] = ep, st
        st = np.where(done[t], 0, st + 1)
        ep = np.where(done[t], (ep + 1) & 0xFFFFFFFF, ep)
    return eps, sts


def eps_tol(eps64, r):
    """Allowed |eps_kernel - eps64| of the in-kernel float32 Box-Muller (module docstring)."""
    return D_EPS * (1.0 + np.abs(eps64)) + D_LOG / r
