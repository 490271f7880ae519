"""The host model of the fused on-policy rollouts' in-kernel action noise (tests/philox_model.py: env_words / env_normal4, the env
stream of csrc/scg_rng.h on channels 5 and 6) on its own, without a GPU.  tests/test_gpu_rollout_noise.py pins scg_rollout_policy,
scg_rollout_adversarial and scg_rollout_cbf to this model draw by draw, so these properties carry over to them.  Over 2^20 counters
(256 global env ids from 100 000 x 64 episodes x 64 steps; seeded, so deterministic), the statistics and critical values of
tests/test_offpolicy_noise_model_cpu.py: KS distance below 1.63 / sqrt(n) (the 1 % critical value), mean / variance / skew / excess
kurtosis within 5 standard errors, the fractions beyond |eps| > 3 and > 4 within 5 binomial sigma, correlations below 5 / sqrt(n).

And the reference alone against the tolerance the GPU tests use: a float32 NumPy restatement of the kernels' Box-Muller text
(u01<float>, logf, sqrtf, the degree-9 cos_2pi of csrc/scg_env_core.h, the sine as cos(2 pi (u -+ 1/4))) stays within eps_tol of the
float64 model over 2^21 blocks x 4 columns; the worst error / bound is printed (0.48 here, 0.97 with both constants halved: the bound is tight to a factor of 2)."""
import numpy as np
import pytest
from scipy.special import ndtr

from tests import philox_model as pm
from tests.test_offpolicy_noise_model_cpu import ks

N = 1 << 20
SEED = (0x9E3779B1 << 32) | 0x2545F491          # both key words non-zero
GID0 = 100000


def grid(n=N):
    i = np.arange(n)
    return GID0 + (i & 255), (i >> 8) & 63, i >> 14        # gid, episode, step


def normal(channel, dg=0, de=0, ds=0):
    g, e, s = grid()
    return pm.env_normal4(SEED, g + dg, e + de, s + ds, channel)[0]


@pytest.fixture(scope='module')
def draws():
    return {5: normal(pm.CH_POLICY), 6: normal(pm.CH_ADVERSARY)}


@pytest.mark.parametrize('col', range(4))
@pytest.mark.parametrize('channel', [5, 6])
def test_column_is_standard_normal(draws, channel, col):
    e = draws[channel][:, col]
    n = e.size
    assert ks(e, ndtr) < 1.63 / np.sqrt(n)
    m = e.mean()
    z = e - m
    var = float(np.mean(z * z))
    skew = float(np.mean(z ** 3)) / var ** 1.5
    kurt = float(np.mean(z ** 4)) / var ** 2 - 3.0
    assert abs(m) < 5 / np.sqrt(n)
    assert abs(var - 1.0) < 5 * np.sqrt(2.0 / n)
    assert abs(skew) < 5 * np.sqrt(6.0 / n)
    assert abs(kurt) < 5 * np.sqrt(24.0 / n)
    for t in (3.0, 4.0):
        p = 2.0 * ndtr(-t)
        assert abs(np.count_nonzero(np.abs(e) > t) - n * p) < 5 * np.sqrt(n * p * (1 - p)), t


def uncorrelated(a, b, what):
    bound = 5 / np.sqrt(N)
    for j in range(4):
        assert abs(np.corrcoef(a[:, j], b[:, j])[0, 1]) < bound, (what, j)
    assert abs(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]) < 5 / np.sqrt(4 * N), what


@pytest.mark.parametrize('channel', [5, 6])
def test_columns_are_uncorrelated(draws, channel):
    c = np.corrcoef(draws[channel].T)
    assert np.max(np.abs(c[~np.eye(4, dtype=bool)])) < 5 / np.sqrt(N)


@pytest.mark.parametrize('channel', [5, 6])
@pytest.mark.parametrize('what,shift', [('next step', dict(ds=1)), ('next episode', dict(de=1)), ('next gid', dict(dg=1))])
def test_neighbouring_counters_are_uncorrelated(draws, channel, what, shift):
    uncorrelated(draws[channel], normal(channel, **shift), what)


def test_channels_are_uncorrelated(draws):
    """The policy's stream against the adversary's, the random-action channel's and the reset channel's blocks at the same counter."""
    uncorrelated(draws[5], draws[6], 'adversary')
    uncorrelated(draws[5], normal(pm.CH_RANDOM_ACTION), 'random action')
    uncorrelated(draws[5], normal(pm.CH_RESET), 'reset')


def test_addressing():
    """Every counter word, the key's high word, the channel, the item and the block select another block; gid, episode and step are
    32-bit words (2^32 - 2 is not 2^31 - 2, and -1 is 2^32 - 1)."""
    g, e, s = grid(4096)
    w = pm.env_words(SEED, g, e, s, 5)
    others = (pm.env_words(SEED & 0xFFFFFFFF, g, e, s, 5), pm.env_words(SEED, g, e, s, 6), pm.env_words(SEED, g + 1, e, s, 5),
              pm.env_words(SEED, g, e + 1, s, 5), pm.env_words(SEED, g, e, s + 1, 5), pm.env_words(SEED, g, e, s, 5, item=1),
              pm.env_words(SEED, g, e, s, 5, block=1), pm.env_words(SEED, g, e + (1 << 32) - 2, s, 5))
    for o in others:
        assert np.count_nonzero(o == w) < 8
    assert np.array_equal(pm.env_words(SEED, g, e - 1, s, 5), pm.env_words(SEED, g, e + (1 << 32) - 1, s, 5))
    # the same block as oracle.rng.PhiloxEnvRng draws
    from oracle.rng import PhiloxEnvRng, make_tag
    rng = PhiloxEnvRng(SEED, g)
    assert np.array_equal(rng.words(np.arange(4096), e, s, make_tag(5, 0, 0)), w)


def test_follow():
    done = np.zeros((6, 3), bool)
    done[1, 0] = done[2, 0] = done[4, 2] = True
    ep, st = pm.follow([7, 0, 248], [0, 65536, (1 << 32) - 1], done)
    assert st.T.tolist() == [[7, 8, 0, 0, 1, 2], [0, 1, 2, 3, 4, 5], [248, 249, 250, 251, 252, 0]]
    assert ep.T.tolist() == [[0, 0, 1, 2, 2, 2], [65536] * 6, [(1 << 32) - 1] * 5 + [0]]


# ---------------------------------------------------------------------------------------------------------------- float32 text
def cos_2pi_f32(u):
    f = np.float32
    r = np.abs(u - f(0.5))
    s = np.minimum(r, f(0.5) - r)
    x = f(3.14159265358979) * s
    x2 = x * x
    sn = x * (f(1.0) + x2 * (f(-1.66666667e-1) + x2 * (f(8.33333333e-3) + x2 * (f(-1.98412698e-4) + x2 * f(2.75573192e-6)))))
    c = f(1.0) - f(2.0) * sn * sn
    return np.where(r > f(0.25), c, -c)


def normal4_f32(w):
    """The kernels' Box-Muller text (scg_rollout_common.h normal4, and the same text inline in rollout_policy_kernel, scg_env_kernels.h) in NumPy
    float32, every operation rounded to float32 (no fused multiply-add)."""
    f = np.float32
    u = ((w >> np.uint32(8)).astype(f) + f(0.5)) * f(1.0 / 16777216.0)
    assert u.dtype == f
    out = np.empty(w.shape, f)
    for p in (0, 2):
        r, a = np.sqrt(f(-2.0) * np.log(u[..., p])), u[..., p + 1]
        out[..., p] = r * cos_2pi_f32(a)
        out[..., p + 1] = r * cos_2pi_f32(np.where(a < f(0.25), a + f(0.75), a - f(0.25)))
    assert out.dtype == f
    return out


def test_float32_box_muller_text_stays_within_eps_tol():
    n = 1 << 21
    i = np.arange(n)
    worst, worst_half = 0.0, 0.0
    for channel in (5, 6):
        w = pm.env_words(SEED, GID0 + (i & 511), (i >> 9) & 63, i >> 15, channel)
        e64, r = pm.box_muller4(w)
        err = np.abs(normal4_f32(w).astype(np.float64) - e64)
        worst = max(worst, float((err / pm.eps_tol(e64, r)).max()))
        worst_half = max(worst_half, float((err / (0.5 * pm.eps_tol(e64, r))).max()))
    # u01<float> itself: exact below 2^31, off by at most 2^-25 above
    w = np.array([0, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 31) + 256, (1 << 32) - 1], dtype=np.uint32)
    u32 = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    du = np.abs(u32.astype(np.float64) - pm.u01_from_word(w))
    assert (du[:4] == 0).all() and (du[4:] > 0).any() and du.max() <= 2.0 ** -25
    print(f'float32 Box-Muller text vs float64 model, 2 x 2^21 x 4 draws: worst error / eps_tol = {worst:.3f} '
          f'(with D_EPS / 2, D_LOG / 2: {worst_half:.3f})')
    assert worst <= 1.0
