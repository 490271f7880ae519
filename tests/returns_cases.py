"""Inputs, float64 reference and error bound shared by tests/test_returns_cpu.py (the PyTorch helpers ppo.advantage_moments /
ppo.normalise_advantages) and tests/test_gpu_returns.py (the scg_ppo_returns_* launches).

Reference: float64 NumPy, `(a - a.mean()) / (a.std() + 1e-6)` — the reference's line (controllers/ppo/ppo.py:300) on the float32 inputs
widened exactly.
Bound: 4 x yardstick + 2 float32 ulps of max |reference|.  The yardstick is that same line evaluated in NumPy float32 (two passes: mean,
then the deviations' spread) against the float64 result: what the reference itself achieves on this input, never the code under test.
Its error is dominated by one rounding of the mean, of which a single sample may sit anywhere below the half-ulp worst case, and a correct
implementation that sums in another order may sit elsewhere in it: the factor 4.  The 2 ulps cover the one rounding of a result that
was formed in float64 (half an ulp) where the yardstick happens to be exact.
"""
import math

import numpy as np

# (mean, std) of the drawn cases and their sizes: the one shape the suite had (7 x 1000) and 5 x 52 429, where every thread of the
# moments launch walks its strided loop four or five times
CONDITIONING = [(0.5, 3.0), (10.0, 1.0), (30.0, 0.3), (100.0, 0.5), (-300.0, 0.3), (1000.0, 0.1)]
SIZES = [(7, 1000), (5, 52429)]
# the collector's post-processing on a cartpole_stab rollout with a time-limit truncation every 15 steps (build() compiles this variant)
CHAIN_TASK = 'cartpole_stab'
CHAIN_OVERRIDE = dict(episode_len_sec=1)
CHAIN_POLICY = (64, 'leaky_relu')


def draw(mean, std, M, seed):
    """float32 [M] around `mean`: drawn on the host, so that the float64 reference sees exactly what the code under test sees."""
    rng = np.random.default_rng(seed)
    return (mean + std * rng.standard_normal(M)).astype(np.float32)


def drawn_cases():
    return [(f'mean{mean:g}_std{std:g}_M{T}x{N}', mean, std, T, N) for (T, N) in SIZES for (mean, std) in CONDITIONING]


def exact_cases():
    """name -> (float32 input, closed-form output or None)."""
    half = np.empty(4096, np.float32)
    half[0::2], half[1::2] = 64.0, 65.0             # mean 64.5, std 0.5, every sum exact
    return {'constant_0.5_M4096': (np.full(4096, 0.5, np.float32), np.zeros(4096)),
            'single_element': (np.array([3.7], np.float32), np.zeros(1)),
            'half_64_half_65': (half, (half.astype(np.float64) - 64.5) / (0.5 + 1e-6))}


def shards(seed=11):
    """Four unequal shards of one array (what four ranks hold): one around +100, one around -100, a single element, a benign one."""
    rng = np.random.default_rng(seed)
    return [(100.0 + 0.5 * rng.standard_normal(70001)).astype(np.float32), (-100.0 + 0.5 * rng.standard_normal(4099)).astype(np.float32),
            np.array([2.25], np.float32), (0.5 + 3.0 * rng.standard_normal(1000)).astype(np.float32)]


def reference(a):
    a = np.asarray(a, np.float64).reshape(-1)
    return (a - a.mean()) / (a.std() + 1e-6)


def yardstick(a):
    """max |the reference's line in float32 - its float64 value| on `a`."""
    a = np.asarray(a, np.float32).reshape(-1)
    y = (a - a.mean()) / (a.std() + 1e-6)
    assert y.dtype == np.float32
    return float(np.abs(y.astype(np.float64) - reference(a)).max())


def bound(a):
    ulp = float(np.spacing(np.float32(np.abs(reference(a)).max())))
    return 4.0 * yardstick(a) + 2.0 * ulp


def deviation(out, a):
    out = np.asarray(out).reshape(-1)
    assert out.dtype == np.float32 and np.isfinite(out).all()
    return float(np.abs(out.astype(np.float64) - reference(a)).max())


def exact_moments(a):
    """(sum, sum of squares, count) of the float32 input, correctly rounded (fsum; a float32's square is exact in float64), and the
    error a float64 accumulation in ANY order may leave: (n - 1) u sum |terms|, u = 2^-53 (Higham, Accuracy and Stability, §4.2)."""
    a = np.asarray(a, np.float64).reshape(-1)
    n, u = a.size, 2.0 ** -53
    s1, s2 = math.fsum(a), math.fsum(a * a)
    return (s1, s2, float(n)), ((n - 1) * u * math.fsum(np.abs(a)), (n - 1) * u * s2)


def check_moments(mom, a):
    mom = np.asarray(mom)
    assert mom.dtype == np.float64 and mom.shape == (3,)
    (s1, s2, n), (e1, e2) = exact_moments(a)
    assert mom[2] == n
    assert abs(mom[0] - s1) <= e1 and abs(mom[1] - s2) <= e2, (mom.tolist(), (s1, s2, n), (e1, e2))


def report(name, a, out):
    """One line of the measured table (printed before anything is asserted) and the three figures."""
    y, b, d = yardstick(a), bound(a), deviation(out, a)
    print(f'{name:32s} yardstick {y:9.3e}  bound {b:9.3e}  deviation {d:9.3e}')
    return y, b, d
