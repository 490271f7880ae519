"""The host model of the off-policy collectors' in-kernel draws (tests/philox_model.py) on its own, without a GPU: its normal4 stream is
N(0, 1) and its warm-up words are U(0, 1), independent across columns and across counter words.  tests/test_gpu_offpolicy_collector.py
pins the kernels to this model, so these properties carry over to them.  Over 2^20 rows x 4 columns (seeded, so deterministic):
KS distance below 1.63 / sqrt(n) (the 1 % critical value), mean / variance / skew / excess kurtosis within 5 standard errors, the
fractions beyond |eps| > 3 and > 4 within 5 binomial sigma, correlations below 5 / sqrt(n)."""
import numpy as np
import pytest
from scipy.special import ndtr

from tests import philox_model as pm

N = 1 << 20
SEED = (0x9E3779B1 << 32) | 0x2545F491          # both key words non-zero


@pytest.fixture(scope='module')
def draws():
    rows = np.arange(N)
    return pm.normal4(SEED, 5, rows), pm.normal4(SEED, 6, rows)


def ks(x, cdf):
    x = np.sort(x)
    c = cdf(x)
    i = np.arange(1, x.size + 1)
    return max(float(np.max(i / x.size - c)), float(np.max(c - (i - 1) / x.size)))


@pytest.mark.parametrize('col', range(4))
def test_normal4_column_is_standard_normal(draws, col):
    e = draws[0][:, col]
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


def test_normal4_columns_and_counter_words_are_uncorrelated(draws):
    e0, e1 = draws
    bound = 5 / np.sqrt(N)
    c = np.corrcoef(e0.T)
    assert np.max(np.abs(c[~np.eye(4, dtype=bool)])) < bound
    for j in range(4):
        assert abs(np.corrcoef(e0[:, j], e1[:, j])[0, 1]) < bound, j
    assert abs(np.corrcoef(e0.reshape(-1), e1.reshape(-1))[0, 1]) < bound


@pytest.mark.parametrize('col', range(4))
def test_uniform_words_are_uniform(col):
    u = pm.uniform01(SEED, 5, np.arange(N))[:, col]
    n = u.size
    assert ks(u, lambda x: x) < 1.63 / np.sqrt(n)
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / n)
    assert abs(u.var() - 1 / 12) < 5 * np.sqrt(1 / 180 / n)       # var of (U - 1/2)^2 = 1/80 - 1/144 = 1/180
    assert u.min() > 0.0 and u.max() < 1.0


def test_streams_and_key_words_are_distinct():
    """The key's high word, the stream and the counter word each select another block; the uniform and normal streams differ."""
    rows = np.arange(4096)
    w = pm.words(SEED, 5, rows, pm.STREAM_NORMAL)
    others = (pm.words(SEED & 0xFFFFFFFF, 5, rows, pm.STREAM_NORMAL), pm.words(SEED, 5, rows, pm.STREAM_UNIFORM),
              pm.words(SEED, 6, rows, pm.STREAM_NORMAL), pm.words(SEED, 5, rows + 1, pm.STREAM_NORMAL))
    for o in others:
        assert np.count_nonzero(o == w) < 8
