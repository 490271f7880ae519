"""Conditions on the INPUTS of tests/test_gpu_extreme_states.py, checked with the oracle alone: every case of
tests/extreme_state_cases.py stays finite, and every wave of 64 lanes really holds the lanes the case is named after — lanes on both
sides of the Quadrotor 2D `free_run` guard, lanes whose +-100 clamp still binds when the control step ends, lanes past the pi/4 cap and
inside the Taylor branch — with at least half of the lanes inside the pitch range on which the derived outputs are compared."""
import numpy as np
import pytest

from tests import extreme_state_cases as X


def _run(name, n):
    case = X.CASE_BY_NAME[name]
    oracle, raw, act, kinds = X.make_oracle(case, n)
    before = X.raw_state(oracle)
    np.testing.assert_array_equal(before[:, X.velocity_columns(oracle)], raw[:, X.velocity_columns(oracle)])   # injection is exact
    pitch_ok = np.ones(n, dtype=bool)
    pred = None
    for t in range(X.N_STEPS):
        b = X.raw_state(oracle)
        obs, rew, done, info = oracle.step(act)
        a = X.raw_state(oracle)
        p = X.predicates(case, oracle, b, a, act)
        pred = pred or p
        pitch_ok &= p['pitch_ok']
        for v in (obs, rew, info['mse'], oracle.state, a) + ((info['constraint_values'],) if 'constraint_values' in info else ()):
            assert np.isfinite(v).all(), (name, t)
        assert not done.any(), (name, t)          # nothing ends an episode here: the comparison never meets a reset
    return oracle, kinds, pred, pitch_ok


@pytest.mark.parametrize('name,n', X.CASE_SIZES)
def test_cases_reach_their_paths(name, n):
    oracle, kinds, pred, pitch_ok = _run(name, n)
    q2 = oracle.NAME == 'quadrotor' and oracle.QUAD_TYPE == 2
    for w in X.waves(n):
        where = (name, n, w.start)
        assert pred['clamp'][w].sum() >= 8, where
        if q2:
            assert pred['guard_false'][w].sum() >= 4 and pred['guard_true'][w].sum() >= 4, where
            # the named kinds are on the side they were built for
            assert pred['guard_false'][w][np.isin(kinds[w], [X.Q2_A, X.Q2_B, X.Q2_D])].all(), where
            assert pred['guard_true'][w][kinds[w] == X.Q2_C].all(), where
        if name == 'q3_cap':
            assert pred['cap'][w].sum() >= 4 and pred['taylor'][w].sum() >= 4, where
            assert pred['cap'][w][kinds[w] == X.Q3_CAP].all() and pred['taylor'][w][np.isin(kinds[w], [X.Q3_T0, X.Q3_T1])].all(), where
            assert not pred['cap'][w][kinds[w] == X.Q3_NOCAP].any(), where
        if name == 'q3_cap_240':
            assert not pred['cap'][w].any(), where                  # out of reach under the clamp: see the case table
    assert pitch_ok.sum() * 2 >= n, (name, n, int(pitch_ok.sum()))
    print(f'{name} n={n}: clamp {int(pred["clamp"].sum())}, guard false/true {int(pred["guard_false"].sum())}/'
          f'{int(pred["guard_true"].sum())}, cap {int(pred["cap"].sum())}, taylor {int(pred["taylor"].sum())}, '
          f'pitch_ok over {X.N_STEPS} steps {int(pitch_ok.sum())}')


def test_every_wave_holds_every_kind():
    for name, n in X.CASE_SIZES:
        _, _, kinds = X.build(X.CASE_BY_NAME[name], n)
        for w in X.waves(n):
            assert set(kinds[w]) == set(kinds), (name, n, w.start)


@pytest.mark.parametrize('name', ['q2_guard', 'q3_cap', 'cartpole_clamp', 'q1_clamp'])
def test_inject_inverts_raw_state_and_trace_sees_the_overshoot(name):
    case = X.CASE_BY_NAME[name]
    oracle, raw, act, _ = X.make_oracle(case, 192)
    got = X.raw_state(oracle)
    if oracle.NAME == 'quadrotor' and oracle.QUAD_TYPE == 2:
        np.testing.assert_allclose(got, raw, rtol=0, atol=1e-15)
    else:
        np.testing.assert_array_equal(got, raw)
    ref, _, _, _ = X.make_oracle(case, 192)
    with X.unclamped_trace() as trace:
        oracle.step(act)
    ref.step(act)
    np.testing.assert_array_equal(X.raw_state(oracle), X.raw_state(ref))        # tracing does not change the step
    assert len(trace) == oracle.PYB_STEPS_PER_CTRL
    vc = X.velocity_columns(oracle)
    free, end = X.last_unclamped(oracle, trace), X.raw_state(oracle)[:, vc]
    np.testing.assert_array_equal(np.clip(free, -X.VMAX, X.VMAX), end)          # the step's end is the clamped unclamped update
    assert ((np.abs(end) == X.VMAX) & (np.abs(free) > X.VMAX + 1e-3)).sum() >= 16
