"""The step kernels OFF their fast paths, against the CPU oracle: host-injected states (tests/extreme_state_cases.py) at Bullet's
+-100 coordinate-velocity clamp, past the exponential map's pi/4 cap, inside its Taylor branch and on both sides of the Quadrotor 2D
recurrence's `free_run` guard — every wave holds all lane kinds of its case, so a wave runs the fast path and the fall-back in sequence.
tests/test_extreme_states_cpu.py shows with the oracle alone that the cases reach those paths.

Primary comparison, every lane and every step: the raw simulator state (scg_get_state) against the oracle's, the quaternion up to
sign and the unwrapped Quadrotor 2D pitch through (sin, cos).  Derived outputs (obs, reward, mse, constraint rows, done, flags,
out.state) on the lanes whose pitch stays within +-1.2 after the step (beyond +-pi/2 the Euler pitch folds); that is at least half of
the lanes of every case.  Bounds, from tests/test_gpu_env_parity.py:

* float64, free-running over the 3 steps: rtol 1e-9, atol 1e-10 (constraint rows: atol 2e-8);
* float32, state re-synchronised to the oracle before every step: rtol 1e-4, atol 2e-5 * max(1, max|oracle.state|) for state and
  obs, rtol 3e-4 / atol 3e-5 * max(1, |value|) for reward and mse, rtol 1e-4 / atol 5e-5 * scale for constraint rows;
* both: a velocity component that the oracle ends at exactly +-100.0, with its unclamped last-substep update overshooting by more than
  1e-3, is exactly +-100.0 on the GPU.

MEASURED (MI355X; max |raw state - oracle| per case over the 3 steps, generic library, n = 192; sin / cos for the 2D pitch; the f32
column also as a fraction of its absolute bound 2e-5 * scale, scale = 100; the tests print these numbers):

    case                  f64        f32                 clamped components checked for exactness
    q2_guard              3.6e-14    1.4e-05  (0.007)    304     (n = 150: 1.5e-05, 252)
    q2_guard_dist         2.1e-14    2.8e-05  (0.014)    287
    q2_slow               2.8e-14    1.1e-05  (0.005)    336     (n = 150: 1.1e-05, 245)
    q3_clamp              8.5e-14    5.6e-05  (0.022)    503
    q3_cap                1.3e-13    2.7e-05  (0.009)    524
    q3_cap_240            7.1e-14    2.2e-05  (0.008)    459
    cartpole_clamp        1.8e-13    5.8e-05  (0.029)    150
    cartpole_clamp_slow   1.4e-14    1.8e-05  (0.009)    197
    cartpole_clamp_dist   1.1e-13    4.9e-05  (0.024)    152
    q1_clamp              1.4e-15    6.7e-05  (0.034)    345

The four specialised builds (q2_guard, q3_clamp, cartpole_clamp f32; q3_cap f64) give the same figures as the generic library.
The state rows of the K = 3 sequence differ from the oracle by at most 3.6e-14 (q2_guard) and 1.8e-13 (q3_cap).

Sensitivity, each shown once with a local edit of csrc/scg_env_core.h that was not kept: `if (!free_run)` fails q2_guard f32 at
both sizes (a clamp lane's rate ends 4.67 rad/s past the clamp); a cap of 0.95 instead of pi/4 fails q3_cap in f64 (0.164), in f32 and
in the sequence test, and leaves q3_cap_240 passing, as the case table says it must.
"""
import numpy as np
import pytest

from tests import extreme_state_cases as X

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SPECIALISED = X.SPECIALISED
DTYPES = {'f32': torch.float32, 'f64': torch.float64}


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _gpu(case, n, dtype, specialize, raw, oracle):
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = X.load_config(case)
    gpu = HipVecEnv(env_id, n, seed=3, dtype=dtype, return_numpy=False, specialize=specialize, **cfg)
    assert gpu.specialized == bool(specialize)
    gpu.reset_tensors()
    gpu.set_raw_state(raw)
    gpu.set_counters(oracle.ctrl_step_counter, oracle.episode)
    return gpu


def _comparable(oracle, got, want):
    """Raw states in a form that compares: the quaternion's sign fixed to the oracle's, the 2D pitch as (sin, cos)."""
    got, want = got.copy(), want.copy()
    if oracle.NAME == 'quadrotor' and oracle.QUAD_TYPE == 3:
        flip = (got[:, 3:7] * want[:, 3:7]).sum(axis=1) < 0
        got[flip, 3:7] *= -1.0
    if oracle.NAME == 'quadrotor' and oracle.QUAD_TYPE == 2:
        got = np.concatenate([got, np.cos(got[:, 4:5])], axis=1)
        want = np.concatenate([want, np.cos(want[:, 4:5])], axis=1)
        got[:, 4], want[:, 4] = np.sin(got[:, 4]), np.sin(want[:, 4])
    return got, want


def _unwrap_to(oracle, got, want):
    """Quadrotor 3D roll / yaw come from atan2: bring `got` to the branch of `want` (a lane at +-pi is the same attitude)."""
    if oracle.NAME == 'quadrotor' and oracle.QUAD_TYPE == 3:
        got = got.copy()
        for c in (6, 8):
            got[:, c] = want[:, c] + (got[:, c] - want[:, c] + np.pi) % (2.0 * np.pi) - np.pi
    return got


def _run(name, n, tag, specialize):
    """3 control steps of a case on the GPU and the oracle, every assertion of the module docstring; returns max |raw - oracle|."""
    case = X.CASE_BY_NAME[name]
    dtype, f64 = DTYPES[tag], tag == 'f64'
    oracle, raw, act, kinds = X.make_oracle(case, n)
    gpu = _gpu(case, n, dtype, specialize, raw, oracle)
    act_t = torch.as_tensor(act, dtype=dtype, device=gpu.device)
    vc = X.velocity_columns(oracle)
    worst, worst_frac, n_exact, n_ok = 0.0, 0.0, 0, n
    for t in range(X.N_STEPS):
        msg = f'{name} n={n} {tag} t={t}'
        before = X.raw_state(oracle)
        if not f64:                     # one-step errors: the float32 state restarts from the oracle's
            gpu.set_raw_state(before)
            gpu.set_counters(oracle.ctrl_step_counter, oracle.episode)
        with X.unclamped_trace() as trace:
            obs_o, rew_o, done_o, info = oracle.step(act)
        after = X.raw_state(oracle)
        out = gpu.step_tensors(act_t)
        got_raw = gpu.get_raw_state()
        pred = X.predicates(case, oracle, before, after, act)
        scale = np.maximum(1.0, np.abs(oracle.state).max())
        tol = dict(rtol=1e-9, atol=1e-10) if f64 else dict(rtol=1e-4, atol=2e-5 * scale)
        # ---- primary: the raw simulator state, every lane
        g, w = _comparable(oracle, got_raw, after)
        dev = np.abs(g - w).max()
        worst, worst_frac = max(worst, dev), max(worst_frac, dev / tol['atol'])
        print(f'{msg}: max|raw - oracle| {dev:.3e} (scale {scale:.1f}; clamp lanes {int(pred["clamp"].sum())}, guard false / true '
              f'{int(pred["guard_false"].sum())} / {int(pred["guard_true"].sum())}, cap {int(pred["cap"].sum())}, taylor '
              f'{int(pred["taylor"].sum())})')
        np.testing.assert_allclose(g, w, err_msg=msg, **tol)
        # ---- exactness of the clamp
        free, end = X.last_unclamped(oracle, trace), after[:, vc]
        sel = (np.abs(end) == X.VMAX) & (np.abs(free) > X.VMAX + 1e-3)
        n_exact += int(sel.sum())
        np.testing.assert_array_equal(got_raw[:, vc][sel], end[sel], err_msg=msg + ' (clamped components)')
        # ---- derived outputs, the lanes inside the pitch range
        ok = pred['pitch_ok']
        n_ok = min(n_ok, int(ok.sum()))
        np.testing.assert_array_equal(_np(out.done).astype(bool), done_o, err_msg=msg)
        assert not done_o.any(), msg
        rtol_r, atol_r = (1e-9, 1e-10) if f64 else (3e-4, 3e-5)
        for label, got, want in (('reward', _np(out.reward), rew_o), ('mse', _np(out.mse), info['mse'])):
            bound = atol_r * (1.0 if f64 else np.maximum(1.0, np.abs(want))) + rtol_r * np.abs(want)
            bad = ok & ~(np.abs(got - want) <= bound)
            assert not bad.any(), (msg, label, np.nonzero(bad)[0][:8], got[bad][:8], want[bad][:8])
        nx = oracle.state.shape[1]
        obs_g = _np(out.obs)
        obs_g[:, :nx] = _unwrap_to(oracle, obs_g[:, :nx], obs_o[:, :nx])
        np.testing.assert_allclose(obs_g[ok], obs_o[ok], err_msg=msg + ' obs', **tol)
        st_g = _unwrap_to(oracle, _np(out.state).T, oracle.state)
        np.testing.assert_allclose(st_g[ok], oracle.state[ok], err_msg=msg + ' state', **tol)
        flags_o = (info['constraint_violation'] > 0).astype(np.uint8) * 2       # (truncation cannot occur within 3 steps)
        sure = ok.copy()
        if 'constraint_values' in info:
            cv = info['constraint_values']
            ctol = dict(rtol=0, atol=2e-8) if f64 else dict(rtol=1e-4, atol=5e-5 * scale)
            np.testing.assert_allclose(_np(out.c_values).T[ok], cv[ok], err_msg=msg + ' c_values', **ctol)
            if not f64:                 # a row within the bound of zero may fall on either side
                sure &= np.abs(cv).min(axis=1) > ctol['atol'] + ctol['rtol'] * np.abs(cv).max()
        np.testing.assert_array_equal((_np(out.flags).astype(np.uint8) & 3)[sure], flags_o[sure], err_msg=msg + ' flags')
    assert n_ok * 2 >= n, (name, n_ok)
    assert n_exact >= 8, (name, n_exact)
    step, ep = gpu.get_counters()
    np.testing.assert_array_equal(step, oracle.ctrl_step_counter)
    np.testing.assert_array_equal(ep.astype(np.int64), oracle.episode)
    gpu.close()
    print(f'MEASURED {name} n={n} {tag} {"specialised" if specialize else "generic"}: max|raw - oracle| {worst:.3e}, '
          f'{worst_frac:.3f} of the absolute bound; exactly clamped components checked {n_exact}; lanes inside the pitch range >= {n_ok}')
    return worst


@pytest.mark.parametrize('name', list(X.CASE_BY_NAME))
def test_f64_generic_free_running_vs_oracle(name):
    _run(name, 192, 'f64', False)


@pytest.mark.parametrize('name,n', X.CASE_SIZES)
def test_f32_generic_one_step_error_vs_oracle(name, n):
    """n = 150: the two disturbance-free Quadrotor 2D cases also with a ragged last wave (22 lanes that still hold every kind)."""
    _run(name, n, 'f32', False)


@pytest.mark.parametrize('name,tag', SPECIALISED, ids=[f'{a}-{b}' for a, b in SPECIALISED])
def test_specialised_builds_vs_oracle(name, tag):
    """The library compiled for the case's very config (parameters as compile-time constants, unrolled substep loops)."""
    _run(name, 192, tag, True)


@pytest.mark.parametrize('name', ['q2_guard', 'q3_cap'])
def test_f64_state_in_registers_across_a_sequence(name):
    """scg_step_sequence, K = 3 from the injected state (the state stays in registers between the steps): its state rows equal three
    scg_step calls bit for bit, and the oracle to 1e-9."""
    case = X.CASE_BY_NAME[name]
    n, K = 192, X.N_STEPS
    oracle, raw, act, _ = X.make_oracle(case, n)
    a, b = (_gpu(case, n, torch.float64, False, raw, oracle) for _ in range(2))
    acts = torch.as_tensor(act, dtype=torch.float64, device=a.device).expand(K, -1, -1).contiguous()
    seq = a.step_sequence(acts, mse=True, state=True)
    tol = dict(rtol=1e-9, atol=1e-10)
    for t in range(K):
        out = b.step_tensors(acts[t])
        for label in ('state', 'obs', 'reward', 'done', 'flags', 'mse'):
            assert torch.equal(seq[label][t], getattr(out, label)), (name, label, t)
        oracle.step(act)
        ok = np.abs(X.pitch_of(oracle, X.raw_state(oracle))) <= X.PITCH_MAX
        assert ok.sum() * 2 >= n
        got = _unwrap_to(oracle, _np(seq['state'][t]).T, oracle.state)
        print(f'{name} sequence t={t}: max|state - oracle| {np.abs(got[ok] - oracle.state[ok]).max():.3e} on {int(ok.sum())} lanes')
        np.testing.assert_allclose(got[ok], oracle.state[ok], err_msg=f'{name} t={t}', **tol)
    np.testing.assert_array_equal(a.get_raw_state(), b.get_raw_state())
    g, w = _comparable(oracle, a.get_raw_state(), X.raw_state(oracle))
    np.testing.assert_allclose(g, w, **tol)
    a.close(); b.close()
