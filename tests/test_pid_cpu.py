"""The pid controller's host side (safe_control_gym_amd/pid.py) against the reference-generated fixture (tests/golden/make_pid.py): no GPU."""
import numpy as np
import pytest

from tests import pid_cases as PC


def test_pid_id_resolves_and_defaults_equal_the_references_yaml():
    from safe_control_gym_amd.pid import PID, PID_DEFAULTS
    from safe_control_gym_amd.registration import get_config
    ctrl = PC.controller('quadrotor_2D_track', num_envs=3)
    assert isinstance(ctrl, PID) and ctrl.spec_id == 'pid' and ctrl.num_envs == 3
    assert get_config('pid') == PID_DEFAULTS == PC.settings()['pid_yaml']
    # the YAML's upper-case keys become attributes and are then overwritten by the constructor's own defaults, as upstream
    odd = PC.controller('quadrotor_2D_track', **dict(PID_DEFAULTS, KF=1.0, P_COEFF_FOR=[9, 9, 9]))
    assert odd.KF == 3.16e-10 and np.array_equal(odd.P_COEFF_FOR, [.4, .4, 1.25]) and odd.g == 9.8
    assert ctrl.GRAVITY == pytest.approx(PC.config('quadrotor_2D_track')['gravity'], rel=1e-15)
    assert PC.controller('quadrotor_2D_prior_mass').GRAVITY == pytest.approx(9.8 * 0.031, rel=1e-15)


def test_error_cases_raise_without_a_device():
    import functools

    from safe_control_gym_amd.registration import load_task, make
    env_id, cfg = load_task('cartpole_stab')
    with pytest.raises(NotImplementedError, match=r'\[ERROR\] PID not implemented for any system other than Quadrotor \(2D and 3D\)\.'):
        make('pid', functools.partial(make, env_id, **cfg))
    with pytest.raises(NotImplementedError, match='Quadrotor 1D'):
        make('pid', PC.env_func('quadrotor_2D_stab', quad_type=1, task_info={'stabilization_goal': [0, 1.2], 'stabilization_goal_tolerance': 0.0},
                                init_state={'init_z': 0.8}))
    with pytest.raises(ValueError, match='normalized_rl_action_space'):
        make('pid', PC.env_func('quadrotor_2D_track', normalized_rl_action_space=True))


@pytest.mark.parametrize('name', PC.cases())
def test_host_law_reproduces_the_references_closed_loops(name):
    """Fed the recorded observations, select_action returns the recorded actions and leaves the recorded state after every step."""
    fx = PC.fixture()
    ctrl = PC.controller(name)
    ctrl.reset()
    xs, us, ss = fx[f'{name}/x'], fx[f'{name}/u'], fx[f'{name}/state']
    got_u, got_s = [], []
    for t in range(us.shape[0]):
        got_u.append(ctrl.select_action(xs[t], {'current_step': t}))
        got_s.append(np.concatenate([ctrl.integral_pos_e, ctrl.last_rpy, ctrl.integral_rpy_e]))
    du, ds = PC.rel(got_u, us), PC.rel(got_s, ss)
    print(f'{name}: action {du:.3e}, state {ds:.3e} (bound {PC.bound():.3e}, floor 1e-9)')
    # (the recorded observations are fed, so nothing is amplified by the loop: the floor of the bound is what holds here)
    assert max(du, ds) <= 1e-9 <= PC.bound()


@pytest.mark.parametrize('qt', [2, 3])
def test_host_law_reproduces_the_one_step_cases(qt):
    fx = PC.fixture()
    name = f'quadrotor_{qt}D_stab'
    obs, pre, us, post = (fx[f'one_step_{qt}D/{k}'] for k in ('obs', 'pre', 'u', 'post'))
    n = obs.shape[0]
    batch = PC.controller(name, num_envs=n)                       # the whole batch in one call
    batch.integral_pos_e, batch.last_rpy, batch.integral_rpy_e = pre[:, 0:3].copy(), pre[:, 3:6].copy(), pre[:, 6:9].copy()
    u = batch.select_action(obs, {'current_step': 0})
    s = np.concatenate([batch.integral_pos_e, batch.last_rpy, batch.integral_rpy_e], axis=1)
    print(f'{qt}D one-step: action {PC.rel(u, us):.3e}, state {PC.rel(s, post):.3e}')
    assert max(PC.rel(u, us), PC.rel(s, post)) <= 1e-9 <= PC.bound()
    one = PC.controller(name)
    for k in (0, 1, n - 1):                                       # and one observation at a time
        one.integral_pos_e, one.last_rpy, one.integral_rpy_e = pre[k, 0:3].copy(), pre[k, 3:6].copy(), pre[k, 6:9].copy()
        assert np.array_equal(one.select_action(obs[k], {'current_step': 0}), u[k])


def test_save_then_load_restores_the_state_exactly(tmp_path):
    fx = PC.fixture()
    ctrl = PC.controller('quadrotor_3D_stab')
    for t in range(5):
        ctrl.select_action(fx['quadrotor_3D_stab/x'][t], {'current_step': t})
    want = [a.copy() for a in (ctrl.integral_pos_e, ctrl.last_rpy, ctrl.integral_rpy_e)]
    assert all(np.abs(a).max() > 0 for a in want)
    path = str(tmp_path / 'sub' / 'pid_state.npz')
    ctrl.save(path)
    ctrl.reset_before_run()
    assert not np.any(ctrl.integral_pos_e) and not np.any(ctrl.last_rpy) and not np.any(ctrl.integral_rpy_e)
    ctrl.load(path)
    for a, b in zip(want, (ctrl.integral_pos_e, ctrl.last_rpy, ctrl.integral_rpy_e)):
        assert np.array_equal(a, b)
