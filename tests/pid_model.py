"""The cascade PID law of include/scg_pid.h in NumPy, float64 or float32, on the oracle's quaternion helpers (oracle/bullet.py): the CPU
model the GPU tests compare scg_rollout_pid with, and whose own deviation from the reference (measured by tests/golden/make_pid.py,
recorded in tests/golden/pid_settings.json) is their yardstick.  One env per call.

float32: every operation of the law runs in float32; the three quaternion helpers are evaluated in float64 on the float32 angles and
rounded once, i.e. they stand for correctly rounded float32 helpers."""
import numpy as np

from oracle import bullet

MIXER = np.array([[.5, -.5, -1], [.5, .5, 1], [-.5, .5, -1], [-.5, -.5, 1]])
CONFIG_KEYS = ('kf', 'gravity', 'pwm2rpm_scale', 'pwm2rpm_const', 'min_pwm', 'max_pwm', 'dt')


def targets(x_goal, tracking, step, nx):
    """(target_pos, target_vel) of pid.py:106-127; the row index saturates at the reference's last row."""
    x_goal = np.atleast_2d(np.asarray(x_goal, dtype=np.float64))
    row = x_goal[min(int(step), x_goal.shape[0] - 1)] if tracking else x_goal[0]
    if nx == 6:
        return np.array([row[0], 0.0, row[2]]), (np.array([row[1], 0.0, row[3]]) if tracking else np.zeros(3))
    return row[[0, 2, 4]].copy(), (row[[1, 3, 5]].copy() if tracking else np.zeros(3))


def law(obs, target_pos, target_vel, state, gains, cfg, dtype=np.float64):
    """One control step.  state = (integral_pos_e, last_rpy, integral_rpy_e); returns (action, new state)."""
    f = dtype
    obs = np.asarray(obs, dtype=f)
    c = {k: f(cfg[k]) for k in CONFIG_KEYS}
    g = np.asarray(gains, dtype=f)
    ipe, last_rpy, ire = (np.asarray(s, dtype=f) for s in state)
    zero = f(0)
    if obs.shape[0] == 6:
        pos, vel, rpy = np.array([obs[0], zero, obs[2]], dtype=f), np.array([obs[1], zero, obs[3]], dtype=f), np.array([zero, obs[4], zero], dtype=f)
    else:
        pos, vel, rpy = obs[[0, 2, 4]], obs[[1, 3, 5]], obs[6:9]
    quat = bullet.quaternion_from_euler(rpy)
    R = bullet.matrix_from_quaternion(quat).astype(f)
    cur_rpy = bullet.euler_from_quaternion(quat).astype(f)
    pos_e, vel_e = np.asarray(target_pos, dtype=f) - pos, np.asarray(target_vel, dtype=f) - vel
    ipe = np.clip(ipe + pos_e * c['dt'], f(-2), f(2))
    ipe[2] = np.clip(ipe[2], f(-0.15), f(0.15))
    F = g[0:3] * pos_e + g[3:6] * ipe + g[6:9] * vel_e + np.array([0, 0, c['gravity']], dtype=f)
    scalar_thrust = max(zero, np.dot(F, R[:, 2]))
    thrust = (np.sqrt(scalar_thrust / (f(4) * c['kf'])) - c['pwm2rpm_const']) / c['pwm2rpm_scale']
    z_ax = F / np.sqrt(np.dot(F, F))
    y_ax = np.cross(z_ax, np.array([1, 0, 0], dtype=f))
    y_ax = y_ax / np.sqrt(np.dot(y_ax, y_ax))
    Rt = np.stack([np.cross(y_ax, z_ax), y_ax, z_ax], axis=1).astype(f)
    E = Rt.T @ R - R.T @ Rt
    rot_e = np.array([E[2, 1], E[0, 2], E[1, 0]], dtype=f)
    rate_e = -(cur_rpy - last_rpy) / c['dt']
    ire = np.clip(ire - rot_e * c['dt'], f(-1500), f(1500))
    ire[0:2] = np.clip(ire[0:2], f(-1), f(1))
    tau = np.clip(-g[9:12] * rot_e + g[15:18] * rate_e + g[12:15] * ire, f(-3200), f(3200))
    pwm = np.clip(thrust + MIXER.astype(f) @ tau, c['min_pwm'], c['max_pwm'])
    rpm = c['pwm2rpm_scale'] * pwm + c['pwm2rpm_const']
    action = c['kf'] * rpm * rpm
    if obs.shape[0] == 6:
        action = np.array([action[0] + action[3], action[1] + action[2]], dtype=f)
    assert action.dtype == f and ipe.dtype == f and ire.dtype == f
    return action, (ipe, cur_rpy, ire)


def trace(obs, target_pos, target_vel, state, gains, cfg):
    """Which clips act in this step (float64): the saturation coverage tests/golden/make_pid.py insists on."""
    obs = np.asarray(obs, dtype=np.float64)
    _, (ipe, _, ire) = law(obs, target_pos, target_vel, state, gains, cfg)
    g = np.asarray(gains, dtype=np.float64)
    # the unclipped torques and PWMs, recomputed
    if obs.shape[0] == 6:
        pos, vel, rpy = np.array([obs[0], 0, obs[2]]), np.array([obs[1], 0, obs[3]]), np.array([0, obs[4], 0])
    else:
        pos, vel, rpy = obs[[0, 2, 4]], obs[[1, 3, 5]], obs[6:9]
    quat = bullet.quaternion_from_euler(rpy)
    R, cur_rpy = bullet.matrix_from_quaternion(quat), bullet.euler_from_quaternion(quat)
    pos_e, vel_e = target_pos - pos, target_vel - vel
    F = g[0:3] * pos_e + g[3:6] * ipe + g[6:9] * vel_e + np.array([0, 0, cfg['gravity']])
    along = float(np.dot(F, R[:, 2]))
    thrust = (np.sqrt(max(0.0, along) / (4 * cfg['kf'])) - cfg['pwm2rpm_const']) / cfg['pwm2rpm_scale']
    z_ax = F / np.linalg.norm(F)
    y_ax = np.cross(z_ax, [1.0, 0, 0]); y_ax /= np.linalg.norm(y_ax)
    Rt = np.stack([np.cross(y_ax, z_ax), y_ax, z_ax], axis=1)
    E = Rt.T @ R - R.T @ Rt
    rot_e = np.array([E[2, 1], E[0, 2], E[1, 0]])
    tau_raw = -g[9:12] * rot_e - g[15:18] * (cur_rpy - np.asarray(state[1])) / cfg['dt'] + g[12:15] * ire
    pwm_raw = thrust + MIXER @ np.clip(tau_raw, -3200, 3200)
    return dict(pwm_low=bool((pwm_raw < cfg['min_pwm']).any()), pwm_high=bool((pwm_raw > cfg['max_pwm']).any()),
                torque=bool((np.abs(tau_raw) > 3200).any()), z_integral=bool(abs(ipe[2]) == 0.15),
                rp_integral=bool((np.abs(ire[0:2]) == 1.0).any()), thrust_zero=bool(along <= 0.0))
