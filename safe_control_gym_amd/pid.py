"""The reference's PID baseline (controllers/pid/pid.py: the DSL cascade position / attitude PID of the Crazyflie) on the HIP engine, for a
batch of envs.

    ctrl = make('pid', env_func, num_envs=4096, init_states=x0)       # registration.py
    ctrl.set_gains(grid)            # optional: one gain set [18] per env
    ctrl.run()                      # the whole episode of every env, closed loop, ONE launch (scg_rollout_pid, include/scg_pid.h)

One env is one closed loop: its own start state, its own gains (`set_gains`), with randomized_inertial_prop its own inertial draw
(`set_params`).  The controller's state (position integral, last rpy, attitude integral) lives in registers during the launch and in a
[9, N] device tensor between launches.  `select_action` is the same law in NumPy on the host, stateful like upstream, for one
observation or a batch.

Served: Quadrotor 2D and 3D, stabilisation and tracking; the env takes physical actions (normalized_rl_action_space off) and observes its
state (cost: quadratic).  `run` has no CPU path.
"""
import os

import numpy as np

from safe_control_gym_amd.env_config import EnvSpec
from safe_control_gym_amd.lqr import BatchedController

# controllers/pid/pid.yaml as shipped.  Its upper-case keys do not meet the constructor's lower-case arguments (upstream neither): they
# become attributes, and the attributes of the same name are then set from the constructor's arguments.
PID_DEFAULTS = dict(g=9.8, KF=3.16e-10, KM=7.94e-12, P_COEFF_FOR=[.4, .4, 1.25], I_COEFF_FOR=[.05, .05, .05], D_COEFF_FOR=[.2, .2, .5],
                    P_COEFF_TOR=[70000., 70000., 60000.], I_COEFF_TOR=[.0, .0, 500.], D_COEFF_TOR=[20000., 20000., 12000.],
                    PWM2RPM_SCALE=0.2685, PWM2RPM_CONST=4070.3, MIN_PWM=20000, MAX_PWM=65535)

MIXER_MATRIX = np.array([[.5, -.5, -1], [.5, .5, 1], [-.5, .5, -1], [-.5, -.5, 1]])


def _pose(rpy):
    """PyBullet's Euler -> quaternion -> (rotation matrix, Euler) round trip (getQuaternionFromEuler, getMatrixFromQuaternion,
    getEulerFromQuaternion with its gimbal branches), batched over the leading axis: what pid.py:99-104, 177, 222-223 compute."""
    hr, hp, hy = 0.5 * rpy[..., 0], 0.5 * rpy[..., 1], 0.5 * rpy[..., 2]
    cr, sr, cp, sp, cy, sy = np.cos(hr), np.sin(hr), np.cos(hp), np.sin(hp), np.cos(hy), np.sin(hy)
    x, y = sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy
    z, w = cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy
    s = 2.0 / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s
    R = np.stack([np.stack([1.0 - (y * ys + z * zs), x * ys - w * zs, x * zs + w * ys], -1),
                  np.stack([x * ys + w * zs, 1.0 - (x * xs + z * zs), y * zs - w * xs], -1),
                  np.stack([x * zs - w * ys, y * zs + w * xs, 1.0 - (x * xs + y * ys)], -1)], -2)
    sarg = -2.0 * (x * z - w * y)
    lo, hi = sarg <= -0.99999, sarg >= 0.99999
    roll = np.where(lo | hi, 0.0, np.arctan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z))
    pitch = np.where(lo, -0.5 * np.pi, np.where(hi, 0.5 * np.pi, np.arcsin(np.clip(sarg, -1.0, 1.0))))
    yaw = np.where(lo, 2.0 * np.arctan2(x, -y), np.where(hi, 2.0 * np.arctan2(-x, y), np.arctan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z)))
    return R, np.stack([roll, pitch, yaw], -1)


class PID(BatchedController):
    """controllers/pid/pid.py closing the loop of `num_envs` envs in one launch.  The lazy device side (fixed initial states, `_restart`,
    `set_params`, `set_initial_states`, `close`) is lqr.BatchedController's, shared with LQR / iLQR."""

    def __init__(self, env_func=None, g=9.8, kf=3.16e-10, km=7.94e-12, p_coeff_for=(.4, .4, 1.25), i_coeff_for=(.05, .05, .05),
                 d_coeff_for=(.2, .2, .5), p_coeff_tor=(70000., 70000., 60000.), i_coeff_tor=(.0, .0, 500.), d_coeff_tor=(20000., 20000., 12000.),
                 pwm2rpm_scale=0.2685, pwm2rpm_const=4070.3, min_pwm=20000, max_pwm=65535, num_envs=1, dtype='float64', init_states=None,
                 prior_info=None, training=True, checkpoint_path='temp/model_latest.pt', output_dir='temp', use_gpu=True, seed=0, **kwargs):
        self._init_common(env_func, num_envs, dtype, init_states, prior_info, training, checkpoint_path, output_dir, use_gpu, seed, kwargs)
        if self.env_id != 'quadrotor':
            raise NotImplementedError('[ERROR] PID not implemented for any system other than Quadrotor (2D and 3D).')
        if int(self.task_config.get('quad_type', 2)) == 1:
            raise NotImplementedError('PID serves Quadrotor 2D and 3D; upstream has no branch for Quadrotor 1D (it ends in an UnboundLocalError)')
        self.spec = EnvSpec(self.env_id, dict(self.task_config))
        spec = self.spec
        if spec.kw.get('normalized_rl_action_space', False):
            raise ValueError('pid computes physical actions: the env must have normalized_rl_action_space=False')
        if spec.obs_dim != spec.nx:
            raise ValueError('pid needs an env that observes its state (cost: quadratic)')
        self.g, self.KF, self.KM = g, kf, km
        self.P_COEFF_FOR, self.I_COEFF_FOR, self.D_COEFF_FOR = np.array(p_coeff_for, dtype=float), np.array(i_coeff_for, dtype=float), np.array(d_coeff_for, dtype=float)
        self.P_COEFF_TOR, self.I_COEFF_TOR, self.D_COEFF_TOR = np.array(p_coeff_tor, dtype=float), np.array(i_coeff_tor, dtype=float), np.array(d_coeff_tor, dtype=float)
        self.PWM2RPM_SCALE, self.PWM2RPM_CONST = np.array(pwm2rpm_scale, dtype=float), np.array(pwm2rpm_const, dtype=float)
        self.MIN_PWM, self.MAX_PWM = np.array(min_pwm, dtype=float), np.array(max_pwm, dtype=float)
        self.MIXER_MATRIX = MIXER_MATRIX
        self.control_timestep = spec.CTRL_TIMESTEP
        self.reference = np.asarray(spec.X_GOAL, dtype=np.float64)
        self._init_episode()
        self.model = self.get_prior()
        self.GRAVITY = self.g * self.model.quad_mass                  # pid.py:250
        self.gains = self.default_gains()                             # [18], or [N, 18] after set_gains
        self._gains_t = None
        self.reset_before_run()

    # ---- gains
    def default_gains(self):
        return np.concatenate([self.P_COEFF_FOR, self.I_COEFF_FOR, self.D_COEFF_FOR, self.P_COEFF_TOR, self.I_COEFF_TOR, self.D_COEFF_TOR])

    def set_gains(self, gains):
        """[18] for every env or [N, 18] per env: P / I / D force, then P / I / D torque, three values each."""
        gains = np.asarray(gains, dtype=np.float64)
        if gains.shape not in ((18,), (self.num_envs, 18)):
            raise ValueError(f'gains must be [18] or [{self.num_envs}, 18]')
        self.gains = gains.copy()
        self._gains_t = None

    def config_struct(self):
        from safe_control_gym_amd import _ilqr
        return _ilqr.PidConfig(kf=float(self.KF), gravity=float(self.GRAVITY), pwm2rpm_scale=float(self.PWM2RPM_SCALE),
                               pwm2rpm_const=float(self.PWM2RPM_CONST), min_pwm=float(self.MIN_PWM), max_pwm=float(self.MAX_PWM),
                               dt=float(self.control_timestep))

    # ---- the controller's state
    def reset(self):
        """pid.py:245-252: the controller's state is cleared (the device env is created lazily, at the first run)."""
        self.reset_before_run()

    def reset_before_run(self, obs=None, info=None, env=None):
        """pid.py:254-266: zero the integrals and the last rpy.  The three arrays are [3] for num_envs = 1 (upstream's shape) and [N, 3] for
        a batch: their shape follows num_envs, not the observation, and select_action broadcasts them against what it is given (a
        num_envs = 1 controller fed a batch [M, nx] returns M actions and leaves [M, 3] state behind)."""
        shape = (3,) if self.num_envs == 1 else (self.num_envs, 3)
        self.integral_pos_e, self.last_rpy, self.integral_rpy_e = np.zeros(shape), np.zeros(shape), np.zeros(shape)

    def save(self, path):
        """The three state arrays (np.savez; upstream pickles a tuple with np.save)."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'wb') as f:
            np.savez(f, integral_pos_e=self.integral_pos_e, last_rpy=self.last_rpy, integral_rpy_e=self.integral_rpy_e)

    def load(self, path):
        with np.load(path) as z:
            self.integral_pos_e, self.last_rpy, self.integral_rpy_e = z['integral_pos_e'], z['last_rpy'], z['integral_rpy_e']

    # ---- the host law
    def select_action(self, obs, info=None):
        """pid.py:83-243 in NumPy for one observation [nx] or a batch [N, nx]; advances the controller's state as upstream does."""
        obs = np.asarray(obs, dtype=np.float64)
        step = 0 if info is None else int(info['current_step'])
        ref, dt = self.reference, self.control_timestep
        two_d = self.spec.nx == 6
        zero = np.zeros_like(obs[..., 0])
        if two_d:
            pos, vel = np.stack([obs[..., 0], zero, obs[..., 2]], -1), np.stack([obs[..., 1], zero, obs[..., 3]], -1)
            rpy = np.stack([zero, obs[..., 4], zero], -1)
            ip, iv = (0, None, 2), (1, None, 3)
        else:
            pos, vel, rpy = obs[..., [0, 2, 4]], obs[..., [1, 3, 5]], obs[..., 6:9]
            ip, iv = (0, 2, 4), (1, 3, 5)
        if self.spec.TASK == 'traj_tracking':
            row = ref[min(step, ref.shape[0] - 1)]
            target_vel = np.array([0.0 if k is None else row[k] for k in iv])
        else:
            row, target_vel = ref.reshape(-1), np.zeros(3)
        target_pos = np.array([0.0 if k is None else row[k] for k in ip])
        G = self.gains
        R, cur_rpy = _pose(rpy)
        pos_e, vel_e = target_pos - pos, target_vel - vel
        ipe = np.clip(self.integral_pos_e + pos_e * dt, -2., 2.)
        ipe[..., 2] = np.clip(ipe[..., 2], -0.15, .15)
        self.integral_pos_e = ipe
        F = G[..., 0:3] * pos_e + G[..., 3:6] * ipe + G[..., 6:9] * vel_e + np.array([0, 0, self.GRAVITY])
        scalar_thrust = np.maximum(0., np.sum(F * R[..., :, 2], -1))
        thrust = (np.sqrt(scalar_thrust / (4 * self.KF)) - self.PWM2RPM_CONST) / self.PWM2RPM_SCALE
        z_ax = F / np.linalg.norm(F, axis=-1, keepdims=True)
        y_ax = np.cross(z_ax, np.array([1.0, 0.0, 0.0]))
        y_ax = y_ax / np.linalg.norm(y_ax, axis=-1, keepdims=True)
        Rt = np.stack([np.cross(y_ax, z_ax), y_ax, z_ax], -1)
        M = np.swapaxes(Rt, -1, -2) @ R
        E = M - np.swapaxes(M, -1, -2)
        rot_e = np.stack([E[..., 2, 1], E[..., 0, 2], E[..., 1, 0]], -1)
        rate_e = -(cur_rpy - self.last_rpy) / dt
        self.last_rpy = cur_rpy
        ire = np.clip(self.integral_rpy_e - rot_e * dt, -1500., 1500.)
        ire[..., 0:2] = np.clip(ire[..., 0:2], -1., 1.)
        self.integral_rpy_e = ire
        tau = np.clip(-G[..., 9:12] * rot_e + G[..., 15:18] * rate_e + G[..., 12:15] * ire, -3200, 3200)
        pwm = np.clip(thrust[..., None] + tau @ self.MIXER_MATRIX.T, self.MIN_PWM, self.MAX_PWM)
        action = self.KF * (self.PWM2RPM_SCALE * pwm + self.PWM2RPM_CONST) ** 2
        if two_d:
            action = np.stack([action[..., 0] + action[..., 3], action[..., 1] + action[..., 2]], -1)
        return action

    # ---- the device side
    def _state_tensor(self):
        s = np.concatenate([np.reshape(a, (self.num_envs, 3)) for a in (self.integral_pos_e, self.last_rpy, self.integral_rpy_e)], axis=1)
        return self._torch.as_tensor(np.ascontiguousarray(s.T), dtype=self._tdtype, device=self._env().device).contiguous()

    def _gain_tensor(self):
        if self._gains_t is None:
            g = self.gains if self.gains.ndim == 1 else np.ascontiguousarray(self.gains.T)
            self._gains_t = self._torch.as_tensor(g, dtype=self._tdtype, device=self._env().device).contiguous()
        return self._gains_t

    def learn(self, env=None, **kwargs):
        """pid.py: nothing to learn."""

    def run(self, env=None, max_steps=None, **kwargs):
        """The closed loop of every env from its initial state, the controller's state zeroed, in ONE launch; the dict LQR.run returns.
        max_steps (at most the episode's length, the default) cuts the launch short.  The controller's state after the run is copied
        back into integral_pos_e / last_rpy / integral_rpy_e."""
        venv = self._env()
        T = self.max_steps if max_steps is None else int(max_steps)
        if not 1 <= T <= self.max_steps:
            raise ValueError(f'max_steps must be in 1 .. {self.max_steps}')
        self._restart()
        self.reset_before_run()
        b = self._buffers()
        state = self._state_tensor()
        venv.rollout_pid(self._gain_tensor(), self.config_struct(), T, b['x'][:T], b['u'][:T], b['final_obs'], b['stats'],
                         b['n_steps'], b['final_flags'], pid_state=state, per_env=self.gains.ndim == 2)
        s = state.cpu().numpy().astype(np.float64).T                  # [N, 9]
        squeeze = (lambda a: a[0]) if self.num_envs == 1 else (lambda a: a)
        self.integral_pos_e, self.last_rpy, self.integral_rpy_e = squeeze(s[:, 0:3].copy()), squeeze(s[:, 3:6].copy()), squeeze(s[:, 6:9].copy())
        stats = b['stats'].cpu().numpy().astype(np.float64)
        n = np.maximum(stats[1], 1.0)
        self.results_dict = {'obs': b['x'], 'action': b['u'], 'final_obs': b['final_obs'], 'n_steps': b['n_steps']}
        return {'ep_returns': -stats[0], 'ep_lengths': stats[1].astype(np.int64), 'constraint_violation': stats[2], 'mse': stats[3] / n}
