"""Case table for the step kernels OFF their fast paths: states at Bullet's +-100 coordinate-velocity clamp, rotation rates past the
exponential map's pi/4-per-substep cap and below its |w| < 1e-3 Taylor branch, and Quadrotor 2D lanes on both sides of the
constant-rotation recurrence's `free_run` guard (csrc/scg_env_core.h, `advance`).  Shared by tests/test_extreme_states_cpu.py (the
oracle alone: do the cases reach the paths they are meant to reach?) and tests/test_gpu_extreme_states.py (kernels against the oracle).
NumPy and the oracle only: neither torch nor the HIP library is imported here.

A case is (name, task, config overrides, builder): `task` names a tests/golden rollout whose config is the base, `builder(n, rng)`
returns (raw, actions, kinds) — the injected raw simulator state in scg_set_state's layout, the PHYSICAL actions (every config has
normalized_rl_action_space off) and the lane kind of every env.  Lane kinds are interleaved with a period of 8 lanes, so every wave of
64 lanes (and a ragged last one) holds all kinds of its case; no kind is given a wave of its own.
"""
import contextlib
import json
import os

import numpy as np

from oracle import bullet
from oracle.envs import OracleQuadrotor, make_oracle_env, make_rng

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
VMAX = bullet.MAX_COORDINATE_VELOCITY
CAP = bullet.ANGULAR_MOTION_THRESHOLD
PITCH_MAX = 1.2           # derived outputs (Euler angles: asin folds / gimbal branches beyond +-pi/2) are compared on |pitch| <= 1.2
N_STEPS = 3
WAVE = 64

COMMON = dict(normalized_rl_action_space=False, randomized_init=False, done_on_out_of_bound=False, auto_reset=False,
              randomized_inertial_prop=False, rew_exponential=False)        # (linear reward: exp(-1e4) would be 0 on every clamp lane)

_Q = OracleQuadrotor
F_MIN = _Q.KF * (_Q.PWM2RPM_SCALE * _Q.MIN_PWM + _Q.PWM2RPM_CONST) ** 2     # one motor's thrust range, N
F_MAX = _Q.KF * (_Q.PWM2RPM_SCALE * _Q.MAX_PWM + _Q.PWM2RPM_CONST) ** 2

# lane kinds
Q2_A, Q2_B, Q2_C, Q2_D, Q2_E = 'w_at_clamp', 'v_at_clamp', 'small', 'into_clamp', 'random'
Q3_CAP, Q3_NOCAP, Q3_T0, Q3_T1, Q3_RANDOM, Q3_SMALL = 'cap', 'no_cap', 'taylor_zero', 'taylor_tiny', 'random', 'small'


def _kinds(pattern, n):
    return np.array([pattern[i % len(pattern)] for i in range(n)])


def _sign(rng, n):
    return rng.choice([-1.0, 1.0], n)


# ------------------------------------------------------------------------------------------------------------------ builders
def q2_builder(spin_pitch0):
    """Quadrotor 2D, raw = (x, vx, z, vz, pitch, w); actions = the two thrust pairs (T1, T2), torque = arm (T2 - T1).
    spin_pitch0: the fast spinners (kinds a, d) start at pitch = -sign(w) * spin_pitch0 (+-0.1), so that one control step carries them
    to about +sign(w) * spin_pitch0."""
    pattern = [Q2_A, Q2_B, Q2_C, Q2_D, Q2_E, Q2_B, Q2_C, Q2_E]

    def build(n, rng):
        kinds = _kinds(pattern, n)
        raw = np.zeros((n, 6))
        raw[:, 0] = rng.uniform(-1, 1, n)
        raw[:, 2] = rng.uniform(0.5, 1.5, n)
        act = rng.uniform(2 * F_MIN, 2 * F_MAX, (n, 2))
        lo, hi = 2 * F_MIN * 1.02, 2 * F_MAX * 0.98
        for i in range(n):
            k, s = kinds[i], _sign(rng, 1)[0]
            if k == Q2_A:               # w0 = +-100 exactly: the guard is false for any torque; two lanes in three push outward
                raw[i, 5] = s * VMAX
                raw[i, 4] = -s * spin_pitch0 + rng.uniform(-0.1, 0.1)
                raw[i, [1, 3]] = rng.uniform(-1, 1, 2)
                t = rng.integers(3)
                if t == 0:
                    act[i] = rng.uniform(lo, hi)                                  # equal pairs: zero torque, w stays at the clamp
                else:
                    act[i] = (lo, hi) if s > 0 else (hi, lo)
            elif k == Q2_B:             # vx or vz = +-100 exactly, thrust pushing outward
                raw[i, 5] = rng.uniform(-1, 1)
                if rng.integers(2):
                    raw[i, 3] = s * VMAX                                          # vz: high thrust lifts, low thrust lets it fall
                    raw[i, 1] = rng.uniform(-1, 1)
                    raw[i, 4] = rng.uniform(-0.2, 0.2)
                    act[i] = hi if s > 0 else lo
                else:
                    raw[i, 1] = s * VMAX                                          # vx: the thrust's x component has the pitch's sign
                    raw[i, 3] = rng.uniform(-1, 1)
                    raw[i, 4] = s * rng.uniform(0.3, 0.5)
                    act[i] = hi
            elif k == Q2_C:             # small: the guard is true
                raw[i, [1, 3, 5]] = rng.uniform(-1, 1, 3)
                raw[i, 4] = rng.uniform(-0.2, 0.2)
            elif k == Q2_D:             # just inside the clamp, pushed into it during the step
                raw[i, 5] = s * 99.9
                raw[i, 4] = -s * spin_pitch0 + rng.uniform(-0.1, 0.1)
                act[i] = (lo, hi) if s > 0 else (hi, lo)
                sv = _sign(rng, 1)[0]
                raw[i, 3] = sv * 99.99
                raw[i, 1] = rng.uniform(-50, 50)
                if sv < 0:                                  # falling: thrust / m <= 8.8 < g, the same torque direction (n dw >= 0.16)
                    act[i] = (lo, lo + 0.008) if s > 0 else (lo + 0.008, lo)
            else:                       # in between
                raw[i, 5] = rng.uniform(-15, 15)
                raw[i, 4] = -np.sign(raw[i, 5]) * rng.uniform(0.0, 0.3)
                raw[i, [1, 3]] = rng.uniform(-60, 60, 2)
        return raw, act, kinds
    return build


def _q3_common(n, rng):
    raw = np.zeros((n, 13))
    raw[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    raw[:, 2] = rng.uniform(0.5, 1.5, n)
    raw[:, 3:7] = bullet.quaternion_from_euler(rng.uniform(-0.3, 0.3, (n, 3)))
    act = rng.uniform(F_MIN, F_MAX, (n, 4))
    return raw, act


def _sink(raw, act, i, rng, v=-VMAX):
    """vz at (or just inside) the lower clamp with all motors near their minimum: thrust / m < g in every attitude, so the clamp binds
    in every substep whatever the body does."""
    raw[i, 9] = v
    act[i] = F_MIN * rng.uniform(1.0, 1.3, 4)


def q3_clamp_builder(n, rng):
    """Quadrotor 3D, raw = (pos, quat xyzw, world velocity, world rates); actions = four motor thrusts.  Rates and velocities per
    component from {+-100, +-95, small}; three lanes in eight have all components small."""
    kinds = _kinds([Q3_RANDOM, Q3_RANDOM, Q3_SMALL, Q3_RANDOM, Q3_RANDOM, Q3_SMALL, Q3_RANDOM, Q3_SMALL], n)
    raw, act = _q3_common(n, rng)
    for i in range(n):
        small = rng.uniform(-1, 1, 6)
        if kinds[i] == Q3_SMALL:
            raw[i, 7:13] = small
            continue
        pick = rng.integers(0, 5, 6)
        vals = np.stack([np.full(6, VMAX), np.full(6, -VMAX), np.full(6, 95.0), np.full(6, -95.0), small])
        raw[i, 7:13] = vals[pick, np.arange(6)]
        if i % 2 == 0:
            _sink(raw, act, i, rng, -VMAX if rng.integers(2) else -99.999)
    return raw, act, kinds


def q3_cap_builder(n, rng):
    """Quadrotor 3D below ~693 Hz (the exponential map with Bullet's cap and Taylor branch).  cap: all three rates at +-100
    (|w| = 173.2); no_cap: |w| in (104, 130) with no component above 100; taylor_zero / taylor_tiny: w = 0 / (5e-4, 0, 0) with four equal
    motor commands (zero torque: |w| < 1e-3 in every substep)."""
    kinds = _kinds([Q3_CAP, Q3_NOCAP, Q3_T0, Q3_T1, Q3_RANDOM, Q3_CAP, Q3_NOCAP, Q3_T1], n)
    raw, act = _q3_common(n, rng)
    for i in range(n):
        k = kinds[i]
        raw[i, 7:10] = rng.uniform(-1, 1, 3)
        if k == Q3_CAP:
            raw[i, 10:13] = _sign(rng, 3) * VMAX
            _sink(raw, act, i, rng)
        elif k == Q3_NOCAP:
            u = _sign(rng, 3) * rng.uniform(0.6, 1.0, 3)
            raw[i, 10:13] = u / np.linalg.norm(u) * rng.uniform(104.0, 130.0)
            if i % 3 == 0:
                _sink(raw, act, i, rng)
        elif k in (Q3_T0, Q3_T1):
            raw[i, 10:13] = (5e-4, 0.0, 0.0) if k == Q3_T1 else 0.0
            act[i] = rng.uniform(F_MIN, F_MAX)
            if i % 2:
                raw[i, 7:10] = _sign(rng, 3) * VMAX
        else:
            raw[i, 10:13] = rng.uniform(-60, 60, 3)
            raw[i, 7:10] = rng.uniform(-60, 60, 3)
    return raw, act, kinds


def cartpole_builder(n, rng):
    """CartPole, raw = (x, x_dot, theta, theta_dot); x_dot and theta_dot from {+-100, +-99.9, small}, force in +-10.  cart_out: the cart
    at (or 0.1 inside) the clamp with a slow pole and the force pushing outward — F / (M + m) = 4.5 .. 9 m/s^2 keeps the clamp binding to
    the end of the step; spin: the pole at +-100 / +-99.9 rad/s (its 500 N centripetal term throws the cart back and forth, so whether a
    clamp still binds at the end is left to the dynamics), the cart at any of the five."""
    kinds = _kinds(['cart_out', 'spin', 'small', 'spin'], n)
    raw = np.zeros((n, 4))
    raw[:, 0] = rng.uniform(-1, 1, n)
    raw[:, 2] = rng.uniform(-0.5, 0.5, n)
    act = rng.uniform(-10, 10, (n, 1))
    vals = np.array([VMAX, -VMAX, 99.9, -99.9, 0.0])
    for i in range(n):
        small = rng.uniform(-1, 1, 2)
        raw[i, [1, 3]] = small
        if kinds[i] == 'cart_out':
            raw[i, 1] = vals[rng.integers(0, 4)]
            act[i] = np.sign(raw[i, 1]) * rng.uniform(5, 10)
        elif kinds[i] == 'spin':
            raw[i, 3] = vals[rng.integers(0, 4)]
            pick = rng.integers(0, 5)
            if pick < 4:
                raw[i, 1] = vals[pick]
    return raw, act, kinds


def q1_builder(n, rng):
    """Quadrotor 1D, raw = (z, vz); vz from {+-100, +-99.99, small}, total thrust from 0 (clipped to the motors' minimum) to max."""
    kinds = _kinds(['up', 'down', 'small', 'up_in', 'down_in', 'small', 'up', 'down'], n)
    raw = np.zeros((n, 2))
    raw[:, 0] = rng.uniform(0.5, 1.5, n)
    act = rng.uniform(0.0, 4 * F_MAX, (n, 1))
    vz = {'up': VMAX, 'down': -VMAX, 'up_in': 99.99, 'down_in': -99.99}
    for i in range(n):
        k = kinds[i]
        if k == 'small':
            raw[i, 1] = rng.uniform(-1, 1)
            continue
        raw[i, 1] = vz[k]
        if i % 4 != 3:                  # three lanes in four push outward (hover thrust is 0.265 N of the 0.113 .. 0.593 N range)
            act[i] = rng.uniform(0.35, 4 * F_MAX) if k.startswith('up') else rng.uniform(0.0, 0.2)
    return raw, act, kinds


def _step_dist(magnitude):
    return {'dynamics': [{'disturbance_func': 'step', 'magnitude': magnitude, 'step_offset': 0}]}


# (name, task, config overrides, builder).  q3_cap_240: at 240 Hz the cap would need |w| > pi/4 * 240 = 188.5, out of reach under the
# +-100 clamp (|w| <= 173.2), so that case pins "no cap, exact sin / cos, not small_angle" at a second substep length and nothing more.
CASES = [
    ('q2_guard', 'quadrotor_2D_track', dict(ctrl_freq=100, pyb_freq=1000), q2_builder(0.5)),
    ('q2_guard_dist', 'quadrotor_2D_track', dict(ctrl_freq=100, pyb_freq=1000, disturbances=_step_dist(0.05)), q2_builder(0.5)),
    ('q2_slow', 'quadrotor_2D_track', dict(ctrl_freq=50, pyb_freq=250), q2_builder(1.0)),
    ('q3_clamp', 'quadrotor_3D_track', dict(ctrl_freq=100, pyb_freq=1000), q3_clamp_builder),
    ('q3_cap', 'quadrotor_3D_track', dict(ctrl_freq=50, pyb_freq=200), q3_cap_builder),
    ('q3_cap_240', 'quadrotor_3D_track', dict(ctrl_freq=60, pyb_freq=240), q3_cap_builder),
    ('cartpole_clamp', 'cartpole_stab', dict(ctrl_freq=15, pyb_freq=750), cartpole_builder),
    ('cartpole_clamp_slow', 'cartpole_stab', dict(ctrl_freq=50, pyb_freq=250), cartpole_builder),
    ('cartpole_clamp_dist', 'cartpole_stab', dict(ctrl_freq=15, pyb_freq=750, disturbances=_step_dist(2.0)), cartpole_builder),
    ('q1_clamp', 'quadrotor_1D_track', dict(), q1_builder),
]
CASE_BY_NAME = {c[0]: c for c in CASES}
Q2_F32_RAGGED = ('q2_guard', 'q2_slow')            # the two disturbance-free Quadrotor 2D cases also run with a ragged last wave
SIZES = {name: ((192, 150) if name in Q2_F32_RAGGED else (192,)) for name in CASE_BY_NAME}
CASE_SIZES = [(name, n) for name in CASE_BY_NAME for n in SIZES[name]]
# (case, dtype) pairs that also run on the library compiled for their very config: one hipcc build each (tools/prebuild_specs.py)
SPECIALISED = [('q2_guard', 'f32'), ('q3_clamp', 'f32'), ('cartpole_clamp', 'f32'), ('q3_cap', 'f64')]


def load_config(case):
    """(env_id, config) of a case: the golden rollout's config with COMMON and the case's overrides on top."""
    name, task, over, _ = case
    g = np.load(os.path.join(GOLDEN, f'rollout_{task}.npz'))
    meta = json.loads(str(g['meta_json']))
    cfg = dict(meta['config'])
    cfg.pop('seed', None)
    cfg.update(COMMON)
    cfg.update(over)
    return meta['task'], cfg


def build(case, n):
    """(raw, actions, kinds) of a case at n lanes; the draw depends on the case and on n only."""
    seed = [sum(case[0].encode()), n]
    return case[3](n, np.random.default_rng(seed))


# ------------------------------------------------------------------------------------------------------------------ oracle <-> raw
def raw_state(oracle):
    """Oracle -> raw simulator state layout of scg_set_state."""
    if oracle.NAME == 'cartpole':
        return oracle.state.copy()
    if oracle.QUAD_TYPE == 1:
        return np.stack([oracle.pos[:, 2], oracle.vel[:, 2]], axis=1)
    if oracle.QUAD_TYPE == 2:
        # unfolded pitch of the pure y-rotation (rpy[1] folds beyond +-pi/2 when done_on_out_of_bound is off)
        theta = 2.0 * np.arctan2(oracle.quat[:, 1], oracle.quat[:, 3])
        return np.stack([oracle.pos[:, 0], oracle.vel[:, 0], oracle.pos[:, 2], oracle.vel[:, 2],
                         theta, oracle.ang_v[:, 1]], axis=1)
    return np.concatenate([oracle.pos, oracle.quat, oracle.vel, oracle.ang_v], axis=1)


def inject(oracle, raw):
    """The inverse of raw_state: fill every env of an oracle from a raw state, through set_body_state."""
    raw = np.asarray(raw, dtype=np.float64)
    idx = np.arange(oracle.num_envs)
    z = np.zeros(len(raw))
    if oracle.NAME == 'cartpole':
        oracle.set_body_state(idx, raw.copy())
        return
    if oracle.QUAD_TYPE == 1:
        pos, vel = np.stack([z, z, raw[:, 0]], axis=1), np.stack([z, z, raw[:, 1]], axis=1)
        quat, ang = np.tile([0.0, 0.0, 0.0, 1.0], (len(raw), 1)), np.zeros((len(raw), 3))
    elif oracle.QUAD_TYPE == 2:
        pos, vel = np.stack([raw[:, 0], z, raw[:, 2]], axis=1), np.stack([raw[:, 1], z, raw[:, 3]], axis=1)
        quat = np.stack([z, np.sin(0.5 * raw[:, 4]), z, np.cos(0.5 * raw[:, 4])], axis=1)
        ang = np.stack([z, raw[:, 5], z], axis=1)
    else:
        pos, quat, vel, ang = raw[:, 0:3].copy(), raw[:, 3:7].copy(), raw[:, 7:10].copy(), raw[:, 10:13].copy()
    oracle.set_body_state(idx, pos, quat, vel, ang)


def make_oracle(case, n, seed=3):
    """A reset oracle env of the case with the case's state injected; returns (oracle, raw, actions, kinds)."""
    env_id, cfg = load_config(case)
    oracle = make_oracle_env(env_id, n, make_rng('philox', n, seed), **cfg)
    oracle.reset()
    raw, act, kinds = build(case, n)
    inject(oracle, raw)
    return oracle, raw, act, kinds


def velocity_columns(oracle):
    """Columns of the raw state that carry Bullet's +-100 clamp."""
    if oracle.NAME == 'cartpole':
        return [1, 3]
    return {1: [1], 2: [1, 3, 5], 3: [7, 8, 9, 10, 11, 12]}[oracle.QUAD_TYPE]


def pitch_of(oracle, raw):
    """The angle whose range bounds the derived-output comparison: the unfolded pitch (Quadrotor 2D), the Euler pitch (3D), none
    (CartPole's angle is never folded, Quadrotor 1D has none)."""
    if oracle.NAME == 'cartpole' or oracle.QUAD_TYPE == 1:
        return np.zeros(len(raw))
    if oracle.QUAD_TYPE == 2:
        return raw[:, 4]
    return bullet.euler_from_quaternion(raw[:, 3:7])[:, 1]


@contextlib.contextmanager
def unclamped_trace():
    """While active, every Bullet substep of the oracle is also evaluated WITHOUT the coordinate-velocity clamp from the same
    (clamped) pre-state; yields a list that receives each substep's unclamped velocities, in the raw layout's column order — the last
    entry after an oracle step is what the final substep's update would have been: its excess over 100 is the overshoot."""
    trace = []
    q_orig, c_orig = bullet.quadrotor_substep, bullet.cartpole_substep

    def free(fn, *a, **k):
        keep = bullet.MAX_COORDINATE_VELOCITY
        bullet.MAX_COORDINATE_VELOCITY = np.inf
        try:
            return fn(*a, **k)
        finally:
            bullet.MAX_COORDINATE_VELOCITY = keep

    def quad(*a, **k):
        _, _, vel, omega = free(q_orig, *a, **k)
        trace.append((vel, omega))
        return q_orig(*a, **k)

    def cart(*a, **k):
        _, xd, _, thd = free(c_orig, *a, **k)
        trace.append((xd, thd))
        return c_orig(*a, **k)

    bullet.quadrotor_substep, bullet.cartpole_substep = quad, cart
    try:
        yield trace
    finally:
        bullet.quadrotor_substep, bullet.cartpole_substep = q_orig, c_orig


def last_unclamped(oracle, trace):
    """The final substep's unclamped velocities as an array over velocity_columns(oracle)."""
    a, b = trace[-1]
    if oracle.NAME == 'cartpole':
        return np.stack([a, b], axis=1)
    if oracle.QUAD_TYPE == 1:
        return a[:, 2:3]
    if oracle.QUAD_TYPE == 2:
        return np.stack([a[:, 0], a[:, 2], b[:, 1]], axis=1)
    return np.concatenate([a, b], axis=1)


# ------------------------------------------------------------------------------------------------------------------ predicates
def predicates(case, oracle, before, after, actions):
    """Per-lane booleans, float64, from the oracle alone: `before` / `after` are raw_state(oracle) around ONE control step taken with
    `actions`; `oracle` supplies the constants (substep length, mass, inertia).

    guard_false / guard_true  Quadrotor 2D: the kernel's `free_run` test, |w0| + n |dw| < 100 and max(|vx|, |vz|) + n h a_max < 100,
                              evaluated in float64 — certainly false when a side reaches 100 (kinds a, b: it starts there) or passes it
                              by 1e-2, certainly true when both sides stay below 99.99 (kind c: below 7).  False everywhere else.
    clamp                     a velocity component ends the step at exactly +-100.0
    cap                       |w0| h > 1.05 pi / 4: the cap binds in the first substep by construction (Quadrotor 3D)
    taylor                    |w| < 1e-3 before and after the step (Quadrotor 3D)
    pitch_ok                  |pitch| <= 1.2 after the step
    """
    n = len(before)
    no = np.zeros(n, dtype=bool)
    out = dict(guard_false=no.copy(), guard_true=no.copy(), cap=no.copy(), taylor=no.copy())
    h, nsub = oracle.PYB_TIMESTEP, oracle.PYB_STEPS_PER_CTRL
    vc = velocity_columns(oracle)
    out['clamp'] = (np.abs(after[:, vc]) == VMAX).any(axis=1)
    out['pitch_ok'] = np.abs(pitch_of(oracle, after)) <= PITCH_MAX
    if oracle.NAME == 'quadrotor' and oracle.QUAD_TYPE == 2:
        f = np.clip(actions, 2 * F_MIN, 2 * F_MAX)                                  # the pairs' total thrusts
        dw = h * _Q.PROP_OFFSET * np.abs(f[:, 1] - f[:, 0]) / oracle.J_env[:, 1]
        fd = 0.0
        if 'dynamics' in oracle.disturbances:
            fd = max(abs(d.magnitude) for d in oracle.disturbances['dynamics'].disturbances) / oracle.mass_env
        amax = f.sum(axis=1) / oracle.mass_env + np.maximum(fd, np.abs(fd - _Q.GRAVITY_ACC))
        lw = np.abs(before[:, 5]) + nsub * dw
        lv = np.abs(before[:, [1, 3]]).max(axis=1) + nsub * h * amax
        at = (np.abs(before[:, 5]) >= VMAX) | (np.abs(before[:, [1, 3]]).max(axis=1) >= VMAX)
        out['guard_false'] = at | (lw >= VMAX + 1e-2) | (lv >= VMAX + 1e-2)
        out['guard_true'] = (lw <= VMAX - 1e-2) & (lv <= VMAX - 1e-2)
    if oracle.NAME == 'quadrotor' and oracle.QUAD_TYPE == 3:
        w0 = np.linalg.norm(before[:, 10:13], axis=1)
        w1 = np.linalg.norm(after[:, 10:13], axis=1)
        out['cap'] = w0 * h > 1.05 * CAP
        out['taylor'] = (w0 < 1e-3) & (w1 < 1e-3)
    return out


def waves(n):
    """Lane slices of the 64-lane waves of an n-lane launch (the last one may be ragged)."""
    return [slice(a, min(a + WAVE, n)) for a in range(0, n, WAVE)]
