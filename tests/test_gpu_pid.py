"""The pid controller on the GPU (csrc/scg_pid.h, safe_control_gym_amd/pid.py): scg_rollout_pid against the reference-generated fixture
(tests/golden/make_pid.py), the NumPy model (tests/pid_model.py) and scg_step_sequence.  N from {1, 64, 65, 130}: a lone thread, a full
wave, a second block of one thread, a ragged third block."""
import numpy as np
import pytest

from tests import pid_cases as PC
from tests import pid_model as M

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


def _setup(name, n, dtype='float64', states=None, **kw):
    ctrl = PC.controller(name, num_envs=n, dtype=dtype, **kw)
    venv = ctrl._env()
    if states is not None:
        ctrl.set_initial_states(states)
    return ctrl, venv


def _spread(name, n, scale=0.02, seed=0):
    """n raw start states around the case's own (Quadrotor 2D: the raw state is the state vector)."""
    base = PC.fixture()[f'{name}/x'][0]
    return base + scale * np.random.default_rng(seed).uniform(-1, 1, size=(n, base.shape[0]))


def _outputs(venv, T, fill=0.0):
    f = dict(dtype=venv.dtype, device=venv.device)
    u8 = dict(dtype=torch.uint8, device=venv.device)
    n, nx, nu = venv.num_envs, venv.spec.nx, venv.spec.nu
    return dict(x=torch.full((T, nx, n), fill, **f), u=torch.full((T, nu, n), fill, **f), final_obs=torch.full((nx, n), fill, **f),
                stats=torch.zeros(4, n, **f), n_steps=torch.zeros(n, dtype=torch.int32, device=venv.device), final_flags=torch.zeros(n, **u8),
                reward=torch.full((T, n), fill, **f), done=torch.full((T, n), 255, **u8), flags=torch.full((T, n), 255, **u8))


def _gains(venv, g):
    g = np.asarray(g, dtype=np.float64)
    return torch.as_tensor(np.ascontiguousarray(g if g.ndim == 1 else g.T), dtype=venv.dtype, device=venv.device).contiguous()


def _state(venv, s=None):
    s = np.zeros((venv.num_envs, 9)) if s is None else np.asarray(s, dtype=np.float64)
    return torch.as_tensor(np.ascontiguousarray(s.T), dtype=venv.dtype, device=venv.device).contiguous()


def _run(ctrl, venv, T, gains=None, state=None, fill=0.0, restart=True):
    gains = ctrl.gains if gains is None else gains
    o = _outputs(venv, T, fill)
    if restart:
        ctrl._restart()
    venv.rollout_pid(_gains(venv, gains), ctrl.config_struct(), T, pid_state=state, per_env=np.ndim(gains) == 2, **o)
    return o


def _replay_law(name, x, n, gains, cfg, start=None):
    """tests/pid_model.py fed the observations x [n, nx] of one env, carrying its own state: (u [n, nu], state [n, 9])."""
    fx = PC.fixture()
    tracking = PC.settings()['cases'][name]['task']['task'] == 'traj_tracking'
    state = (np.zeros(3), np.zeros(3), np.zeros(3)) if start is None else (start[0:3], start[3:6], start[6:9])
    us, ss = [], []
    for t in range(n):
        tp, tv = M.targets(fx[f'{name}/x_goal'], tracking, t, x.shape[1])
        u, state = M.law(x[t], tp, tv, state, gains, cfg)
        us.append(u); ss.append(np.concatenate(state))
    return np.asarray(us), np.asarray(ss)


@pytest.mark.parametrize('name', PC.cases())
def test_fixture_parity_float64(name):
    """The reference's closed loop, replicated over 65 envs, through PID.run.  Against the reference: max(1e-9, 10 x model_deviation), the
    bound the fixture's generator measured — closed loops included, and this law's closed loop amplifies a rounding-level difference by
    ~15 % per step (the attitude loop's D_tor / dt ~ 1e6 against the +-3200 torque clip), so over 250 steps that bound is wide.  What
    pins the kernel: over the first 32 steps the closed loop equals the reference's within the bound's floor, 1e-9, and the NumPy model fed the KERNEL'S OWN observations must return the kernel's actions and its final
    state within 1e-9 at every step of the whole episode (nothing is amplified there), and every env equals env 0 bit for bit."""
    fx = PC.fixture()
    ctrl, venv = _setup(name, 65)
    res = ctrl.run()
    xs, us, ss = fx[f'{name}/x'], fx[f'{name}/u'], fx[f'{name}/state']
    n = us.shape[0]
    assert (res['ep_lengths'] == n).all()
    x = ctrl.results_dict['obs'][:n].cpu().numpy()
    u = ctrl.results_dict['action'][:n].cpu().numpy()
    final = ctrl.results_dict['final_obs'].cpu().numpy()
    state = np.concatenate([ctrl.integral_pos_e, ctrl.last_rpy, ctrl.integral_rpy_e], axis=1)
    for a in (x, u, final):
        assert np.array_equal(a, np.repeat(a[..., :1], 65, axis=-1))
    assert np.array_equal(state, np.repeat(state[:1], 65, axis=0)) and np.array_equal(res['ep_returns'], np.repeat(res['ep_returns'][:1], 65))
    dev = max(PC.rel(x[:, :, 0], xs[:n]), PC.rel(final[:, 0], xs[n]), PC.rel(u[:, :, 0], us), PC.rel(state[0], ss[n - 1]),
              abs(res['ep_returns'][0] - float(fx[f'{name}/ret'])) / abs(float(fx[f'{name}/ret'])))
    h = min(n, 32)
    head = max(PC.rel(x[:h, :, 0], xs[:h]), PC.rel(u[:h, :, 0], us[:h]))
    mu, ms = _replay_law(name, x[:, :, 0], n, fx[f'{name}/gains'], PC.config(name))
    law = max(PC.rel(mu, u[:, :, 0]), PC.rel(ms[-1], state[0]))
    print(f'{name}: against the reference {dev:.3e} (bound {PC.bound():.3e}), first {h} steps {head:.3e}; the model on the kernel\'s observations {law:.3e}')
    assert dev <= PC.bound()
    # the first 32 steps, where the loop has amplified a device-against-oracle physics difference of ~1e-13 by no more than 1.15^32 ~ 90:
    # the floor of the bound holds against the reference itself
    assert head <= 1e-9
    assert law <= 1e-9
    ctrl.close()


def _raw_states(obs):
    """Raw simulator states that present `obs` to the controller (Quadrotor 3D: position, quaternion, velocity, WORLD body rates)."""
    if obs.shape[1] == 6:
        return obs.copy()
    from oracle import bullet
    quat = bullet.quaternion_from_euler(obs[:, 6:9])
    R = bullet.matrix_from_quaternion(quat)
    return np.concatenate([obs[:, [0, 2, 4]], quat, obs[:, [1, 3, 5]], np.einsum('nij,nj->ni', R, obs[:, 9:12])], axis=1)


@pytest.mark.parametrize('qt', [2, 3])
def test_one_step_differential(qt):
    """The recorded one-step cases (random observations, random preset controller state; thrust clamped at 0 in half of them, the roll /
    pitch integral at its limit in a quarter) as raw states + d_pid_state, k_steps = 1, N = 130 (the 128 cases and two repeats).  The
    kernel restates PyBullet's Euler -> quaternion -> Euler round trip, so its domain is not restricted: ALL cases are compared, u and
    the state written back, with the NumPy model on the observation the kernel saw (x[0]).  The env itself never reports |pitch| >=
    pi/2 (it observes an equivalent attitude), so for Quadrotor 3D those cases reach the kernel as the same rotation in other angles;
    the cases with |pitch| < pi/2 reach it as recorded and are compared with the reference's recorded action as well."""
    fx = PC.fixture()
    name = f'quadrotor_{qt}D_stab'
    idx = np.concatenate([np.arange(128), [5, 77]])
    obs, pre, ref_u = fx[f'one_step_{qt}D/obs'][idx], fx[f'one_step_{qt}D/pre'][idx], fx[f'one_step_{qt}D/u'][idx]
    ctrl, venv = _setup(name, 130, states=_raw_states(obs))
    state = _state(venv, pre)
    o = _run(ctrl, venv, 1, state=state)
    x0, u, post = o['x'][0].cpu().numpy().T, o['u'][0].cpu().numpy().T, state.cpu().numpy().T
    cfg, gains = PC.config(name), fx[f'{name}/gains']
    tp, tv = M.targets(fx[f'{name}/x_goal'], False, 0, obs.shape[1])
    mu, ms, zero = [], [], 0
    for k in range(130):
        a, s = M.law(x0[k], tp, tv, (pre[k, 0:3], pre[k, 3:6], pre[k, 6:9]), gains, cfg)
        zero += M.trace(x0[k], tp, tv, (pre[k, 0:3], pre[k, 3:6], pre[k, 6:9]), gains, cfg)['thrust_zero']
        mu.append(a); ms.append(np.concatenate(s))
    assert zero >= 8
    inside = np.abs(obs[:, 4 if qt == 2 else 7]) < 0.5 * np.pi - 0.01
    assert inside.sum() >= 64
    seen = PC.rel(x0[inside], obs[inside])
    d_model, d_ref = max(PC.rel(u, np.asarray(mu)), PC.rel(post, np.asarray(ms))), PC.rel(u[inside], ref_u[inside])
    print(f'{qt}D one-step: against the model {d_model:.3e}; |pitch| < pi/2 ({int(inside.sum())} cases): observation {seen:.3e}, against the reference {d_ref:.3e}')
    # (an observation off by up to 1e-12 reaches the torque through D_tor / dt = 1e6 and the mixer: <= 4e-6 on PWM values >= 2e4, squared)
    assert d_model <= 1e-9 and seen <= 1e-12 and d_ref <= 1e-8 <= PC.bound()
    ctrl.close()


@pytest.mark.parametrize('name,T', [('quadrotor_2D_saturating', 36), ('quadrotor_3D_track', 40)])
def test_rollout_equals_step_sequence_fed_its_actions(name, T):
    n = 65
    states = _spread(name, n) if '2D' in name else None
    ctrl, venv = _setup(name, n, states=states)
    g = np.tile(ctrl.gains, (n, 1)) * (1.0 + 0.1 * np.linspace(-1, 1, n))[:, None]           # gains that differ from env to env
    o = _run(ctrl, venv, T, gains=g)
    ns = o['n_steps'].long()
    assert (ns >= 1).all()
    ctrl._restart()
    seq = venv.step_sequence(torch.nan_to_num(o['u']).permute(0, 2, 1).contiguous(), terminal_obs=False)
    nx = ctrl.spec.nx
    took = torch.arange(T, device=venv.device).view(T, 1) < ns.view(1, n)
    obs = seq['obs'].permute(0, 2, 1)
    nxt = took[1:].view(T - 1, 1, n).expand(T - 1, nx, n)
    assert torch.equal(obs[:-1][nxt], o['x'][1:][nxt])
    assert torch.equal(obs.gather(0, (ns - 1).view(1, 1, n).expand(1, nx, n))[0], o['final_obs'])
    for k in ('reward', 'done', 'flags'):
        assert torch.equal(seq[k][took], o[k][took]), k
    ctrl.close()


def test_shared_and_per_env_gains():
    name, n, T = 'quadrotor_2D_stab', 130, 30
    ctrl, venv = _setup(name, n, states=_spread(name, n))
    a = _run(ctrl, venv, T)
    b = _run(ctrl, venv, T, gains=np.tile(ctrl.gains, (n, 1)))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    rng = np.random.default_rng(5)
    g = np.tile(ctrl.gains, (n, 1)) * rng.uniform(0.5, 1.5, size=(n, 18))
    state = _state(venv)
    c = _run(ctrl, venv, T, gains=g, state=state)
    # 130 distinct closed loops (whole action sequences: the first actions alone coincide wherever both motors sit at the PWM clip)
    uc = c['u'].cpu().numpy()
    assert len({uc[:, :, i].tobytes() for i in range(n)}) == n
    # every lane: the same envs as two batches of 65 (another stride, another block layout) ...
    for lo in (0, 65):
        part, vp = _setup(name, 65, states=ctrl._x0[lo:lo + 65])
        sp = _state(vp)
        d = _run(part, vp, T, gains=g[lo:lo + 65], state=sp)
        for k in c:
            assert torch.equal(c[k][..., lo:lo + 65], d[k]), (lo, k)
        assert torch.equal(state[:, lo:lo + 65], sp), lo
        part.close()
    # ... and the lanes at the block edges as single-env runs, through the shared-gain addressing
    for i in (0, 63, 64, 129):
        one, v1 = _setup(name, 1, states=ctrl._x0[i:i + 1])
        s1 = _state(v1)
        d = _run(one, v1, T, gains=g[i], state=s1)
        for k in c:
            assert torch.equal(c[k][..., i], d[k][..., 0]), (i, k)
        assert torch.equal(state[:, i], s1[:, 0]), i
        one.close()
    ctrl.close()


def test_chained_launches_carry_the_controller_state():
    name, n, T = 'quadrotor_3D_stab', 64, 40
    ctrl, venv = _setup(name, n)
    whole_state = _state(venv)
    whole = _run(ctrl, venv, T, state=whole_state)
    assert (whole['n_steps'] == T).all()
    null = _run(ctrl, venv, T, state=None)                       # NULL: starts from zeros
    for k in whole:
        assert torch.equal(whole[k], null[k]), k
    state = _state(venv)
    parts = []
    ctrl._restart()
    for _ in range(5):
        parts.append(_run(ctrl, venv, T // 5, state=state, restart=False))
    for k in ('x', 'u', 'reward', 'done', 'flags'):
        assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
    assert torch.equal(parts[-1]['final_obs'], whole['final_obs']) and torch.equal(state, whole_state)
    ctrl.close()


def test_stops_at_done_and_writes_nothing_after():
    name, n, T = 'quadrotor_2D_saturating', 65, 36
    fx = PC.fixture()
    ctrl, venv = _setup(name, n)
    state = _state(venv)
    o = _run(ctrl, venv, T, state=state, fill=float('nan'))
    ns = o['n_steps'].cpu().numpy()
    assert (ns == fx[f'{name}/u'].shape[0]).all() and (ns < T).all()                               # the reference leaves the bounds at step 14
    assert ((o['final_flags'] & 4) != 0).all()
    past = torch.arange(T, device=venv.device).view(T, 1) >= o['n_steps'].view(1, n)
    for k in ('x', 'u'):
        nan = torch.isnan(o[k])
        assert torch.equal(nan, past.view(T, 1, n).expand_as(nan)), k
    assert torch.equal(torch.isnan(o['reward']), past) and torch.equal(o['done'] == 255, past) and torch.equal(o['flags'] == 255, past)
    # the state written back is that of the last step taken: a launch of exactly n_steps steps leaves the same
    exact = _state(venv)
    _run(ctrl, venv, int(ns[0]), state=exact)
    assert torch.equal(state, exact)
    assert PC.rel(state[:, 0].cpu().numpy(), fx[f'{name}/state'][ns[0] - 1]) <= PC.bound()
    ctrl.close()


@pytest.mark.parametrize('name', ['quadrotor_2D_track', 'quadrotor_3D_track'])
def test_float32_closed_loop(name):
    """float32 kernel against the reference's float64 closed loop.  Over the recorded 250 steps the yardstick is meaningless: the float32
    MODEL on the CPU already drifts by model_deviation_f32 = O(0.1 .. 1) of the signal there (the loop amplifies rounding by ~15 % per
    step; pid_settings.json).  So the first 32 steps are bound, by 10 x the float32 model's deviation over the same 32 steps
    (model_deviation_f32_first_32_steps, measured by the generator)."""
    fx = PC.fixture()
    ctrl, venv = _setup(name, 64, dtype='float32')
    o = _run(ctrl, venv, 32)
    assert (o['n_steps'] == 32).all()
    x, u = o['x'].double().cpu().numpy(), o['u'].double().cpu().numpy()
    assert np.array_equal(u, np.repeat(u[..., :1], 64, axis=-1))
    dev = max(PC.rel(x[:, :, 0], fx[f'{name}/x'][:32]), PC.rel(u[:, :, 0], fx[f'{name}/u'][:32]))
    bound = 10.0 * PC.settings()['model_deviation_f32_first_32_steps'][name]
    print(f'{name} float32, first 32 steps: {dev:.3e} (bound {bound:.3e})')
    assert dev <= bound
    ctrl.close()


@pytest.mark.parametrize('task,rmse_max', [('quadrotor_2D_track', 0.2), ('quadrotor_3D_track', 0.4)])
def test_controller_surface(task, rmse_max):
    from safe_control_gym_amd.registration import make
    ctrl = make('pid', PC.env_func(task), num_envs=65)
    ctrl.reset()
    ctrl.learn()
    res = ctrl.run()
    assert set(res) == {'ep_returns', 'ep_lengths', 'constraint_violation', 'mse'}
    assert (res['ep_lengths'] == 250).all()
    rmse = np.sqrt(res['mse'])
    print(f'{task}: RMSE {rmse.max():.4f}')
    assert (rmse < rmse_max).all()
    ctrl.close()


@pytest.mark.parametrize('qt', [2, 3])
def test_disturbed_variant(qt):
    """The kernels' DIST variants: the tracking tasks with a white-noise dynamics disturbance (settings only, no recorded flight).  Every
    env draws its own noise; scg_step_sequence fed the rollout's actions reproduces it bit for bit, and the model on the kernel's own
    observations returns its actions within 1e-9."""
    from safe_control_gym_amd.registration import make
    fx = PC.fixture()
    name, base, n, T = f'quadrotor_{qt}D_track_disturbed', f'quadrotor_{qt}D_track', 65, 40
    c = PC.settings()['disturbed'][name]
    ctrl = make('pid', __import__('functools').partial(make, c['env'], **c['task']), num_envs=n)
    venv = ctrl._env()
    state = _state(venv)
    o = _run(ctrl, venv, T, state=state)
    assert (o['n_steps'] == T).all()
    x, u = o['x'].cpu().numpy(), o['u'].cpu().numpy()
    assert len({x[:, :, i].tobytes() for i in range(n)}) == n                                    # per-env noise
    ctrl._restart()
    seq = venv.step_sequence(o['u'].permute(0, 2, 1).contiguous(), terminal_obs=False)
    assert torch.equal(seq['obs'].permute(0, 2, 1)[:-1], o['x'][1:]) and torch.equal(seq['obs'][-1].t(), o['final_obs'])
    for k in ('reward', 'done', 'flags'):
        assert torch.equal(seq[k], o[k]), k
    worst = 0.0
    for i in (0, 63, 64):
        mu, ms = _replay_law(base, x[:, :, i], T, fx[f'{base}/gains'], PC.config(base))
        worst = max(worst, PC.rel(mu, u[:, :, i]), PC.rel(ms[-1], state[:, i].cpu().numpy()))
    print(f'{name}: the model on the kernel\'s observations {worst:.3e}')
    assert worst <= 1e-9
    ctrl.close()


@pytest.mark.parametrize('name', ['cartpole_stab', 'quadrotor_1D_stab'])
def test_unserved_systems_answer_invalid(name):
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd.registration import make
    from tests import ilqr_cases as IC
    a = IC.settings()['cases'][name]['algo']
    ctrl = make('lqr', IC.env_func(name), q_lqr=a['q_lqr'], r_lqr=a['r_lqr'], num_envs=1, dtype='float64')
    venv = ctrl._env()
    pid = PC.controller('quadrotor_2D_stab')
    # SCG_ERR_INVALID = -1 (include/scg_hip.h), with the entry point's own message
    with pytest.raises(L.ScgError, match=r'error -1: scg_rollout_pid serves Quadrotor 2D and 3D'):
        venv.rollout_pid(_gains(venv, pid.gains), pid.config_struct(), 4, pid_state=None, **_outputs(venv, 4))
    ctrl.close()
