"""LQR / iLQR on the GPU (csrc/scg_ilqr.hip, safe_control_gym_amd/lqr.py): the feedback rollout against scg_step_sequence, the backward
pass against the reference-generated fixture (tests/golden/make_ilqr.py) and the NumPy model (tests/ilqr_model.py), the controllers end
to end.  N = 67 envs unless stated (more than one wave, not a multiple of 64), T = 60."""
import numpy as np
import pytest

from tests import ilqr_cases as IC
from tests import ilqr_model as M

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
N, T = 67, 60


def _ctrl(name, algo='ilqr', **kw):
    from safe_control_gym_amd.registration import make
    c = IC.settings()['cases'][name]
    a = {k: v for k, v in c['algo'].items() if algo == 'ilqr' or k in ('q_lqr', 'r_lqr', 'discrete_dynamics')}
    return make(algo, IC.env_func(name), **dict(a, **kw))


def _x0(ctrl, n, spread, seed=0):
    base = np.atleast_2d(IC.fixture()[f'{ctrl.case_name}/lqr_x'][0])
    rng = np.random.default_rng(seed)
    return base + spread * rng.uniform(-1, 1, size=(n, base.shape[1]))


def _setup(name, dtype, spread=0.02, n=N):
    ctrl = _ctrl(name, 'lqr', num_envs=n, dtype=dtype)
    ctrl.case_name = name
    ctrl.init_states = _x0(ctrl, n, spread)
    venv = ctrl._env()
    return ctrl, venv


def _outputs(venv, nx, nu, fill=0.0):
    f = dict(dtype=venv.dtype, device=venv.device)
    n = venv.num_envs
    u8 = dict(dtype=torch.uint8, device=venv.device)
    return dict(x=torch.full((T, nx, n), fill, **f), u=torch.full((T, nu, n), fill, **f), final_obs=torch.full((nx, n), fill, **f),
                stats=torch.zeros(4, n, **f), n_steps=torch.zeros(n, dtype=torch.int32, device=venv.device), final_flags=torch.zeros(n, **u8),
                reward=torch.full((T, n), fill, **f), done=torch.full((T, n), 255, **u8), flags=torch.full((T, n), 255, **u8))


def _run(ctrl, venv, K, ff, per_env, fill=0.0):
    o = _outputs(venv, ctrl.spec.nx, ctrl.spec.nu, fill)
    ctrl._restart()
    venv.rollout_feedback(K, ff, T, per_env=per_env, **o)
    return o


def _replay(ctrl, venv, u):
    ctrl._restart()
    return venv.step_sequence(torch.nan_to_num(u).permute(0, 2, 1).contiguous(), terminal_obs=False)


@pytest.mark.parametrize('name,dtype', [('cartpole_stab', 'float64'), ('cartpole_stab', 'float32'), ('quadrotor_2D_stab', 'float64'),
                                        ('quadrotor_2D_stab', 'float32'), ('cartpole_track', 'float64')])
def test_rollout_equals_step_sequence_fed_its_actions(name, dtype):
    # (scg_step_sequence needs num_envs x obs_dim x sizeof(T) to be a multiple of 16: 67 float32 rows of 6 are not, 70 are — still more
    #  than one wave and no multiple of 64)
    N = 70 if (name, dtype) == ('quadrotor_2D_stab', 'float32') else 67
    ctrl, venv = _setup(name, dtype, n=N)
    nx, nu = ctrl.spec.nx, ctrl.spec.nu
    K0, ff0 = ctrl._as_schedule(*ctrl.lqr_schedule())
    Ts = K0.shape[0]
    scale = 1.0 + 0.1 * torch.linspace(-1, 1, N, dtype=venv.dtype, device=venv.device)
    K = (K0.unsqueeze(-1) * scale).contiguous()                   # per-env gains that differ from env to env
    ff = ff0.unsqueeze(-1).expand(Ts, nu, N).contiguous()
    o = _run(ctrl, venv, K, ff, True)
    n = o['n_steps'].cpu().numpy()
    assert (n >= 1).all() and (n == T).sum() > N // 2
    seq = _replay(ctrl, venv, o['u'])
    # every env, every step it took: rows t < n_steps[i] (an env that stopped early is compared up to its last step)
    ns = o['n_steps'].long()
    took = torch.arange(T, device=venv.device).view(T, 1) < ns.view(1, N)                      # [T, N]
    obs = seq['obs'].permute(0, 2, 1)                             # [T, nx, N]: obs[t] is the observation after step t
    nxt = took[1:].view(T - 1, 1, N).expand(T - 1, nx, N)
    assert torch.equal(obs[:-1][nxt], o['x'][1:][nxt])
    assert torch.equal(obs.gather(0, (ns - 1).view(1, 1, N).expand(1, nx, N))[0], o['final_obs'])
    for k in ('reward', 'done', 'flags'):
        assert torch.equal(seq[k][took], o[k][took]), k
    full = took.view(T, 1, N).expand(T, nu, N)
    # u = K x + ff recomputed in float64
    s = torch.arange(T, device=venv.device).clamp(max=Ts - 1)
    Kd, fd, xd = K[s].double(), ff[s].double(), o['x'].double()
    ref = torch.einsum('tjkn,tkn->tjn', Kd, xd) + fd
    mag = torch.einsum('tjkn,tkn->tjn', Kd.abs(), xd.abs()) + fd.abs()
    # float64: 1e-12 of the terms' magnitude.  float32: nx products and nx additions, each rounded once (contracted or not): the
    # classical dot-product bound (nx + 1) u sum|terms| with u = 2^-24, + one u for the final sum
    rel = 1e-12 if dtype == 'float64' else (nx + 2) * 2.0 ** -24
    err = ((o['u'].double() - ref).abs() / mag)[full].max().item()
    print(f'{name} {dtype}: max |u - (K x + ff)| / sum|terms| = {err:.3e} (bound {rel:.3e})')
    assert err <= rel
    # shared schedule == the same schedule per env, bit for bit
    a = _run(ctrl, venv, K0, ff0, False)
    b = _run(ctrl, venv, K0.unsqueeze(-1).expand(Ts, nu, nx, N).contiguous(), ff, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ctrl.close()


def test_rollout_stops_at_done_and_writes_nothing_after():
    ctrl, venv = _setup('cartpole_stab', 'float64', spread=0.0)
    ctrl.init_states[:, 2] = 0.3                                  # tilted pole
    ctrl.set_initial_states(ctrl.init_states)
    nx, nu = 4, 1
    K0, ff0 = ctrl._as_schedule(*ctrl.lqr_schedule())
    on = torch.as_tensor((np.arange(N) % 2).astype(np.float64), device=venv.device)          # odd envs: LQR; even envs: zero gains
    K = (K0.unsqueeze(-1) * on).contiguous()
    ff = (ff0.unsqueeze(-1) * on).contiguous()
    o = _run(ctrl, venv, K, ff, True, fill=float('nan'))
    n = o['n_steps'].cpu().numpy()
    assert (n[1::2] == T).all() and (n[0::2] < T).all() and (n[0::2] >= 1).all()         # ragged
    t = torch.arange(T, device=venv.device).view(T, 1)
    past = t >= o['n_steps'].view(1, N)
    for k in ('x', 'u'):
        nan = torch.isnan(o[k])
        assert torch.equal(nan, past.view(T, 1, N).expand_as(nan)), k
    assert torch.equal(torch.isnan(o['reward']), past) and torch.equal(o['done'] == 255, past) and torch.equal(o['flags'] == 255, past)
    seq = _replay(ctrl, venv, o['u'])
    last = (o['n_steps'].long() - 1).view(1, N)
    assert torch.equal(seq['obs'].permute(0, 2, 1).gather(0, last.view(1, 1, N).expand(1, nx, N))[0], o['final_obs'])
    assert torch.equal(seq['flags'].gather(0, last)[0], o['final_flags'])
    oob = ((o['final_flags'] & 4) != 0).cpu().numpy()
    assert oob[0::2].all() and not oob[1::2].any()
    stats = o['stats'].cpu().numpy()
    np.testing.assert_array_equal(stats[1], n)
    ctrl.close()


@pytest.mark.parametrize('name', list(IC.settings()['cases']))
def test_lqr_closed_loop_equals_the_references(name):
    fx = IC.fixture()
    ctrl = _ctrl(name, 'lqr', num_envs=1, dtype='float64')
    res = ctrl.run()
    xs, us = fx[f'{name}/lqr_x'], fx[f'{name}/lqr_u']
    n = us.shape[0]
    assert int(res['ep_lengths'][0]) == n
    x = ctrl.results_dict['obs'][:n, :, 0].cpu().numpy()
    final = ctrl.results_dict['final_obs'][:, 0].cpu().numpy()
    err = max(np.abs(x - xs[:n]).max(), np.abs(final - xs[n]).max())
    print(f'{name}: max |x - x_ref| = {err:.3e}')
    np.testing.assert_allclose(x, xs[:n], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(final, xs[n], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ctrl.results_dict['action'][:n, :, 0].cpu().numpy(), us.reshape(n, -1), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res['ep_returns'][0], float(fx[f'{name}/lqr_return']), rtol=1e-9)
    ctrl.close()


def _backward_inputs(ctrl, venv, stacks, lambs, sentinel=7.0):
    """Device tensors of per-env stacks [(x [n + 1, nx], u [n, nu])]."""
    nx, nu, n_env = ctrl.spec.nx, ctrl.spec.nu, len(stacks)
    x, u = np.zeros((T + 1, nx, n_env)), np.zeros((T, nu, n_env))
    ns = np.zeros(n_env, dtype=np.int32)
    for i, (xs, us) in enumerate(stacks):
        n = us.shape[0]
        x[:n + 1, :, i], u[:n, :, i], ns[i] = xs[:n + 1], us, n
    f = dict(dtype=venv.dtype, device=venv.device)
    return dict(x=torch.as_tensor(x, **f), u=torch.as_tensor(u, **f), n_steps=torch.as_tensor(ns, device=venv.device),
                lamb=torch.as_tensor(np.asarray(lambs, dtype=np.float64), **f), mask=None,
                gains=torch.full((T, nu, nx, n_env), sentinel, **f), ff=torch.full((T, nu, n_env), sentinel, **f),
                unstable=torch.zeros(n_env, dtype=torch.uint8, device=venv.device))


def _model(ctrl, name, xs, us, lamb, R=None, sentinel=7.0):
    n = us.shape[0]
    K, ff = np.full((T, ctrl.spec.nu, ctrl.spec.nx), sentinel), np.full((T, ctrl.spec.nu), sentinel)
    with np.errstate(all='ignore'):
        bad = M.backward(ctrl.model.f, xs, us, n, lamb, IC.fixture()[f'{name}/x_goal'], ctrl.spec.TASK == 'traj_tracking', ctrl.Q,
                         ctrl.R if R is None else R, ctrl.model.U_EQ, ctrl.model.dt, K, ff)
    return K, ff, bad


@pytest.mark.parametrize('name', IC.ilqr_cases())
def test_backward_pass_equals_the_references(name):
    ctrl = _ctrl(name, num_envs=N, dtype='float64')
    venv = ctrl._env()
    its = [it for it in IC.iterations(name) if 'K' in it]
    stacks, lambs, expect = [], [], []
    for i in range(N):
        it = its[i % len(its)]
        n = it['u'].shape[0]
        if i % 3 == 2:                                            # a truncated stack with another lambda: the model is the yardstick
            m = max(2, n - 7 * (1 + i % 5))
            xs, us, lamb = it['x'][:m + 1], it['u'][:m], 1.0 + i
            expect.append(_model(ctrl, name, xs, us, lamb)[:2])
        else:                                                     # a recorded iteration: the reference is the yardstick
            xs, us, lamb = it['x'], it['u'], float(it['lamb'])
            Kr, fr = np.full((T, ctrl.spec.nu, ctrl.spec.nx), 7.0), np.full((T, ctrl.spec.nu), 7.0)
            Kr[:n], fr[:n] = it['K'][:n], it['ff'][:n]
            expect.append((Kr, fr))
        stacks.append((xs, us)); lambs.append(lamb)
    bad_env = 5
    xs_bad = stacks[bad_env][0].copy(); xs_bad[5, :] = np.inf
    stacks[bad_env] = (xs_bad, stacks[bad_env][1])
    Kb, fb, was_bad = _model(ctrl, name, xs_bad, stacks[bad_env][1], lambs[bad_env])
    assert was_bad and (Kb[5] == 7.0).all()
    expect[bad_env] = (Kb, fb)
    d = _backward_inputs(ctrl, venv, stacks, lambs)
    venv.ilqr_backward(ctrl.model_struct(), T, **d)
    K, ff = d['gains'].permute(3, 0, 1, 2).cpu().numpy(), d['ff'].permute(2, 0, 1).cpu().numpy()
    unstable = d['unstable'].cpu().numpy()
    assert unstable[bad_env] == 1 and unstable.sum() == 1
    assert (K[bad_env, 5] == 7.0).all() and (ff[bad_env, 5] == 7.0).all()
    bound, worst = IC.bound(name), 0.0
    for i in range(N):
        Ke, fe = expect[i]
        ok = np.isfinite(Ke)
        assert np.array_equal(np.isfinite(K[i]), ok)
        worst = max(worst, np.abs(K[i][ok] - Ke[ok]).max() / np.abs(Ke[ok]).max(), np.abs(ff[i] - fe)[np.isfinite(fe)].max() / np.abs(fe[np.isfinite(fe)]).max())
    print(f'{name}: max relative deviation of K / ff = {worst:.3e} (bound {bound:.3e})')
    assert worst <= bound
    ctrl.close()


@pytest.mark.parametrize('name,r,lamb', IC.CLIP_CASES)
def test_backward_pass_clips_negative_eigenvalues(name, r, lamb):
    """R negative enough that H = R + Bd' Sm Bd has a negative eigenvalue at most steps (asserted on H, through the model's trace): one
    input (scalar clip) and two inputs (both forms of the closed-form eigenvector)."""
    ctrl = _ctrl(name, num_envs=N, dtype='float64')
    venv = ctrl._env()
    it = IC.iterations(name)[0]
    n = IC.CLIP_STEPS
    it = dict(it, x=it['x'][:n + 1], u=it['u'][:n])
    R = np.diag(r)
    lambs = [lamb * (0.9 + 0.003 * i) for i in range(N)]           # (a larger lambda keeps Sm positive: no eigenvalue left to clip)
    d = _backward_inputs(ctrl, venv, [(it['x'], it['u'])] * N, lambs)
    ms = ctrl.model_struct()
    for j, v in enumerate(r):
        ms.r[j] = v
    venv.ilqr_backward(ms, T, **d)
    K, ff = d['gains'].permute(3, 0, 1, 2).cpu().numpy(), d['ff'].permute(2, 0, 1).cpu().numpy()
    worst = 0.0
    for i in (0, 1, 33, 64, 66):
        tr = []
        Ke, fe = np.full((T, ctrl.spec.nu, ctrl.spec.nx), 7.0), np.full((T, ctrl.spec.nu), 7.0)
        assert not M.backward(ctrl.model.f, it['x'], it['u'], n, lambs[i], IC.fixture()[f'{name}/x_goal'], False, ctrl.Q, R, ctrl.model.U_EQ,
                              ctrl.model.dt, Ke, fe, trace=tr)
        assert sum(t < 0 for t in tr) >= n // 2
        worst = max(worst, np.abs(K[i] - Ke).max() / np.abs(Ke).max(), np.abs(ff[i] - fe).max() / np.abs(fe).max())
    print(f'{name} R = diag{tuple(r)}: max relative deviation from the model = {worst:.3e}')
    assert worst <= 1e-9                      # same equations in float64 on both sides: operation order and FMA contraction only
    assert d['unstable'].sum().item() == 0
    ctrl.close()


@pytest.mark.parametrize('name', ['cartpole_stab', 'quadrotor_2D_stab'])
def test_float32_backward_pass_against_the_float64_kernel(name):
    """The float32 kernel (central-difference step 1e-3) against the float64 kernel (1e-6) on the same stacks.  Bound: 10 x the deviation
    of the float32 MODEL from the reference, measured on the CPU by the generator and recorded in ilqr_settings.json (IC.bound_f32)."""
    its = [it for it in IC.iterations(name) if 'K' in it]
    stacks = [(its[i % len(its)]['x'], its[i % len(its)]['u']) for i in range(N)]
    stacks = [(x[:u.shape[0] - 5 * (i % 4) + 1], u[:u.shape[0] - 5 * (i % 4)]) for i, (x, u) in enumerate(stacks)]       # ragged n_steps
    lambs = [1.0 + (i % 7) for i in range(N)]
    res = {}
    for dtype in ('float64', 'float32'):
        ctrl = _ctrl(name, num_envs=N, dtype=dtype)
        venv = ctrl._env()
        d = _backward_inputs(ctrl, venv, stacks, lambs)
        venv.ilqr_backward(ctrl.model_struct(), T, **d)
        assert d['unstable'].sum().item() == 0
        res[dtype] = (d['gains'].double().cpu().numpy(), d['ff'].double().cpu().numpy())
        ctrl.close()
    (K64, f64), (K32, f32) = res['float64'], res['float32']
    worst = 0.0
    for i in range(N):
        worst = max(worst, np.abs(K32[..., i] - K64[..., i]).max() / np.abs(K64[..., i][K64[..., i] != 7.0]).max(),
                    np.abs(f32[..., i] - f64[..., i]).max() / np.abs(f64[..., i][f64[..., i] != 7.0]).max())
    print(f'{name}: float32 against float64 backward pass, max relative deviation {worst:.3e} (bound {IC.bound_f32(name):.3e})')
    assert worst <= IC.bound_f32(name)


@pytest.mark.parametrize('name', IC.ilqr_cases())
def test_ilqr_learn_takes_the_references_branches(name):
    fx = IC.fixture()
    ctrl = _ctrl(name, num_envs=1, dtype='float64')
    ctrl.learn()
    its = IC.iterations(name)
    got = []
    for j, h in enumerate(ctrl.history):
        got.append('init' if j == 0 and bool(h['accept'][0]) else 'oob' if j == 0 else 'reject' if bool(h['reject'][0]) else
                   'converged' if bool(h['converged'][0]) else 'accept')
    costs = [float(h['cost'][0]) for h in ctrl.history]
    print(name, got, costs)
    assert got == [it['branch'] for it in its]
    bound = IC.bound(name)
    for c, it in zip(costs, its):
        assert abs(c - float(it['cost'])) <= bound * abs(float(it['cost'])), (c, float(it['cost']))
    Kb, fb = fx[f'{name}/best_K'], fx[f'{name}/best_ff']
    n = Kb.shape[0]
    dK = np.abs(ctrl.gains_fb_best[:n] - Kb).max() / np.abs(Kb).max()
    df = np.abs(ctrl.input_ff_best.T[:n] - fb).max() / np.abs(fb).max()
    print(f'{name}: best schedule deviation K {dK:.3e} ff {df:.3e} (bound {bound:.3e})')
    assert max(dK, df) <= bound
    assert int(ctrl.best_iteration) == int(fx[f'{name}/best_iteration'])
    ctrl.close()


def test_batch_envs_are_independent():
    name, n, distinct = 'quadrotor_2D_stab', 256, 64
    rng = np.random.default_rng(3)
    base = IC.fixture()[f'{name}/lqr_x'][0]
    states = base + rng.uniform(-1, 1, size=(distinct, 6)) * np.array([0.3, 0.1, 0.2, 0.1, 0.0, 0.1])
    states[:, 4] = np.linspace(-1.5, 1.5, distinct)             # pitch: from level through the reject region to starts LQR loses
    states[0] = base
    x0 = np.tile(states, (n // distinct, 1))
    ctrl = _ctrl(name, num_envs=n, dtype='float64', init_states=x0)
    ctrl.learn()
    K, best = ctrl.gains_fb_best, ctrl.best_cost
    rejected = torch.stack([h['reject'] for h in ctrl.history]).any(0).cpu().numpy()
    lost = ctrl.initial_policy_unstable
    print(f'rejecting envs {int(rejected.sum())}, out of bounds at iteration 0: {int(lost.sum())}')
    assert rejected.any() and lost.any() and not lost.all()
    for c in range(1, n // distinct):                           # copies of one state agree bit for bit
        assert np.array_equal(K[:distinct], K[c * distinct:(c + 1) * distinct]) and np.array_equal(best[:distinct], best[c * distinct:(c + 1) * distinct])
    cost0 = ctrl.history[0]['cost'].cpu().numpy()
    assert (best[~lost] <= cost0[~lost]).all()
    picks = sorted({0, int(np.flatnonzero(rejected)[0]) % distinct, int(np.flatnonzero(lost)[0]) % distinct, 9, 21, 37, 50, 63})
    for i in picks:
        one = _ctrl(name, num_envs=1, dtype='float64', init_states=states[i:i + 1])
        one.learn()
        assert np.array_equal(one.gains_fb_best, K[i]) and np.array_equal(one.input_ff_best, ctrl.input_ff_best[i]), i
        assert one.best_cost == best[i] and int(one.best_iteration) == int(ctrl.best_iteration[i])
        one.close()
    ctrl.close()


def test_refusals():
    with pytest.raises(NotImplementedError, match='Quadrotor 3D'):
        _ctrl('quadrotor_3D_stab', 'ilqr')
    from safe_control_gym_amd.registration import make
    with pytest.raises(ValueError, match='normalized_rl_action_space'):
        make('ilqr', IC.env_func('cartpole_stab', normalized_rl_action_space=True))
    # the library itself refuses the backward pass on Quadrotor 3D
    ctrl = _ctrl('quadrotor_3D_stab', 'lqr', num_envs=1, dtype='float64')
    venv = ctrl._env()
    from safe_control_gym_amd import _ilqr
    from safe_control_gym_amd import _lib as L
    f = dict(dtype=torch.float64, device=venv.device)
    with pytest.raises(L.ScgError):
        venv.ilqr_backward(_ilqr.IlqrModel(dt=0.1, eps=1e-6), T, torch.zeros(T + 1, 12, 1, **f), torch.zeros(T, 4, 1, **f),
                           torch.ones(1, dtype=torch.int32, device=venv.device), torch.ones(1, **f), None, torch.zeros(T, 4, 12, 1, **f),
                           torch.zeros(T, 4, 1, **f), torch.zeros(1, dtype=torch.uint8, device=venv.device))
    ctrl.close()
