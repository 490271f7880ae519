"""The fused SAC / DDPG actor rollout at hidden width 256 (csrc/scg_actor_rollout_wide.h, scg_mlp_rows.h, scg_cbf_wide.hip) on the
device: the head against the agent's own actor in float64, the env step against scg_step_sequence bit for bit, the two launch
geometries, chaining, the packed actor vector of a non-fused agent, the controllers' `wide_actor` key, the CBF filter behind the actor,
and the refusals.  Helpers and bounds are those of tests/test_gpu_rollout_actor.py and tests/test_gpu_offpolicy_collector.py.

Shapes: K = 40 control steps, episodes of 25; N = 67 envs (G = 1: three workgroups, the last with 3 envs; G = 8: one workgroup with two
full tiles, a ragged one and five empty ones) and N = 291 (G = 8: a full workgroup and a ragged second).  The agents are the ordinary
non-fused 256-wide ones (the learner libraries do not serve the width), head weights x 6.

Head tolerance: Bounds.bound with TAU = 1e-5, unchanged.  A float32 PyTorch forward pass at H = 256 stays at 0.04 of TAU S (relu / tanh /
leaky_relu, obs dims 4 / 12 / 24, both trunks), so the bound has room for the kernel's order of summation: 128 sequential MFMA steps per
output row of layer 2, a 16-term fmaf chain per lane half and wave in layer 3, then 1 + 7 additions."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import actor_rollout_wide_cases as arw
from tests import test_gpu_rollout_actor as tra
from tests.test_gpu_rollout_actor import _assert_bits, _bufs, _check_canaries, _controller, _env, _n, _rollout

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, N2, K = 67, 291, 40
FLAG_VIOLATION = 2
CASE_IDS = ['-'.join(str(v) for v in c) for c in arw.CASES]


def _new_agent(kind, obs_dim, nu, act, lo, hi, seed):
    from safe_control_gym_amd import ddpg
    from safe_control_gym_amd.sac import SACAgent, SACConfig
    torch.manual_seed(seed)
    if kind == 'sac':
        ag = SACAgent(obs_dim, nu, torch.tensor(lo, device=DEV), torch.tensor(hi, device=DEV), SACConfig(hidden_dim=arw.HIDDEN, activation=act), DEV)
        head = ag.ac.actor.mu_layer
    else:
        ag = ddpg.DDPGAgent(obs_dim, nu, lo, hi, ddpg.DDPGConfig(hidden_dim=arw.HIDDEN, activation=act), DEV)
        head = ag.ac.actor.net.fcs[-1]
    assert not ag.use_fused and ag._flat is None          # the ordinary agent at this width: PyTorch modules, no flat vector
    with torch.no_grad():               # pre-squash values of order one: both tails of tanh are visited
        head.weight.mul_(6.0)
    return ag


_agents = {}


def _agent(kind, obs_dim, nu, act, bound_set=0):
    """(agent, Bounds) with the agent's bounds = the first nu columns of BOUND_SETS[bound_set]; one per shape."""
    key = (kind, obs_dim, nu, act, bound_set)
    if key not in _agents:
        oc = tra._oc()
        B = oc.Bounds(oc.BOUND_SETS[bound_set], nu)
        _agents[key] = (_new_agent(kind, obs_dim, nu, act, B.lo.astype(np.float32), B.hi.astype(np.float32), 41 + obs_dim + 31 * nu), B)
    return _agents[key]


_reference = {}


def _case(case, n=None, bound_set=0):
    """The K-step rollout of a case, computed once and shared (left unchanged): (outputs, final ep_stats, agent, Bounds)."""
    n = _n(case) if n is None else n
    key = (case, n, bound_set)
    if key not in _reference:
        task, kind, hidden, act = case
        env = _env(task, (hidden, act, kind), n)
        assert env.actor_kind == kind and env.policy_shape == (arw.HIDDEN, act, kind) and env.spec.max_episode_steps == arw.EPISODE_STEPS
        ag, B = _agent(kind, env.spec.obs_dim, env.spec.nu, act, bound_set)
        o = _rollout(env, ag.actor_struct(), K)
        _reference[key] = (o, env.ep_stats.clone(), ag, B)
        env.close()
    return _reference[key]


# ------------------------------------------------------------------------------------------------------------ 1. the head
@pytest.mark.parametrize('case', arw.CASES, ids=CASE_IDS)
@pytest.mark.parametrize('bound_set', [0, 1])
def test_head_matches_the_agents_actor_in_float64(case, bound_set):
    oc = tra._oc()
    o, _, ag, B = _case(case, bound_set=bound_set)
    kind, nu = case[1], B.lo.size
    x = o['obs'][:K].reshape(-1, o['obs'].shape[-1])
    assert bool(torch.isfinite(x).all())
    u, S = oc.sac_ref(ag, x)[:2] if kind == 'sac' else oc.ddpg_ref(ag, x)
    want, bound = B.squash(u), B.bound(u, S)
    got = o['act'].reshape(-1, nu)
    assert bool(torch.isfinite(got).all())
    for j in B.degenerate:
        assert bool((got[:, j] == float(np.float32(B.lo[j]))).all()), f'degenerate column {j} is not low'
    ratio = float(((got.double() - want).abs() / bound).max())
    span = float((u.max() - u.min()))
    print(f'[ratio] rollout_actor wide head {CASE_IDS[arw.CASES.index(case)]} bounds {bound_set}: worst error/bound {ratio:.4f} '
          f'(pre-squash span {span:.2f})')
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------ 2. the env step
@pytest.mark.parametrize('case', arw.CASES, ids=CASE_IDS)
def test_env_step_is_untouched(case):
    task, kind, hidden, act = case
    o, ep_final, ag, B = _case(case)
    _check_canaries(o)
    env2 = _env(task, (hidden, act, kind), _n(case))
    q = env2.step_sequence(o['act'].contiguous(), terminal_obs=True)
    torch.cuda.synchronize()
    _assert_bits(q['obs'], o['obs'][1:], 'obs')
    _assert_bits(q['reward'], o['rew'], 'reward')
    assert torch.equal(q['done'].cpu(), o['done'].cpu()) and torch.equal(q['flags'].cpu(), o['flags'].cpu())
    done = o['done'].cpu().bool()
    assert bool(done.any(0).all()), 'every env finishes an episode inside the launch'
    _assert_bits(q['terminal_obs'][done], o['term'][done], 'terminal_obs')
    _assert_bits(env2.ep_stats, ep_final, 'ep_stats')
    assert torch.equal(o['acc'][:, 0].cpu(), done.sum(0).float())
    env2.close()


# ------------------------------------------------------------------------------------------------------------ 3. geometry
@pytest.mark.parametrize('n', [N, N2])
@pytest.mark.parametrize('case', arw.CASES[:3], ids=CASE_IDS[:3])
def test_results_do_not_depend_on_the_launch_geometry(case, n, monkeypatch):
    task, kind, hidden, act = case
    outs = []
    for tiles in ('1', '8'):
        monkeypatch.setenv('SCG_ROLLOUT_WIDE_TILES', tiles)
        env = _env(task, (hidden, act, kind), n)
        ag, _ = _agent(kind, env.spec.obs_dim, env.spec.nu, act)
        o = _rollout(env, ag.actor_struct(), K)
        o['ep'] = env.ep_stats.clone()
        _check_canaries(o)
        outs.append(o)
        env.close()
    assert bool(outs[0]['done'].bool().any(0).all())
    for key in ('obs', 'act', 'rew', 'done', 'flags', 'acc', 'ep'):
        _assert_bits(outs[0][key], outs[1][key], key)
    done = outs[0]['done'].bool()
    _assert_bits(outs[0]['term'][done], outs[1]['term'][done], 'terminal_obs')


# ------------------------------------------------------------------------------------------------------------ 4. chaining
@pytest.mark.parametrize('case', [arw.CASES[0], arw.CASES[3]], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_chained_launches_equal_one(case):
    """17 + 23 steps against one 40-step launch, bit for bit; then max_episodes = 1.
    The tasks are those of the narrow kernel's chaining test, CartPole and Quadrotor 2D tracking: there the row a launch starts on
    (state_vector() of the stored state) is the row EnvOps::step returned.  On Quadrotor 3D it is not (the Euler angles
    differ by one ulp, in scg_env_core.h, for the narrow kernels alike), so chained launches are not bit-equal to one there."""
    task, kind, hidden, act = case
    o, ep_final, ag, _ = _case(case)
    env = _env(task, (hidden, act, kind))
    c = _bufs(env, K)
    _rollout(env, ag.actor_struct(), 17, c, 0)
    _rollout(env, ag.actor_struct(), 23, c, 17)
    for key in ('obs', 'act', 'rew', 'done', 'flags', 'acc'):
        _assert_bits(c[key], o[key], key)
    _assert_bits(env.ep_stats, ep_final, 'ep_stats')
    env.close()
    # max_episodes = 1: the accumulator stops after an env's first episode while the env goes on stepping
    env = _env(task, (hidden, act, kind))
    m = _rollout(env, ag.actor_struct(), K, max_episodes=1)
    for key in ('obs', 'act', 'rew', 'done', 'flags'):
        _assert_bits(m[key], o[key], key)
    done = o['done'].cpu().bool()
    assert bool((done.sum(0) >= 1).all()) and bool((o['acc'][:, 0] >= 1).all())
    first = ((done.float().cumsum(0) - done.float()) < 1)                     # steps of each env's first episode
    assert torch.equal(m['acc'][:, 0].cpu(), torch.ones(N))
    assert torch.equal(m['acc'][:, 2].cpu(), first.sum(0).float())
    viol = ((o['flags'].cpu() & FLAG_VIOLATION) != 0)
    assert torch.equal(m['acc'][:, 3].cpu(), (viol & first).sum(0).float())
    env.close()


# ------------------------------------------------------------------------------------------------------------ 5. the packed vector
@pytest.mark.parametrize('case', [arw.CASES[0], arw.CASES[2]], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_the_packed_vector_follows_the_weights(case):
    task, kind, hidden, act = case
    oc = tra._oc()
    env = _env(task, (hidden, act, kind))
    obs_dim, nu = env.spec.obs_dim, env.spec.nu
    B = oc.Bounds(oc.BOUND_SETS[0], nu)
    lo, hi = B.lo.astype(np.float32), B.hi.astype(np.float32)
    ag = _new_agent(kind, obs_dim, nu, act, lo, hi, 5)
    s0 = ag.actor_struct()
    before = _rollout(env, s0, K)
    env.close()
    # one optimiser step of the eager agent's actor, in place
    x = torch.randn(64, obs_dim, device=DEV)
    ag.actor_opt.zero_grad(set_to_none=False)
    a = ag.ac.actor(x, True, False)[0] if kind == 'sac' else ag.ac.actor(x)
    a.pow(2).sum().backward()
    ag.actor_opt.step()
    env = _env(task, (hidden, act, kind))
    s1 = ag.actor_struct()
    assert s1.d_params == s0.d_params, 'the packed vector moved'
    after = _rollout(env, s1, K)
    env.close()
    assert not torch.equal(after['act'], before['act']), 'the optimiser step changed nothing'
    fresh = _new_agent(kind, obs_dim, nu, act, lo, hi, 6)
    fresh.ac.load_state_dict(ag.ac.state_dict())
    env = _env(task, (hidden, act, kind))
    want = _rollout(env, fresh.actor_struct(), K)
    env.close()
    for key in ('obs', 'act', 'rew', 'done', 'flags', 'acc'):
        _assert_bits(after[key], want[key], key)


# ------------------------------------------------------------------------------------------------------------ 6. controllers
WIDE = dict(fused_rollout=True, wide_actor=True)


@pytest.mark.parametrize('cc', arw.CONTROLLER_CASES, ids=[c[0] for c in arw.CONTROLLER_CASES])
def test_controller_run_is_one_launch_and_agrees_with_the_eager_loop(cc, tmp_path):
    from safe_control_gym_amd.vec_env import HipVecEnv
    cid, task, hidden, act = cc
    n = 64
    fused = _controller(cid, task, hidden, act, tmp_path, **WIDE)
    assert fused.impl._fused_rollout and fused.env.actor_kind == cid and not fused.agent.use_fused
    res = fused.run(n_episodes=n)
    assert fused._run_env.actor_kind == cid and hasattr(fused._run_env, '_eval_fused') and getattr(fused._run_env, '_eval_cache', None) is None
    # an explicit rollout_actor call on an identically seeded env
    env_id, cfg = arw.task_config(task)
    env = HipVecEnv(env_id, n, seed=fused.seed * 111, return_numpy=False, policy=(hidden, act, cid), **cfg)
    env.reset_tensors()
    o = _rollout(env, fused.agent.actor_struct(), env.spec.max_episode_steps, max_episodes=1)
    for key, col in (('ep_returns', 1), ('ep_lengths', 2), ('constraint_violation', 3), ('mse', 4)):
        assert np.array_equal(res[key], o['acc'][:, col].double().cpu().numpy()), key
    env.close()
    # the same controller without the keys: the eager loop (see tests/test_gpu_rollout_actor.py on the episode indices)
    eager = _controller(cid, task, hidden, act, tmp_path)
    assert not eager.impl._fused_rollout and eager.env.policy_shape is None
    ref = eager.run(n_episodes=n)
    ev = HipVecEnv(env_id, n, seed=fused.seed * 111, return_numpy=False, policy=(hidden, act, cid), **cfg)
    ev.reset_tensors()
    res2 = fused.run(env=ev)
    assert hasattr(ev, '_eval_fused')
    ev.close()
    assert np.array_equal(ref['ep_lengths'], res2['ep_lengths'])
    e, f = float(ref['ep_returns'].mean()), float(res2['ep_returns'].mean())
    print(f'[eval] {cid} 256: eager mean return {e:.6f}, fused {f:.6f}, |diff| {abs(e - f):.3g}')
    assert abs(e - f) <= 1e-3 * max(1.0, abs(e))
    fused.close()
    eager.close()


def test_wide_actor_changes_nothing_at_narrow_widths(tmp_path):
    cid, task, hidden, act = tra.arc.CONTROLLER_CASES[0]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        a = _controller(cid, task, hidden, act, tmp_path, **WIDE)
        b = _controller(cid, task, hidden, act, tmp_path, fused_rollout=True)
    assert a.impl._fused_rollout and a.agent.use_fused and a.env.policy_shape == b.env.policy_shape == (hidden, act, cid)
    ra, rb = a.run(n_episodes=16), b.run(n_episodes=16)
    for key in ('ep_returns', 'ep_lengths', 'constraint_violation', 'mse'):
        assert np.array_equal(ra[key], rb[key]), key
    a.close()
    b.close()


def test_wide_actor_alone_raises(tmp_path):
    cid, task, hidden, act = arw.CONTROLLER_CASES[0]
    with pytest.raises(ValueError, match='wide_actor'):
        _controller(cid, task, hidden, act, tmp_path, wide_actor=True)


def test_a_running_normaliser_warns_and_keeps_the_eager_numbers(tmp_path):
    cid, task, hidden, act = arw.CONTROLLER_CASES[0]
    with pytest.warns(UserWarning, match='fused_rollout=True is not served'):
        a = _controller(cid, task, hidden, act, tmp_path, norm_obs=True, **WIDE)
    assert not a.impl._fused_rollout and a.env.policy_shape is None
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        b = _controller(cid, task, hidden, act, tmp_path, norm_obs=True)
    ra, rb = a.run(n_episodes=16), b.run(n_episodes=16)
    for key in ('ep_returns', 'ep_lengths', 'constraint_violation', 'mse'):
        assert np.array_equal(ra[key], rb[key]), key
    a.close()
    b.close()


def test_learn_evaluates_through_the_fused_rollout(tmp_path):
    cid, task, hidden, act = arw.CONTROLLER_CASES[0]
    ctrl = _controller(cid, task, hidden, act, tmp_path, max_env_steps=400, warm_up_steps=100, train_interval=50,
                       train_batch_size=32, max_buffer_size=10000, eval_interval=200, eval_batch_size=8, rollout_batch_size=4, **WIDE)
    evals = []
    step = ctrl.train_step

    def recording_step():
        r = step()
        evals.append(r)
        return r
    ctrl.train_step = recording_step
    ctrl.learn()
    got = [r['eval'] for r in evals if 'eval' in r]
    assert got and all(g['ep_returns'].shape == (8,) and np.isfinite(g['ep_returns']).all() for g in got)
    assert any(r.get('updates') for r in evals), 'no gradient step ran (the packed vector must follow them)'
    assert hasattr(ctrl._run_env, '_eval_fused') and ctrl._run_env.actor_kind == cid and ctrl._run_env.policy_shape[0] == arw.HIDDEN
    ctrl.close()


# ------------------------------------------------------------------------------------------------------------ 7. CBF
@pytest.mark.parametrize('normalized', [False, True], ids=['physical', 'normalized'])
@pytest.mark.parametrize('cc', arw.CBF_CASES, ids=[c[0] for c in arw.CBF_CASES])
def test_cbf_rows_equal_certify_and_the_env_step_is_untouched(cc, normalized):
    kind, hidden, act = cc
    env = tra._cbf_env(kind, hidden, act, normalized)
    sf = tra._cbf_filter().attach(env)
    ag = tra._space_agent(kind, env, hidden, act)
    assert not ag.use_fused
    o = _bufs(env, K)
    env.rollout_cbf_actor(ag.actor_struct(), sf.params(), K, o['obs'], o['act'], o['rew'], o['done'], o['flags'], o['rows'], o['applied'],
                          terminal_obs=o['term'], episode_acc=o['acc'])
    torch.cuda.synchronize()
    _check_canaries(o)
    act_scale = np.float32(env.spec.action_scale)
    a_pol = o['act'][..., 0].cpu().numpy()
    u_phys = (act_scale * a_pol) if normalized else a_pol                      # float32 product, as the kernel's
    st = o['obs'][:K, :, :4].reshape(-1, 4).contiguous()
    up = torch.tensor(u_phys.reshape(-1), device=env.device)
    rows = o['rows'].reshape(-1, 4)
    lo, hi = float(sf.params().lo), float(sf.params().hi)
    _assert_bits(rows[:, 0], torch.tensor(np.clip(u_phys.reshape(-1), np.float32(lo), np.float32(hi)), device=env.device), 'u0')
    # certify_tensors of this library, and of a library built from scg_cbf.hip (the filter's home): both bit for bit
    nk, nh, na = arw.CBF_NARROW
    narrow = tra._cbf_env(nk, nh, na, normalized)
    for which, f in (('wide', sf), ('scg_cbf.hip', tra._cbf_filter().attach(narrow))):
        u, s, feas = f.certify_tensors(st, up)
        _assert_bits(rows[:, 1], u, f'u* ({which})')
        _assert_bits(rows[:, 2], s, f'slack ({which})')
        assert torch.equal(rows[:, 3].cpu(), feas.float().cpu()), which
    narrow.close()
    feasible = rows[:, 3].cpu().numpy() != 0
    u_star = rows[:, 1].cpu().numpy()
    want = np.where(feasible, (u_star / act_scale) if normalized else u_star, a_pol.reshape(-1)).astype(np.float32)
    _assert_bits(o['applied'].reshape(-1), torch.tensor(want), 'applied')
    corrected = (np.abs(u_star - rows[:, 0].cpu().numpy()) > 1e-6) & feasible
    print(f'[cbf] {kind} 256 normalized={normalized}: corrected share {corrected.mean():.4f}, infeasible share {(~feasible).mean():.4f}')
    assert corrected.any()
    env3 = tra._cbf_env(kind, hidden, act, normalized)
    q = env3.step_sequence(o['applied'].reshape(K, N, 1).contiguous(), terminal_obs=True)
    torch.cuda.synchronize()
    _assert_bits(q['obs'], o['obs'][1:], 'obs')
    _assert_bits(q['reward'], o['rew'], 'reward')
    assert torch.equal(q['done'].cpu(), o['done'].cpu()) and torch.equal(q['flags'].cpu(), o['flags'].cpu())
    done = o['done'].cpu().bool()
    _assert_bits(q['terminal_obs'][done], o['term'][done], 'terminal_obs')
    _assert_bits(env3.ep_stats, env.ep_stats, 'ep_stats')
    env.close()
    env3.close()


def test_sac_run_with_the_safety_filter(tmp_path):
    kind, hidden, act = arw.CBF_CASES[0]
    env_id, cfg, _ = arw.cbf_task_config(False)
    ctrl = _controller('sac', None, hidden, act, tmp_path, task_cfg=(env_id, cfg), **WIDE)
    res = ctrl.run(n_episodes=32, safety_filter=tra._cbf_filter())
    data = res['safety_filter_data']
    assert set(data) == {'steps', 'corrected_steps', 'infeasible_steps', 'mean_correction'}
    assert all(v.shape == (32,) for v in data.values())
    assert np.array_equal(data['steps'], res['ep_lengths'])
    assert ctrl._run_env_cbf.actor_kind == 'sac' and ctrl._run_env_cbf.cbf_shape == (arw.HIDDEN, act, 'sac')
    ctrl.close()


# ------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_launch_nothing():
    from safe_control_gym_amd import _lib as L
    task, kind, hidden, act = arw.CASES[0]
    env = _env(task, (hidden, act, kind))
    ag, _ = _agent(kind, env.spec.obs_dim, env.spec.nu, act)
    actor = ag.actor_struct()

    def refused(fn, a, k=4):
        o = _bufs(env, max(k, 1))
        out = env._actor_rollout_out(o['obs'], o['act'], o['rew'], o['done'], o['flags'], None, None, 0)
        before = env.ep_stats.clone()
        with pytest.raises(L.ScgError):
            L.check(getattr(env._lib, fn)(env._h, C.byref(a), int(k), C.byref(out), env._stream()), env._lib)
        torch.cuda.synchronize()
        # nothing ran: every output still holds its canary, the env's accumulators are as they were
        assert bool(torch.isnan(o['_flat']['obs']).all()) and bool(torch.isnan(o['_flat']['act']).all()) and bool((o['_flat']['done'] == 0xAB).all())
        assert torch.equal(env.ep_stats, before)

    for field, value in (('hidden', 128), ('kind', L.ACTOR_KINDS['ddpg']), ('activation', L.POLICY_ACTS['tanh'])):
        bad = ag.actor_struct()
        setattr(bad, field, value)
        refused('scg_rollout_actor', bad)
    refused('scg_rollout_actor', actor, k=0)
    refused('scg_rollout_actor', actor, k=-3)
    # scg_rollout_policy on a 256 library: exported by the simulator's translation unit, which was compiled without a policy shape
    pol = L.Policy(d_params=actor.d_params, W1=actor.W1, b1=actor.b1, W2=actor.W2, b2=actor.b2, W3=actor.W3, b3=actor.b3, logstd_off=actor.b3,
                   hidden=arw.HIDDEN, activation=L.POLICY_ACTS[act], deterministic=1)
    refused('scg_rollout_policy', pol)
    # scg_rollout_cbf_actor needs an env built with cbf=True
    before = env.ep_stats.clone()
    o = _bufs(env, 4)
    with pytest.raises(L.ScgError):
        env.rollout_cbf_actor(actor, None, 4, o['obs'], o['act'], o['rew'], o['done'], o['flags'], o['rows'], o['applied'])
    torch.cuda.synchronize()
    assert bool(torch.isnan(o['_flat']['obs']).all()) and torch.equal(env.ep_stats, before)
    env.close()
