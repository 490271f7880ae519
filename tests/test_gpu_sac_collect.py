"""SAC's fused training collection (scg_rollout_sac_collect; include/scg_actor_collect.h, csrc/scg_actor_collect.h) on the device: the
sampled and the warm-up action against float64 on the host Philox model, the env step against scg_step_sequence bit for bit, the replay
ring against the host model of scg_sac_push pushed step by step, launch geometries, chaining, the refusals and the `sac` controller's
`collect_steps` key.

Shapes: N = 67 envs (66 with 6-float rows, as tests/test_gpu_rollout_actor._n), K = 40 control steps, episodes of 25 control steps
(tests/actor_collect_cases.py), so every env finishes, auto-resets and goes on inside the launch.  Action bounds: BOUND_SETS of
tests/test_gpu_offpolicy_collector.py (wide, degenerate and asymmetric columns); the mean head is scaled x 6 (tests/test_gpu_rollout_actor._agent).

Tolerance of a sampled action, per element — the one tests/test_gpu_offpolicy_collector.test_sac_sample_in_kernel_draw derives, imported
from there: |a - squash(u64)| <= Bounds.bound(u64, S, sigma eps_tol(eps64, r)), with u64 = mu64 + exp(clamp(ls64, -20, 2)) eps64 on the
stored observation, S = S_mu + sigma |eps| (1 + S_ls where the clamp is not active) (sampled_terms) and eps_tol the on-policy rollouts'
Box-Muller tolerance (tests/philox_model.py).  Warm-up action: uniform_bound of the same file (the float32 expression's two roundings)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import actor_collect_cases as acc
from tests import philox_model as pm

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, K, SEED = 67, 40, 5
PAD = 64
CASE_IDS = ['-'.join(str(v) for v in c) for c in acc.CASES]
RING_KEYS = ('obs', 'act', 'rew', 'next_obs', 'mask', 'pos', 'size_f', 'size_i32')
TRACE_KEYS = ('obs', 'act', 'rew', 'done', 'flags')


def _oc():
    from tests import test_gpu_offpolicy_collector as oc
    return oc


def _ra():
    from tests import test_gpu_rollout_actor as ra
    return ra


def _n(case):
    return 66 if case[0] == 'quadrotor_2D_stab' else N


def _env(task, shape, n, task_cfg=None):
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = task_cfg if task_cfg is not None else acc.task_config(task)
    env = HipVecEnv(env_id, n, seed=SEED, return_numpy=False, policy=shape, **cfg)
    env.reset_tensors()
    return env


class RingView:
    """The host-modelled Ring of tests/test_gpu_offpolicy_collector.py under the names HipVecEnv.sac_collect_struct reads (DeviceReplay's)."""

    def __init__(self, R):
        self.obs, self.act, self.rew, self.next_obs, self.mask = R.obs, R.act, R.rew, R.next_obs, R.mask
        self.capacity, self.pos_t, self.size_t, self.size_i32 = R.cap, R.pos, R.size_f, R.size_i32


def _ring(env, cap, start, full=False):
    R = _oc().Ring(cap, env.spec.obs_dim, env.spec.nu, start)
    if full:                            # a ring that has wrapped before: size == capacity
        R.size_f.fill_(float(cap))
        R.size_i32.fill_(cap)
        R.host['size_f'], R.host['size_i32'] = np.float32(cap), np.array([cap], np.int32)
    return R


def _trace(o):
    return dict(obs=o['obs'], act=o['act'], reward=o['rew'], done=o['done'], flags=o['flags'], terminal_obs=o['term'])


def _collect(env, actor, k, R, o=None, t0=0, uniform=False, cur=None):
    """One launch into ring R with the trace into rows [t0, t0 + k) of canary-filled buffers; returns (trace buffers, cur_obs flat)."""
    ra = _ra()
    o = o if o is not None else ra._bufs(env, k, pad=PAD)
    n, nobs = env.num_envs, env.spec.obs_dim
    cur = cur if cur is not None else torch.full((n * nobs + PAD,), float('nan'), device=env.device)
    tr = {name: t[t0:t0 + k + 1] if name == 'obs' else t[t0:t0 + k] for name, t in _trace(o).items()}
    env.rollout_sac_collect(actor, k, RingView(R), cur[:n * nobs].view(n, nobs), uniform=uniform, trace=tr, episode_acc=o['acc'])
    torch.cuda.synchronize()
    return o, cur


def _host_push(R, o, k):
    """The host model pushed step by step with the trace (the counter word is scg_sac_push's own: not part of this entry point)."""
    obs, act, rew, term = (o[name].cpu().numpy() for name in ('obs', 'act', 'rew', 'term'))
    done, flags = o['done'].cpu().numpy(), o['flags'].cpu().numpy()
    for t in range(k):
        R.host_push(obs[t], act[t], rew[t], obs[t + 1], term[t], done[t], flags[t])


def _check_ring(R, tag):
    oc = _oc()
    for key in RING_KEYS:
        assert np.array_equal(oc.bits(getattr(R, key)), np.ascontiguousarray(R.host[key]).view(np.uint8)), f'{tag}: ring {key} differs'
    assert int(R.counter.item()) == 11, f'{tag}: the noise counter word is not this entry point\'s'


_agents = {}


def _biased_agent(obs_dim, hidden, nu, act):
    """The x 6 agent with log_std biases +10 (even columns) / -40 (odd columns): the clamp bites at both ends."""
    key = (obs_dim, hidden, nu, act)
    if key not in _agents:
        oc = _oc()
        from safe_control_gym_amd.sac import SACAgent, SACConfig
        B = oc.Bounds(oc.BOUND_SETS[0], nu)
        torch.manual_seed(43 + obs_dim + 31 * nu)
        ag = SACAgent(obs_dim, nu, torch.tensor(B.lo.astype(np.float32), device=DEV), torch.tensor(B.hi.astype(np.float32), device=DEV),
                      SACConfig(hidden_dim=hidden, activation=act), DEV)
        assert ag.use_fused
        with torch.no_grad():
            ag.ac.actor.mu_layer.weight.mul_(6.0)
            ag.ac.actor.log_std_layer.bias.add_(torch.tensor([10.0, -40.0, 10.0, -40.0][:nu], device=DEV))
        _agents[key] = (ag, B)
    return _agents[key]


_reference = {}


def _case(case, bound_set=0, uniform=False, biased=False):
    """The K-step launch of a case into a ring of exactly K N rows from position 0, computed once and shared (left unchanged)."""
    key = (case, bound_set, uniform, biased)
    if key not in _reference:
        task, hidden, act = case
        env = _env(task, (hidden, act, 'sac'), _n(case))
        assert env.sac_collect_supported and env.spec.max_episode_steps == acc.EPISODE_STEPS
        ag, B = (_biased_agent if biased else lambda *a: _ra()._agent('sac', *a, bound_set))(env.spec.obs_dim, hidden, env.spec.nu, act)
        step0, ep0 = env.get_counters()
        R = _ring(env, K * env.num_envs, 0)
        o, cur = _collect(env, ag.actor_struct(), K, R, uniform=uniform)
        _reference[key] = dict(o=o, cur=cur, R=R, ep=env.ep_stats.clone(), ag=ag, B=B, start=(step0, ep0, np.arange(env.num_envs)),
                               seed=env.seed_value, n=env.num_envs)
        env.close()
    return _reference[key]


def _addresses(ref):
    """(episode [K, n], step [K, n], global id [1, n]) every step of the launch drew at."""
    step0, ep0, gid = ref['start']
    done = ref['o']['done'].cpu().numpy()
    assert done.max() <= 1
    ep, st = pm.follow(step0, ep0, done)
    return ep, st, np.asarray(gid)[None, :]


# ------------------------------------------------------------------------------------------------------------ 1. the sampled action
@pytest.mark.parametrize('case,bound_set,biased', [(c, b, False) for c in acc.CASES for b in (0, 1)] + [(acc.CASES[2], 0, True)],
                         ids=[f'{i}-bounds{b}' for i in CASE_IDS for b in (0, 1)] + [CASE_IDS[2] + '-clamped'])
def test_sampled_action_matches_float64(case, bound_set, biased):
    oc = _oc()
    ref = _case(case, bound_set, biased=biased)
    o, ag, B = ref['o'], ref['ag'], ref['B']
    nu = B.lo.size
    x = o['obs'][:K].reshape(-1, o['obs'].shape[-1])
    assert bool(torch.isfinite(x).all())
    ep, st, gid = _addresses(ref)
    e64, r = pm.env_normal4(ref['seed'], gid, ep, st, pm.CH_POLICY)
    eps = torch.as_tensor(e64[..., :nu].reshape(-1, nu), device=DEV)
    tol = torch.as_tensor(pm.eps_tol(e64, r)[..., :nu].reshape(-1, nu), device=DEV)
    mu, S_mu, ls, S_ls = oc.sac_ref(ag, x)
    if biased:
        assert int((ls < -20).sum()) > 0 and int((ls > 2).sum()) > 0, 'the log_std clamp did not bite at both ends'
    u, S, sig = oc.sampled_terms(mu, S_mu, ls, S_ls, eps)
    want, bound = B.squash(u), B.bound(u, S, sig * tol)
    got = o['act'].reshape(-1, nu)
    assert bool(torch.isfinite(got).all())
    for j in B.degenerate:
        assert bool((got[:, j] == float(np.float32(B.lo[j]))).all()), f'degenerate column {j} is not low'
    ratio = float(((got.double() - want).abs() / bound).max())
    print(f'[ratio] sac_collect sampled action {CASE_IDS[acc.CASES.index(case)]} bounds {bound_set} biased {biased}: worst error/bound {ratio:.4f} '
          f'(pre-squash span {float(u.max() - u.min()):.2f})')
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------ 2. the warm-up action
@pytest.mark.parametrize('case', acc.CASES, ids=CASE_IDS)
@pytest.mark.parametrize('bound_set', [0, 1])
def test_warm_up_action_is_the_envs_own_uniform_draw(case, bound_set):
    from oracle.rng import u01_from_word
    oc = _oc()
    ref = _case(case, bound_set, uniform=True)
    o, B = ref['o'], ref['B']
    nu = B.lo.size
    ep, st, gid = _addresses(ref)
    u = torch.as_tensor(u01_from_word(pm.env_words(ref['seed'], gid, ep, st, pm.CH_RANDOM_ACTION))[..., :nu].reshape(-1, nu), device=DEV)
    want = B.t_lo + (B.t_hi - B.t_lo) * u
    got = o['act'].reshape(-1, nu)
    assert bool(torch.isfinite(got).all())
    for j in B.degenerate:
        assert bool((got[:, j] == float(np.float32(B.lo[j]))).all()), f'degenerate column {j} is not low'
    ratio = float(((got.double() - want).abs() / oc.uniform_bound(B, want)).max())
    print(f'[ratio] sac_collect warm-up action {CASE_IDS[acc.CASES.index(case)]} bounds {bound_set}: worst error/bound {ratio:.4f}')
    assert ratio <= 1.0
    for j in (j for j in range(nu) if j not in B.degenerate):
        first = o['act'][0, :, j].cpu().numpy()
        assert np.unique(first).size == first.size, f'column {j}: envs share actions'
    # the ring is the host model's in this mode as well
    _host_push(ref['R'], o, K)
    _check_ring(ref['R'], 'warm-up')


# ------------------------------------------------------------------------------------------------------------ 3. the env step
@pytest.mark.parametrize('case', acc.CASES, ids=CASE_IDS)
def test_env_step_is_untouched(case):
    ra = _ra()
    task, hidden, act = case
    ref = _case(case)
    o = ref['o']
    ra._check_canaries(o, pad=PAD)
    assert bool(torch.isnan(ref['cur'][-PAD:]).all()), 'cur_obs: written past its last row'
    env2 = _env(task, (hidden, act, 'sac'), _n(case))
    q = env2.step_sequence(o['act'].contiguous(), terminal_obs=True)
    torch.cuda.synchronize()
    ra._assert_bits(q['obs'], o['obs'][1:], 'obs')
    ra._assert_bits(q['reward'], o['rew'], 'reward')
    assert torch.equal(q['done'].cpu(), o['done'].cpu()) and torch.equal(q['flags'].cpu(), o['flags'].cpu())
    done = o['done'].cpu().bool()
    assert bool(done.any(0).all()), 'every env finishes an episode inside the launch'
    ra._assert_bits(q['terminal_obs'][done], o['term'][done], 'terminal_obs')
    ra._assert_bits(env2.ep_stats, ref['ep'], 'ep_stats')
    assert torch.equal(o['acc'][:, 0].cpu(), done.sum(0).float())
    env2.close()


# ------------------------------------------------------------------------------------------------------------ 4. the ring
def _ring_run(case, cap, start, full, task_cfg=None, bound_set=0):
    task, hidden, act = case
    env = _env(task, (hidden, act, 'sac'), _n(case), task_cfg=task_cfg)
    ag, _ = _ra()._agent('sac', env.spec.obs_dim, hidden, env.spec.nu, act, bound_set)
    n = env.num_envs
    cap = cap(n) if callable(cap) else cap
    start = start(n) if callable(start) else start
    R = _ring(env, cap, start, full)
    o, cur = _collect(env, ag.actor_struct(), K, R)
    tag = f'{case} cap={cap} start={start} full={full}'
    _host_push(R, o, K)
    _check_ring(R, tag)                 # rows, truncation fix-up, pos / size_f / size_i32; rows outside the written range still NaN
    _ra()._assert_bits(cur[:n * env.spec.obs_dim].view(n, -1), o['obs'][K], 'cur_obs')
    assert bool(torch.isnan(cur[-PAD:]).all())
    _ra()._check_canaries(o, pad=PAD)
    env.close()
    done, flags = o['done'].cpu().numpy() != 0, o['flags'].cpu().numpy()
    return done & ((flags & 1) != 0), done & ((flags & 1) == 0)


RING_PAIRS = [(lambda n: K * n, 0, False), (lambda n: K * n, 17, False), (lambda n: K * n + 300, lambda n: K * n + 250, False),
              (lambda n: K * n + 300, 100, True)]


@pytest.mark.parametrize('pair', range(4), ids=['exact-0', 'exact-17-wraps', 'plus300-wraps', 'full-ring'])
@pytest.mark.parametrize('case', acc.CASES, ids=CASE_IDS)
def test_ring_is_the_host_model_pushed_step_by_step(case, pair):
    cap, start, full = RING_PAIRS[pair]
    trunc, term = _ring_run(case, cap, start, full)
    print(f'[ring] {CASE_IDS[acc.CASES.index(case)]} pair {pair}: {int(trunc.sum())} truncated, {int(term.sum())} terminated rows of {term.size}')
    # the quadrotors reach the time limit in some envs: fix-up rows (terminal observation, mask 1) on the transposed and the row-by-row
    # path.  CartPole's pole falls within 25 steps under these actions: its rows are terminations
    if case[0] != 'cartpole_stab':
        assert trunc.any(), 'no env was truncated by the time limit'


def test_ring_rows_of_terminated_episodes():
    cap, start, full = RING_PAIRS[1]
    trunc, term = _ring_run(acc.CASES[0], cap, start, full, task_cfg=acc.terminating_task_config())
    print(f'[ring] terminating task: {int(term.sum())} terminated, {int(trunc.sum())} truncated rows of {term.size}')
    assert term.any(), 'the state constraint terminated no episode'


# ------------------------------------------------------------------------------------------------------------ 5. geometry
@pytest.mark.parametrize('n', [67, 33])
@pytest.mark.parametrize('case', [acc.CASES[0], acc.CASES[2], acc.CASES[3]], ids=[CASE_IDS[0], CASE_IDS[2], CASE_IDS[3]])
def test_results_do_not_depend_on_the_launch_geometry(case, n, monkeypatch):
    ra = _ra()
    task, hidden, act = case
    outs = []
    for geo in (('32', '4'), ('32', '8'), ('64', '4'), ('64', '8')):
        monkeypatch.setenv('SCG_ROLLOUT_EPW', geo[0])
        monkeypatch.setenv('SCG_ROLLOUT_WPW', geo[1])
        env = _env(task, (hidden, act, 'sac'), n)
        ag, _ = ra._agent('sac', env.spec.obs_dim, hidden, env.spec.nu, act)
        R = _ring(env, K * n + 300, K * n + 250)
        o, cur = _collect(env, ag.actor_struct(), K, R)
        ra._check_canaries(o, pad=PAD)
        o.update(ep=env.ep_stats.clone(), cur=cur, R=R)
        outs.append(o)
        env.close()
    for other in outs[1:]:
        for key in TRACE_KEYS + ('acc', 'ep', 'cur'):
            ra._assert_bits(outs[0][key], other[key], key)
        done = outs[0]['done'].bool()
        ra._assert_bits(outs[0]['term'][done], other['term'][done], 'terminal_obs')
        for key in RING_KEYS:
            assert np.array_equal(_oc().bits(getattr(outs[0]['R'], key)), _oc().bits(getattr(other['R'], key))), f'ring {key}'


# ------------------------------------------------------------------------------------------------------------ 6. chaining
# (Quadrotor 3D is not comparable, as for the existing rollouts: tests/test_gpu_rollout_actor.test_chained_launches_equal_one)
@pytest.mark.parametrize('case', [acc.CASES[0], acc.CASES[1]], ids=[CASE_IDS[0], CASE_IDS[1]])
def test_chained_launches_equal_one(case):
    ra = _ra()
    task, hidden, act = case
    ref = _case(case)
    env = _env(task, (hidden, act, 'sac'), _n(case))
    R = _ring(env, K * env.num_envs, 0)
    c = ra._bufs(env, K, pad=PAD)
    cur = torch.full((env.num_envs * env.spec.obs_dim + PAD,), float('nan'), device=env.device)
    _collect(env, ref['ag'].actor_struct(), 17, R, c, 0, cur=cur)
    assert int(R.pos.item()) == 17 * env.num_envs
    _collect(env, ref['ag'].actor_struct(), 23, R, c, 17, cur=cur)
    for key in TRACE_KEYS + ('acc',):
        ra._assert_bits(c[key], ref['o'][key], key)
    ra._assert_bits(cur, ref['cur'], 'cur_obs')
    ra._assert_bits(env.ep_stats, ref['ep'], 'ep_stats')
    for key in RING_KEYS:
        assert np.array_equal(_oc().bits(getattr(R, key)), _oc().bits(getattr(ref['R'], key))), f'ring {key}'
    env.close()


# ------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing():
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd.vec_env import HipVecEnv
    ra = _ra()
    task, hidden, act = acc.CASES[0]
    ag, _ = ra._agent('sac', 4, hidden, 1, act)
    k = 4

    def refused(env, match, actor=None, k=k, cap=None, direct=False, **edit):
        """The call raises with `match` in the message; ring, counters, every canary-filled output and ep_stats are as they were."""
        n, nobs = env.num_envs, env.spec.obs_dim
        R = _ring(env, cap if cap is not None else max(k, 1) * n + 5, 3)
        o = ra._bufs(env, max(k, 1), pad=PAD)
        cur = torch.full((n * nobs + PAD,), float('nan'), device=env.device)
        c = env.sac_collect_struct(RingView(R), cur[:n * nobs].view(n, nobs), trace=_trace(o), episode_acc=o['acc'])
        for field, value in edit.items():
            setattr(c, field, value)
        before = env.ep_stats.clone()
        a = actor if actor is not None else ag.actor_struct()
        with pytest.raises(L.ScgError, match=match):
            if direct:                  # a library whose env has no actor kind: the exported entry point itself
                L.check(env._lib.scg_rollout_sac_collect(env._h, C.byref(a), int(k), C.byref(c), env._stream()), env._lib)
            else:
                env.rollout_sac_collect(a, k, None, None, struct=c)
        torch.cuda.synchronize()
        _check_ring(R, match)           # (nothing was pushed on the host model: NaN rows, pos 3, sizes 3)
        assert all(bool(torch.isnan(o['_flat'][name]).all()) for name in ('obs', 'act', 'rew', 'term')) and bool((o['_flat']['done'] == 0xAB).all())
        assert bool(torch.isnan(cur).all()) and bool((o['acc'] == 0).all())
        assert torch.equal(env.ep_stats, before)

    env = _env(task, (hidden, act, 'sac'), N)
    assert env.sac_collect_supported
    refused(env, 'k_steps must be positive', k=0)
    refused(env, 'k_steps must be positive', k=-3)
    refused(env, 'exceeds the replay capacity', cap=k * N - 1)
    for field, value in (('kind', L.ACTOR_KINDS['ddpg']), ('hidden', 32), ('activation', L.POLICY_ACTS['tanh'])):
        bad = ag.actor_struct()
        setattr(bad, field, value)
        refused(env, 'another actor shape', actor=bad)
    bad = ag.actor_struct()
    bad.d_params = None
    refused(env, 'needs d_params', actor=bad)
    for field in ('d_ring_obs', 'd_ring_act', 'd_ring_rew', 'd_ring_next_obs', 'd_ring_mask', 'd_pos', 'd_cur_obs'):
        refused(env, 'needs d_params', **{field: None})
    for field in ('d_obs', 'd_act', 'd_reward', 'd_done', 'd_flags', 'd_terminal_obs'):
        refused(env, 'all together or not at all', **{field: None})
    env.close()
    # libraries that export the entry point and refuse: kind ddpg, hidden width 256
    for (t2, h2, a2, k2), match in zip(acc.REFUSING, ('serves kind sac', 'hidden width 256')):
        other = _env(t2, (h2, a2, k2), N)
        assert other.actor_kind == k2 and not other.sac_collect_supported
        refused(other, match)
        other.close()
    # a library built without a kind: the CBF library exports the entry point and refuses; the PPO library does not carry it at all
    env_c, cfg_c, s_c = ra.arc.cbf_task_config(False)
    plain_cbf = HipVecEnv(env_c, N, seed=SEED, return_numpy=False, policy=(s_c['algo_config']['hidden_dim'], s_c['algo_config']['activation']),
                          cbf=True, **cfg_c)
    plain_cbf.reset_tensors()
    assert plain_cbf.actor_kind is None and not plain_cbf.sac_collect_supported
    refused(plain_cbf, 'with kind sac', direct=True)
    refused(plain_cbf, 'not built with an actor kind')
    plain_cbf.close()
    env_id, cfg = acc.task_config(task)
    plain = HipVecEnv(env_id, N, seed=SEED, return_numpy=False, policy=(hidden, act), **cfg)
    plain.reset_tensors()
    assert not hasattr(plain._lib, 'scg_rollout_sac_collect') and not plain.sac_collect_supported
    refused(plain, 'not built with an actor kind')
    plain.close()


# ------------------------------------------------------------------------------------------------------------ 8. the trainer
TRAIN = dict(fused_rollout=True, collect_steps=8, rollout_batch_size=16, warm_up_steps=100, train_interval=64, train_batch_size=32,
             max_buffer_size=10000, max_env_steps=400, eval_batch_size=8)


def _controller(tmp_path, cid='sac', **over):
    hidden, act = acc.TRAINER_SHAPE
    return _ra()._controller(cid, acc.TRAINER_TASK, hidden, act, tmp_path, **dict(TRAIN, **over))


def _stepwise_schedule(n, warm_up, interval, max_steps, k_max):
    """(chunk length, uniform, updates) per train_step, from the stepwise loop's rule: a chunk ends at k_max steps, at the last warm-up
    step and where the stepwise trainer would update."""
    total = since = 0
    seq, k, mode = [], 0, None
    while total < max_steps or k:
        if k == 0:
            if total >= max_steps:
                break
            mode = total < warm_up
        k += 1
        total += n
        since += n
        upd = since if total > warm_up and since >= interval else 0
        if upd or k == k_max or (total < warm_up) != mode:
            seq.append((k, int(mode), upd))
            since, k = (0 if upd else since), 0
    return seq


def _run(ctrl, max_steps, calls):
    out = []
    while ctrl.total_steps < max_steps:
        before = len(calls)
        r = ctrl.train_step()
        assert len(calls) == before + 1, 'one rollout_sac_collect call per chunk'
        out.append(calls[-1] + (r.get('updates', 0),))
    return out


def _wrap(ctrl):
    calls = []
    inner = ctrl.env.rollout_sac_collect

    def counting(actor, k, *a, struct=None, **kw):
        calls.append((int(k), int(struct.uniform)))
        return inner(actor, k, *a, struct=struct, **kw)
    ctrl.env.rollout_sac_collect = counting
    return calls


def test_trainer_keeps_the_stepwise_schedule(tmp_path):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        ctrl = _controller(tmp_path)
    assert not [w for w in caught if 'collect_steps' in str(w.message) or 'fused_rollout' in str(w.message)]
    assert ctrl.impl._collect_k == 8 and ctrl.env.sac_collect_supported and ctrl.impl._fused_collect
    calls = _wrap(ctrl)
    seq = _run(ctrl, 400, calls)
    want = _stepwise_schedule(16, 100, 64, 400, 8)
    assert seq == want, (seq, want)
    # 7 uniform steps (total_steps 0 .. 96 < 100) owe 112 updates, then a chunk ends wherever 64 env steps have passed: 4 vector steps
    assert want[0] == (7, 1, 112) and want[1:] == [(4, 0, 64)] * (len(want) - 1) and sum(k for k, _, _ in want) * 16 == ctrl.total_steps
    buf = ctrl.impl.buffer
    assert buf.size == ctrl.total_steps == int(buf.size_i32.item()) == int(buf.size_t.item()) and buf.pos == int(buf.pos_t.item())
    assert bool(torch.isfinite(ctrl.agent._flat['p']).all())
    assert bool(torch.isfinite(buf.obs[:buf.size]).all()) and bool(torch.isfinite(buf.next_obs[:buf.size]).all())
    assert int(ctrl.impl._collect_counter.item()) == 0, 'collect_counter belongs to the stepwise collector'
    ctrl.close()


def test_trainer_resumes_bit_for_bit(tmp_path):
    ctrl = _controller(tmp_path)
    calls = _wrap(ctrl)
    _run(ctrl, 208, calls)
    path = str(tmp_path / 'sac_chunked.pt')
    ctrl.save(path, save_buffer=True)
    again = _controller(tmp_path)
    again.load(path)
    assert again.total_steps == ctrl.total_steps and again.impl._since_update == ctrl.impl._since_update
    calls2 = _wrap(again)
    a, b = _run(ctrl, 400, calls), _run(again, 400, calls2)
    assert a == b and any(u for _, _, u in a)
    ra = _ra()
    ra._assert_bits(ctrl.agent._flat['p'], again.agent._flat['p'], 'parameters')
    ra._assert_bits(ctrl.agent._flat['targ'], again.agent._flat['targ'], 'target parameters')
    n = ctrl.impl.buffer.size
    for key in ('obs', 'act', 'rew', 'next_obs', 'mask'):
        ra._assert_bits(getattr(ctrl.impl.buffer, key)[:n], getattr(again.impl.buffer, key)[:n], f'ring {key}')
    ra._assert_bits(ctrl.impl.obs, again.impl.obs, 'current observation')
    ctrl.close()
    again.close()


def test_collect_steps_key_needs(tmp_path):
    with pytest.raises(ValueError, match='fused_rollout'):
        _controller(tmp_path, fused_rollout=False)
    with pytest.raises(ValueError, match='shared noise process'):
        _ra()._controller('ddpg', 'cartpole_stab', 32, 'tanh', tmp_path, **TRAIN)
    with pytest.raises(ValueError, match='max_buffer_size'):
        _controller(tmp_path, max_buffer_size=100)
    with pytest.warns(UserWarning, match='collect_steps=8 needs'):
        ctrl = _controller(tmp_path, norm_obs=True, updates_per_step=4)
    assert ctrl.impl._collect_k == 0
    ctrl.env.rollout_sac_collect = None         # (the stepwise collector never asks for it)
    res = [ctrl.train_step() for _ in range(8)]
    assert ctrl.total_steps == 8 * 16 and [r.get('updates', 0) for r in res] == [0] * 6 + [4, 0]
    ctrl.close()
