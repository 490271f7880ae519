"""The CBF safety filter on the device: scg_cbf_certify against the float64 restatement (tests/cbf_model.py) on the reference-generated
fixture rows, scg_rollout_cbf against scg_cbf_certify (one arithmetic), against step_sequence (the env step is untouched) and against
scg_rollout_policy (the policy's own draw), the filter's semantics, its effect with the reference example's shipped policy, is_cbf on
the reference's default grid, and ppo.evaluate(safety_filter=).

Tolerance of certify vs the float64 restatement.  Not known in advance (u* ~ -k / b is ill-conditioned where |b| is small and the
result is not clipped), so it is MEASURED against something that is not the code under test: the same closed form in NumPy float32 on
the CPU against float64 on the fixture rows; the kernel is allowed 4x the worst |du*| and |ds*| of that (other sin / cos, other
contraction).  On the fixture (3000 rows up to 1.1x the limits, actions in [-12, 12]) the CPU measurement is
    default prior   |du*| <= 8.1e-6   |ds*| <= 4.5e-6        non-default prior   |du*| <= 4.8e-6   |ds*| <= 4.7e-6
so the bounds are 3.2e-5 / 1.8e-5 and 1.9e-5 / 1.9e-5.  Rows whose float64 s* lies within the slack bound of slack_tolerance, or
whose r(u0) lies within it of 0 (either side of the branch is then a correct float32 answer), are left out of the flag and value
comparison: at most 1 % of the rows, asserted."""
import copy
import json
import os

import numpy as np
import pytest

from tests import cbf_model as M

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
D = np.load(os.path.join(GOLDEN, 'cbf.npz'))
S = json.load(open(os.path.join(GOLDEN, 'cbf_settings.json')))
SF = S['sf_config']
LO, HI = (float(v) for v in D['action_bounds'])
HIDDEN, ACT = S['algo_config']['hidden_dim'], S['algo_config']['activation']
FLAG_VIOLATION = 2


def _cfg(**over):
    cfg = copy.deepcopy(S['task_config'])
    cfg.pop('seed', None)
    cfg.update(randomized_init=True)                    # the example's init_state_randomization_info
    cfg.update(over)
    return cfg


def _env(n, seed=7, cbf=True, **over):
    from safe_control_gym_amd.vec_env import HipVecEnv
    env = HipVecEnv(S['task'], n, seed=seed, return_numpy=False, policy=(HIDDEN, ACT), cbf=cbf, **_cfg(**over))
    assert env.cbf_shape == (HIDDEN, ACT)
    env.reset_tensors()
    return env


def _filter(prior_prop=None, **over):
    from functools import partial
    from safe_control_gym_amd.registration import make
    sf = dict(copy.deepcopy(SF), **over)
    if prior_prop:
        sf['prior_info'] = {'prior_prop': prior_prop}
    return make('cbf', partial(make, S['task'], **_cfg()), **sf)


def _policy(dev, det, scale=1.0, logstd=None):
    """(flat parameters, _lib.Policy, ActorPtrs) of the example's shipped PPO actor; `scale` multiplies the output layer (a policy
    that asks for more than the filter allows), `logstd` overrides the shipped one."""
    from safe_control_gym_amd import _cbf
    from safe_control_gym_amd import _lib as L
    parts = [D[f'actor/actor.pi_net.fcs.{i}.{k}'] for i in range(3) for k in ('weight', 'bias')] + [D['actor/actor.logstd']]
    parts = [np.asarray(p, dtype=np.float32).reshape(-1) for p in parts]
    parts[4], parts[5] = parts[4] * np.float32(scale), parts[5] * np.float32(scale)
    if logstd is not None:
        parts[6] = np.full_like(parts[6], logstd)
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    flat = torch.tensor(np.concatenate(parts), device=dev)
    pol = L.Policy(d_params=flat.data_ptr(), W1=int(offs[0]), b1=int(offs[1]), W2=int(offs[2]), b2=int(offs[3]), W3=int(offs[4]),
                   b3=int(offs[5]), logstd_off=int(offs[6]), hidden=HIDDEN, activation=L.POLICY_ACTS[ACT], deterministic=int(det))
    return flat, pol, _cbf.actor_ptrs_of_policy(pol)


def _actor_module(flat, dev):
    """The ppo.MLPActor whose parameters are `flat` (the layout _policy packs)."""
    from safe_control_gym_amd.ppo import MLPActor
    m = MLPActor(4, 1, [HIDDEN, HIDDEN], ACT).to(dev)
    tensors = [t for fc in m.pi_net.fcs for t in (fc.weight, fc.bias)] + [m.logstd]
    at = 0
    with torch.no_grad():
        for t in tensors:
            t.copy_(flat[at:at + t.numel()].view_as(t))
            at += t.numel()
    assert at == flat.numel()
    return m


def _bufs(env, k):
    n, nobs, nu = env.num_envs, env.spec.obs_dim, env.spec.nu
    f = dict(device=env.device, dtype=torch.float32)
    u8 = dict(device=env.device, dtype=torch.uint8)
    return {'obs': torch.zeros(k + 1, n, nobs, **f), 'act': torch.zeros(k, n, nu, **f), 'logp': torch.zeros(k, n, **f),
            'rew': torch.zeros(k, n, **f), 'done': torch.zeros(k, n, **u8), 'flags': torch.zeros(k, n, **u8),
            'term': torch.zeros(k, n, nobs, **f), 'acc': torch.zeros(n, 8, **f),
            'rows': torch.full((k, n, 4), float('nan'), **f), 'applied': torch.full((k, n), float('nan'), **f)}


def _rollout_cbf(env, sf, actor, k, det):
    o = _bufs(env, k)
    env.rollout_cbf(actor, sf.params(), k, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'], o['rows'], o['applied'],
                    deterministic=det, terminal_obs=o['term'], episode_acc=o['acc'])
    torch.cuda.synchronize()
    return o


def _rollout_policy(env, pol, k):
    o = _bufs(env, k)
    env.rollout_policy(pol, k, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'], terminal_obs=o['term'], episode_acc=o['acc'])
    torch.cuda.synchronize()
    return o


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


def _assert_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f'{what}: not bit-identical'


@pytest.mark.parametrize('tag', ['default', 'alt'])
@pytest.mark.parametrize('mode', ['soft', 'hard'])
def test_certify_matches_the_float64_restatement(tag, mode):
    soft = mode == 'soft'
    args = (D['states'], D['actions'], D['limits'], D[f'{tag}/prior'], SF['slope'], SF['slack_weight'], SF['slack_tolerance'], LO, HI)
    r64 = M.certify(*args, soft=soft)
    r32 = M.certify(*args, soft=soft, dtype=np.float32)
    # the float32 cost of the closed form, measured on the CPU
    tol_u_cpu = np.abs(r32['u'].astype(np.float64) - r64['u']).max()
    tol_s_cpu = np.abs(r32['s'].astype(np.float64) - r64['s']).max()
    bound_u, bound_s = 4 * tol_u_cpu, 4 * tol_s_cpu
    env = _env(64)
    sf = _filter(S['non_default_prior_prop'] if tag == 'alt' else None, soft_constrained=soft).attach(env)
    st = torch.tensor(D['states'], dtype=torch.float32, device=env.device)
    ac = torch.tensor(D['actions'], dtype=torch.float32, device=env.device)
    u, s, feas = sf.certify_tensors(st, ac)
    u, s, feas = u.double().cpu().numpy(), s.double().cpu().numpy(), feas.cpu().numpy().astype(bool)
    near = np.abs(r64['r0']) <= bound_s
    if soft:
        near |= np.abs(r64['s'] - SF['slack_tolerance']) <= bound_s
    keep = ~near
    du, ds = np.abs(u - r64['u'])[keep].max(), np.abs(s - r64['s'])[keep].max()
    print(f'{tag} {mode}: CPU float32 |du*| {tol_u_cpu:.3e} |ds*| {tol_s_cpu:.3e}; bounds {bound_u:.3e} / {bound_s:.3e}; kernel |du*| {du:.3e} '
          f'|ds*| {ds:.3e}; boundary rows {int(near.sum())} / {len(near)}; flag mismatches {int((feas != r64["feasible"])[keep].sum())}')
    assert near.mean() <= 0.01
    assert (feas == r64['feasible'])[keep].all()
    cmp = keep & (r64['feasible'] if not soft else np.ones(len(keep), bool))        # hard, empty feasible set: the flag only
    assert np.abs(u - r64['u'])[cmp].max() <= bound_u and np.abs(s - r64['s'])[cmp].max() <= bound_s
    # single-state call: the reference's surface and bookkeeping
    c1, ok1 = sf.certify_action(D['states'][3], np.array([D['actions'][3]]))
    assert c1.shape == () and ok1 == bool(feas[3]) and abs(float(c1) - u[3]) == 0.0
    assert len(sf.results_dict['feasible']) == 1 and sf.results_dict['uncertified_action'][0] == np.clip(D['actions'][3], LO, HI)
    cb, okb = sf.certify_action(D['states'][:5], D['actions'][:5])
    assert np.array_equal(cb, u[:5]) and np.array_equal(okb, feas[:5])
    env.close()


@pytest.mark.parametrize('normalized', [False, True])
@pytest.mark.parametrize('det', [False, True])
def test_rollout_rows_equal_certify_and_the_env_step_is_untouched(normalized, det):
    """One arithmetic (filter rows == scg_cbf_certify of the recorded observations and policy actions, bit for bit), the semantics
    (feasible: normalize(u*) applied; infeasible: the policy's own action; deterministic: the mean), and the env step (replaying the
    applied actions through step_sequence reproduces every output bit for bit)."""
    n, k, seed = 320, 40, 11
    env = _env(n, seed=seed, normalized_rl_action_space=normalized)
    sf = _filter().attach(env)
    scale_out = 30.0 if not normalized else 3.0          # asks for up to +-30 N: corrections, infeasible rows and the input clip all occur
    flat, pol, actor = _policy(env.device, det, scale=scale_out, logstd=-0.5)
    o = _rollout_cbf(env, sf, actor, k, det)
    act_scale = np.float32(env.spec.action_scale)
    a_pol = o['act'][..., 0].cpu().numpy()
    u_phys = (act_scale * a_pol) if normalized else a_pol                      # float32 product, as the kernel's
    st = o['obs'][:k, :, :4].reshape(-1, 4).contiguous()
    u, s, feas = sf.certify_tensors(st, torch.tensor(u_phys.reshape(-1), device=env.device))
    rows = o['rows'].reshape(-1, 4)
    _assert_bits(rows[:, 1], u, 'u*')
    _assert_bits(rows[:, 2], s, 's*')
    assert torch.equal(rows[:, 3].cpu(), feas.float().cpu())
    np.testing.assert_array_equal(rows[:, 0].cpu().numpy(), np.clip(u_phys.reshape(-1), np.float32(LO), np.float32(HI)))
    # semantics
    f = rows[:, 3].cpu().numpy() != 0
    ustar = rows[:, 1].cpu().numpy()
    want = np.where(f, (ustar / act_scale) if normalized else ustar, a_pol.reshape(-1)).astype(np.float32)
    np.testing.assert_array_equal(o['applied'].cpu().numpy().reshape(-1).view(np.int32), want.view(np.int32))
    corrected = np.abs(ustar - rows[:, 0].cpu().numpy()) > 1e-6
    print(f'normalized {normalized} det {det}: feasible {f.mean():.3f}, corrected {corrected.mean():.3f}, clipped {(np.abs(u_phys) > HI).mean():.3f}')
    assert 0 < f.mean() < 1 and corrected.mean() > 0.01 and (np.abs(u_phys) > HI).any()
    # the policy's own action and log-probability: scg_rollout_policy's on the first step (same state, same Philox draw)
    env2 = _env(n, seed=seed, normalized_rl_action_space=normalized)
    p = _rollout_policy(env2, pol, 1)
    _assert_bits(p['act'][0], o['act'][0], 'act[0]')
    _assert_bits(p['logp'][0], o['logp'][0], 'logp[0]')
    _assert_bits(p['obs'][0], o['obs'][0], 'obs[0]')
    # ... and on every step: the float64 actor on the recorded observation + sigma x the host Philox model's channel-5 draw at the
    # env's counters (one reset: episode 0, step 0; auto-resets followed), the log-probability the float64 Gaussian's
    from tests import philox_model as pm
    from tests import test_gpu_rollout_noise as RN
    start = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.arange(n))
    RN.check_actor('scg_rollout_cbf', _actor_module(flat, env.device), o['obs'][:k], o['act'], o['logp'], det,
                   *RN.model_draws(o, start, pm.CH_POLICY, 1, seed=seed))
    if det:                                             # the mean: no noise in the action
        flat2, pol2, actor2 = _policy(env.device, True, scale=scale_out, logstd=2.0)
        env4 = _env(n, seed=seed, normalized_rl_action_space=normalized)
        o2 = _rollout_cbf(env4, sf, actor2, 2, True)
        _assert_bits(o2['act'], o['act'][:2], 'deterministic act does not depend on logstd')
        env4.close()
    # the env step: replay the applied actions
    env3 = _env(n, seed=seed, normalized_rl_action_space=normalized)
    q = env3.step_sequence(o['applied'].reshape(k, n, 1).contiguous(), terminal_obs=True)
    torch.cuda.synchronize()
    _assert_bits(q['obs'], o['obs'][1:], 'obs')
    _assert_bits(q['reward'], o['rew'], 'reward')
    assert torch.equal(q['done'].cpu(), o['done'].cpu()) and torch.equal(q['flags'].cpu(), o['flags'].cpu())
    done = o['done'].cpu().bool()
    assert done.any()
    _assert_bits(q['terminal_obs'][done], o['term'][done], 'terminal_obs')
    for e in (env, env2, env3):
        e.close()


@pytest.mark.parametrize('geometry', [('64', '4'), ('32', '8'), ('64', '8')])
def test_results_do_not_depend_on_the_launch_geometry(geometry, monkeypatch):
    n, k = 320, 12
    outs = []
    for geo in (('32', '4'), geometry):
        monkeypatch.setenv('SCG_ROLLOUT_EPW', geo[0])
        monkeypatch.setenv('SCG_ROLLOUT_WPW', geo[1])
        env = _env(n, seed=3)
        sf = _filter().attach(env)
        flat, _, actor = _policy(env.device, False, scale=30.0, logstd=-0.5)     # (flat held: actor points into its memory)
        outs.append(_rollout_cbf(env, sf, actor, k, False))
        env.close()
    for key in ('obs', 'act', 'logp', 'rew', 'done', 'flags', 'rows', 'applied', 'acc'):
        _assert_bits(outs[0][key], outs[1][key], key)


def test_the_filter_filters():
    """The shipped policy on the example's task, 4 096 envs, randomised init, full episodes: the share of steps that violate the state
    constraint with the filter is not larger than without it, and the filter does correct.  (No threshold on the size of the
    improvement: the two rates are printed; DESIGN.md records them.)"""
    n = 4096
    k = int(S['task_config']['episode_len_sec'] * S['task_config']['ctrl_freq'])
    rates = {}
    for filtered in (False, True):
        env = _env(n, seed=21)
        assert env.spec.max_episode_steps == k
        _, pol, actor = _policy(env.device, True)
        if filtered:
            sf = _filter().attach(env)
            o = _rollout_cbf(env, sf, actor, k, True)
        else:
            o = _rollout_policy(env, pol, k)
        done = o['done'].float()
        first = ((done.cumsum(0) - done) < 1).cpu().numpy()                      # steps of each env's first episode
        viol = ((o['flags'] & FLAG_VIOLATION) != 0).cpu().numpy()
        rates[filtered] = viol[first].mean()
        if filtered:
            rows = o['rows'].cpu().numpy()
            corrected = (np.abs(rows[..., 1] - rows[..., 0]) > 1e-6) & (rows[..., 3] != 0)
            share, infeasible = corrected[first].mean(), (rows[..., 3] == 0)[first].mean()
            ret = (o['acc'][:, 1].sum() / o['acc'][:, 0].sum()).item()
        else:
            ret0 = (o['acc'][:, 1].sum() / o['acc'][:, 0].sum()).item()
        env.close()
    print(f'violating share of steps: unfiltered {rates[False]:.5f}, filtered {rates[True]:.5f}; corrected share {share:.5f}, infeasible share '
          f'{infeasible:.5f}; mean return unfiltered {ret0:.3f}, filtered {ret:.3f}')
    assert rates[True] <= rates[False]
    assert share > 0


def test_is_cbf_equals_the_restatement_on_the_default_grid():
    from safe_control_gym_amd.cbf import state_grid
    env = _env(64)
    sf = _filter().attach(env)
    valid, infeasible = sf.is_cbf()
    grid = state_grid(D['limits'], 100, 0.01)
    assert grid.shape == (26 ** 4, 4)
    args = (grid, np.ones(len(grid)), D['limits'], D['default/prior'], SF['slope'], SF['slack_weight'], SF['slack_tolerance'], LO, HI)
    r64 = M.certify(*args)
    r32 = M.certify(*args, dtype=np.float32)
    bound_s = 4 * np.abs(r32['s'].astype(np.float64) - r64['s']).max()
    near = (np.abs(r64['r0']) <= bound_s) | (np.abs(r64['s'] - SF['slack_tolerance']) <= bound_s)
    bad64 = ~r64['feasible']
    h = 1.0 - ((grid / D['limits']) ** 2).sum(axis=1)
    valid64 = not (bad64 & (h > 1e-6)).any()
    got = np.zeros(len(grid), bool)
    index = {tuple(np.round(g, 9)): i for i, g in enumerate(grid)}
    for sx in infeasible:
        got[index[tuple(np.round(sx, 9))]] = True
    print(f'is_cbf: valid {valid} (float64 {valid64}), infeasible states {int(got.sum())} (float64 {int(bad64.sum())}), boundary rows '
          f'{int(near.sum())} / {len(grid)}, slack bound {bound_s:.3e}')
    assert near.mean() <= 0.01
    assert (got == bad64)[~near].all()
    assert valid == valid64 or (near & (h > 1e-6) & (got != bad64)).any()
    env.close()


def test_evaluate_with_the_filter_equals_an_explicit_rollout():
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd.ppo import evaluate
    n = 256
    env = _env(n, seed=5)
    sf = _filter()
    _, pol, actor = _policy(env.device, True)
    res = evaluate(None, env, policy=pol, safety_filter=sf)
    k = env.spec.max_episode_steps
    env2 = _env(n, seed=5)
    env2.reset_tensors()                                # evaluate() resets the env it is given once more: the same episodes here
    o = _bufs(env2, k)
    env2.rollout_cbf(actor, sf.params(), k, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'], o['rows'], o['applied'],
                     deterministic=True, episode_acc=o['acc'], max_episodes=1)
    torch.cuda.synchronize()
    a = o['acc']
    cnt = a[:, 0].sum().item()
    assert res['episodes'] == cnt == n
    for key, col in (('ep_return', 1), ('ep_length', 2), ('ep_constraint_violation', 3), ('ep_mse', 4)):
        assert res[key] == (a[:, col].sum() / a[:, 0].sum().clamp(min=1.0)).item(), key
    _assert_bits(env._eval_cbf['rows'], o['rows'], 'filter rows')
    fd = res['safety_filter_data']
    assert set(fd) == {'steps', 'corrected_steps', 'infeasible_steps', 'mean_correction'}
    assert torch.equal(fd['steps'].cpu(), a[:, 2].cpu())                          # first-episode steps = the episode length
    done = o['done'].float()
    first = ((done.cumsum(0) - done) < 1).float()
    assert torch.equal(fd['infeasible_steps'].cpu(), ((1 - o['rows'][..., 3]) * first).sum(0).cpu())
    assert fd['corrected_steps'].sum().item() > 0
    # without a fused filter library there is no filtered evaluation
    plain = _envless_cbf(n)
    with pytest.raises(L.ScgError, match='cbf=True'):
        evaluate(None, plain, policy=pol, safety_filter=sf)
    for e in (env, env2, plain):
        e.close()


def _envless_cbf(n):
    from safe_control_gym_amd.vec_env import HipVecEnv
    return HipVecEnv(S['task'], n, seed=5, return_numpy=False, policy=(HIDDEN, ACT), **_cfg())
