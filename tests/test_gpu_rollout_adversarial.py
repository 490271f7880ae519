"""scg_rollout_adversarial — the RARL / RAP collector as one launch (protagonist, adversary or population, env step) — against the
step-by-step path, the PyTorch actors, itself under other launch geometries and populations, scg_rollout_policy, and the collectors
and controllers built on it."""
import functools
import os
import warnings

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import __graft_entry__ as G                                         # noqa: E402  (the adversary settings of the prebuilt variants)

H, ACT, N, K = 64, 'tanh', 320, 12                                 # 320 envs: 5 / 10 waves, a partial workgroup
GEOMETRIES = [('64', '4'), ('32', '4'), ('32', '8'), ('64', '8')]


def _task(over, task='quadrotor_2D_track'):
    from safe_control_gym_amd.registration import load_task
    env_id, cfg = load_task(task)
    return env_id, dict(cfg, **over)


def _env(over, n_adv, n=N, seed=5, **kw):
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = _task(over)
    env = HipVecEnv(env_id, n, seed=seed, return_numpy=False, policy=(H, ACT), adversaries=n_adv, **cfg, **kw)
    env.reset_tensors()
    return env


def _actors(env, n_adv, seed=0):
    """A protagonist PPOAgent (flat parameter vector) and n adversary actors with distinct weights and noise scales."""
    from safe_control_gym_amd.ppo import MLPActor, PPOAgent, PPOConfig
    torch.manual_seed(seed)
    agent = PPOAgent(env.spec.obs_dim, env.spec.nu, PPOConfig(hidden_dim=H, activation=ACT), env.device)
    advs = []
    for k in range(n_adv):
        a = MLPActor(env.spec.obs_dim, env.spec.adversary_dim, [H, H], ACT).to(env.device)
        with torch.no_grad():
            a.logstd.copy_(torch.linspace(-1.0, 0.2, env.spec.adversary_dim) - 0.3 * k)
        advs.append(a)
    return agent, advs


def _policy(agent, deterministic=False):
    from safe_control_gym_amd import _lib as L
    a_lay, _, ls_off, _ = agent._layouts()
    return L.Policy(d_params=agent._flat['p'].data_ptr(), W1=a_lay.W1, b1=a_lay.b1, W2=a_lay.W2, b2=a_lay.b2, W3=a_lay.W3, b3=a_lay.b3,
                    logstd_off=ls_off, hidden=H, activation=0, deterministic=int(deterministic))


def _groups(n, n_adv):
    """Sorted contiguous groups whose boundaries fall inside waves (100, 213 are not multiples of 32)."""
    idx = np.zeros(n, dtype=np.int32)
    for k, b in enumerate((100, 213, 290)[:n_adv - 1]):
        idx[b:] = k + 1
    return idx


def _run(env, agent, advs, idx=None, det=False, det_adv=False, k=K):
    from safe_control_gym_amd import _adversarial
    n, nobs, nu, ad = env.num_envs, env.spec.obs_dim, env.spec.nu, env.spec.adversary_dim
    f = dict(device=env.device, dtype=torch.float32)
    u8 = dict(device=env.device, dtype=torch.uint8)
    o = {'obs': torch.zeros(k + 1, n, nobs, **f), 'act': torch.zeros(k, n, nu, **f), 'logp': torch.zeros(k, n, **f),
         'rew': torch.zeros(k, n, **f), 'done': torch.zeros(k, n, **u8), 'flags': torch.zeros(k, n, **u8),
         'term': torch.zeros(k, n, nobs, **f), 'aact': torch.zeros(k, n, ad, **f), 'alogp': torch.zeros(k, n, **f),
         'acc': torch.zeros(n, 8, **f)}
    ix = torch.as_tensor(idx, device=env.device) if idx is not None else None
    env.rollout_adversarial(_policy(agent, det), [_adversarial.actor_ptrs(a) for a in advs], k, o['obs'], o['act'], o['logp'], o['rew'],
                            o['done'], o['flags'], o['aact'], o['alogp'], adv_index=ix, deterministic_adversary=det_adv,
                            terminal_obs=o['term'], episode_acc=o['acc'])
    torch.cuda.synchronize()
    return o


CASES = [(G.ADV_ACTION, 1), (G.ADV_DYNAMICS, 1), (G.ADV_DYNAMICS, 2), (G.ADV_DYNAMICS, 3)]


@pytest.mark.parametrize('over,n_adv', CASES, ids=['rarl-action', 'rarl-dynamics', 'rap2', 'rap3'])
@pytest.mark.parametrize('epw,wpw', GEOMETRIES)
def test_env_trajectory_is_bit_exact_against_step_sequence(over, n_adv, epw, wpw, monkeypatch):
    """The kernel's stored protagonist actions, with its raw adversary actions through set_adversary_control, replayed through
    scg_step_sequence on a second identically seeded handle: obs, reward, done, flags and terminal obs match bit for bit."""
    monkeypatch.setenv('SCG_ROLLOUT_EPW', epw)
    monkeypatch.setenv('SCG_ROLLOUT_WPW', wpw)
    env, ref = _env(over, n_adv), _env(over, n_adv)
    assert env.adversary_shape == (H, ACT, n_adv)
    agent, advs = _actors(env, n_adv)
    o = _run(env, agent, advs, idx=_groups(N, n_adv) if n_adv > 1 else None)
    o0 = ref.out.obs.clone()
    assert torch.equal(o['obs'][0], o0)
    ctrl = []
    for t in range(K):
        ref.set_adversary_control(o['aact'][t])
        ctrl.append(ref._adv)
    ref._adv = None
    seq = ref.step_sequence(o['act'].contiguous(), adv_actions=torch.stack(ctrl).contiguous(), terminal_obs=True)
    torch.cuda.synchronize()
    assert torch.equal(o['obs'][1:], seq['obs'])
    assert torch.equal(o['rew'], seq['reward'])
    assert torch.equal(o['done'], seq['done']) and torch.equal(o['flags'], seq['flags'])
    d = o['done'].bool()
    assert torch.equal(o['term'][d], seq['terminal_obs'][d])
    assert torch.isfinite(o['aact']).all() and torch.isfinite(o['alogp']).all()
    # the adversary acted: its control is not all zero and the trajectory differs from one without it
    assert float(torch.stack(ctrl).abs().max()) > 0
    env.close(); ref.close()


@pytest.mark.parametrize('n_adv', [1, 3])
def test_actions_and_log_probs_against_pytorch_actors(n_adv):
    from tests import philox_model as pm
    from tests import test_gpu_rollout_noise as RN
    env = _env(G.ADV_DYNAMICS, n_adv)
    agent, advs = _actors(env, n_adv, seed=1)
    idx = _groups(N, n_adv) if n_adv > 1 else np.zeros(N, dtype=np.int32)
    sel = torch.as_tensor(idx, device=env.device, dtype=torch.long)
    nu, ad = env.spec.nu, env.spec.adversary_dim

    def check(o, start, det, det_adv):          # the protagonist's and each env's own adversary's rows against the float64 actors
        RN.check_actor('protagonist', agent.ac.actor, o['obs'][:K], o['act'], o['logp'], det, *RN.model_draws(o, start, pm.CH_POLICY, nu, seed=5))
        e6, r6 = RN.model_draws(o, start, pm.CH_ADVERSARY, ad, seed=5)
        for j, adv in enumerate(advs):
            rows = idx == j
            RN.check_actor(f'adversary {j}', adv, o['obs'][:K][:, sel == j], o['aact'][:, sel == j], o['alogp'][:, sel == j], det_adv,
                           e6[:, rows], r6[:, rows])
    # deterministic on both sides: the actors' means on the stored observations; stochastic: both actions are mean + sigma x the host
    # Philox model's draw (channel 5 / channel 6) at the env's counters, both log-probabilities the float64 Gaussian log-prob; and the
    # two mixed modes
    for det, det_adv in ((True, True), (False, False), (False, True), (True, False)):
        env.reset_tensors()
        start = env.get_counters() + (np.arange(N),)
        check(_run(env, agent, advs, idx=idx if n_adv > 1 else None, det=det, det_adv=det_adv), start, det, det_adv)
    env.close()


def test_outputs_do_not_depend_on_the_launch_geometry(monkeypatch):
    runs = []
    for epw, wpw in GEOMETRIES:
        monkeypatch.setenv('SCG_ROLLOUT_EPW', epw)
        monkeypatch.setenv('SCG_ROLLOUT_WPW', wpw)
        env = _env(G.ADV_DYNAMICS, 3)
        agent, advs = _actors(env, 3, seed=2)
        runs.append(_run(env, agent, advs, idx=_groups(N, 3)))
        env.close()
    for r in runs[1:]:
        for k in runs[0]:
            assert torch.equal(runs[0][k], r[k]), k


def test_default_two_waves_per_simd_launch_at_65536_envs(monkeypatch):
    """65 536 envs: the default launch (32 envs per wave, 8 waves per workgroup = two waves per SIMD) against a forced one."""
    runs = []
    for geo in (None, ('64', '4')):
        if geo:
            monkeypatch.setenv('SCG_ROLLOUT_EPW', geo[0])
            monkeypatch.setenv('SCG_ROLLOUT_WPW', geo[1])
        env = _env(G.ADV_DYNAMICS, 1, n=65536)
        agent, advs = _actors(env, 1, seed=3)
        runs.append(_run(env, agent, advs, k=4))
        env.close()
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_rap_env_results_do_not_depend_on_its_wave_mates():
    """Env e under the mixed index vector equals env e in a run where every env faces adversary idx[e]."""
    idx = _groups(N, 3)
    env = _env(G.ADV_DYNAMICS, 3)
    agent, advs = _actors(env, 3, seed=4)
    mixed = _run(env, agent, advs, idx=idx)
    env.close()
    for k in range(3):
        env = _env(G.ADV_DYNAMICS, 3)
        agent, advs = _actors(env, 3, seed=4)
        pure = _run(env, agent, advs, idx=np.full(N, k, dtype=np.int32))
        env.close()
        rows = torch.as_tensor(idx == k, device=mixed['rew'].device)
        for name in ('act', 'logp', 'rew', 'done', 'flags', 'term', 'aact', 'alogp'):
            assert torch.equal(mixed[name][:, rows], pure[name][:, rows]), (k, name)
        assert torch.equal(mixed['obs'][:, rows], pure['obs'][:, rows]) and torch.equal(mixed['acc'][rows], pure['acc'][rows])


def test_adversary_noise_is_a_separate_stream_from_the_protagonists():
    """Scale = offset = 0: the adversary cannot act, so the protagonist's rows equal scg_rollout_policy's on an identically seeded handle
    (step 0 bit for bit); the adversary's noise is the host Philox model's channel 6, the protagonist's its channel 5."""
    env, ref = _env(G.ADV_ZERO, 1), _env(G.ADV_ZERO, 1)
    agent, advs = _actors(env, 1, seed=5)
    with torch.no_grad():
        advs[0].logstd.copy_(agent.ac.actor.logstd[:env.spec.adversary_dim])
    start = env.get_counters() + (np.arange(N),)
    o = _run(env, agent, advs)
    nobs, nu = env.spec.obs_dim, env.spec.nu
    f = dict(device=env.device, dtype=torch.float32)
    obs, act, logp, rew = torch.zeros(K + 1, N, nobs, **f), torch.zeros(K, N, nu, **f), torch.zeros(K, N, **f), torch.zeros(K, N, **f)
    done, flags = torch.zeros(K, N, dtype=torch.uint8, device=env.device), torch.zeros(K, N, dtype=torch.uint8, device=env.device)
    ref.rollout_policy(_policy(agent), K, obs, act, logp, rew, done, flags)
    torch.cuda.synchronize()
    assert torch.equal(o['act'][0], act[0]) and torch.equal(o['logp'][0], logp[0]) and torch.equal(o['obs'][0], obs[0])
    torch.testing.assert_close(o['act'], act, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(o['rew'], rew, rtol=2e-4, atol=2e-5)
    # the protagonist's noise is the host model's channel 5, the adversary's its channel 6, at the same counters
    from tests import philox_model as pm
    from tests import test_gpu_rollout_noise as RN
    RN.check_actor('protagonist', agent.ac.actor, o['obs'][:K], o['act'], o['logp'], False, *RN.model_draws(o, start, pm.CH_POLICY, nu, seed=5))
    RN.check_actor('adversary', advs[0], o['obs'][:K], o['aact'], o['alogp'], False,
                   *RN.model_draws(o, start, pm.CH_ADVERSARY, env.spec.adversary_dim, seed=5))
    env.close(); ref.close()


def test_unserved_population_size_is_an_error_not_an_abort():
    from safe_control_gym_amd import _adversarial
    from safe_control_gym_amd import _lib as L
    env = _env(G.ADV_DYNAMICS, 1)
    agent, advs = _actors(env, 2)
    with pytest.raises(L.ScgError, match='compiled for 1 adversaries'):
        env.rollout_adversarial(_policy(agent), [_adversarial.actor_ptrs(a) for a in advs], 4, *[torch.zeros(1, device=env.device)] * 8,
                                adv_index=torch.zeros(N, dtype=torch.int32, device=env.device))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- collectors
def _ppo_cfg(**extra):
    from safe_control_gym_amd.ppo import PPOConfig
    return PPOConfig(hidden_dim=H, activation=ACT, use_gae=True, opt_epochs=1, mini_batch_size=1024, rollout_steps=8, extra=extra)


def _check_returns(r, ret, adv, crit_v, crit_vt, rew, T=8, n=256):
    """ppo_utils.py:374-402 with a critic given by its values on obs[0..T] and on the terminal observations."""
    mask = 1.0 - r.done.float()
    trunc = ((r.flags & 1).bool() & r.done.bool())
    rews = rew + 0.99 * torch.where(trunc, crit_vt, torch.zeros_like(rew))
    vals = crit_v
    run_ret, run_adv = vals[T], torch.zeros(n, device=r.device)
    for i in reversed(range(T)):
        run_ret = rews[i] + 0.99 * mask[i] * run_ret
        run_adv = run_adv * 0.95 * 0.99 * mask[i] + rews[i] + 0.99 * mask[i] * vals[i + 1] - vals[i]
        torch.testing.assert_close(ret[i], run_ret, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(adv[i], run_adv, rtol=1e-5, atol=1e-5)


def test_rarl_fused_collector():
    from safe_control_gym_amd.rarl import RARL
    env = _env(G.ADV_DYNAMICS, 1, n=256)
    r = RARL(env, _ppo_cfg(), seed=3)
    assert r._fused_two_sided and not r._fused_rollout
    n_done = 0
    for _ in range(2):
        (ret, adv, mom), (ret_a, adv_a, mom_a) = r.collect()
        n_done += int(r.done.sum())
    assert r._two_graph[0] is not None                      # first collection eager, the second captured and replayed
    with torch.no_grad():
        c, ca = r.agent.ac.critic, r.adversary.ac.critic
        v = c(r.obs).squeeze(-1)
        va = ca(r.obs).squeeze(-1)
        torch.testing.assert_close(r.v, v[:8], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(r.v_adv, va[:8], rtol=1e-5, atol=1e-5)
        _check_returns(r, ret, adv, v, c(r.term_obs).squeeze(-1), r.rew)
        _check_returns(r, ret_a, adv_a, va, ca(r.term_obs).squeeze(-1), -r.rew)
        mean, logstd = r.adversary.ac.actor(r.obs[5])
        lp = (-0.5 * ((r.act_adv[5] - mean) / logstd.exp()) ** 2 - logstd - 0.9189385332046727).sum(-1)
        torch.testing.assert_close(r.logp_adv[5], lp, rtol=1e-4, atol=1e-4)
    assert float(mom[2]) == float(mom_a[2]) == 8 * 256
    assert r.total_steps == 2 * 8 * 256
    assert int(r.ep_count) == n_done                        # finished episodes counted once, not once per side
    wa = {k: v.clone() for k, v in r.agent.ac.state_dict().items()}
    wd = {k: v.clone() for k, v in r.adversary.ac.state_dict().items()}
    res = r.train_step()
    assert res['step'] == r.total_steps == 4 * 8 * 256
    assert any(not torch.equal(v, wa[k]) for k, v in r.agent.ac.state_dict().items())
    assert any(not torch.equal(v, wd[k]) for k, v in r.adversary.ac.state_dict().items())
    env.close()


def test_rarl_graph_replay_equals_per_launch_enqueue():
    from safe_control_gym_amd.rarl import RARL
    outs = []
    for graphs in (True, False):
        env = _env(G.ADV_DYNAMICS, 1, n=256)
        r = RARL(env, _ppo_cfg(), seed=3)
        r._graph_rollout = graphs
        seq = []
        for _ in range(4):
            (ret, adv, mom), (ret_a, adv_a, mom_a) = r.collect()
            seq.append([t.clone() for t in (ret, adv, mom, ret_a, adv_a, mom_a, r.obs, r.act, r.act_adv, r.logp_adv, r.v, r.v_adv, r._ep_tot)])
            r.obs[0].copy_(r.obs[8])
        assert (r._two_graph is not None and r._two_graph[0] is not None) == graphs
        outs.append(seq)
        env.close()
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_rap_fused_collector_selects_each_envs_adversary():
    from safe_control_gym_amd.rarl import RAP
    env = _env(G.ADV_DYNAMICS, 3, n=256)
    r = RAP(env, _ppo_cfg(), seed=4, num_adversaries=3)
    assert r._fused_two_sided
    r._rng = type('R', (), {'randint': staticmethod(lambda k, size: np.where(np.arange(size) < 100, 0, 2))})()   # adversaries 0 and 2
    (ret, adv, mom), (ret_a, adv_a, mom_a) = r.collect()
    sel = r.adv_index
    with torch.no_grad():
        va = torch.stack([a.ac.critic(r.obs).squeeze(-1) for a in r.adversaries])          # [3, T + 1, N]
        va = va.gather(0, sel.view(1, 1, -1).expand(1, 9, 256))[0]
        vt = torch.stack([a.ac.critic(r.term_obs).squeeze(-1) for a in r.adversaries]).gather(0, sel.view(1, 1, -1).expand(1, 8, 256))[0]
        torch.testing.assert_close(r.v_adv, va[:8], rtol=1e-5, atol=1e-5)
        _check_returns(r, ret_a, adv_a, va, vt, -r.rew)
    w = [{k: v.clone() for k, v in a.ac.state_dict().items()} for a in r.adversaries]
    res = r.train_step()                                    # (a fresh collection: the graph is captured on the second)
    r.train_step()
    assert res['adv_indices'] == [0, 2] and r.total_steps == 3 * 8 * 256
    changed = [any(not torch.equal(v, w[k][n]) for n, v in a.ac.state_dict().items()) for k, a in enumerate(r.adversaries)]
    assert changed == [True, False, True]
    env.close()


# ---------------------------------------------------------------------------------------------------------------- controllers
@pytest.mark.parametrize('algo,n_adv', [('rarl', 1), ('rap', 2)])
def test_controller_fused_rollout_key(algo, n_adv, tmp_path):
    from safe_control_gym_amd.registration import make
    env_id, cfg = _task(G.ADV_DYNAMICS)
    env_func = functools.partial(make, env_id, **cfg)
    common = dict(output_dir=str(tmp_path), checkpoint_path=os.path.join(str(tmp_path), 'model_latest.pt'), seed=2, use_gae=True,
                  rollout_batch_size=256, rollout_steps=8, opt_epochs=1, mini_batch_size=512, max_env_steps=3 * 256 * 8,
                  agent_iterations=1, adversary_iterations=1)
    if algo == 'rap':
        common.pop('agent_iterations'); common.pop('adversary_iterations')
    fused = make(algo, env_func, fused_rollout=True, **common)
    assert fused.impl._fused_two_sided and fused.env.adversary_shape == (64, 'tanh', n_adv)
    fused.learn()
    assert fused.total_steps >= 3 * 256 * 8
    assert fused.run(n_episodes=4)['ep_returns'].shape == (4,)
    fused.close()
    plain = make(algo, env_func, **common)
    assert not plain.impl._fused_two_sided and plain.env.adversary_shape is None
    plain.close()


def test_over_budget_shape_warns_and_keeps_the_pytorch_collector():
    from safe_control_gym_amd.ppo import PPOConfig
    from safe_control_gym_amd.rarl import RAP
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = _task(G.ADV_DYNAMICS, 'quadrotor_3D_track')
    env = HipVecEnv(env_id, 128, seed=5, return_numpy=False, policy=(128, 'relu'), adversaries=3, **cfg)
    assert env.adversary_shape is None and env.adversaries_requested == 3
    pcfg = PPOConfig(hidden_dim=128, activation='relu', use_gae=True, opt_epochs=1, mini_batch_size=512, rollout_steps=4)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        r = RAP(env, pcfg, seed=1, num_adversaries=3)
    assert not r._fused_two_sided and any('PyTorch collector' in str(x.message) for x in w)
    (ret, adv, mom), _ = r.collect()
    assert float(mom[2]) == 4 * 128 and torch.isfinite(ret).all()
    env.close()
