"""scg_rollout_policy — K control steps per launch with the actor in the loop — against the step-by-step path
(PyTorch actor + scg_step), and the PPO collector / evaluation built on it."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


STAB6 = dict(task='stabilization', obs_goal_horizon=0, episode_len_sec=1.0)         # Quadrotor2D with the reference's default 6-float rows


def _setup(task, n, hidden, act, seed=5, override=None):
    from safe_control_gym_amd.ppo import PPO, PPOConfig
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = load_task(task)
    if override:
        cfg = {k: v for k, v in dict(cfg, **override).items() if k != 'task_info'}
    env = HipVecEnv(env_id, n, seed=seed, return_numpy=False, policy=(hidden, act), **cfg)
    ref = HipVecEnv(env_id, n, seed=seed, return_numpy=False, **cfg)
    assert env.policy_shape == (hidden, act)
    pcfg = PPOConfig(hidden_dim=hidden, activation=act, use_gae=True, rollout_batch_size=n, rollout_steps=8, mini_batch_size=n * 8 // 2,
                     opt_epochs=1)
    torch.manual_seed(0)
    ppo = PPO(env, pcfg, seed=0)
    assert ppo._fused_rollout and ppo.agent.use_fused
    return env, ref, ppo


def _twin(task, n, hidden, act, override, seed=5):
    """A second handle on the policy library `_setup` gives `env`, without a PPO (its constructor's reset is the caller's)."""
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = load_task(task)
    if override:
        cfg = {k: v for k, v in dict(cfg, **override).items() if k != 'task_info'}
    return HipVecEnv(env_id, n, seed=seed, return_numpy=False, policy=(hidden, act), **cfg)


@pytest.mark.parametrize('task,hidden,act,override', [('quadrotor_2D_track', 128, 'tanh', None), ('cartpole_stab', 64, 'leaky_relu', None),
                                                      ('quadrotor_3D_track', 128, 'relu', None),
                                                      ('quadrotor_2D_track', 96, 'tanh', None),       # three feature tiles per hidden layer
                                                      ('quadrotor_2D_track', 64, 'tanh', STAB6)])     # rows of 24 bytes: no LDS transpose
# launch geometry: envs per wave (lane = env / lane pair = env) x waves per workgroup behind one weight image (8 = two waves per SIMD: what shards
# above 32 768 envs get by default — forced here on a small batch)
@pytest.mark.parametrize('epw,wpw', [('64', '4'), ('32', '4'), ('32', '8'), ('64', '8')])
def test_fused_rollout_equals_step_by_step(task, hidden, act, override, epw, wpw, monkeypatch):
    monkeypatch.setenv('SCG_ROLLOUT_EPW', epw)
    monkeypatch.setenv('SCG_ROLLOUT_WPW', wpw)
    n, K = 320, 12                                 # 5 / 10 waves: a partial workgroup as well
    env, ref, ppo = _setup(task, n, hidden, act, override=override)
    assert env.spec.obs_dim == (6 if override else env.spec.obs_dim)
    nobs, nu = env.spec.obs_dim, env.spec.nu
    f = dict(device=env.device, dtype=torch.float32)
    obs, actb, logp, rew = torch.zeros(K + 1, n, nobs, **f), torch.zeros(K, n, nu, **f), torch.zeros(K, n, **f), torch.zeros(K, n, **f)
    done, flags = torch.zeros(K, n, dtype=torch.uint8, device=env.device), torch.zeros(K, n, dtype=torch.uint8, device=env.device)
    term, acc = torch.zeros(K, n, nobs, **f), torch.zeros(n, 8, **f)
    # (a) deterministic policy: the actor's mean actions (float64 actor, forward-pass bound), and the env step: the stored actions
    # replayed through scg_step_sequence on an identically seeded handle of the same library reproduce every output bit for bit
    from tests import philox_model as pm
    from tests import test_gpu_rollout_noise as RN
    ref.reset_tensors()                             # (PPO's constructor already reset `env` once: keep the episode indices equal)
    env.reset_tensors(); o = ref.reset_tensors().clone()
    twin = _twin(task, n, hidden, act, override)
    twin.reset_tensors(); twin.reset_tensors()
    env.rollout_policy(ppo._policy_struct(True), K, obs, actb, logp, rew, done, flags, terminal_obs=term, episode_acc=acc)
    torch.cuda.synchronize()
    ac = ppo.agent.ac
    if task == 'quadrotor_3D_track':                 # (obs[0] comes from the stored quaternion, the reset's from the drawn Euler angles)
        torch.testing.assert_close(obs[0], o, rtol=RN.OBS0_TOL, atol=RN.OBS0_TOL)
        assert torch.equal(o, twin.out.obs)
    else:
        assert torch.equal(obs[0], o) and torch.equal(obs[0], twin.out.obs)
    seq = twin.step_sequence(actb.contiguous(), terminal_obs=True, fin_stats=True)
    torch.cuda.synchronize()
    assert torch.equal(obs[1:], seq['obs']) and torch.equal(rew, seq['reward'])
    assert torch.equal(done, seq['done']) and torch.equal(flags, seq['flags'])
    d = done.bool()
    assert torch.equal(term[d], seq['terminal_obs'][d])
    RN.check_accumulators(acc, seq)
    assert torch.equal(env.ep_stats, twin.ep_stats)
    for t in range(K):                              # the step-by-step path on the plain library: same flags, same trajectory
        out = ref.step_tensors(actb[t])
        assert torch.equal(done[t], out.done) and torch.equal(flags[t], out.flags)
        torch.testing.assert_close(obs[t + 1], out.obs, rtol=2e-4, atol=2e-4)
    RN.check_actor('scg_rollout_policy', ac.actor, obs[:K], actb, logp, True)
    # (b) stochastic: every draw is the host Philox model's at the env's counters, the action and its log-prob the float64 actor's
    for reseed in (False, True):
        if reseed:
            a1 = actb.clone()
            env.seed(5)                                              # same key, fresh episodes -> other draws (episode index)
        env.reset_tensors()
        step0, ep0 = env.get_counters()
        env.rollout_policy(ppo._policy_struct(False), K, obs, actb, logp, rew, done, flags, terminal_obs=term, episode_acc=acc)
        torch.cuda.synchronize()
        e64, r = RN.model_draws({'done': done}, (step0, ep0, np.arange(n)), pm.CH_POLICY, nu, seed=5)
        RN.check_actor('scg_rollout_policy', ac.actor, obs[:K], actb, logp, False, e64, r)
    assert not torch.equal(a1, actb)
    twin.close()
    env.close(); ref.close()



def test_rollout_does_not_depend_on_the_launch_geometry(monkeypatch):
    """Stochastic rollouts with 64 and with 32 envs per wave, 4 and 8 waves per workgroup are the same rollouts: the noise is a per-env
    Philox stream, the actor's arithmetic per env is the same MFMA sequence."""
    outs = []
    for epw, wpw in (('64', '4'), ('32', '4'), ('32', '8'), ('64', '8')):
        monkeypatch.setenv('SCG_ROLLOUT_EPW', epw)
        monkeypatch.setenv('SCG_ROLLOUT_WPW', wpw)
        env, ref, ppo = _setup('quadrotor_2D_track', 1000, 128, 'tanh')
        n, K, nobs, nu = 1000, 40, 12, 2
        f = dict(device=env.device, dtype=torch.float32)
        obs, actb, logp, rew = torch.zeros(K + 1, n, nobs, **f), torch.zeros(K, n, nu, **f), torch.zeros(K, n, **f), torch.zeros(K, n, **f)
        done, flags = torch.zeros(K, n, dtype=torch.uint8, device=env.device), torch.zeros(K, n, dtype=torch.uint8, device=env.device)
        env.seed(5); env.reset_tensors()
        env.rollout_policy(ppo._policy_struct(False), K, obs, actb, logp, rew, done, flags)
        torch.cuda.synchronize()
        outs.append((obs.clone(), actb.clone(), logp.clone(), rew.clone(), done.clone(), env.get_raw_state() if hasattr(env, 'get_raw_state') else None))
        env.close(); ref.close()
    for other in outs[1:]:
        for a, b in zip(outs[0][:5], other[:5]):
            assert torch.equal(a, b)
    assert int(outs[0][4].sum()) > 0                # episodes ended and were reset inside the launch


def test_ppo_iteration_and_evaluation_on_the_fused_rollout():
    from safe_control_gym_amd.ppo import evaluate
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.vec_env import HipVecEnv
    env, ref, ppo = _setup('quadrotor_2D_track', 1024, 128, 'tanh')
    res = ppo.train_step()
    assert np.isfinite([res['policy_loss'], res['value_loss'], res['approx_kl']]).all() and res['minibatches'] == 2
    st = ppo.episode_stats()
    assert st['episodes'] > 0 and 0 < st['ep_length'] <= 250
    # evaluation: the fused one-launch path == the graphed PyTorch-policy path
    env_id, cfg = load_task('quadrotor_2D_track')
    ev_cfg = dict(cfg, randomized_init=False)
    e1 = HipVecEnv(env_id, 128, seed=9, return_numpy=False, policy=(128, 'tanh'), **ev_cfg)
    e2 = HipVecEnv(env_id, 128, seed=9, return_numpy=False, **ev_cfg)
    a = evaluate(ppo.agent.ac, e1, policy=ppo._policy_struct(True))
    b = evaluate(ppo.agent.ac, e2)
    assert a['episodes'] == b['episodes'] == 128
    for k in ('ep_return', 'ep_length', 'ep_constraint_violation', 'ep_mse'):
        assert abs(a[k] - b[k]) <= 1e-3 * max(1.0, abs(b[k])), (k, a[k], b[k])
    # the evaluation as a sequence of short launches (what AsyncEvaluator enqueues beside the training stream) == the one launch, bit for bit
    from safe_control_gym_amd.ppo import _evaluate_fused_device
    r1, a1 = _evaluate_fused_device(e1, ppo._policy_struct(True), 1)
    r1, a1 = r1.clone(), a1.clone()
    for chunk in (25, 64, 250, 1000):
        r2, a2 = _evaluate_fused_device(e1, ppo._policy_struct(True), 1, chunk=chunk)
        assert torch.equal(r1, r2) and torch.equal(a1, a2), chunk
    for e in (env, ref, e1, e2):
        e.close()
