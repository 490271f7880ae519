"""The action noise of the fused on-policy rollouts — scg_rollout_policy (the PPO collector), scg_rollout_adversarial (RARL / RAP) and
scg_rollout_cbf — pinned draw by draw to the host Philox model (tests/philox_model.py: env stream, channel 5 for the policy, 6 for the
adversary, counter (global env id, episode, step in episode) followed through the launch's auto-resets), their actions and
log-probabilities to a float64 copy of the actor, and scg_rollout_policy's housekeeping to a bit-exact replay.

  (a) read-out   W3 = b3 = 0 and logstd = 0: the stored action IS the kernel's draw (fma(1, eps, 0)).  Every element within
                 eps_tol = D_EPS (1 + |eps64|) + D_LOG / r of env_normal4 at the followed counters, no row left out; logp within
                 rtol 1e-5 / atol 2e-5 of sum(-eps64^2 / 2 - ln(2 pi) / 2).
  (b) real actors, random weights, logstd over [-1, 0.2], the float64 actor on the kernel's stored obs[t]:
                 |act - (mean64 + e^ls eps64)| <= TAU S + sigma eps_tol + SIG sigma |eps64|,   TAU = 1e-5, S = |b3| + sum |W3| |h2|
                 (the forward-pass bound of tests/test_gpu_offpolicy_collector.py), SIG the relative error of the kernel's
                 __expf(logstd); deterministic: |act - mean64| <= TAU S and logp the constant; logp as in (a).
  (c) scg_rollout_policy's env step replayed through scg_step_sequence bit for bit, its episode accumulators, max_episodes.
  (d) a stochastic rollout as two launches (5 + 7 steps) == one launch of 12, bit for bit, state and counters included.

Sizes: 320 envs (5 / 10 waves, a partial workgroup), 67 and 33 (surplus lanes shadow the last env); 12 steps, and per kernel one
launch of max_episode_steps + 10 in which every env auto-resets.  Every handle: a seed with a non-zero high word, env_id_offset
100 000 (global id != lane), and counters preset per env to steps 0 / mid-episode / 1-3 before the time limit (resets land inside 12
steps) x episodes 0, 1, 65 536, 2^32 - 2.

Measured on an MI355X (each test prints its own [ratio] line), worst |eps_kernel - eps64| / eps_tol of the read-out:
    scg_rollout_policy        0.283   (20 788 distinct draws)
    scg_rollout_adversarial   0.275 (protagonist, channel 5)   0.303 (adversary, channel 6)   (26 448 draws each)
    scg_rollout_cbf           0.283   (9 099 draws)
(the float32 NumPy restatement of the same text on the CPU: 0.48 over 2^23 draws, tests/test_onpolicy_noise_model_cpu.py; no constant
was widened), the worst error / bound of (b): 0.14 sampled, 0.022 deterministic, and
    SIG: worst |sigma_kernel / e^ls - 1| over 44 columns of ls in [-1, 0.2] = 1.07e-7 (including the 2^-24 of the product's
    rounding); SIG = 2.2e-7 = 2 x that.

Quadrotor 3D: obs[0] of a launch is recomputed from the stored quaternion, the reset's own observation from the drawn Euler angles, so
the two agree to float32 rounding of that round trip (OBS0_TOL), not bit for bit; every later row is bit-exact against the replay."""
import copy

import numpy as np
import pytest

from tests import philox_model as pm

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import __graft_entry__ as G                                         # noqa: E402  (the adversary settings of the prebuilt variants)

SEED = (0x5DEECE66 << 32) | 0x1234ABCD                              # the key's high word is non-zero
OFFSET = 100000
GEOMETRIES = [('64', '4'), ('32', '4'), ('32', '8'), ('64', '8')]
TAU = 1e-5
SIG = 2.2e-7
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
K = 12
OBS0_TOL = 2e-6                                                     # rpy -> quaternion -> rpy and R^T w in float32: a few ulp of O(1) values
POLICY_BUILDS = {'quadrotor_2D_track': (128, 'tanh'), 'cartpole_stab': (64, 'leaky_relu'), 'quadrotor_3D_track': (128, 'relu')}


# ---------------------------------------------------------------------------------------------------------------- handles
def policy_env(task, n):
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = load_task(task)
    env = HipVecEnv(env_id, n, seed=SEED, return_numpy=False, policy=POLICY_BUILDS[task], env_id_offset=OFFSET, **cfg)
    assert env.policy_shape == POLICY_BUILDS[task]
    env.reset_tensors()
    return env


def adv_env(n_adv, n):
    from tests import test_gpu_rollout_adversarial as A
    env = A._env(G.ADV_DYNAMICS, n_adv, n=n, seed=SEED, env_id_offset=OFFSET)
    assert env.adversary_shape == (A.H, A.ACT, n_adv)
    return env


def cbf_env(n):
    from safe_control_gym_amd.vec_env import HipVecEnv
    from tests import test_gpu_cbf as C
    env = HipVecEnv(C.S['task'], n, seed=SEED, return_numpy=False, policy=(C.HIDDEN, C.ACT), cbf=True, env_id_offset=OFFSET, **C._cfg())
    assert env.cbf_shape == (C.HIDDEN, C.ACT)
    env.reset_tensors()
    return env


def preset(env):
    """Mixed per-env counters (every step kind x every episode value within 24 envs); returns (step, episode, global id)."""
    n, M = env.num_envs, env.spec.max_episode_steps
    i = np.arange(n)
    step = np.array([0, 17, M // 2, M - 1, M - 2, M - 3], dtype=np.int64)[i % 6]
    ep = np.array([0, 1, 65536, (1 << 32) - 2], dtype=np.int64)[(i // 2) % 4]
    env.set_counters(step.astype(np.int32), ep.astype(np.uint32))
    s, e = env.get_counters()
    assert np.array_equal(s, step) and np.array_equal(e.astype(np.int64), ep)
    return step, ep, OFFSET + i


class Net:
    """A ppo.MLPActor with seeded random weights, as the flat vector + offsets (scg_policy) and as per-tensor pointers; read-out:
    output layer zero (logstd = 0 is the caller's)."""

    def __init__(self, env, nout, hidden, act, seed, logstd, readout=False):
        from safe_control_gym_amd.ppo import MLPActor
        torch.manual_seed(seed)
        m = MLPActor(env.spec.obs_dim, nout, [hidden, hidden], act)
        with torch.no_grad():
            m.logstd.copy_(torch.as_tensor(np.asarray(logstd, dtype=np.float32)))
            if readout:
                m.pi_net.fcs[2].weight.zero_()
                m.pi_net.fcs[2].bias.zero_()
        self.m, self.hidden, self.act = m.to(env.device), hidden, act
        parts = [t.detach().reshape(-1) for fc in self.m.pi_net.fcs for t in (fc.weight, fc.bias)] + [self.m.logstd.detach()]
        self.offs = [int(v) for v in np.concatenate([[0], np.cumsum([p.numel() for p in parts])])]
        self.flat = torch.cat(parts).contiguous()
        self.ls = self.m.logstd.detach().double()                   # the float32 values, in float64

    def policy(self, det):
        from safe_control_gym_amd import _lib as L
        o = self.offs
        return L.Policy(d_params=self.flat.data_ptr(), W1=o[0], b1=o[1], W2=o[2], b2=o[3], W3=o[4], b3=o[5], logstd_off=o[6],
                        hidden=self.hidden, activation=L.POLICY_ACTS[self.act], deterministic=int(det))

    def ptrs(self):
        from safe_control_gym_amd import _adversarial
        return _adversarial.actor_ptrs(self.m)


@torch.no_grad()
def actor_ref(actor, obs):
    """float64 (mean, S = |b3| + sum |W3| |h2|) of a ppo.MLPActor on obs [..., nobs]."""
    m = copy.deepcopy(actor).double()
    f = m.pi_net.fcs
    h = m.pi_net.act(f[1](m.pi_net.act(f[0](obs.double()))))
    return f[2](h), f[2].bias.abs() + h.abs() @ f[2].weight.abs().T


def logstds(nout, k=0):
    return np.linspace(-1.0 + 0.1 * k, 0.2 - 0.1 * k, nout) if nout > 1 else np.array([-1.0 + 0.6 * k])


def bufs(env, k, **more):
    n, nobs, nu = env.num_envs, env.spec.obs_dim, env.spec.nu
    nan = lambda *s: torch.full(s, float('nan'), device=env.device)                         # noqa: E731
    u8 = lambda *s: torch.full(s, 255, dtype=torch.uint8, device=env.device)                # noqa: E731
    o = {'obs': nan(k + 1, n, nobs), 'act': nan(k, n, nu), 'logp': nan(k, n), 'rew': nan(k, n), 'done': u8(k, n), 'flags': u8(k, n),
         'term': torch.zeros(k, n, nobs, device=env.device), 'acc': torch.zeros(n, 8, device=env.device)}
    for name, width in more.items():
        o[name] = nan(k, n, width) if width else nan(k, n)
    return o


def run_policy(env, net, k, det, acc=None, max_episodes=0):
    o = bufs(env, k)
    if acc is not None:
        o['acc'] = acc
    env.rollout_policy(net.policy(det), k, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'], terminal_obs=o['term'],
                       episode_acc=o['acc'], max_episodes=max_episodes)
    torch.cuda.synchronize()
    return o


def run_adv(env, net, advs, k, det, det_adv, idx=None, acc=None):
    o = bufs(env, k, aact=env.spec.adversary_dim, alogp=0)
    if acc is not None:
        o['acc'] = acc
    ix = torch.as_tensor(np.asarray(idx, dtype=np.int32), device=env.device) if idx is not None else None
    env.rollout_adversarial(net.policy(det), [a.ptrs() for a in advs], k, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'],
                            o['aact'], o['alogp'], adv_index=ix, deterministic_adversary=det_adv, terminal_obs=o['term'],
                            episode_acc=o['acc'])
    torch.cuda.synchronize()
    return o


_cbf_filter = []


def run_cbf(env, net, k, det):
    from tests import test_gpu_cbf as C
    if not _cbf_filter:
        _cbf_filter.append(C._filter())
    o = bufs(env, k, rows=4, applied=0)
    env.rollout_cbf(net.ptrs(), _cbf_filter[0].params(), k, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'], o['rows'],
                    o['applied'], deterministic=det, terminal_obs=o['term'], episode_acc=o['acc'])
    torch.cuda.synchronize()
    return o


# ---------------------------------------------------------------------------------------------------------------- checks
def model_draws(o, start, channel, ncol, seed=SEED):
    """(eps64, r) [K, n, ncol] of the host model at the counters the launch went through; start = (step, episode, global id) at entry."""
    step0, ep0, gid = start
    done = o['done'].cpu().numpy()
    assert done.max() <= 1
    ep, st = pm.follow(step0, ep0, done)
    e64, r = pm.env_normal4(seed, np.asarray(gid)[None, :], ep, st, channel)
    return e64[..., :ncol], r[..., :ncol]


def check_readout(kernel, act, logp, e64, r):
    got = act.double().cpu().numpy()
    assert np.isfinite(got).all()
    ratio = float((np.abs(got - e64) / pm.eps_tol(e64, r)).max())
    print(f'[ratio] {kernel}: read-out of {got.size} draws, worst |eps - eps64| / eps_tol = {ratio:.3f}')
    assert ratio <= 1.0, f'{kernel}: error / bound = {ratio:.3g}'
    np.testing.assert_allclose(logp.double().cpu().numpy(), (-0.5 * e64 * e64 - HALF_LOG_2PI).sum(-1), rtol=1e-5, atol=2e-5)


def check_actor(kernel, net, obs, act, logp, det, e64=None, r=None):
    """(b): the stored actions and log-probabilities against the float64 copy of the actor (a Net or a ppo.MLPActor) on the stored
    observations."""
    actor = getattr(net, 'm', net)
    mean, S = actor_ref(actor, obs)
    mean, S, ls = mean.cpu().numpy(), S.cpu().numpy(), actor.logstd.detach().double().cpu().numpy()
    got = act.double().cpu().numpy()
    assert np.isfinite(got).all()
    if det:
        ratio = float((np.abs(got - mean) / (TAU * S)).max())
        want_lp = np.full(logp.shape, -(ls + HALF_LOG_2PI).sum())
    else:
        sigma = np.exp(ls)
        bound = TAU * S + sigma * pm.eps_tol(e64, r) + SIG * sigma * np.abs(e64)
        ratio = float((np.abs(got - (mean + sigma * e64)) / bound).max())
        want_lp = (-0.5 * e64 * e64 - ls - HALF_LOG_2PI).sum(-1)
    print(f'[ratio] {kernel} {"deterministic" if det else "sampled"}: {got.size} actions against the float64 actor, worst error / bound = '
          f'{ratio:.3f}')
    assert ratio <= 1.0, f'{kernel}: error / bound = {ratio:.3g}'
    np.testing.assert_allclose(logp.double().cpu().numpy(), want_lp, rtol=1e-6 if det else 1e-5, atol=1e-5 if det else 2e-5)


def assert_resets(o, every_env=False):
    d = o['done'].bool()
    assert bool(d.any()), 'auto-resets happened inside the launch'
    if every_env:
        assert bool(d.any(0).all()), 'every env auto-reset inside the launch'


# ---------------------------------------------------------------------------------------------------------------- (a) read-out
POLICY_READOUT = [('quadrotor_2D_track', 320, 0, g) for g in GEOMETRIES] + \
                 [('cartpole_stab', 67, 0, ('32', '4')), ('quadrotor_3D_track', 33, 0, ('64', '4')), ('cartpole_stab', 67, 10, ('64', '8'))]


@pytest.mark.parametrize('task,n,over,geometry', POLICY_READOUT, ids=lambda v: '-'.join(v) if isinstance(v, tuple) else str(v))
def test_rollout_policy_draws(task, n, over, geometry, monkeypatch):
    monkeypatch.setenv('SCG_ROLLOUT_EPW', geometry[0])
    monkeypatch.setenv('SCG_ROLLOUT_WPW', geometry[1])
    env = policy_env(task, n)
    k = env.spec.max_episode_steps + over if over else K
    nu = env.spec.nu
    net = Net(env, nu, *POLICY_BUILDS[task], seed=1, logstd=np.zeros(nu), readout=True)
    start = preset(env)
    o = run_policy(env, net, k, det=False)
    assert_resets(o, every_env=bool(over))
    check_readout('scg_rollout_policy', o['act'], o['logp'], *model_draws(o, start, pm.CH_POLICY, nu))
    o = run_policy(env, net, K, det=True)                           # deterministic: no draw reaches the action
    assert bool((o['act'] == 0).all())
    torch.testing.assert_close(o['logp'], torch.full_like(o['logp'], -nu * HALF_LOG_2PI), rtol=1e-6, atol=1e-5)
    env.close()


@pytest.mark.parametrize('n_adv,n,over,geometry', [(1, 67, 0, ('64', '8')), (3, 320, 0, ('32', '8')), (1, 33, 10, ('64', '4'))],
                         ids=['rarl-67', 'rap3-320', 'rarl-33-full-episode'])
def test_rollout_adversarial_draws(n_adv, n, over, geometry, monkeypatch):
    """Protagonist columns on channel 5 and adversary columns on channel 6 in the same launch; with a population, under the mixed
    index vector and under a rotated one (the noise does not depend on the adversary an env faces)."""
    from tests import test_gpu_rollout_adversarial as A
    monkeypatch.setenv('SCG_ROLLOUT_EPW', geometry[0])
    monkeypatch.setenv('SCG_ROLLOUT_WPW', geometry[1])
    env = adv_env(n_adv, n)
    k = env.spec.max_episode_steps + over if over else K
    nu, ad = env.spec.nu, env.spec.adversary_dim
    net = Net(env, nu, A.H, A.ACT, seed=2, logstd=np.zeros(nu), readout=True)
    advs = [Net(env, ad, A.H, A.ACT, seed=3 + j, logstd=np.zeros(ad), readout=True) for j in range(n_adv)]
    idx = A._groups(n, n_adv) if n_adv > 1 else None
    start = preset(env)
    o = run_adv(env, net, advs, k, False, False, idx=idx)
    assert_resets(o, every_env=bool(over))
    check_readout('scg_rollout_adversarial protagonist', o['act'], o['logp'], *model_draws(o, start, pm.CH_POLICY, nu))
    check_readout('scg_rollout_adversarial adversary', o['aact'], o['alogp'], *model_draws(o, start, pm.CH_ADVERSARY, ad))
    if n_adv > 1:
        twin = adv_env(n_adv, n)
        preset(twin)
        o2 = run_adv(twin, net, advs, k, False, False, idx=(idx + 1) % n_adv)
        for name in ('act', 'logp', 'aact', 'alogp'):
            assert torch.equal(o[name], o2[name]), name
        twin.close()
    env.close()


@pytest.mark.parametrize('n,over,geometry', [(320, 0, ('32', '4')), (67, 0, ('64', '4')), (33, 10, ('32', '8'))],
                         ids=['320', '67', '33-full-episode'])
def test_rollout_cbf_draws(n, over, geometry, monkeypatch):
    """Every step's policy action (the filter changes what is applied, not what the policy drew), not only step 0."""
    from tests import test_gpu_cbf as C
    monkeypatch.setenv('SCG_ROLLOUT_EPW', geometry[0])
    monkeypatch.setenv('SCG_ROLLOUT_WPW', geometry[1])
    env = cbf_env(n)
    k = env.spec.max_episode_steps + over if over else K
    net = Net(env, 1, C.HIDDEN, C.ACT, seed=4, logstd=np.zeros(1), readout=True)
    start = preset(env)
    o = run_cbf(env, net, k, det=False)
    assert_resets(o, every_env=bool(over))
    check_readout('scg_rollout_cbf', o['act'], o['logp'], *model_draws(o, start, pm.CH_POLICY, 1))
    env.close()


def test_sigma_of_the_rollouts():
    """SIG: the kernel's sigma = __expf(logstd) against exp in float64, read out of two launches on twin handles — logstd = 0 stores
    eps, logstd = ls stores fl(sigma eps) — at step 0, over the logstd values (b) uses and random ones in [-1, 0.2]."""
    task, n = 'quadrotor_3D_track', 33
    gen = np.random.default_rng(5)
    sets = [logstds(4), logstds(2), logstds(2, 1), logstds(2, 2), logstds(1)] + [gen.uniform(-1.0, 0.2, 4) for _ in range(6)]
    env = policy_env(task, n)
    nu = env.spec.nu
    eps = run_policy(env, Net(env, nu, *POLICY_BUILDS[task], seed=1, logstd=np.zeros(nu), readout=True), 1, det=False)['act'][0].double()
    env.close()
    worst, count = 0.0, 0
    for ls in sets:
        ls = np.resize(ls, nu)
        twin = policy_env(task, n)
        net = Net(twin, nu, *POLICY_BUILDS[task], seed=1, logstd=ls, readout=True)
        act = run_policy(twin, net, 1, det=False)['act'][0].double()
        twin.close()
        rel = (act / (eps * torch.exp(net.ls)) - 1.0).abs()
        worst, count = max(worst, float(rel.max())), count + nu
    print(f'[ratio] sigma: worst |sigma_kernel / e^ls - 1| over {count} values of ls = {worst:.3e} (SIG = {SIG:g})')
    assert worst <= SIG


# ---------------------------------------------------------------------------------------------------------------- (b) real actors
@pytest.mark.parametrize('det', [False, True], ids=['sampled', 'deterministic'])
@pytest.mark.parametrize('task,n', [('quadrotor_2D_track', 320), ('cartpole_stab', 67), ('quadrotor_3D_track', 33)])
def test_rollout_policy_against_the_float64_actor(task, n, det):
    env = policy_env(task, n)
    nu = env.spec.nu
    net = Net(env, nu, *POLICY_BUILDS[task], seed=6, logstd=logstds(nu))
    start = preset(env)
    o = run_policy(env, net, K, det)
    assert_resets(o)
    check_actor('scg_rollout_policy', net, o['obs'][:K], o['act'], o['logp'], det, *model_draws(o, start, pm.CH_POLICY, nu))
    env.close()


@pytest.mark.parametrize('det,det_adv', [(False, False), (True, True), (False, True), (True, False)],
                         ids=['sampled', 'deterministic', 'adversary-deterministic', 'protagonist-deterministic'])
@pytest.mark.parametrize('n_adv,n', [(3, 320), (1, 67)])
def test_rollout_adversarial_against_the_float64_actors(n_adv, n, det, det_adv):
    from tests import test_gpu_rollout_adversarial as A
    env = adv_env(n_adv, n)
    nu, ad = env.spec.nu, env.spec.adversary_dim
    net = Net(env, nu, A.H, A.ACT, seed=7, logstd=logstds(nu))
    advs = [Net(env, ad, A.H, A.ACT, seed=8 + j, logstd=logstds(ad, j)) for j in range(n_adv)]
    idx = A._groups(n, n_adv) if n_adv > 1 else np.zeros(n, dtype=np.int32)
    start = preset(env)
    o = run_adv(env, net, advs, K, det, det_adv, idx=idx if n_adv > 1 else None)
    assert_resets(o)
    check_actor('scg_rollout_adversarial protagonist', net, o['obs'][:K], o['act'], o['logp'], det, *model_draws(o, start, pm.CH_POLICY, nu))
    e6, r6 = model_draws(o, start, pm.CH_ADVERSARY, ad)
    for j, adv in enumerate(advs):                                  # each env's own adversary
        rows = torch.as_tensor(idx == j, device=env.device)
        sel = idx == j
        check_actor(f'scg_rollout_adversarial adversary {j}', adv, o['obs'][:K][:, rows], o['aact'][:, rows], o['alogp'][:, rows], det_adv,
                    e6[:, sel], r6[:, sel])
    env.close()


@pytest.mark.parametrize('det', [False, True], ids=['sampled', 'deterministic'])
def test_rollout_cbf_against_the_float64_actor(det):
    from tests import test_gpu_cbf as C
    env = cbf_env(67)
    net = Net(env, 1, C.HIDDEN, C.ACT, seed=9, logstd=logstds(1))
    start = preset(env)
    o = run_cbf(env, net, K, det)
    assert_resets(o)
    check_actor('scg_rollout_cbf', net, o['obs'][:K], o['act'], o['logp'], det, *model_draws(o, start, pm.CH_POLICY, 1))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- (c) housekeeping
def replay(twin, act):
    seq = twin.step_sequence(act.contiguous(), terminal_obs=True, fin_stats=True, mse=True)
    torch.cuda.synchronize()
    return seq


def check_accumulators(acc, seq, max_episodes=0):
    """episode_acc[:, 0:5] = (episodes, return, length, violations, mse) summed over each env's finished episodes (the first
    max_episodes of them), from the replay's fin_stats: counts and lengths exact, sums at rtol 1e-5."""
    d = seq['done'].bool()
    take = d & (d.cumsum(0) <= max_episodes) if max_episodes else d
    fin = seq['fin_stats'] * take[..., None]
    assert torch.equal(acc[:, 0], take.sum(0).to(torch.float32))
    torch.testing.assert_close(acc[:, 1], fin[..., 0].sum(0), rtol=1e-5, atol=1e-4)
    assert torch.equal(acc[:, 2], fin[..., 1].sum(0))
    assert torch.equal(acc[:, 3], fin[..., 2].sum(0))
    torch.testing.assert_close(acc[:, 4], fin[..., 3].sum(0), rtol=1e-5, atol=1e-4)
    assert bool((acc[:, 5:] == 0).all())


@pytest.mark.parametrize('task,n,over', [('quadrotor_2D_track', 320, 0), ('cartpole_stab', 67, 10), ('quadrotor_3D_track', 33, 0)])
def test_rollout_policy_env_step_and_accumulators_against_step_sequence(task, n, over):
    """The kernel's stored actions replayed through scg_step_sequence on an identically seeded and preset twin: obs, reward, done,
    flags and terminal obs bit for bit; the episode accumulators and the running totals against the replay's."""
    env, twin = policy_env(task, n), policy_env(task, n)
    k = env.spec.max_episode_steps + over if over else K
    nu = env.spec.nu
    net = Net(env, nu, *POLICY_BUILDS[task], seed=10, logstd=logstds(nu))
    first = twin.out.obs.clone()
    start = preset(env)
    preset(twin)
    o = run_policy(env, net, k, det=False)
    assert_resets(o, every_env=bool(over))
    seq = replay(twin, o['act'])
    fresh = torch.as_tensor(start[0] == 0, device=env.device)       # (a preset step moves the tracking reference of obs[0])
    if task == 'quadrotor_3D_track':
        print(f'obs[0] against the reset observation: worst difference {float((o["obs"][0][fresh] - first[fresh]).abs().max()):.3e}')
        torch.testing.assert_close(o['obs'][0][fresh], first[fresh], rtol=OBS0_TOL, atol=OBS0_TOL)
    else:
        assert torch.equal(o['obs'][0][fresh], first[fresh])
    assert torch.equal(o['obs'][1:], seq['obs'])
    assert torch.equal(o['rew'], seq['reward'])
    assert torch.equal(o['done'], seq['done']) and torch.equal(o['flags'], seq['flags'])
    d = o['done'].bool()
    assert torch.equal(o['term'][d], seq['terminal_obs'][d])
    check_accumulators(o['acc'], seq)
    assert torch.equal(env.ep_stats, twin.ep_stats)
    for a, b in zip(env.get_counters(), twin.get_counters()):
        assert np.array_equal(a, b)
    assert np.array_equal(env.get_raw_state(), twin.get_raw_state())
    env.close(); twin.close()


def test_rollout_policy_max_episodes():
    """max_episodes = 1 and 2: each env's accumulator stops after its first / second episode; stepping and the stored rows go on
    unchanged."""
    task, n = 'cartpole_stab', 67
    runs = {}
    for m in (0, 1, 2):
        env = policy_env(task, n)
        k = env.spec.max_episode_steps + 10
        net = Net(env, 1, *POLICY_BUILDS[task], seed=10, logstd=logstds(1))
        preset(env)
        runs[m] = run_policy(env, net, k, det=False, max_episodes=m)
        runs[m]['ep_stats'], runs[m]['counters'], runs[m]['state'] = env.ep_stats.clone(), env.get_counters(), env.get_raw_state()
        env.close()
    twin = policy_env(task, n)
    preset(twin)
    seq = replay(twin, runs[0]['act'])
    twin.close()
    count = seq['done'].bool().sum(0)
    print(f'episodes per env: {int(count.min())} .. {int(count.max())}')
    for m in (1, 2):
        assert bool((count > m).any()), f'an env finished more than {m} episodes'
        for name in ('obs', 'act', 'logp', 'rew', 'done', 'flags', 'term', 'ep_stats'):
            assert torch.equal(runs[m][name], runs[0][name]), (m, name)
        assert np.array_equal(runs[m]['state'], runs[0]['state'])
        for a, b in zip(runs[m]['counters'], runs[0]['counters']):
            assert np.array_equal(a, b)
        check_accumulators(runs[m]['acc'], seq, max_episodes=m)
    check_accumulators(runs[0]['acc'], seq)


# ---------------------------------------------------------------------------------------------------------------- (d) chaining
def chain(launch, make):
    """One 12-step launch on one handle, a 5-step and a 7-step launch on its twin (the accumulator handed on): every output, the
    raw state, the counters and the running episode totals bit for bit."""
    one_env, two_env = make(), make()
    preset(one_env)
    preset(two_env)
    one = launch(one_env, K, None)
    a = launch(two_env, 5, None)
    b = launch(two_env, 7, a['acc'])
    assert_resets(one)
    for name in one:
        if name == 'acc':
            assert torch.equal(one['acc'], b['acc'])
        elif name == 'obs':
            assert torch.equal(a['obs'][5], b['obs'][0])
            assert torch.equal(one['obs'], torch.cat([a['obs'][:5], b['obs']])), name
        else:
            assert torch.equal(one[name], torch.cat([a[name], b[name]])), name
    assert np.array_equal(one_env.get_raw_state(), two_env.get_raw_state())
    for x, y in zip(one_env.get_counters(), two_env.get_counters()):
        assert np.array_equal(x, y)
    assert torch.equal(one_env.ep_stats, two_env.ep_stats)
    one_env.close(); two_env.close()


def test_rollout_policy_two_launches_equal_one():
    task, n = 'quadrotor_2D_track', 320
    nets = {}

    def launch(env, k, acc):
        net = nets.setdefault('p', Net(env, env.spec.nu, *POLICY_BUILDS[task], seed=11, logstd=logstds(env.spec.nu)))
        o = run_policy(env, net, k, det=False, acc=acc)
        return o
    chain(launch, lambda: policy_env(task, n))


def test_rollout_adversarial_two_launches_equal_one():
    from tests import test_gpu_rollout_adversarial as A
    n, n_adv = 320, 3
    nets = {}

    def launch(env, k, acc):
        nu, ad = env.spec.nu, env.spec.adversary_dim
        if not nets:
            nets['p'] = Net(env, nu, A.H, A.ACT, seed=12, logstd=logstds(nu))
            nets['a'] = [Net(env, ad, A.H, A.ACT, seed=13 + j, logstd=logstds(ad, j)) for j in range(n_adv)]
        o = run_adv(env, nets['p'], nets['a'], k, False, False, idx=A._groups(n, n_adv), acc=acc)
        return o
    chain(launch, lambda: adv_env(n_adv, n))
