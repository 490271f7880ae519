"""The cbf_nn safety filter on the device: scg_cbf_nn_certify against the float64 restatement (tests/cbf_nn_model.py) and the
reference-derived minimisers of the fixture, scg_rollout_cbf_nn against scg_cbf_nn_certify (one arithmetic), scg_step_sequence (the env
step is untouched), scg_rollout_policy / scg_rollout_random (the uncertified action's draws), the blend rules, learn(), the controller
path and the refusals.

Tolerances.
  d_ab      |a_b - a_b64| <= TAU S per output, TAU = 1e-5, S = |b3| + sum |W3| |h2| in float64 (tests/test_gpu_offpolicy_collector.py's
            bound of a float32 forward pass); every test prints its worst ratio.
  u*, s*    against the float64 model FED THE KERNEL'S OWN d_ab: bound_u / bound_s of tests/test_cbf_nn_cpu.py (4 x the float32
            model's deviation from the float64 one on the fixture rows, measured on the CPU, not on the code under test).  Rows whose
            float64 r(u0) lies within bound_s of 0 or whose s* lies within it of slack_tolerance may take either branch: left out, at
            most 1 % (of n, rounded up).
  against the reference-derived minimisers (which used the float64 forward): the same bounds plus the propagated forward error.  With
            dk = TAU S_b (the error of b_nn enters k') and db = TAU S_a (a_nn enters b'):
                |du*| <= |du*/dk'| dk + |du*/db'| db            (cbf_nn_model.sensitivity: analytic derivatives of the closed form, zero
                                                                  where u* = u0 or u* is clipped)
                |ds*| <= |ds*/dk'| dk + |ds*/db'| db            (s* = -k' - b' u* where positive: ds*/dk' = -1 - b' du*/dk' and
                                                                  ds*/db' = -u* - b' du*/db', signed, so the unclipped soft row's
                                                                  1 / (1 + 2 w b'^2) shows)
            taken twice (second-order terms: dk / |k'|, db / |b'| are ~1e-5).  Boundary rows: r(u0) within bound_s + dk + |u0| db of 0
            (r(u0) = -k' - b' u0 term by term), s* within its own tolerance of slack_tolerance.
"""
import copy
import ctypes as C
import os
from functools import partial

import numpy as np
import pytest

from tests import cbf_nn_cases as CN
from tests import cbf_nn_model as NM
from tests.test_cbf_nn_cpu import D, HI, LO, S, SF, TAU, WEIGHTS, bounds

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SHAPE = (S['algo_config']['hidden_dim'], S['algo_config']['activation'])
CERT_SIZES = (1, 31, 33, 67, 257, 291)       # one ragged tile, a tile boundary, a ragged workgroup, a workgroup boundary
K = 40


def _env(n, seed=7, normalized=False, shape=SHAPE, auto_reset=True, **kw):
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = CN.task_config(normalized)
    env = HipVecEnv(env_id, n, seed=seed, return_numpy=False, policy=shape, cbf_nn=True, auto_reset=auto_reset, **cfg, **kw)
    assert env.cbf_nn_shape == shape
    env.reset_tensors()
    return env


def _filter(weights=WEIGHTS, **over):
    from safe_control_gym_amd.registration import make
    env_id, cfg = CN.task_config(False)
    sf = make('cbf_nn', partial(make, env_id, **cfg), **dict(copy.deepcopy(SF), **over))
    sf.mlp.load_state_dict({k: torch.tensor(np.asarray(w, dtype=np.float32)) for k, w in zip(NM.KEYS, weights)})
    return sf


def _actor(dev, shape, det, seed=3, scale=30.0, logstd=-0.5, obs_dim=4):
    """(flat, _lib.Policy, ActorPtrs) of a PPO actor of `shape`: the example's shipped one at 64 tanh (tests/golden/cbf.npz), seeded
    random weights otherwise; the output layer scaled so that corrections, infeasible rows and the input clip all occur."""
    from safe_control_gym_amd import _cbf
    from safe_control_gym_amd import _lib as L
    h = shape[0]
    if shape == SHAPE:
        G = np.load(os.path.join(CN.GOLDEN, 'cbf.npz'))
        parts = [np.asarray(G[f'actor/actor.pi_net.fcs.{i}.{k}'], dtype=np.float32).reshape(-1) for i in range(3) for k in ('weight', 'bias')]
    else:
        rng = np.random.default_rng(seed)
        parts = [rng.normal(0, 0.5, h * obs_dim), rng.normal(0, 0.1, h), rng.normal(0, 1.0 / np.sqrt(h), h * h), rng.normal(0, 0.1, h),
                 rng.normal(0, 0.05, h), rng.normal(0, 0.1, 1)]
        parts = [p.astype(np.float32) for p in parts]
    parts[4], parts[5] = parts[4] * np.float32(scale), parts[5] * np.float32(scale)
    parts.append(np.full(1, logstd, dtype=np.float32))
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    flat = torch.tensor(np.concatenate(parts), device=dev)
    pol = L.Policy(d_params=flat.data_ptr(), W1=int(offs[0]), b1=int(offs[1]), W2=int(offs[2]), b2=int(offs[3]), W3=int(offs[4]),
                   b3=int(offs[5]), logstd_off=int(offs[6]), hidden=h, activation=L.POLICY_ACTS[shape[1]], deterministic=int(det))
    return flat, pol, _cbf.actor_ptrs_of_policy(pol)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


def _assert_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f'{what}: not bit-identical'


def _certify(sf, env, states, actions):
    st = torch.tensor(np.asarray(states), dtype=torch.float32, device=env.device)
    ac = torch.tensor(np.asarray(actions), dtype=torch.float32, device=env.device)
    u, s, f, ab = sf.certify_tensors(st, ac, with_ab=True)
    torch.cuda.synchronize()
    return u.double().cpu().numpy(), s.double().cpu().numpy(), f.cpu().numpy().astype(bool), ab.double().cpu().numpy()


@pytest.fixture(scope='module')
def cert_env():
    env = _env(64)
    yield env
    env.close()


def _check_against_own_ab(u, s, f, ab, states, actions, soft, what):
    """ab within TAU S of the float64 forward; (u*, s*, flags) within the CPU-measured bounds of the float64 model fed the kernel's ab."""
    n = len(u)
    ab64, mag = NM.forward(WEIGHTS, states, with_magnitude=True)
    ratio = (np.abs(ab - ab64) / (TAU * mag)).max()
    _, _, bound_u, bound_s, _ = bounds(soft)
    r = NM.certify(states, actions, ab, D['limits'], D['prior'], SF['slope'], SF['slack_weight'], SF['slack_tolerance'], LO, HI, soft=soft)
    near = np.abs(r['r0']) <= bound_s
    if soft:
        near |= np.abs(r['s'] - SF['slack_tolerance']) <= bound_s
    keep = ~near
    cmp = keep & (r['feasible'] if not soft else np.ones(n, bool))                   # hard, empty feasible set: the flag only
    du = np.abs(u - r['u'])[cmp].max() if cmp.any() else 0.0
    ds = np.abs(s - r['s'])[cmp].max() if cmp.any() else 0.0
    print(f'{what}: n {n}, ab worst error / (TAU S) {ratio:.3f}; |du*| {du:.3e} (bound {bound_u:.3e}) |ds*| {ds:.3e} (bound {bound_s:.3e}); boundary '
          f'rows {int(near.sum())}; flag mismatches {int((f != r["feasible"])[keep].sum())}')
    assert ratio <= 1.0
    assert near.sum() <= np.ceil(0.01 * n)
    assert (f == r['feasible'])[keep].all()
    assert du <= bound_u and ds <= bound_s


@pytest.mark.parametrize('n', CERT_SIZES)
def test_certify_sizes(cert_env, n):
    sf = _filter().attach(cert_env)
    states, actions = D['states'][:n], D['actions'][:n]
    u, s, f, ab = _certify(sf, cert_env, states, actions)
    _check_against_own_ab(u, s, f, ab, states, actions, True, 'soft')
    # a row's result does not depend on where it sits in a launch: the same rows inside the full fixture
    u2, s2, f2, ab2 = _certify(sf, cert_env, D['states'], D['actions'])
    assert np.array_equal(u, u2[:n]) and np.array_equal(s, s2[:n]) and np.array_equal(f, f2[:n]) and np.array_equal(ab, ab2[:n])
    if n == CERT_SIZES[-1]:
        hard = _filter(soft_constrained=False).attach(cert_env)
        _check_against_own_ab(*_certify(hard, cert_env, states, actions), states, actions, False, 'hard')
        a, b = sf.extract_a_b(states[5])
        assert a.shape == (1,) and float(a[0]) == np.float32(ab[5, 0]) and float(b) == np.float32(ab[5, 1])
        c1, ok1 = sf.certify_action(states[3], np.array([actions[3]]))
        assert c1.shape == () and ok1 == bool(f[3]) and float(c1) == u[3] and len(sf.results_dict['feasible']) == 1
    # n = 0 is a no-op: nothing is launched, nothing is written
    st = torch.zeros(4, 4, device=cert_env.device)
    out = torch.full((4,), 7.0, device=cert_env.device)
    flag = torch.full((4,), 9, dtype=torch.uint8, device=cert_env.device)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rc = cert_env._lib.scg_cbf_nn_certify(cert_env._h, C.byref(sf.params()), C.byref(sf.residual(cert_env.device)), p(st), p(out), p(out), p(out),
                                          p(flag), None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and (out == 7.0).all() and (flag == 9).all()
    empty = sf.certify_tensors(st[:0], out[:0])
    assert all(t.numel() == 0 for t in empty)


@pytest.mark.parametrize('mode', ['soft', 'hard'])
def test_fixture_rows_match_the_reference_minimisers(cert_env, mode):
    soft = mode == 'soft'
    sf = _filter(soft_constrained=soft).attach(cert_env)
    u, s, f, ab = _certify(sf, cert_env, D['states'], D['actions'])
    _check_against_own_ab(u, s, f, ab, D['states'], D['actions'], soft, mode)
    ab64, mag = NM.forward(WEIGHTS, D['states'], with_magnitude=True)
    r = NM.certify(D['states'], D['actions'], ab64, D['limits'], D['prior'], SF['slope'], SF['slack_weight'], SF['slack_tolerance'], LO, HI, soft=soft)
    _, _, bound_u, bound_s, _ = bounds(soft)
    dk, db = TAU * mag[:, 1], TAU * mag[:, 0]
    du_dk, du_db, ds_dk, ds_db = NM.sensitivity(r, SF['slack_weight'], LO, HI, soft)
    tol_u = bound_u + 2 * (du_dk * dk + du_db * db)
    tol_s = bound_s + 2 * (ds_dk * dk + ds_db * db)
    near = np.abs(r['r0']) <= bound_s + dk + np.abs(r['u0']) * db
    if soft:
        near |= np.abs(r['s'] - SF['slack_tolerance']) <= tol_s
    acc = D[f'{mode}/accepted'] & ~near
    print(f'{mode}: accepted and off the boundary {int(acc.sum())} / {len(acc)}, boundary rows {int(near.sum())}; propagated forward error: '
          f'median {np.median(2 * (du_dk * dk + du_db * db)):.2e}, max {(2 * (du_dk * dk + du_db * db)).max():.2e}')
    assert near.mean() <= 0.01
    if soft:
        assert (np.abs(u - D['soft/u']) <= tol_u)[acc].all() and (np.abs(s - D['soft/s']) <= tol_s)[acc].all()
        assert (f == (D['soft/s'] <= SF['slack_tolerance']))[acc].all()
    else:
        ne = D['hard/nonempty']
        assert (f == ne)[acc].all()
        assert (np.abs(u - D['hard/u']) <= tol_u)[acc & ne].all()


def test_zero_residual_equals_the_plain_filter(cert_env):
    """W3 = 0 and b3 = 0: every output equals scg_cbf_certify of a scg_cbf.hip library on the same rows."""
    from safe_control_gym_amd.registration import make
    from safe_control_gym_amd.vec_env import HipVecEnv
    zero = [w if i < 4 else np.zeros_like(w) for i, w in enumerate(WEIGHTS)]
    env_id, cfg = CN.task_config(False)
    plain_env = HipVecEnv(env_id, 64, seed=7, return_numpy=False, policy=SHAPE, cbf=True, **cfg)
    for soft in (True, False):
        sf = _filter(zero, soft_constrained=soft).attach(cert_env)
        plain = make('cbf', partial(make, env_id, **cfg), **{k: v for k, v in dict(SF, soft_constrained=soft).items()
                                                               if k in ('slope', 'soft_constrained', 'slack_weight', 'slack_tolerance')}).attach(plain_env)
        st = torch.tensor(D['states'], dtype=torch.float32, device=cert_env.device)
        ac = torch.tensor(D['actions'], dtype=torch.float32, device=cert_env.device)
        u, s, f, ab = sf.certify_tensors(st, ac, with_ab=True)
        pu, ps, pf = plain.certify_tensors(st, ac)
        assert (ab == 0).all() and (u == pu).all() and (s == ps).all() and (f == pf).all()
    plain_env.close()


def _rollout(env, sf, actor, k=K, **kw):
    o = sf.rollout(env, k, actor=actor, **kw)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('n', [67, 291])
@pytest.mark.parametrize('shape', [SHAPE, (128, 'relu')], ids=lambda s: f'{s[0]}{s[1]}')
def test_rollout_rows_equal_certify_and_the_env_step_is_untouched(n, shape, monkeypatch):
    from safe_control_gym_amd import _cbf_nn
    seed = 11
    env = _env(n, seed=seed, shape=shape)
    sf = _filter().attach(env)
    flat, pol, actor = _actor(env.device, shape, False)
    o = _rollout(env, sf, actor, deterministic=False, blend=-1.0)
    a_pol = o['act'][..., 0]
    st = o['obs'][:K, :, :4].reshape(-1, 4).contiguous()
    u, s, feas, ab = sf.certify_tensors(st, a_pol.reshape(-1).contiguous(), with_ab=True)
    rows = o['rows'].reshape(-1, 4)
    _assert_bits(rows[:, 1], u, 'u*')
    _assert_bits(rows[:, 2], s, 's*')
    assert torch.equal(rows[:, 3].cpu(), feas.float().cpu())
    _assert_bits(o['ab'].reshape(-1, 2), ab, 'a_b')
    np.testing.assert_array_equal(rows[:, 0].cpu().numpy(), np.clip(a_pol.reshape(-1).cpu().numpy(), np.float32(LO), np.float32(HI)))
    # blend = -1: CbfActorFilter's rule
    f = rows[:, 3].cpu().numpy() != 0
    want = np.where(f, rows[:, 1].cpu().numpy(), a_pol.reshape(-1).cpu().numpy()).astype(np.float32)
    np.testing.assert_array_equal(o['applied'].cpu().numpy().reshape(-1).view(np.int32), want.view(np.int32))
    corrected = np.abs(rows[:, 1].cpu().numpy() - rows[:, 0].cpu().numpy()) > 1e-6
    print(f'n {n} {shape}: feasible {f.mean():.3f}, corrected {corrected.mean():.3f}, done {o["done"].float().mean().item():.4f}')
    assert 0 < f.mean() < 1 and corrected.mean() > 0.01
    # the env step: replay the applied actions
    env3 = _env(n, seed=seed, shape=shape)
    q = env3.step_sequence(o['applied'].reshape(K, n, 1).contiguous(), terminal_obs=True)
    torch.cuda.synchronize()
    _assert_bits(q['obs'], o['obs'][1:], 'obs')
    _assert_bits(q['reward'], o['rew'], 'reward')
    assert torch.equal(q['done'].cpu(), o['done'].cpu()) and torch.equal(q['flags'].cpu(), o['flags'].cpu())
    assert o['done'].any()
    # the sampled action and its log-probability: scg_rollout_policy's on the first step (same state, same Philox draw)
    env2 = _env(n, seed=seed, shape=shape)
    f32 = dict(device=env.device, dtype=torch.float32)
    p = {'obs': torch.zeros(2, n, 4, **f32), 'act': torch.zeros(1, n, 1, **f32), 'logp': torch.zeros(1, n, **f32), 'rew': torch.zeros(1, n, **f32),
         'done': torch.zeros(1, n, dtype=torch.uint8, device=env.device), 'flags': torch.zeros(1, n, dtype=torch.uint8, device=env.device)}
    env2.rollout_policy(pol, 1, p['obs'], p['act'], p['logp'], p['rew'], p['done'], p['flags'])
    torch.cuda.synchronize()
    _assert_bits(p['act'][0], o['act'][0], 'act[0]')
    _assert_bits(p['logp'][0], o['logp'][0], 'logp[0]')
    # 17 + 23 chained steps equal 40
    env4 = _env(n, seed=seed, shape=shape)
    o1 = _rollout(env4, sf, actor, k=17, deterministic=False)
    o2 = _rollout(env4, sf, actor, k=23, deterministic=False)
    for key in ('act', 'logp', 'rew', 'done', 'flags', 'rows', 'applied', 'ab'):
        _assert_bits(torch.cat([o1[key], o2[key]]), o[key], 'chained ' + key)
    _assert_bits(torch.cat([o1['obs'], o2['obs'][1:]]), o['obs'], 'chained obs')
    # G = 1 equals G = 8 where both fit
    if _cbf_nn.rollout_lds_bytes(4, shape[0], 8) <= _cbf_nn.LDS_LIMIT:
        outs = []
        for g in ('1', '8'):
            monkeypatch.setenv('SCG_ROLLOUT_WIDE_TILES', g)
            e = _env(n, seed=seed, shape=shape)
            outs.append(_rollout(e, sf, actor, deterministic=False))
            e.close()
        monkeypatch.delenv('SCG_ROLLOUT_WIDE_TILES')
        for key in ('obs', 'act', 'logp', 'rew', 'done', 'flags', 'rows', 'applied', 'ab'):
            _assert_bits(outs[0][key], outs[1][key], 'G ' + key)
            _assert_bits(outs[0][key], o[key], 'G vs default ' + key)
    else:
        assert _cbf_nn.lds_of(env._lib, 8) > _cbf_nn.LDS_LIMIT >= _cbf_nn.lds_of(env._lib, 1)
    assert _cbf_nn.lds_of(env._lib, 1) == _cbf_nn.rollout_lds_bytes(4, shape[0], 1)
    del flat
    for e in (env, env2, env3, env4):
        e.close()


@pytest.mark.parametrize('normalized', [False, True])
def test_blend_rules_uniform_draws_and_fresh_weights(normalized):
    n, seed = 67, 5
    scale = np.float32(10.0)
    sf = _filter()
    flat, pol, actor = _actor(torch.device('cuda'), SHAPE, True, scale=30.0 if not normalized else 3.0)
    for blend in (0.0, 0.5, 1.0):
        env = _env(n, seed=seed, normalized=normalized)
        o = _rollout(env, sf.attach(env), actor, k=12, deterministic=True, blend=blend)
        a = o['act'][..., 0].cpu().numpy()
        ustar = o['rows'][..., 1].cpu().numpy()
        u_env = (ustar / scale).astype(np.float32) if normalized else ustar
        w = np.float32(blend)
        want = ((np.float32(1.0) - w) * a).astype(np.float32) + (w * u_env).astype(np.float32)
        np.testing.assert_array_equal(o['applied'].cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32))
        if normalized:                                  # the filter saw the physical action
            np.testing.assert_array_equal(o['rows'][..., 0].cpu().numpy(), np.clip((scale * a).astype(np.float32), np.float32(LO), np.float32(HI)))
        env.close()
    # uniform = 1, blend = 0: the env receives action_space.sample() of Philox channel 4, i.e. scg_rollout_random's trajectory
    env = _env(n, seed=seed, normalized=normalized)
    o = _rollout(env, sf.attach(env), None, k=12, uniform=True, blend=0.0)
    _assert_bits(o['applied'], o['act'][..., 0], 'blend 0 applies the uncertified action')
    lim = 1.0 if normalized else 10.0
    a = o['act'].cpu().numpy()
    assert (a >= -lim).all() and (a < lim).all() and a.std() > 0.4 * lim
    assert (o['logp'] == 0).all()
    if normalized:
        ref = _env(n, seed=seed, normalized=True)
        _, done_count, viol_count, last_obs = ref.rollout_random(12)
        torch.cuda.synchronize()
        _assert_bits(last_obs, o['obs'][-1], 'rollout_random last obs')
        assert torch.equal(done_count.cpu(), o['done'].sum(0).to(torch.int32).cpu())
        ref.close()
    # a launch whose weights were changed between two calls sees the new weights
    env5 = _env(n, seed=seed, normalized=normalized)
    sf.attach(env5)
    o_a = _rollout(env5, sf, actor, k=3, deterministic=True)
    with torch.no_grad():
        sf.mlp.fcs[2].bias[1].add_(0.25)               # b3 of the b_nn output only
    env6 = _env(n, seed=seed, normalized=normalized)
    o_b = _rollout(env6, sf.attach(env6), actor, k=3, deterministic=True)
    _assert_bits(o_a['ab'][0, :, 0], o_b['ab'][0, :, 0], 'a_nn')
    np.testing.assert_allclose(o_b['ab'][0, :, 1].cpu().numpy(), o_a['ab'][0, :, 1].cpu().numpy() + 0.25, rtol=0, atol=1e-5)
    assert not torch.equal(o_a['ab'][0, :, 1], o_b['ab'][0, :, 1])
    del flat, pol
    for e in (env, env5, env6):
        e.close()


def test_learn_buffer_update_and_checkpoint(tmp_path):
    """learn at num_episodes = 3, max_num_steps = 12, num_envs = 67, train_iterations = 2, batch 8.  Conditioning of the two float64
    columns: barrier_dot = a + b u is a sum of a few terms of size <= ~50 (rounding ~1e-14); barrier_dot_approx is a difference of two
    barrier values of size O(1) (each exact to ~2e-16) multiplied by CTRL_FREQ / 2 = 12.5, i.e. good to ~5e-15 however close the two
    values are — an ABSOLUTE error, so both columns are compared at an absolute 1e-12."""
    n, steps, episodes, iters, batch = 67, 12, 3, 2, 8
    sf = _filter(num_episodes=episodes, max_num_steps=steps, train_iterations=iters, train_batch_size=batch, max_buffer_size=4096, seed=4)
    before = copy.deepcopy(sf.mlp.state_dict())
    traces = []
    orig = sf.rollout

    def spy(*a, **kw):
        o = orig(*a, **kw)
        traces.append({k: v.clone() for k, v in o.items()})
        return o
    sf.rollout = spy
    sf.learn(num_envs=n)
    torch.cuda.synchronize()
    assert sf.blend_weights == [0.0, 0.5, 1.0] and len(traces) == episodes
    env = sf._learn_env
    assert not env.auto_reset and env.num_envs == n
    freq = float(env.spec.CTRL_FREQ)
    rows_per_env = steps - 2
    buf = sf.buffer
    assert buf.pos == episodes * n * rows_per_env
    for ep, o in enumerate(traces):
        w = np.float32(sf.blend_weights[ep])
        a, ustar = o['act'][..., 0].cpu().numpy(), o['rows'][..., 1].cpu().numpy()
        want = ((np.float32(1.0) - w) * a).astype(np.float32) + (w * ustar).astype(np.float32)
        np.testing.assert_array_equal(o['applied'].cpu().numpy().view(np.int32), want.view(np.int32))
        obs, applied = o['obs'].double().cpu().numpy(), o['applied'].double().cpu().numpy()
        base = ep * n * rows_per_env
        for e in (0, 31, 66):
            m = NM.pushed_arrays(obs[1:, e, :4], applied[:, e], D['limits'], D['prior'], freq)
            sl = slice(base + e * rows_per_env, base + (e + 1) * rows_per_env)
            assert np.array_equal(buf.state[sl].cpu().numpy(), m['state'].astype(np.float32))
            assert np.array_equal(buf.act[sl].cpu().numpy(), m['act'].astype(np.float32))
            np.testing.assert_allclose(buf.barrier_dot[sl].cpu().numpy(), m['barrier_dot'], rtol=0, atol=1e-12)
            assert abs(m['barrier_dot_approx']).max() > 1e-3                      # (multiplied by CTRL_FREQ / 2 on both sides)
            np.testing.assert_allclose(buf.barrier_dot_approx[sl].cpu().numpy(), m['barrier_dot_approx'], rtol=0, atol=1e-12)
    # the same Adam steps, eagerly, on the same sampled indices
    assert len(sf.sampled_indices) == episodes * iters and all(len(i) == batch for i in sf.sampled_indices)
    from safe_control_gym_amd import cbf_nn
    from safe_control_gym_amd.ppo import MLP
    ref = MLP(4, 2, [256, 256], 'relu').to(env.device)
    ref.load_state_dict(before)
    opt = torch.optim.Adam(ref.parameters(), SF['learning_rate'])
    snap = type(buf)(4, 1, buf.max_size, env.device, batch)
    it = iter(sf.sampled_indices)
    for ep, o in enumerate(traces):
        st, ac, bd, ap = cbf_nn.pushed_arrays(o['obs'][1:, :, :4], o['applied'].double(), sf.state_limits, D['prior'], freq)
        snap.push({'state': st, 'act': ac, 'barrier_dot': bd, 'barrier_dot_approx': ap})
        for _ in range(iters):
            b = snap.gather(next(it))
            a_b = ref(b['state'])
            loss = (b['barrier_dot'] + torch.unsqueeze(a_b[:, 0], 1) * b['act'] + torch.unsqueeze(a_b[:, 1], 1) - b['barrier_dot_approx']).pow(2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
    for k in NM.KEYS:
        assert torch.equal(ref.state_dict()[k], sf.mlp.state_dict()[k]), k
    assert not torch.equal(before['fcs.2.weight'].to(env.device), sf.mlp.state_dict()['fcs.2.weight'])
    # save / load round-trips and resumes
    path = str(tmp_path / 'cbf_nn.pt')
    sf.save(path)
    other = _filter(num_episodes=episodes, max_num_steps=steps, train_iterations=iters, train_batch_size=batch, max_buffer_size=4096, seed=4)
    other.load(path)
    for k in NM.KEYS:
        assert torch.equal(other.mlp.state_dict()[k].cpu(), sf.mlp.state_dict()[k].cpu())
    assert (other.buffer.pos, other.buffer.buffer_size) == (buf.pos, buf.buffer_size)
    assert torch.equal(other.buffer.barrier_dot.cpu(), buf.barrier_dot.cpu())
    other.learn(num_envs=n)
    assert other.buffer.pos == 2 * episodes * n * rows_per_env
    other.close()
    sf.close()


def test_controller_run_and_is_cbf():
    from safe_control_gym_amd import _cbf
    from safe_control_gym_amd.cbf import state_grid
    from safe_control_gym_amd.registration import make
    env_id, cfg = CN.task_config(False)
    n = 64
    ctrl = make('ppo', partial(make, env_id, **cfg), training=False, seed=2, hidden_dim=SHAPE[0], activation=SHAPE[1], eval_batch_size=n)
    sf = _filter()
    out = ctrl.run(n_episodes=n, safety_filter=sf)
    ev = ctrl._run_env_cbf
    assert ev.cbf_nn_shape == SHAPE and set(out['safety_filter_data']) == {'steps', 'corrected_steps', 'infeasible_steps', 'mean_correction'}
    k = ev.spec.max_episode_steps
    env2 = _env(n, seed=ctrl.seed * 111)                # (one reset after construction, as evaluate() gives the controller's env)
    acc = torch.zeros(n, 8, device=env2.device)
    o = sf.rollout(env2, k, actor=_cbf.actor_ptrs_of_policy(ctrl.impl._policy_struct(True)), deterministic=True, blend=-1.0, episode_acc=acc,
                   max_episodes=1)
    torch.cuda.synchronize()
    _assert_bits(ev._eval_cbf['rows'], o['rows'], 'filter rows')
    _assert_bits(ev._eval_cbf['ab'], o['ab'], 'a_b')
    np.testing.assert_array_equal(out['ep_returns'], acc[:, 1].double().cpu().numpy())
    # a CBF_NN on an env without cbf_nn=True raises, as cbf does
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd.ppo import evaluate
    from safe_control_gym_amd.vec_env import HipVecEnv
    plain = HipVecEnv(env_id, n, seed=5, return_numpy=False, policy=SHAPE, cbf=True, **cfg)
    with pytest.raises(L.ScgError, match='cbf_nn=True'):
        evaluate(None, plain, policy=ctrl.impl._policy_struct(True), safety_filter=sf)
    plain.close()
    # is_cbf on the default grid: one launch of 456 976 rows
    sf.attach(env2)
    valid, infeasible = sf.is_cbf()
    grid = state_grid(D['limits'], 100, 0.01)
    assert grid.shape == (26 ** 4, 4)
    st = torch.tensor(grid, dtype=torch.float32, device=env2.device)
    _, _, _, ab = sf.certify_tensors(st, torch.ones(len(grid), device=env2.device), with_ab=True)
    args = (grid, np.ones(len(grid)), ab.double().cpu().numpy(), D['limits'], D['prior'], SF['slope'], SF['slack_weight'], SF['slack_tolerance'], LO, HI)
    r64, r32 = NM.certify(*args), NM.certify(*args, dtype=np.float32)
    bound_s = 4 * np.abs(r32['s'].astype(np.float64) - r64['s']).max()
    near = (np.abs(r64['r0']) <= bound_s) | (np.abs(r64['s'] - SF['slack_tolerance']) <= bound_s)
    bad64 = ~r64['feasible']
    got = np.zeros(len(grid), bool)
    index = {tuple(np.round(g, 9)): i for i, g in enumerate(grid)}
    for sx in infeasible:
        got[index[tuple(np.round(sx, 9))]] = True
    h = 1.0 - ((grid / D['limits']) ** 2).sum(axis=1)
    print(f'is_cbf: valid {valid}, infeasible states {int(got.sum())} (float64 {int(bad64.sum())}), boundary rows {int(near.sum())} / {len(grid)}, '
          f'slack bound {bound_s:.3e}')
    assert near.mean() <= 0.01
    assert (got == bad64)[~near].all()
    assert valid == (not (bad64 & (h > 1e-6)).any()) or (near & (h > 1e-6) & (got != bad64)).any()
    env2.close()
    ctrl.close()


def test_refusals(cert_env):
    from safe_control_gym_amd import _cbf_nn
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd.env_config import EnvSpec
    from safe_control_gym_amd.vec_env import HipVecEnv
    from tests import actor_rollout_cases as arc
    env = cert_env
    sf = _filter().attach(env)
    res = sf.residual(env.device)
    dev = env.device
    st = torch.zeros(8, 4, device=dev)
    ac = torch.zeros(8, device=dev)
    # misaligned rows, a residual of another width, NULL parameters
    big = torch.zeros(9 * 4 + 1, device=dev)
    with pytest.raises(L.ScgError, match='16-byte aligned'):
        env.certify_nn_tensors(sf.params(), res, big[1:33].view(8, 4), ac)
    bad = _cbf_nn.Residual(d_params=res.d_params, mlp=res.mlp, hidden=128)
    with pytest.raises(L.ScgError, match='4 -> 256 -> 256 -> 2'):
        env.certify_nn_tensors(sf.params(), bad, st, ac)
    with pytest.raises(L.ScgError, match='d_params is NULL'):
        env.certify_nn_tensors(sf.params(), _cbf_nn.Residual(d_params=None, mlp=res.mlp, hidden=256), st, ac)
    with pytest.raises(ValueError):
        _cbf_nn.residual_of(torch.zeros(100, device=dev))
    # the rollout: k_steps < 1, a missing actor, wrong blend
    flat, pol, actor = _actor(dev, SHAPE, True)
    with pytest.raises(L.ScgError, match='k_steps must be positive'):
        sf.rollout(env, 0, actor=actor)
    with pytest.raises(ValueError, match='needs an actor'):
        sf.rollout(env, 2, actor=None)
    with pytest.raises(L.ScgError, match='blend'):
        sf.rollout(env, 2, actor=actor, blend=1.5)
    # wrong actor shape: the controller's shape must be the env's
    _, pol128, _ = _actor(dev, (128, 'relu'), True)
    sf.uncertified_controller = pol128
    with pytest.raises(L.ScgError, match='was built for an actor of shape'):
        sf.learn(env=_NoAutoReset(env))
    sf.uncertified_controller = None
    with pytest.raises(L.ScgError, match='auto_reset=False'):
        sf.learn(env=env)
    # an env without the library, another system, an actor kind, an actor + residual that does not fit the LDS
    env_id, cfg = CN.task_config(False)
    with pytest.raises(L.ScgError, match='no SAC / DDPG actor'):
        HipVecEnv(env_id, 8, return_numpy=False, policy=(64, 'tanh', 'sac'), cbf_nn=True, **cfg)
    q_id, q_cfg = arc.task_config(CN.REFUSING[0])
    with pytest.raises(NotImplementedError, match='only implemented for the cartpole'):
        HipVecEnv(q_id, 8, return_numpy=False, policy=CN.REFUSING[1:], cbf_nn=True, **q_cfg)
    assert _cbf_nn.rollout_tiles(4, 160, 1) is None and not _cbf_nn.supported('cartpole', 4, 160, 1, 'tanh')
    # a library of another task exports the entry points and refuses
    c, _ = EnvSpec(q_id, dict(q_cfg)).to_c_config(1, L.F32, 0)
    so = _cbf_nn.lib_path(L.spec_source(c)[1], *CN.REFUSING[1:])
    assert os.path.exists(so), 'build() compiles the refusing library'
    lib = _cbf_nn.bind(so)
    assert _cbf_nn.shape_of(lib) == (0, 0, 0, 0, 0) and _cbf_nn.lds_of(lib, 1) == 0
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    out = torch.zeros(8, device=dev)
    rc = lib.scg_cbf_nn_certify(env._h, C.byref(sf.params()), C.byref(res), p(st), p(ac), p(out), None, p(out), None, 8, None)
    with pytest.raises(L.ScgError, match='float32 cartpole'):
        L.check(rc, lib)
    del flat, pol


class _NoAutoReset:
    """A view of an env that reports auto_reset off (learn()'s argument checks run before any launch)."""

    def __init__(self, env):
        self._env = env

    def __getattr__(self, k):
        return False if k == 'auto_reset' else getattr(self._env, k)
