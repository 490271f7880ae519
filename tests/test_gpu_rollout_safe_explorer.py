"""scg_rollout_safe — the Safe-Explorer PPO collector as one launch (actor, safety layer, projection, sampling, env step, next constraint
values) — against the step-by-step path, float64 PyTorch restatements of the actor and SafetyLayer.get_safe_action, the Philox channel-5
host model, itself under other launch geometries and placements, and the collector / controller built on it."""
import functools
import os
import warnings

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, 'tests', 'golden', 'safe_explorer_ppo')
SLACK_Q2 = [0.05, 0.05, 0.05, 0.05, 0.01, 0.01] * 2                 # safe_explorer_ppo_quadrotor_2D*.yaml
GEOMETRIES = [('64', '4'), ('32', '4'), ('32', '8'), ('64', '8')]
N = 320                                                             # 5 / 10 waves, a partial workgroup


def _env(task='quadrotor_2D_track', H=32, hc=16, n=N, seed=5, **over):
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = load_task(task)
    env = HipVecEnv(env_id, n, seed=seed, return_numpy=False, policy=(H, 'tanh'), safety_layer=hc, **dict(cfg, **over))
    assert env.safety_shape == (H, 'tanh', hc)
    env.reset_tensors()
    return env


def _nets(env, H, hc, seed=0, slack=0.05, golden=False, zero_g=()):
    """(actor, safety layer): seeded random ones, or the shipped Quadrotor2D-tracking policy and pre-trained safety layer."""
    from safe_control_gym_amd.ppo import MLPActor
    from safe_control_gym_amd.safe_explorer import SafetyLayer
    torch.manual_seed(seed)
    spec = env.spec
    actor = MLPActor(spec.obs_dim, spec.nu, [H, H], 'tanh').to(env.device)
    layer = SafetyLayer(spec.obs_dim, spec.nu, spec.n_state_con_rows, hc, slack=slack, device=env.device)
    if golden:
        sd = torch.load(os.path.join(MODELS, 'safe_explorer_ppo_model_quadrotor_2D_track.pt'), map_location='cpu', weights_only=False)
        actor.load_state_dict({k[len('actor.'):]: v for k, v in sd['agent']['ac'].items() if k.startswith('actor.')})
        pre = torch.load(os.path.join(MODELS, 'safe_explorer_ppo_pretrain_quadrotor_2D_track.pt'), map_location='cpu', weights_only=False)
        layer.constraint_models.load_state_dict(pre['safety_layer']['constraint_models'])
    else:
        with torch.no_grad():
            for m in layer.constraint_models:                       # sensitivities of the size the shipped layer has
                m.fcs[1].weight.mul_(3.0)
            actor.logstd.copy_(torch.linspace(-0.9, -0.3, spec.nu))
    with torch.no_grad():
        for i in zero_g:                                            # g_i == 0: numer / 1e-8, times a zero sensitivity
            layer.constraint_models[i].fcs[1].weight.zero_()
            layer.constraint_models[i].fcs[1].bias.zero_()
    return actor, layer


def _run(env, actor, layer, k, det=False, carry=None):
    from safe_control_gym_amd import _adversarial, _safe_explorer
    n, nobs, nu, C = env.num_envs, env.spec.obs_dim, env.spec.nu, env.spec.n_state_con_rows
    f = dict(device=env.device, dtype=torch.float32)
    u8 = dict(device=env.device, dtype=torch.uint8)
    o = {'obs': torch.zeros(k + 1, n, nobs, **f), 'act': torch.zeros(k, n, nu, **f), 'logp': torch.zeros(k, n, **f),
         'rew': torch.zeros(k, n, **f), 'done': torch.zeros(k, n, **u8), 'flags': torch.zeros(k, n, **u8),
         'term': torch.zeros(k, n, nobs, **f), 'c_rows': torch.full((k, n, C), float('nan'), **f), 'acc': torch.zeros(n, 8, **f)}
    if carry is None:
        carry = env.spec.state_constraint_values(env.out.state.t()).to(torch.float32)
    o['carry_in'] = carry.clone()
    o['carry'] = carry.clone().contiguous()
    packed = _safe_explorer.pack_safety_layer(layer.constraint_models, nobs, nu, env.safety_shape[2])
    env.rollout_safe(_adversarial.actor_ptrs(actor), packed, layer.slack, k, o['obs'], o['act'], o['logp'], o['rew'], o['done'],
                     o['flags'], o['c_rows'], o['carry'], deterministic=det, terminal_obs=o['term'], episode_acc=o['acc'])
    torch.cuda.synchronize()
    return o


def _reference(actor, layer, obs, c):
    """float64 actor mean, g [B, C, A], multipliers [B, C] and SafetyLayer.get_safe_action."""
    import copy
    a64 = copy.deepcopy(actor).double()
    m64 = copy.deepcopy(layer.constraint_models).double()
    with torch.no_grad():
        x = obs.double()
        mean = a64.pi_net(x)
        g = torch.stack([m(x) for m in m64], dim=1)
        numer = (g * mean[:, None, :]).sum(-1) + c.double() + layer.slack.double()
        denom = (g * g).sum(-1) + 1e-8
        mult = torch.relu(numer / denom)
        best, idx = mult.max(-1)
        gb = g[torch.arange(g.shape[0], device=g.device), idx]
        safe = mean - best[:, None] * gb
        # error bound of the float32 kernel (exact-f32 MFMA chains, IEEE division): per-quantity relative errors propagated
        da = 2e-5 * (1 + mean.abs())
        # |g| error: relative to the magnitudes summed (exactly 0 for a constraint model with zero output weights)
        gabs = torch.stack([torch.relu(m.fcs[0](x)) @ m.fcs[1].weight.abs().T + m.fcs[1].bias.abs() for m in m64], dim=1)
        dg = 2e-5 * gabs
        # (the float32 sums g.a, + c, + slack round relative to their own results: exact where g == 0 and c + slack cancels)
        dot = (g * mean[:, None, :]).sum(-1)
        dnum = (g.abs() * da[:, None, :]).sum(-1) + (mean.abs()[:, None, :] * dg).sum(-1) + \
            1.2e-7 * ((g * mean[:, None, :]).abs().sum(-1) + (dot + c.double()).abs() + numer.abs())
        dden = (2 * g.abs() * dg).sum(-1) + 1.2e-7 * (g * g).sum(-1) + 1e-15
        # the UNCLAMPED ratio numer / denom and its error: a multiplier can reach [relu(r - dr), relu(r + dr)] in float32
        r = numer / denom
        dr = (dnum + r.abs() * dden) / denom + 2.4e-7 * r.abs()
        lo, up = torch.relu(r - dr), torch.relu(r + dr)
        rows = torch.arange(g.shape[0], device=g.device)
        dmb, dgb = dr[rows, idx], dg[rows, idx]
        bound = 2 * (da + dmb[:, None] * gb.abs() + best[:, None] * dgb)
        # rows whose argmax is not decided in float32: another constraint with different sensitivities can reach a positive multiplier at
        # least as large as the winner's lowest (constraints whose ratio is negative beyond its error, e.g. g == 0 rows with c + slack < 0,
        # stay at 0 and never compete; constraints with the winner's g give the same action either way)
        same_g = (g == gb[:, None, :]).all(-1)
        rival = torch.where(same_g, torch.zeros_like(up), up).amax(-1)
        ambiguous = (rival > 0) & (rival >= lo[rows, idx])
    return mean, g, mult, safe, bound, ambiguous


def _channel5(env, done, k):
    """The kernel's channel-5 N(0, 1) draws (scg_rollout_policy's) per step and env from the host Philox model (tests/philox_model.py):
    counter (env, episode, step in episode, tag(5, 0, 0)); the envs were reset once (episode 0) and auto-reset where done."""
    from tests import philox_model as pm
    n = env.num_envs
    ep, st = pm.follow(np.zeros(n, np.int64), np.zeros(n, np.int64), done[:k].cpu().numpy())
    return pm.env_normal4(env.seed_value, env.env_id_offset + np.arange(n)[None, :], ep, st, pm.CH_POLICY)[0]


@pytest.mark.parametrize('epw,wpw', GEOMETRIES)
def test_trajectory_and_constraint_rows_against_step_sequence(epw, wpw, monkeypatch):
    """The kernel's actions replayed through scg_step_sequence on an identically seeded handle: obs, reward, done, flags, terminal obs
    and the episode totals bit for bit, over enough steps (> one 250-step episode) for auto-resets; c_rows[t + 1] = the state rows of
    step t's c_values (continuing envs, exact) or EnvSpec.state_constraint_values of the fresh state (reset envs); c_rows[0] = the
    carry passed in; the carry afterwards = what the step after the last one needs."""
    monkeypatch.setenv('SCG_ROLLOUT_EPW', epw)
    monkeypatch.setenv('SCG_ROLLOUT_WPW', wpw)
    K = 260
    env, ref = _env(), _env()
    spec, C = env.spec, env.spec.n_state_con_rows
    actor, layer = _nets(env, 32, 16, seed=3)
    o = _run(env, actor, layer, K)
    assert torch.equal(o['obs'][0], ref.out.obs)
    seq = ref.step_sequence(o['act'].contiguous(), terminal_obs=True, c_values=True, state=True, fin_stats=True)
    torch.cuda.synchronize()
    assert torch.equal(o['obs'][1:], seq['obs'])
    assert torch.equal(o['rew'], seq['reward'])
    assert torch.equal(o['done'], seq['done']) and torch.equal(o['flags'], seq['flags'])
    d = o['done'].bool()
    assert int(d.sum()) >= N, 'auto-resets happened'
    assert torch.equal(o['term'][d], seq['terminal_obs'][d])
    # episode totals of the finished episodes (count, return, length, violations) and the running ones
    fin = seq['fin_stats']
    assert torch.equal(o['acc'][:, 0], d.sum(0).to(torch.float32))
    torch.testing.assert_close(o['acc'][:, 1], (fin[..., 0] * d).sum(0), rtol=1e-5, atol=1e-4)
    assert torch.equal(o['acc'][:, 2], (fin[..., 1] * d).sum(0))
    assert torch.equal(env.ep_stats, ref.ep_stats)
    # constraint values
    assert torch.equal(o['c_rows'][0], o['carry_in'])
    nxt = torch.cat([o['c_rows'][1:], o['carry'][None]], 0)                   # c after step t, t = 0..K-1
    cont = ~d
    step_rows = seq['c_values'][:, :C, :].permute(0, 2, 1)                     # [K, N, C]
    assert torch.equal(nxt[cont], step_rows[cont])
    fresh = spec.state_constraint_values(seq['state'].permute(0, 2, 1).reshape(K * N, spec.nx)).reshape(K, N, C).to(torch.float32)
    torch.testing.assert_close(nxt[d], fresh[d], rtol=1e-5, atol=1e-5)
    env.close(); ref.close()


CASES = [('quadrotor_2D_track', 128, 150, 'golden', ()), ('cartpole_stab', 32, 100, 'random', ()),
         ('quadrotor_3D_track', 128, 150, 'random', ()), ('quadrotor_2D_track', 32, 16, 'random', (0, 3, 7))]


@pytest.mark.parametrize('task,H,hc,kind,zero_g', CASES, ids=['q2track-shipped', 'cartpole-stab', 'q3track', 'q2track-zero-g'])
def test_policy_against_float64_pytorch(task, H, hc, kind, zero_g):
    """deterministic=1: actions = float64 actor + SafetyLayer.get_safe_action from the recorded obs and c rows within a propagated
    float32 bound; sampled: (act - safe mean) exp(-logstd) = the host Philox model's channel-5 draw and the log-probabilities match.
    The projection fires on a non-trivial share of the rows; rows whose top two multipliers are within the bound are counted and
    left out of the comparison."""
    slack = SLACK_Q2 if task == 'quadrotor_2D_track' else 0.05
    K = 24
    for det in (True, False):
        env = _env(task, H, hc, seed=9)
        actor, layer = _nets(env, H, hc, seed=4, slack=slack, golden=kind == 'golden', zero_g=zero_g)
        o = _run(env, actor, layer, K, det=det)
        n, nu = env.num_envs, env.spec.nu
        obs, c = o['obs'][:K].reshape(K * n, -1), o['c_rows'].reshape(K * n, -1)
        mean, g, mult, safe, bound, amb = _reference(actor, layer, obs, c)
        act = o['act'].reshape(K * n, nu).double()
        fired = (mult.max(-1).values > 0)
        assert float(fired.double().mean()) > 0.05, f'projection fired on {float(fired.double().mean()):.3f} of the rows'
        assert float(amb.double().mean()) < 0.05, f'{int(amb.sum())} ambiguous rows'
        ok = ~amb
        ls = actor.logstd.detach().double()
        if det:
            err = (act - safe).abs()
            assert bool((err[ok] <= bound[ok]).all()), f'max err/bound {float((err / bound)[ok].max()):.3g}'
            torch.testing.assert_close(o['logp'], torch.full_like(o['logp'], float(-(ls + 0.5 * np.log(2 * np.pi)).sum())), rtol=1e-6, atol=1e-5)
        else:
            eps = torch.as_tensor(_channel5(env, o['done'], K)[..., :nu], device=env.device).reshape(K * n, nu)
            rec = (act - safe) * torch.exp(-ls)
            tol = 4e-6 * (1 + eps.abs()) + bound * torch.exp(-ls) + 6e-8
            assert bool(((rec - eps).abs()[ok] <= tol[ok]).all()), f'max err/bound {float(((rec - eps).abs() / tol)[ok].max()):.3g}'
            logp = (-0.5 * eps * eps - ls - 0.5 * np.log(2 * np.pi)).sum(-1)
            torch.testing.assert_close(o['logp'].reshape(-1).double(), logp, rtol=1e-5, atol=2e-5)
        if zero_g:
            assert bool((g[:, list(zero_g)] == 0).all())
        env.close()


def test_placements_are_bit_identical_and_over_budget_refuses(monkeypatch):
    """SCG_SAFE_WEIGHTS=lds and =global on a shape that fits both give the same outputs bit for bit; forcing LDS on the shipped
    Quadrotor2D-tracking shape (actor image + layer > 160 KiB) returns an error and writes nothing."""
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd import _safe_explorer
    outs = []
    for where in ('lds', 'global'):
        monkeypatch.setenv('SCG_SAFE_WEIGHTS', where)
        env = _env(seed=21)
        assert _safe_explorer.launch_plan(env._lib, 4)[2] == (where == 'lds')
        actor, layer = _nets(env, 32, 16, seed=8)
        outs.append(_run(env, actor, layer, 40))
        env.close()
    for k in ('obs', 'act', 'logp', 'rew', 'done', 'flags', 'term', 'c_rows', 'carry', 'acc'):
        assert torch.equal(outs[0][k], outs[1][k]), k
    monkeypatch.setenv('SCG_SAFE_WEIGHTS', 'lds')
    env = _env(H=128, hc=150, seed=21)
    b, w, il = _safe_explorer.launch_plan(env._lib, 4)
    assert w == 0 and il and b > 163840
    actor, layer = _nets(env, 128, 150, seed=8)
    with pytest.raises(L.ScgError, match='LDS'):
        _run(env, actor, layer, 4)
    monkeypatch.delenv('SCG_SAFE_WEIGHTS')
    assert _safe_explorer.launch_plan(env._lib, 4)[1:] == (4, False)
    o = _run(env, actor, layer, 4)                                  # the launcher's own choice: memory placement
    assert torch.isfinite(o['act']).all()
    env.close()


def test_other_envs_do_not_see_one_envs_perturbation():
    """Changing one env's constraint-value input (its carry) changes that env's outputs and leaves every other env's bit for bit."""
    outs = []
    for bump in (False, True):
        env = _env(H=128, hc=150, seed=33)
        actor, layer = _nets(env, 128, 150, slack=SLACK_Q2, golden=True)
        carry = env.spec.state_constraint_values(env.out.state.t()).to(torch.float32)
        if bump:
            carry[77] += 0.75
        outs.append(_run(env, actor, layer, 16, carry=carry))
        env.close()
    keep = torch.ones(N, dtype=torch.bool)
    keep[77] = False
    for k in ('obs', 'act', 'logp', 'rew', 'done', 'term', 'c_rows'):
        assert torch.equal(outs[0][k][:, keep.to(outs[0][k].device)], outs[1][k][:, keep.to(outs[1][k].device)]), k
    assert not torch.equal(outs[0]['act'][:, 77], outs[1]['act'][:, 77])


def test_controller_fused_rollout_learns_resumes_and_evaluates():
    """make('safe_explorer_ppo', ..., fused_rollout=True) with the shipped pre-trained safety layer: the PPO phase collects through
    scg_rollout_safe, total_steps is right, the layer never moves, a save / load round trip resumes; run() of the shipped second-phase
    model evaluates through the deterministic kernel and meets the eager path's bar.  An unservable shape warns and falls back."""
    import tempfile
    from safe_control_gym_amd.registration import load_task, make
    env_id, cfg = load_task('quadrotor_2D_track')
    env_func = functools.partial(make, env_id, output_dir='/tmp/scg', seed=1337, **cfg)
    ship = dict(hidden_dim=128, constraint_hidden_dim=150, use_gae=True, rollout_batch_size=256, rollout_steps=8, opt_epochs=1,
                mini_batch_size=512, constraint_slack=SLACK_Q2, constraint_batch_size=256, fused_rollout=True)
    pre = os.path.join(MODELS, 'safe_explorer_ppo_pretrain_quadrotor_2D_track.pt')
    with tempfile.TemporaryDirectory() as out:
        ctrl = make('safe_explorer_ppo', env_func, training=True, checkpoint_path=os.path.join(out, 'model_latest.pt'), output_dir=out,
                    seed=2, pretraining=False, pretrained=pre, max_env_steps=3 * 256 * 8, log_interval=256 * 8, **ship)
        ctrl.reset()
        assert ctrl.env.safety_shape == (128, 'tanh', 150) and ctrl.impl._fused_safe == (128, 'tanh', 150)
        layer0 = {k: v.clone() for k, v in ctrl.safety_layer.constraint_models.state_dict().items()}
        hist = ctrl.learn()
        assert ctrl.total_steps == 3 * 256 * 8 and len(hist) == 3
        for k, v in ctrl.safety_layer.constraint_models.state_dict().items():
            assert torch.equal(v, layer0[k]), k
        assert torch.isfinite(ctrl.impl.c).all() and ctrl.impl.c.shape == (256, 12)
        st = torch.load(os.path.join(out, 'model_latest.pt'), weights_only=False)
        assert {'agent', 'safety_layer', 'c', 'obs', 'total_steps'} <= set(st)
        res = make('safe_explorer_ppo', env_func, training=True, checkpoint_path=os.path.join(out, 'res.pt'), output_dir=out, seed=2,
                   pretraining=False, pretrained=pre, max_env_steps=4 * 256 * 8, **ship)
        res.reset()
        res.load(os.path.join(out, 'model_latest.pt'))
        assert res.total_steps == 3 * 256 * 8 and torch.equal(res.impl.c.cpu(), st['c'])
        res.learn()
        assert res.total_steps == 4 * 256 * 8
        ctrl.close(); res.close()
    eval_func = functools.partial(make, env_id, output_dir='/tmp/scg', seed=1337, **dict(cfg, randomized_init=False))
    t = make('safe_explorer_ppo', eval_func, training=False, output_dir='/tmp/scg', seed=2, pretraining=False, **ship)
    t.load(os.path.join(MODELS, 'safe_explorer_ppo_model_quadrotor_2D_track.pt'))
    r = t.run(n_episodes=16)
    assert t._run_env.safety_shape == (128, 'tanh', 150) and hasattr(t._run_env, '_eval_safe')
    assert r['ep_lengths'].mean() > 200 and r['ep_returns'].mean() > 150, r
    t.close()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        u = make('safe_explorer_ppo', env_func, training=True, output_dir='/tmp/scg', seed=2, pretraining=False, pretrained=pre,
                 **dict(ship, hidden_dim=48))                        # hidden 48: no fused actor tile
    assert any('eager collector' in str(x.message) for x in w)
    assert u.impl._fused_safe is None and u.env.safety_shape is None
    u.close()
