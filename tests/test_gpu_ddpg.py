"""The fused DDPG step (csrc/scg_ddpg.hip) against the reference's answers and the eager update, its reproducibility, the noisy-action
kernel against a float64 sequential recurrence, and the `ddpg` controller end to end."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from safe_control_gym_amd import _ddpg, ddpg
from tests.test_ddpg_cpu import CASES, case_agent, golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def ring_of(batches, device=DEV):
    """A DeviceReplay holding the batches back to back (rows k B .. (k + 1) B - 1 = batch k)."""
    cat = {k: torch.cat([b[k] for b in batches]).to(device) for k in ('obs', 'act', 'rew', 'next_obs', 'mask')}
    n, obs_dim = cat['obs'].shape
    buf = ddpg.DeviceReplay(n, obs_dim, cat['act'].shape[1], torch.device(device))
    buf.push(cat['obs'], cat['act'], cat['rew'], cat['next_obs'], cat['mask'])
    return buf


def fused_steps(ag, buf, B, idx_rows):
    """One fused step per index vector (d_idx_in); the steps' statistics."""
    out = []
    for idx in idx_rows:
        F = ag._fused_args(buf, B, idx=idx)
        ag.fused_step(F)
        torch.cuda.synchronize()
        out.append(F['stats'].tolist())
    return out


def random_ring(obs_dim, act_dim, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    b = {'obs': torch.randn(n, obs_dim, generator=g), 'act': torch.rand(n, act_dim, generator=g) * 2 - 1,
         'rew': torch.randn(n, 1, generator=g), 'next_obs': torch.randn(n, obs_dim, generator=g),
         'mask': (torch.rand(n, 1, generator=g) > 0.1).float()}
    return ring_of([b])


def agent_pair(obs_dim, hidden, act_dim, act, seed=3):
    cfg = ddpg.DDPGConfig(hidden_dim=hidden, activation=act)
    torch.manual_seed(seed)
    f = ddpg.DDPGAgent(obs_dim, act_dim, -np.ones(act_dim), np.ones(act_dim), cfg, DEV)
    cfg_e = ddpg.DDPGConfig(hidden_dim=hidden, activation=act, extra={'fused_update': False})
    e = ddpg.DDPGAgent(obs_dim, act_dim, -np.ones(act_dim), np.ones(act_dim), cfg_e, DEV)
    e.ac.load_state_dict(f.ac.state_dict())
    e.ac_targ.load_state_dict(f.ac_targ.state_dict())
    assert f.use_fused and not e.use_fused
    return f, e


def batch_at(buf, idx):
    return {'obs': buf.obs[idx], 'act': buf.act[idx], 'rew': buf.rew[idx], 'next_obs': buf.next_obs[idx], 'mask': buf.mask[idx]}


def eager_grads(e):
    return torch.cat([p.grad.reshape(-1) for p in list(e.ac.actor.parameters()) + list(e.ac.q.parameters())])


@pytest.mark.parametrize('name', CASES)
def test_fused_step_reproduces_the_reference(name):
    z = golden()
    p = f'agent/{name}'
    ag, batches = case_agent(z, name, device=DEV)
    assert ag.use_fused
    B = batches[0]['obs'].shape[0]
    buf = ring_of(batches)
    stats = fused_steps(ag, buf, B, [torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device=DEV) for k in range(3)])
    np.testing.assert_allclose(stats, z[f'{p}/stats'], rtol=1e-4, atol=1e-5)
    for mod, pre in ((ag.ac, 'ac'), (ag.ac_targ, 'ac_targ')):
        for n, t in mod.state_dict().items():
            np.testing.assert_allclose(t.cpu().numpy(), z[f'{p}/final/{pre}/{n}'], rtol=1e-4, atol=1e-5, err_msg=f'{pre}.{n}')
    assert ag._flat['steps'].tolist() == [3.0, 3.0]
    sd = ag.state_dict()            # the flat moments in torch.optim's layout (checkpoints)
    for oname, module in (('actor_opt', ag.ac.actor), ('critic_opt', ag.ac.q)):
        names = {id(t): n for n, t in module.named_parameters()}
        for i, prm in enumerate(getattr(ag, oname).param_groups[0]['params']):
            st = sd[oname]['state'][i]
            assert float(st['step']) == 3.0
            np.testing.assert_allclose(st['exp_avg'].cpu().numpy(), z[f'{p}/final/{oname}/{names[id(prm)]}/exp_avg'], rtol=1e-3, atol=1e-6)


SHAPES = [(24, 128, 4, 'relu'), (1, 32, 1, 'tanh'), (7, 96, 1, 'relu'), (17, 96, 3, 'tanh'), (27, 64, 4, 'leaky_relu'), (12, 128, 2, 'relu')]


@pytest.mark.parametrize('shape', SHAPES)
def test_fused_gradients_match_eager(shape):
    obs_dim, hidden, act_dim, act = shape
    B = 4096 if shape == SHAPES[0] else 256
    f, e = agent_pair(obs_dim, hidden, act_dim, act)
    buf = random_ring(obs_dim, act_dim, 2 * B)
    idx = torch.randint(0, 2 * B, (B,), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    st = fused_steps(f, buf, B, [idx])[0]
    ref = e.update(batch_at(buf, idx.long()))
    np.testing.assert_allclose(st, [ref['policy_loss'], ref['critic_loss']], rtol=1e-4, atol=1e-6)
    g, ge = f._flat['g'], eager_grads(e)
    scale = ge.abs().max().item()
    torch.testing.assert_close(g, ge, rtol=1e-3, atol=1e-4 * scale)


def test_fused_parameters_match_eager_after_8_steps():
    f, e = agent_pair(24, 128, 4, 'relu')
    B = 4096
    buf = random_ring(24, 4, 2 * B, seed=5)
    gen = torch.Generator(DEV).manual_seed(2)
    rows = [torch.randint(0, 2 * B, (B,), dtype=torch.int32, device=DEV, generator=gen) for _ in range(8)]
    fused_steps(f, buf, B, rows)
    for idx in rows:
        e.update(batch_at(buf, idx.long()))
    pf = torch.cat([t.reshape(-1) for t in f.ac.state_dict().values()])
    pe = torch.cat([t.reshape(-1) for t in e.ac.state_dict().values()])
    d = (pf - pe).abs()
    # Adam's first steps move a weight by ~lr sign(g): a gradient that is ~0 in both may differ in sign, bounded by 2 lr per step
    assert float(d.max()) <= 2 * 8 * 1e-3 + 1e-6
    assert float((d > 1e-4).float().mean()) < 1e-3, float((d > 1e-4).float().mean())


def test_fused_step_is_reproducible_and_update_n_equals_n_steps():
    def run(mode):
        torch.manual_seed(9)
        cfg = ddpg.DDPGConfig(hidden_dim=128, activation='relu')
        ag = ddpg.DDPGAgent(24, 4, -np.ones(4), np.ones(4), cfg, DEV)
        ag._flat['seed'] = 1234
        buf = random_ring(24, 4, 8192, seed=3)
        F = ag._fused_args(buf, 4096)
        if mode == 'single':
            for _ in range(4):
                ag.fused_step(F)
        elif mode == 'n':
            ag.fused_step(F, 4)
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ag.fused_step(F, 4)
            g.replay()
        torch.cuda.synchronize()
        return torch.cat([ag._flat['p'], ag._flat['targ'], ag._flat['m'], ag._flat['v'], F['acc']]).cpu(), int(ag._flat['counter'].item())
    a, ca = run('single')
    b, cb = run('single')
    c, cc = run('n')
    d, cd = run('graph')
    assert ca == cb == cc == cd == 4
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


# ---------------------------------------------------------------- noisy actions
def ou_reference(eps, x0, calls0, start, end, inc, theta=0.15, dt=1e-2):
    """The reference's OrnsteinUhlenbeckProcess.sample, once per env in env order, in float64."""
    x = np.array(x0, np.float64)
    out = np.empty_like(eps, dtype=np.float64)
    for i in range(eps.shape[0]):
        v = start + (calls0 + i) * inc
        sd = min(v, end) if end > start else max(v, end)
        x = x + theta * (0 - x) * dt + sd * np.sqrt(dt) * eps[i]
        out[i] = x
    return out


def noisy_setup(obs_dim=24, hidden=128, act_dim=4):
    torch.manual_seed(4)
    ag = ddpg.DDPGAgent(obs_dim, act_dim, -np.ones(act_dim) * 2, np.ones(act_dim), ddpg.DDPGConfig(hidden_dim=hidden), DEV)
    D = _ddpg.lib(obs_dim, hidden, act_dim, 'relu')
    return ag, D


def call_noisy(ag, D, obs, noise, eps=None, uniform=0, counter=None):
    lo, hi = ag.act_bounds()
    out = torch.empty(obs.shape[0], ag.act_dim, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _ddpg.check(D, D.scg_ddpg_noisy_act(ag._flat['p'].data_ptr(), C.byref(ag._flat['actor']), lo, hi, obs.data_ptr(), obs.shape[0], 77,
                                        counter.data_ptr() if counter is not None else None, uniform,
                                        C.byref(noise.struct) if noise is not None else None, eps.data_ptr() if eps is not None else None,
                                        out.data_ptr(), st))
    if noise is not None:
        _ddpg.check(D, D.scg_ddpg_noise_commit(C.byref(noise.struct), st))
    return out


@pytest.mark.parametrize('N,steps', [(16384, 4), (32768, 2)])
def test_noisy_action_equals_the_sequential_ou_recurrence(N, steps):
    """32 768 envs: every workgroup past env 23 090 starts its scan at a truncated window (terms weighing less than 2^-50 dropped,
    the carry decayed by a^W0) — the branch the single-launch scan exists for; 16 384: every workgroup folds all envs in front of it."""
    ag, D = noisy_setup()
    window = int(np.ceil(50 * np.log(2) / -np.log(1 - 0.15 * 1e-2)))
    assert (N > window) == (N == 32768)
    cfg = {'func': 'OrnsteinUhlenbeckProcess', 'std': {'func': 'LinearSchedule', 'args': 0.3, 'end': 0.05, 'steps': 50000}}
    noise = ddpg.DeviceNoise(cfg, 4, torch.device(DEV))
    rng = np.random.default_rng(0)
    x, calls = np.zeros(4), 0
    # contractive recurrence evaluated in float64 on both sides: the only float32 rounding is the action's (|a| <= 2 + |x|: ~3e-7);
    # the actor's MFMA-vs-torch difference is ~1e-6.  1e-5 leaves a margin and is tighter than the 1e-4 ceiling.
    for t in range(steps):
        obs = torch.randn(N, 24, device=DEV)
        eps = rng.standard_normal((N, 4))
        got = call_noisy(ag, D, obs, noise, eps=torch.as_tensor(eps, dtype=torch.float32, device=DEV))
        ref_x = ou_reference(eps.astype(np.float32).astype(np.float64), x, calls, 0.3, 0.05, (0.05 - 0.3) / 50000)
        x, calls = ref_x[-1], calls + N
        want = ag.ac.act(obs).double().cpu().numpy() + ref_x
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-5)
    np.testing.assert_allclose(noise.x_prev[:4].cpu().numpy(), x, rtol=0, atol=1e-12)
    assert int(noise.calls.item()) == N * steps
    sd = noise.state_dict()
    # (65 536 calls: past the schedule's 50 000 steps, the std stays at its end value)
    assert set(sd) == {'x_prev', 'std'} and abs(sd['std']['current'] - max(0.3 + N * steps * (0.05 - 0.3) / 50000, 0.05)) < 1e-12


def test_noisy_action_gaussian_uniform_and_deterministic_modes():
    ag, D = noisy_setup()
    N = 5000
    obs = torch.randn(N, 24, device=DEV)
    cfg = {'func': 'GaussianProcess', 'std': {'func': 'LinearSchedule', 'args': 0.3, 'end': 0.05, 'steps': 4000}}
    noise = ddpg.DeviceNoise(cfg, 4, torch.device(DEV))
    eps = torch.randn(N, 4, device=DEV)
    got = call_noisy(ag, D, obs, noise, eps=eps)
    c = np.arange(N)
    sd = np.maximum(0.3 + c * (0.05 - 0.3) / 4000, 0.05)
    want = ag.ac.act(obs).double().cpu().numpy() + eps.double().cpu().numpy() * sd[:, None]
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-5)
    assert int(noise.calls.item()) == N
    # warm-up: action_space.sample(), inside the bounds, the process does not advance
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    u = call_noisy(ag, D, obs, noise, uniform=1, counter=cnt).cpu()
    assert (u >= -2).all() and (u < 1).all() and float(u.std()) > 0.5 and int(noise.calls.item()) == N
    # the deterministic actor (scg_ddpg_act)
    torch.testing.assert_close(ag.act(obs), ag.ac.act(obs), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(call_noisy(ag, D, obs, None), ag.ac.act(obs), rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------- the controller
def test_ddpg_controller_end_to_end():
    from safe_control_gym_amd.registration import load_task, make
    env_id, cfg = load_task('quadrotor_2D_track')
    env_func = functools.partial(make, env_id, output_dir='/tmp/scg', **cfg)
    kw = dict(rollout_batch_size=2048, hidden_dim=128, warm_up_steps=4096, train_interval=2048, train_batch_size=512,
              updates_per_step=8, max_env_steps=2048 * 6, max_buffer_size=100000)
    with tempfile.TemporaryDirectory() as out:
        ctrl = make('ddpg', env_func, training=True, output_dir=out, seed=2, **kw)
        assert ctrl.impl.agent.use_fused and ctrl.impl._fused_collect
        ctrl.reset()
        res = [ctrl.train_step() for _ in range(6)]
        assert [r.get('updates', 0) for r in res] == [0, 0, 8, 8, 8, 8]
        for r in res[2:]:
            assert np.isfinite(r['policy_loss']) and np.isfinite(r['critic_loss'])
        ev = ctrl.run(n_episodes=8)
        assert set(ev) == {'ep_returns', 'ep_lengths', 'constraint_violation', 'mse'} and ev['ep_returns'].shape == (8,)
        path = os.path.join(out, 'ddpg.pt')
        ctrl.save(path, save_buffer=True)
        st = torch.load(path, weights_only=False)
        assert set(st['agent']) >= {'ac', 'ac_targ', 'actor_opt', 'critic_opt'} and set(st['noise_process']) == {'x_prev', 'std'}
        assert {'obs_normalizer', 'reward_normalizer', 'total_steps', 'obs', 'random_state', 'env_random_state', 'buffer'} <= set(st)
        again = make('ddpg', env_func, training=True, output_dir=out, seed=2, **dict(kw, max_env_steps=2048 * 9))
        again.load(path)
        for _ in range(3):
            a, b = ctrl.train_step(), again.train_step()
            assert a['policy_loss'] == b['policy_loss'] and a['critic_loss'] == b['critic_loss']
        for k, v in ctrl.agent.ac.state_dict().items():
            assert torch.equal(v, again.agent.ac.state_dict()[k]), k
        assert torch.equal(ctrl.impl.noise_process.x_prev, again.impl.noise_process.x_prev)
        ctrl.close()
        again.close()


def test_fused_collector_reproduces_the_reference_buffer():
    """The fused collector (scg_ddpg_noisy_act + env step + scg_ddpg_push, as DDPG._collect_body_fused enqueues them) against the
    REFERENCE's own DDPG.train_step (tests/golden/make_ddpg_collector.py), fed the reference's N(0, 1) noise draws through eps_in and its
    actor weights: the actions (MFMA actor + the device OU scan carried across vector steps), the replay ring after the wrap and the
    process's state afterwards.  The two warm-up steps draw their own uniform actions (the replay ignores them, and their rows are
    overwritten by the wrap)."""
    from tests.test_ddpg_cpu import COLLECTOR, collector_setup
    G = np.load(COLLECTOR)
    env, d = collector_setup(DEV, G, {'cuda_graphs': False})
    assert d._fused_collect and isinstance(d.noise_process, ddpg.DeviceNoise)
    W, N = int(G['warm_vector_steps']), 4
    draws = torch.as_tensor(G['noise/draws'], dtype=torch.float32, device=DEV)
    acts = G['transitions/act']
    for t in range(acts.shape[0]):
        d._collect_body_fused(t < W, eps_in=None if t < W else draws[(t - W) * N:(t - W + 1) * N].contiguous())
        d.buffer.advance_host(N)
    torch.cuda.synchronize()
    np.testing.assert_allclose(env.seen_act[W:].cpu().numpy(), acts[W:], rtol=0, atol=1e-5)
    assert [d.buffer.pos, d.buffer.size] == G['buffer/pos_size'].tolist()
    for k in ('obs', 'act', 'rew', 'next_obs', 'mask'):
        got = getattr(d.buffer, k).cpu().numpy().reshape(G[f'buffer/{k}'].shape)
        np.testing.assert_allclose(got, G[f'buffer/{k}'], rtol=0, atol=1e-5 if k == 'act' else 1e-6, err_msg=k)
    sd = d.noise_process.state_dict()
    # the kernel reads its draws as float32 (as Philox hands them over): each of the 152 OU terms carries std sqrt(dt) |eps| 2^-24
    # ~ 1e-9 of input rounding, so the float64 carry agrees with the reference's to ~1e-8, not to float64 precision
    np.testing.assert_allclose(sd['x_prev'], G['noise/x_prev'], rtol=0, atol=1e-7)
    assert abs(sd['std']['current'] - float(G['noise/std_current'])) < 1e-12
