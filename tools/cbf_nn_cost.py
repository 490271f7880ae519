#!/usr/bin/env python3
"""What the cbf_nn safety filter costs on the device, measured, not promised.

  evaluation   one 250-step filtered evaluation launch (scg_rollout_cbf_nn, deterministic actor, blend = -1) at 256 / 4 096 / 65 536 envs
               against scg_rollout_cbf (the plain filter, same actor, same task, same box) and against the per-step loop a caller
               without the fused kernel runs: per control step the actor and the residual network in PyTorch, one
               scg_cbf_nn_certify launch and one step launch
  learn        one learn() episode (reset, one 250-step launch, the push, train_iterations = 200 Adam steps) at num_envs 1 / 256,
               and the launch alone
  is_cbf       the default grid (26^4 = 456 976 states): one scg_cbf_nn_certify launch, against cbf's scg_cbf_certify

Setup: the reference's examples/cbf task (tests/golden/cbf_nn_settings.json, randomised initial states) with its shipped 64-64 tanh
actor and the fixture's residual weights.  Device-event times around each piece, medians of --reps interleaved repeats after --warmup
rounds (the learn episode: wall clock around learn(), synchronised).  Writes profiles/cbf_nn_cost.json (or --out).

usage: cbf_nn_cost.py [--reps 5] [--warmup 2] [--envs 256 4096 65536] [--steps 250] [--out profiles/cbf_nn_cost.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import cbf_nn_cases as CN  # noqa: E402
from tests import cbf_nn_model as NM  # noqa: E402


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def stats(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'all': [float(x) for x in v]}


def shipped_actor(dev, shape):
    from safe_control_gym_amd import _cbf
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd.ppo import MLPActor
    G = np.load(os.path.join(CN.GOLDEN, 'cbf.npz'))
    parts = [np.asarray(G[f'actor/actor.pi_net.fcs.{i}.{k}'], dtype=np.float32).reshape(-1) for i in range(3) for k in ('weight', 'bias')]
    parts.append(np.asarray(G['actor/actor.logstd'], dtype=np.float32).reshape(-1))
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    flat = torch.tensor(np.concatenate(parts), device=dev)
    pol = L.Policy(d_params=flat.data_ptr(), W1=int(offs[0]), b1=int(offs[1]), W2=int(offs[2]), b2=int(offs[3]), W3=int(offs[4]), b3=int(offs[5]),
                   logstd_off=int(offs[6]), hidden=shape[0], activation=L.POLICY_ACTS[shape[1]], deterministic=1)
    module = MLPActor(4, 1, [shape[0], shape[0]], shape[1]).to(dev)
    at = 0
    with torch.no_grad():
        for t in [t for fc in module.pi_net.fcs for t in (fc.weight, fc.bias)] + [module.logstd]:
            t.copy_(flat[at:at + t.numel()].view_as(t))
            at += t.numel()
    return flat, pol, _cbf.actor_ptrs_of_policy(pol), module


def make_filter(idx, S, D, **over):
    from safe_control_gym_amd.registration import make
    env_id, cfg = CN.task_config(False)
    keys = ('slope', 'soft_constrained', 'slack_weight', 'slack_tolerance') if idx == 'cbf' else tuple(S['sf_config'])
    sf = make(idx, partial(make, env_id, **cfg), **dict({k: S['sf_config'][k] for k in keys}, **over))
    if idx == 'cbf_nn':
        sf.mlp.load_state_dict({k: torch.tensor(D['mlp/' + k]) for k in NM.KEYS})
    return sf


def main():
    from safe_control_gym_amd import _cbf_nn
    from safe_control_gym_amd.vec_env import HipVecEnv
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--envs', type=int, nargs='+', default=[256, 4096, 65536])
    ap.add_argument('--steps', type=int, default=250)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cbf_nn_cost.json'))
    a = ap.parse_args()
    S = CN.settings()
    D = np.load(os.path.join(CN.GOLDEN, 'cbf_nn.npz'))
    shape = (S['algo_config']['hidden_dim'], S['algo_config']['activation'])
    env_id, cfg = CN.task_config(False)
    K = a.steps
    res = {'device': torch.cuda.get_device_name(0), 'steps': K, 'reps': a.reps, 'warmup': a.warmup, 'evaluation': [], 'learn': []}
    for n in a.envs:
        env = HipVecEnv(env_id, n, seed=1, return_numpy=False, policy=shape, cbf_nn=True, **cfg)
        plain_env = HipVecEnv(env_id, n, seed=1, return_numpy=False, policy=shape, cbf=True, **cfg)
        step_env = HipVecEnv(env_id, n, seed=1, return_numpy=False, policy=shape, cbf_nn=True, **cfg)
        sf, plain = make_filter('cbf_nn', S, D).attach(env), make_filter('cbf', S, D).attach(plain_env)
        flat, pol, actor, module = shipped_actor(env.device, shape)
        f = dict(device=env.device, dtype=torch.float32)
        u8 = dict(device=env.device, dtype=torch.uint8)
        o = {'obs': torch.zeros(K + 1, n, 4, **f), 'act': torch.zeros(K, n, 1, **f), 'logp': torch.zeros(K, n, **f), 'rew': torch.zeros(K, n, **f),
             'done': torch.zeros(K, n, **u8), 'flags': torch.zeros(K, n, **u8), 'rows': torch.zeros(K, n, 4, **f), 'applied': torch.zeros(K, n, **f),
             'ab': torch.zeros(K, n, 2, **f)}
        params, residual = sf.params(), sf.residual(env.device)

        def fused_nn():
            env.reset_tensors()
            env.rollout_cbf_nn(actor, params, residual, K, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'], o['rows'], o['applied'],
                               o['ab'], deterministic=True, blend=-1.0)

        def fused_plain():
            plain_env.reset_tensors()
            plain_env.rollout_cbf(actor, params, K, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'], o['rows'], o['applied'],
                                  deterministic=True)

        @torch.no_grad()
        def per_step():
            obs = step_env.reset_tensors()
            for _ in range(K):
                act = module.pi_net(obs)
                sf.mlp(obs[:, :4])                         # the residual in PyTorch, as upstream's extract_a_b per step
                cert, _, feas, _ = step_env.certify_nn_tensors(params, residual, obs[:, :4].contiguous(), act.reshape(-1).contiguous())
                obs = step_env.step_tensors(torch.where(feas.bool(), cert, act.reshape(-1)).unsqueeze(-1)).obs
        run = {'cbf_nn': fused_nn, 'cbf': fused_plain, 'per_step': per_step}
        for _ in range(a.warmup):
            for k in run:
                timed(run[k])
        t = {k: [] for k in run}
        for _ in range(a.reps):
            for k in run:                                  # interleaved
                t[k].append(timed(run[k]))
        case = {'envs': n, 'tiles': _cbf_nn.rollout_tiles(4, shape[0], n)}
        for k, v in t.items():
            case[k + '_ms'] = stats(v)
        case['cbf_nn_over_cbf'] = case['cbf_nn_ms']['median'] / case['cbf_ms']['median']
        case['per_step_over_cbf_nn'] = case['per_step_ms']['median'] / case['cbf_nn_ms']['median']
        print(f"evaluation {n} envs x {K} steps (G = {case['tiles']}): cbf_nn {case['cbf_nn_ms']['median']:.2f} ms, cbf {case['cbf_ms']['median']:.2f} ms "
              f"(x{case['cbf_nn_over_cbf']:.2f}), per-step loop {case['per_step_ms']['median']:.2f} ms (x{case['per_step_over_cbf_nn']:.2f})")
        res['evaluation'].append(case)
        if n == a.envs[0]:                                 # is_cbf on the default grid
            from safe_control_gym_amd.cbf import state_grid
            g = torch.tensor(state_grid(sf.state_limits), dtype=torch.float32, device=env.device)
            ones = torch.ones(len(g), **f)
            run2 = {'cbf_nn': lambda: env.certify_nn_tensors(params, residual, g, ones), 'cbf': lambda: plain_env.certify_tensors(plain.params(), g, ones)}
            t2 = {k: [] for k in run2}
            for r in range(a.warmup + a.reps):
                for k in run2:
                    v = timed(run2[k])
                    if r >= a.warmup:
                        t2[k].append(v)
            wall = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    sf.is_cbf()
                wall.append((time.perf_counter() - t0) * 1e3)
            res['is_cbf'] = {'grid_states': int(len(g)), 'cbf_nn_launch_ms': stats(t2['cbf_nn']), 'cbf_launch_ms': stats(t2['cbf']),
                             'cbf_nn_wall_ms': stats(wall)}
            print(f"is_cbf grid ({len(g)} states): cbf_nn launch {np.median(t2['cbf_nn']):.3f} ms, cbf launch {np.median(t2['cbf']):.3f} ms, "
                  f"is_cbf() wall {np.median(wall):.1f} ms")
        for e in (env, plain_env, step_env):
            e.close()
        del flat, pol
    for n in (1, 256):                                     # one learn() episode
        sf = make_filter('cbf_nn', S, D, num_episodes=1, max_num_steps=K)
        wall, launch = [], []
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sf.learn(num_envs=n)
            torch.cuda.synchronize()
            if r >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                launch.append(timed(lambda: sf.rollout(sf._learn_env, K, uniform=True, blend=0.0)))
        case = {'num_envs': n, 'episode_wall_ms': stats(wall), 'launch_ms': stats(launch), 'train_iterations': sf.train_iterations}
        print(f"learn episode, num_envs {n}: {np.median(wall):.1f} ms wall ({sf.train_iterations} Adam steps included), the {K}-step launch "
              f"{np.median(launch):.2f} ms")
        res['learn'].append(case)
        sf.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fjson:
        json.dump(res, fjson, indent=1)
        fjson.write('\n')


if __name__ == '__main__':
    main()
