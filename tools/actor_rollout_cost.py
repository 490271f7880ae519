#!/usr/bin/env python3
"""Cost of the fused SAC / DDPG actor rollout on one GPU -> profiles/actor_rollout_cost.json.  One deterministic evaluation of 250
control steps (ppo.evaluate: reset, the rollout, the per-env totals and their reduction) at 256, 4 096 and 65 536 envs, for SAC
(Quadrotor 3D tracking, hidden 128, relu) and DDPG (CartPole, hidden 64, relu; episodes lengthened to 250 steps,
tests/actor_rollout_cases.py), same process, same device, interleaved repeats, medians of device-event times:
  (a) fused          ONE scg_rollout_actor launch (HipVecEnv(policy=(H, act, kind)), ppo.evaluate(policy=agent.actor_struct()));
  (b) eager_graph    the eager evaluation loop as ppo.evaluate runs it: 250 x (scg_sac_act | scg_ddpg_act, env step, totals), captured
                     once and replayed as one HIP graph;
  (c) eager_bare     the same loop launched op by op (use_graph=False);
  (d) ppo_fused      scg_rollout_policy on the same task with a PPO actor of the same width and activation (deterministic): the heads
                     differ by one activation layer and a tanhf.
The eager loop's code is not touched by the fused path; each path has an env of its own (same task, same seed).

usage: actor_rollout_cost.py [--out profiles/actor_rollout_cost.json] [--reps 7] [--envs 256 4096 65536]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from safe_control_gym_amd import _lib as L  # noqa: E402
from safe_control_gym_amd import ddpg  # noqa: E402
from safe_control_gym_amd.ppo import evaluate  # noqa: E402
from safe_control_gym_amd.sac import SACAgent, SACConfig  # noqa: E402
from safe_control_gym_amd.vec_env import HipVecEnv  # noqa: E402
from tests import actor_rollout_cases as arc  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3            # us


def ppo_policy(obs_dim, hidden, nu, act, dev):
    """(flat parameters, _lib.Policy, deterministic) of a PPO actor obs -> hidden -> hidden -> nu with nn.Linear's default init."""
    torch.manual_seed(5)
    layers = [torch.nn.Linear(obs_dim, hidden), torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, nu)]
    parts = [p.detach().reshape(-1) for fc in layers for p in (fc.weight, fc.bias)] + [torch.zeros(nu)]
    offs = np.concatenate([[0], np.cumsum([p.numel() for p in parts])])
    flat = torch.cat(parts).to(dev).contiguous()
    pol = L.Policy(d_params=flat.data_ptr(), W1=int(offs[0]), b1=int(offs[1]), W2=int(offs[2]), b2=int(offs[3]), W3=int(offs[4]),
                   b3=int(offs[5]), logstd_off=int(offs[6]), hidden=hidden, activation=L.POLICY_ACTS[act], deterministic=1)
    return flat, pol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'actor_rollout_cost.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--envs', type=int, nargs='*', default=[256, 4096, 65536])
    a = ap.parse_args()
    dev = torch.device('cuda', torch.cuda.current_device())
    rows = []
    for task, kind, hidden, act in arc.COST_CASES:
        env_id, cfg = arc.cost_task_config(task)
        for N in a.envs:
            mk = lambda policy: HipVecEnv(env_id, N, seed=7, return_numpy=False, policy=policy, **cfg)   # noqa: E731
            envs = dict(fused=mk((hidden, act, kind)), eager_graph=mk(None), eager_bare=mk(None), ppo_fused=mk((hidden, act)))
            spec = envs['fused'].spec
            assert spec.max_episode_steps == arc.COST_STEPS and envs['fused'].actor_kind == kind
            lo, hi = (np.asarray(v, np.float32).reshape(-1) for v in (spec.action_space.low, spec.action_space.high))
            torch.manual_seed(3)
            if kind == 'sac':
                agent = SACAgent(spec.obs_dim, spec.nu, torch.tensor(lo, device=dev), torch.tensor(hi, device=dev),
                                 SACConfig(hidden_dim=hidden, activation=act), dev)
            else:
                agent = ddpg.DDPGAgent(spec.obs_dim, spec.nu, lo, hi, ddpg.DDPGConfig(hidden_dim=hidden, activation=act), dev)
            assert agent.use_fused
            det, actor = agent.deterministic_policy(), agent.actor_struct()
            flat, pol = ppo_policy(spec.obs_dim, hidden, spec.nu, act, dev)
            res = {}
            fns = dict(fused=lambda: res.__setitem__('fused', evaluate(det, envs['fused'], policy=actor)),
                       eager_graph=lambda: res.__setitem__('eager_graph', evaluate(det, envs['eager_graph'], use_graph=True)),
                       eager_bare=lambda: res.__setitem__('eager_bare', evaluate(det, envs['eager_bare'], use_graph=False)),
                       ppo_fused=lambda: res.__setitem__('ppo_fused', evaluate(None, envs['ppo_fused'], policy=pol)))
            for fn in fns.values():                                 # warm-up: buffers, kernel attributes, the graph capture
                fn(); fn()
            t = {k: [] for k in fns}
            for _ in range(a.reps):                                 # interleaved
                for k, fn in fns.items():
                    t[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = dict(task=task, kind=kind, hidden=hidden, activation=act, envs=N, steps=arc.COST_STEPS, reps=a.reps,
                       fused_us=med['fused'], eager_graph_us=med['eager_graph'], eager_bare_us=med['eager_bare'], ppo_fused_us=med['ppo_fused'],
                       eager_graph_over_fused=med['eager_graph'] / med['fused'], eager_bare_over_fused=med['eager_bare'] / med['fused'],
                       fused_over_ppo_fused=med['fused'] / med['ppo_fused'],
                       mean_length={k: res[k]['ep_length'] for k in res}, spread_us={k: [min(v), max(v)] for k, v in t.items()})
            print(json.dumps(row), flush=True)
            rows.append(row)
            for e in envs.values():
                e.close()
            del envs, agent, det, actor, flat, pol, fns, res
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0),
                   'method': 'medians of device-event times around one ppo.evaluate call (reset + rollout + totals), interleaved repeats, same '
                             'process; each path on an env of its own', 'rows': rows}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
