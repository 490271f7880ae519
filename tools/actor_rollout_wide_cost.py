#!/usr/bin/env python3
"""Cost of the fused SAC / DDPG actor rollout at hidden width 256 on one GPU -> profiles/actor_rollout_wide_cost.json.  One
deterministic evaluation of 250 control steps (ppo.evaluate: reset, the rollout, the per-env totals and their reduction) at 256,
4 096 and 65 536 envs (--envs adds sizes: the geometry threshold is where the two fused curves cross), for SAC (Quadrotor 3D tracking,
256 relu) and DDPG (CartPole, 256 relu; episodes lengthened to 250 steps, tests/actor_rollout_wide_cases.py), same process, same
device, interleaved repeats, medians of device-event times:
  (a) fused_g1       ONE scg_rollout_actor launch with one column tile per workgroup (SCG_ROLLOUT_WIDE_TILES=1: 32 envs per workgroup);
  (b) fused_g8       the same with eight (SCG_ROLLOUT_WIDE_TILES=8: 256 envs per workgroup);
  (c) eager_graph    the eager evaluation loop of the same (non-fused, PyTorch) agent as ppo.evaluate runs it: 250 x (actor forward, env
                     step, totals), captured once and replayed as one HIP graph.
The agent is the ordinary 256-wide one; the fused launches read its packed actor vector (FlatAgent.packed_actor).  Each path has an
env of its own (same task, same seed).

usage: actor_rollout_wide_cost.py [--out profiles/actor_rollout_wide_cost.json] [--reps 7] [--envs 256 4096 65536]"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from safe_control_gym_amd import ddpg  # noqa: E402
from safe_control_gym_amd.ppo import evaluate  # noqa: E402
from safe_control_gym_amd.sac import SACAgent, SACConfig  # noqa: E402
from safe_control_gym_amd.vec_env import HipVecEnv  # noqa: E402
from tests import actor_rollout_wide_cases as arw  # noqa: E402

KNOB = 'SCG_ROLLOUT_WIDE_TILES'


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3            # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'actor_rollout_wide_cost.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--envs', type=int, nargs='*', default=[256, 4096, 65536])
    a = ap.parse_args()
    dev = torch.device('cuda', torch.cuda.current_device())
    rows = []
    for task, kind, hidden, act in arw.COST_CASES:
        env_id, cfg = arw.cost_task_config(task)
        for N in a.envs:
            mk = lambda policy: HipVecEnv(env_id, N, seed=7, return_numpy=False, policy=policy, **cfg)   # noqa: E731
            envs = dict(fused_g1=mk((hidden, act, kind)), fused_g8=mk((hidden, act, kind)), eager_graph=mk(None))
            spec = envs['fused_g1'].spec
            assert spec.max_episode_steps == arw.COST_STEPS and envs['fused_g1'].actor_kind == kind
            lo, hi = (np.asarray(v, np.float32).reshape(-1) for v in (spec.action_space.low, spec.action_space.high))
            torch.manual_seed(3)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')                     # ("no fused update" at this width)
                if kind == 'sac':
                    agent = SACAgent(spec.obs_dim, spec.nu, torch.tensor(lo, device=dev), torch.tensor(hi, device=dev),
                                     SACConfig(hidden_dim=hidden, activation=act), dev)
                else:
                    agent = ddpg.DDPGAgent(spec.obs_dim, spec.nu, lo, hi, ddpg.DDPGConfig(hidden_dim=hidden, activation=act), dev)
            assert not agent.use_fused
            det, actor = agent.deterministic_policy(), agent.actor_struct()
            res = {}

            def fused(name, tiles):
                os.environ[KNOB] = tiles                            # (read by the library at every launch)
                try:
                    res[name] = evaluate(det, envs[name], policy=actor)
                finally:
                    del os.environ[KNOB]
            fns = dict(fused_g1=lambda: fused('fused_g1', '1'), fused_g8=lambda: fused('fused_g8', '8'),
                       eager_graph=lambda: res.__setitem__('eager_graph', evaluate(det, envs['eager_graph'], use_graph=True)))
            for fn in fns.values():                                 # warm-up: buffers, kernel attributes, the graph capture
                fn(); fn()
            t = {k: [] for k in fns}
            for _ in range(a.reps):                                 # interleaved
                for k, fn in fns.items():
                    t[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in t.items()}
            best = min(med['fused_g1'], med['fused_g8'])
            row = dict(task=task, kind=kind, hidden=hidden, activation=act, envs=N, steps=arw.COST_STEPS, reps=a.reps,
                       fused_g1_us=med['fused_g1'], fused_g8_us=med['fused_g8'], eager_graph_us=med['eager_graph'],
                       g8_over_g1=med['fused_g8'] / med['fused_g1'], eager_graph_over_fused_g1=med['eager_graph'] / med['fused_g1'],
                       eager_graph_over_fused_g8=med['eager_graph'] / med['fused_g8'], eager_graph_over_best_fused=med['eager_graph'] / best,
                       mean_length={k: res[k]['ep_length'] for k in res}, spread_us={k: [min(v), max(v)] for k, v in t.items()})
            print(json.dumps(row), flush=True)
            rows.append(row)
            for e in envs.values():
                e.close()
            del envs, agent, det, actor, fns, res
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0),
                   'method': 'medians of device-event times around one ppo.evaluate call (reset + rollout + totals), interleaved repeats, same '
                             'process; each path on an env of its own; the fused geometries forced with SCG_ROLLOUT_WIDE_TILES', 'rows': rows},
                  f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
