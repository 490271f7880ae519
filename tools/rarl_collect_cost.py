#!/usr/bin/env python3
"""Device time of ONE RARL / RAP collection (both sides' T control steps, critic passes, bootstrap and GAE) on the fused collector
(scg_rollout_adversarial, rarl._TwoSided._collect_fused_both) against the captured PyTorch collector (one HIP graph of T x (both
actors, set_adversary_control, env step) + both GAE passes), in the same process, alternating the two.

Setup: hidden_dim 64 (rarl.yaml / rap.yaml), Quadrotor2D tracking with a `dynamics` adversary, RARL and RAP with two adversaries,
16 384 and 65 536 envs, T = 32 and T = 100 (rarl.yaml's rollout_steps).  Each timing is a pair of device events around one
collection; --reps repetitions per path, reported as median / min / max.  Writes profiles/rarl_collect_cost.json (or --out).

Kernel times: run it once more under `rocprofv3 --kernel-trace --stats -- python tools/rarl_collect_cost.py --reps 2 --out <tmp>`.
usage: rarl_collect_cost.py [--reps 7] [--envs 16384 65536] [--steps 32 100] [--out profiles/rarl_collect_cost.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ADV = dict(adversary_disturbance='dynamics', adversary_disturbance_scale=0.1)


def make(algo, n, T, fused):
    from safe_control_gym_amd.ppo import PPOConfig
    from safe_control_gym_amd.rarl import RAP, RARL
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = load_task('quadrotor_2D_track')
    n_adv = 2 if algo == 'rap' else 1
    kw = dict(policy=(64, 'tanh'), adversaries=n_adv) if fused else {}
    env = HipVecEnv(env_id, n, seed=1, return_numpy=False, **dict(cfg, **ADV), **kw)
    pcfg = PPOConfig(hidden_dim=64, activation='tanh', use_gae=True, rollout_steps=T, opt_epochs=1, mini_batch_size=n * T // 4)
    torch.manual_seed(0)
    r = RAP(env, pcfg, seed=0, num_adversaries=2) if algo == 'rap' else RARL(env, pcfg, seed=0)
    assert r._fused_two_sided == fused
    if algo == 'rap':
        r.collect()                                     # draws the groups (and, fused, runs the first, eager collection)
    return env, r


def timed(r):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    r._collect_both()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--envs', type=int, nargs='+', default=[16384, 65536])
    ap.add_argument('--steps', type=int, nargs='+', default=[32, 100])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rarl_collect_cost.json'))
    a = ap.parse_args()
    rows = []
    for algo in ('rarl', 'rap'):
        for n in a.envs:
            for T in a.steps:
                pair = {True: make(algo, n, T, True), False: make(algo, n, T, False)}
                for fused in (True, False):
                    for _ in range(3):                  # eager, capture, first replay
                        pair[fused][1]._collect_both()
                torch.cuda.synchronize()
                ms = {True: [], False: []}
                for _ in range(a.reps):
                    for fused in (True, False):
                        ms[fused].append(timed(pair[fused][1]))
                for env, _ in pair.values():
                    env.close()
                del pair
                torch.cuda.empty_cache()
                st = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v)), 'max_ms': float(np.max(v))}   # noqa: E731
                row = {'algo': algo, 'n_adversaries': 2 if algo == 'rap' else 1, 'envs': n, 'T': T, 'fused': st(ms[True]),
                       'torch_graph': st(ms[False]), 'speedup_median': float(np.median(ms[False]) / np.median(ms[True])),
                       'fused_env_steps_per_s': float(n * T / (np.median(ms[True]) * 1e-3)),
                       'torch_graph_env_steps_per_s': float(n * T / (np.median(ms[False]) * 1e-3))}
                rows.append(row)
                print(json.dumps(row), flush=True)
    meta = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'hidden_dim': 64, 'activation': 'tanh',
            'task': 'quadrotor_2D_track', 'adversary': ADV, 'what': 'one collection (_TwoSided._collect_both), device events, alternating',
            'date': time.strftime('%Y-%m-%d')}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'_meta': meta, 'rows': rows}, f, indent=1)
    print(f'wrote {a.out}')


if __name__ == '__main__':
    main()
