#!/usr/bin/env python3
"""Device time of ONE Safe-Explorer PPO collection (T control steps with the safety-filtered policy, values) on the fused collector
(scg_rollout_safe + one batched critic pass, safe_explorer.SafeExplorerPPO._collect_fused) against the eager collector (T x (actor,
C constraint models, projection, sampling, log-prob, critic, env step, next constraint values) in PyTorch, _collect_body), in the same
process, alternating the two.

Setup: the shipped Quadrotor2D-tracking shape (hidden_dim 128 tanh, constraint_hidden_dim 150, the YAML's slack) with the shipped
pre-trained safety layer, 4 096 and 65 536 envs, T = 32.  Each timing is a pair of device events around one collection; --reps
repetitions per path, reported as median / min / max.  Writes profiles/safe_explorer_collect_cost.json (or --out).

usage: safe_explorer_collect_cost.py [--reps 5] [--envs 4096 65536] [--steps 32] [--out profiles/safe_explorer_collect_cost.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, HC = 128, 150
SLACK = [0.05, 0.05, 0.05, 0.05, 0.01, 0.01] * 2
PRETRAIN = os.path.join(ROOT, 'tests', 'golden', 'safe_explorer_ppo', 'safe_explorer_ppo_pretrain_quadrotor_2D_track.pt')


def make(n, T, fused):
    from safe_control_gym_amd.ppo import PPOConfig
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.safe_explorer import SafeExplorerPPO
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = load_task('quadrotor_2D_track')
    kw = dict(policy=(H, 'tanh'), safety_layer=HC) if fused else {}
    env = HipVecEnv(env_id, n, seed=1, return_numpy=False, **cfg, **kw)
    pcfg = PPOConfig(hidden_dim=H, activation='tanh', use_gae=True, rollout_steps=T, opt_epochs=1, mini_batch_size=n * T // 4,
                     extra={'fused_rollout': fused})
    torch.manual_seed(0)
    r = SafeExplorerPPO(env, pcfg, seed=0, constraint_hidden_dim=HC, constraint_slack=SLACK)
    r.load_safety_layer(PRETRAIN)
    assert (r._fused_safe is not None) == fused
    return env, r


def collect(r):
    with torch.no_grad():
        if r._fused_safe is not None:
            r._collect_fused()
        else:
            r.collect()


def timed(r):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    collect(r)
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--envs', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--steps', type=int, nargs='+', default=[32])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'safe_explorer_collect_cost.json'))
    a = ap.parse_args()
    from safe_control_gym_amd import _safe_explorer
    rows = []
    for n in a.envs:
        for T in a.steps:
            pair = {True: make(n, T, True), False: make(n, T, False)}
            plan = _safe_explorer.launch_plan(pair[True][0]._lib, 4 if n <= 32768 else 8)
            for fused in (True, False):
                for _ in range(2):                          # warm-up: libraries load, kernels are set up
                    collect(pair[fused][1])
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
            row = {'envs': n, 'T': T, 'fused': st(ms[True]), 'eager': st(ms[False]),
                   'speedup_median': float(np.median(ms[False]) / np.median(ms[True])),
                   'fused_us_per_step': float(1e3 * np.median(ms[True]) / T), 'eager_us_per_step': float(1e3 * np.median(ms[False]) / T),
                   'fused_env_steps_per_s': float(n * T / (np.median(ms[True]) * 1e-3)),
                   'eager_env_steps_per_s': float(n * T / (np.median(ms[False]) * 1e-3)),
                   'fused_lds_bytes': plan[0], 'fused_waves_per_workgroup': plan[1], 'fused_safety_layer_in_lds': plan[2]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    meta = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'hidden_dim': H, 'activation': 'tanh', 'constraint_hidden_dim': HC,
            'n_constraints': 12, 'task': 'quadrotor_2D_track', 'safety_layer': 'shipped pre-trained (tests/golden/safe_explorer_ppo)',
            'what': 'one collection (fused: _collect_fused; eager: collect), device events, alternating', 'date': time.strftime('%Y-%m-%d')}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'_meta': meta, 'rows': rows}, f, indent=1)
    print(f'wrote {a.out}')


if __name__ == '__main__':
    main()
