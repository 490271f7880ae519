#!/usr/bin/env python3
"""Time of ONE Safe-Explorer pre-training epoch (SafeExplorerPPO.pretrain_step: collect random-action transitions, one pass of shuffled
minibatches over them) and of ONE eval_constraint_models, on the fused path (cfg.extra['fused_pretrain']: one scg_collect_constraints
launch + one scg_safety_update launch) against the eager path (a Python loop of env steps, then forward / backward / Adam over C small MLPs
per minibatch), in the same process, alternating the two.

Setup: the shipped Quadrotor-2D pre-training config (constraint_hidden_dim 150, constraint_batch_size 256, 3000 steps per epoch, 1500
evaluation steps, lr 1e-4) at 4 (upstream's rollout_batch_size), 256 and 4096 envs.  Each timing is a host clock around the call, which
ends in a device synchronise (the losses are read back); --reps repetitions per path after 2 warm-up calls, reported as median / min / max.
Also recorded: the fused update's distance to the reference's own runs (tests/golden/safety_pretrain.npz), as tests/test_gpu_safe_pretrain.py
measures it.  Writes profiles/safe_pretrain_cost.json (or --out).

--loop K runs nothing but K fused epochs and then K fused evaluations per env count and writes no file: the workload for a kernel trace
(`rocprofv3 --kernel-trace --stats -- python tools/safe_pretrain_cost.py --loop 20`; profiles/safe_pretrain_kernel_trace.json holds the
medians of collect_constraints_kernel and safety_update_kernel from such a run).

usage: safe_pretrain_cost.py [--reps 7] [--envs 4 256 4096] [--out profiles/safe_pretrain_cost.json] [--loop K]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, HC, BATCH, STEPS, EVAL_STEPS, LR = 128, 150, 256, 3000, 1500, 1e-4
SLACK = [0.05, 0.05, 0.05, 0.05, 0.01, 0.01] * 2


def make(n, fused):
    from safe_control_gym_amd.ppo import PPOConfig
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.safe_explorer import SafeExplorerPPO
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = load_task('quadrotor_2D_track')
    kw = dict(policy=(H, 'tanh'), safety_layer=HC) if fused else {}
    env = HipVecEnv(env_id, n, seed=1, return_numpy=False, **cfg, **kw)
    pcfg = PPOConfig(hidden_dim=H, activation='tanh', use_gae=True, rollout_steps=8, opt_epochs=1, mini_batch_size=max(8 * n // 4, 1),
                     extra={'fused_pretrain': fused, 'fused_rollout': False})
    torch.manual_seed(0)
    r = SafeExplorerPPO(env, pcfg, seed=0, constraint_hidden_dim=HC, constraint_lr=LR, constraint_slack=SLACK, constraint_batch_size=BATCH)
    assert r._fused_pretrain == fused
    return env, r


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def fixture_distances():
    """max |kernel - reference float64| per quantity and fixture case (the cases run embedded in the library's observation width)."""
    from tests import safety_pretrain_model as M
    from tests import test_gpu_safe_pretrain as T
    out = {}
    for name in M.CASES:
        g = M.load_case(name)
        env = T._env(name, n=64)
        init, data, rows = T._fixture_on(env, g)
        r = T._fixture_part(env, g, T._fused_run(T._flat_layer(env, g['Hc'], g['lr'], init), data, rows, g['batch']))
        out[name] = {k: float(np.abs(np.asarray(r[k], dtype=np.float64) - g[k + '64']).max()) for k in ('loss', 'final', 'm', 'v', 'grad')}
        out[name]['reference_float32_to_float64'] = {k: float(np.abs(g[k + '32'].astype(np.float64) - g[k + '64']).max())
                                                     for k in ('loss', 'final', 'm', 'v', 'grad')}
        env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--envs', type=int, nargs='+', default=[4, 256, 4096])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'safe_pretrain_cost.json'))
    ap.add_argument('--loop', type=int, default=0)
    a = ap.parse_args()
    if a.loop > 0:
        for n in a.envs:
            env, r = make(n, True)
            for _ in range(a.loop):
                r.pretrain_step(STEPS, BATCH)
            for _ in range(a.loop):
                r.eval_constraint_models(EVAL_STEPS, BATCH)
            torch.cuda.synchronize()
            env.close()
        return
    from safe_control_gym_amd import _safe_explorer
    rows = []
    for n in a.envs:
        pair = {True: make(n, True), False: make(n, False)}
        calls = {'epoch': lambda r: r.pretrain_step(STEPS, BATCH), 'eval': lambda r: r.eval_constraint_models(EVAL_STEPS, BATCH)}
        ms = {(k, f): [] for k in calls for f in (True, False)}
        for fused in (True, False):
            for k, fn in calls.items():
                for _ in range(2):                              # warm-up: libraries load, kernels are set up
                    fn(pair[fused][1])
        for _ in range(a.reps):
            for k, fn in calls.items():
                for fused in (True, False):
                    ms[(k, fused)].append(timed(lambda: fn(pair[fused][1])))
        lds = _safe_explorer.pretrain_lds_of(pair[True][0]._lib)
        for env, _ in pair.values():
            env.close()
        del pair
        torch.cuda.empty_cache()
        st = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v)), 'max_ms': float(np.max(v))}   # noqa: E731
        steps = -(-STEPS // n)
        row = {'envs': n, 'control_steps_per_epoch': steps, 'transitions_per_epoch': steps * n, 'minibatches_per_epoch': steps * n // BATCH,
               'update_lds_bytes': lds}
        for k in calls:
            row[k] = {'fused': st(ms[(k, True)]), 'eager': st(ms[(k, False)]),
                      'eager_over_fused_median': float(np.median(ms[(k, False)]) / np.median(ms[(k, True)]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    meta = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'task': 'quadrotor_2D_track', 'constraint_hidden_dim': HC,
            'n_constraints': 12, 'constraint_batch_size': BATCH, 'constraint_steps_per_epoch': STEPS, 'constraint_eval_steps': EVAL_STEPS,
            'constraint_lr': LR, 'update_kernel': 'vector ALU, exact float32 (the MFMA form of layer 1 / dW1 was not built: not measured)',
            'what': 'one pretrain_step / one eval_constraint_models; host clock around the call, device synchronised before and after; '
                    'fused and eager alternating in one process', 'date': time.strftime('%Y-%m-%d')}
    out = {'_meta': meta, 'rows': rows, 'fixture_distance_to_reference_float64': fixture_distances()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(f'wrote {a.out}')


if __name__ == '__main__':
    main()
