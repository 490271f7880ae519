#!/usr/bin/env python3
"""Device time of K control steps of the filtered policy rollout (scg_rollout_cbf: actor, CBF-QP filter, env step) against the plain
policy rollout (scg_rollout_policy) of the SAME library, in the same process, alternating the two; and of the default CBF.is_cbf grid
(26^4 = 456 976 states: one scg_cbf_certify launch plus the copy back of the flags).

Setup: the reference's examples/cbf task (tests/golden/cbf_settings.json, randomised initial states) with its shipped 64-64 tanh actor,
sampled actions, 4 096 and 65 536 envs, K = 32.  Each timing is a pair of device events around one launch, after --warmup launches of
each kernel; --reps repetitions per kernel, reported as median / min / max and the ratio of the medians.  scg_rollout_policy is not
touched by the filter's sources: it is the cost of the same rollout without the filter.  Writes profiles/cbf_rollout_cost.json (or --out).

usage: cbf_rollout_cost.py [--reps 7] [--warmup 3] [--envs 4096 65536] [--steps 32] [--out profiles/cbf_rollout_cost.json]"""
import argparse
import copy
import json
import os
import sys
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def setup(n):
    from safe_control_gym_amd import _cbf
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd.registration import make
    from safe_control_gym_amd.vec_env import HipVecEnv
    S = json.load(open(os.path.join(GOLDEN, 'cbf_settings.json')))
    D = np.load(os.path.join(GOLDEN, 'cbf.npz'))
    cfg = copy.deepcopy(S['task_config'])
    cfg.pop('seed', None)
    cfg['randomized_init'] = True
    shape = (S['algo_config']['hidden_dim'], S['algo_config']['activation'])
    env = HipVecEnv(S['task'], n, seed=1, return_numpy=False, policy=shape, cbf=True, **cfg)
    env.reset_tensors()
    sf = make('cbf', partial(make, S['task'], **cfg), **S['sf_config']).attach(env)
    parts = [np.asarray(D[f'actor/actor.pi_net.fcs.{i}.{k}'], dtype=np.float32).reshape(-1) for i in range(3) for k in ('weight', 'bias')]
    parts.append(np.asarray(D['actor/actor.logstd'], dtype=np.float32).reshape(-1))
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    flat = torch.tensor(np.concatenate(parts), device=env.device)
    pol = L.Policy(d_params=flat.data_ptr(), W1=int(offs[0]), b1=int(offs[1]), W2=int(offs[2]), b2=int(offs[3]), W3=int(offs[4]), b3=int(offs[5]),
                   logstd_off=int(offs[6]), hidden=shape[0], activation=L.POLICY_ACTS[shape[1]], deterministic=0)
    return env, sf, flat, pol, _cbf.actor_ptrs_of_policy(pol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--envs', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cbf_rollout_cost.json'))
    a = ap.parse_args()
    K = a.steps
    res = {'device': torch.cuda.get_device_name(0), 'steps': K, 'reps': a.reps, 'warmup': a.warmup, 'cases': []}
    for n in a.envs:
        env, sf, flat, pol, actor = setup(n)
        f = dict(device=env.device, dtype=torch.float32)
        u8 = dict(device=env.device, dtype=torch.uint8)
        o = {'obs': torch.zeros(K + 1, n, env.spec.obs_dim, **f), 'act': torch.zeros(K, n, 1, **f), 'logp': torch.zeros(K, n, **f),
             'rew': torch.zeros(K, n, **f), 'done': torch.zeros(K, n, **u8), 'flags': torch.zeros(K, n, **u8),
             'rows': torch.zeros(K, n, 4, **f), 'applied': torch.zeros(K, n, **f)}
        params = sf.params()
        run = {'policy': lambda: env.rollout_policy(pol, K, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags']),
               'cbf': lambda: env.rollout_cbf(actor, params, K, o['obs'], o['act'], o['logp'], o['rew'], o['done'], o['flags'], o['rows'],
                                              o['applied'])}

        def timed(fn):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1])
        for _ in range(a.warmup):
            for k in run:
                timed(run[k])
        t = {k: [] for k in run}
        for _ in range(a.reps):
            for k in run:                                  # alternating
                t[k].append(timed(run[k]))
        case = {'envs': n}
        for k, v in t.items():
            case[k + '_ms'] = {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'all': [float(x) for x in v]}
        case['ratio_cbf_over_policy'] = case['cbf_ms']['median'] / case['policy_ms']['median']
        corrected = ((o['rows'][..., 1] - o['rows'][..., 0]).abs() > 1e-6).float().mean().item()
        case['corrected_share_last_launch'] = corrected
        print(f"{n} envs x {K} steps: policy {case['policy_ms']['median']:.3f} ms, cbf {case['cbf_ms']['median']:.3f} ms, "
              f"ratio {case['ratio_cbf_over_policy']:.3f} (corrected share {corrected:.3f})")
        res['cases'].append(case)
        if n == a.envs[0]:                                 # the default is_cbf grid: one launch + the copy back
            import contextlib
            import io
            with contextlib.redirect_stdout(io.StringIO()):
                sf.is_cbf()                                # warm-up (allocations)
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    valid, bad = sf.is_cbf()
                ts.append((time.perf_counter() - t0) * 1e3)
            from safe_control_gym_amd.cbf import state_grid
            g = torch.tensor(state_grid(sf.state_limits), dtype=torch.float32, device=env.device)
            ones = torch.ones(len(g), **f)
            env.certify_tensors(params, g, ones)
            tk = [timed(lambda: env.certify_tensors(params, g, ones)) for _ in range(a.reps)]
            res['is_cbf'] = {'grid_states': int(len(g)), 'valid': bool(valid), 'infeasible_states': len(bad),
                             'wall_ms_median': float(np.median(ts)), 'certify_launch_ms_median': float(np.median(tk))}
            print(f"is_cbf default grid ({len(g)} states): {np.median(ts):.1f} ms wall (grid build, launch, copy back, host bookkeeping); "
                  f"the certify launch alone {np.median(tk):.3f} ms")
        env.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fjson:
        json.dump(res, fjson, indent=1)
        fjson.write('\n')


if __name__ == '__main__':
    main()
