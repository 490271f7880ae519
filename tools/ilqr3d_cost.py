#!/usr/bin/env python3
"""Cost of iLQR on Quadrotor 3D (the LDS-resident backward pass, scg_ilqr_backward_wide) on one GPU -> profiles/ilqr3d_cost.json,
next to the unchanged register-resident scg_ilqr_backward on Quadrotor 2D in the same process on the same device.  Per shape
(256 / 4 096 / 65 536 envs, T = 64, float32 and float64), interleaved repeats, medians of device-event times:
  (a) the backward launch alone: Quadrotor 3D wide, Quadrotor 2D register, Quadrotor 2D wide (the same kernel template on the small system);
  (b) one whole iLQR iteration (state restore + rollout + bookkeeping + backward pass) as lqr.iLQR.learn(to_host=False) runs it, on both.
Both tasks are the stabilisation tasks of the reference-generated fixtures with 64 control steps and a start LQR holds, so no env stops
early and every launch does all T steps.

usage: ilqr3d_cost.py [--out profiles/ilqr3d_cost.json] [--reps 7] [--envs 256 4096 65536]"""
import argparse
import json
import os
import statistics
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from safe_control_gym_amd.registration import make  # noqa: E402

T = 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3                         # us


def tasks():
    with open(os.path.join(ROOT, 'tests', 'golden', 'ilqr3d_settings.json')) as f:
        q3 = json.load(f)['cases']['q3_stab']
    with open(os.path.join(ROOT, 'tests', 'golden', 'ilqr_settings.json')) as f:
        q2 = json.load(f)['cases']['quadrotor_2D_stab']
    # (the variants __graft_entry__.build() compiles)
    t3 = dict(q3['task'], episode_len_sec=T / q3['task']['ctrl_freq'], init_state={'init_x': 0.1, 'init_y': -0.1, 'init_z': 0.9, 'init_phi': 0.05})
    t2 = dict(q2['task'], episode_len_sec=T / q2['task']['ctrl_freq'], init_state={'init_x': 0.0, 'init_z': 1.0, 'init_theta': 0.05})
    return (q3, t3), (q2, t2)


def controller(case, task, n, dtype, wide):
    ctrl = make('ilqr', partial(make, case['env'], **task), num_envs=n, dtype=dtype, wide_backward=wide, **dict(case['algo'], max_iterations=1))
    ctrl.learn(to_host=False)                              # fills the stacks and the per-env schedule the backward launch reads
    assert ctrl.max_steps == T and int(ctrl._buffers()['n_steps'].min()) == T, 'an env stopped early: the shapes would not be comparable'
    return ctrl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ilqr3d_cost.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--envs', type=int, nargs='*', default=[256, 4096, 65536])
    a = ap.parse_args()
    (q3, t3), (q2, t2) = tasks()
    rows = []
    for dtype in ('float32', 'float64'):
        for n in a.envs:
            c3, c2 = controller(q3, t3, n, dtype, True), controller(q2, t2, n, dtype, False)
            fns = {}
            for key, ctrl, wide in (('q3_backward_wide_us', c3, True), ('q2_backward_us', c2, False), ('q2_backward_wide_us', c2, True)):
                venv, b, model = ctrl._env(), ctrl._buffers(), ctrl.model_struct()
                lamb = torch.ones(n, dtype=venv.dtype, device=venv.device)
                unstable = torch.zeros(n, dtype=torch.uint8, device=venv.device)
                fns[key] = partial(venv.ilqr_backward, model, T, b['x'], b['u'], b['n_steps'], lamb, None, ctrl._gains, ctrl._ff, unstable, wide=wide)
            fns['q3_iteration_us'] = partial(c3.learn, to_host=False)
            fns['q2_iteration_us'] = partial(c2.learn, to_host=False)
            for fn in fns.values():                        # warm-up
                fn()
            torch.cuda.synchronize()
            t = {k: [] for k in fns}
            for _ in range(a.reps):                        # interleaved
                for k, fn in fns.items():
                    t[k].append(timed(fn))
            row = dict(dtype=dtype, envs=n, steps=T, reps=a.reps, **{k: statistics.median(v) for k, v in t.items()})
            row.update({k.replace('_us', '_min_us'): min(v) for k, v in t.items()})
            row['q3_over_q2_backward'] = row['q3_backward_wide_us'] / row['q2_backward_us']
            row['q3_over_q2_iteration'] = row['q3_iteration_us'] / row['q2_iteration_us']
            row['q2_wide_over_register'] = row['q2_backward_wide_us'] / row['q2_backward_us']
            print(json.dumps(row), flush=True)
            rows.append(row)
            c3.close(); c2.close()
            del c3, c2, fns
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'method': 'medians (and minima) of device-event times, interleaved repeats, same '
                   'process; q3 = Quadrotor 3D stabilisation with scg_ilqr_backward_wide, q2 = Quadrotor 2D stabilisation with scg_ilqr_backward '
                   '(and the wide kernel on the same stacks); iteration = learn(max_iterations=1, to_host=False): restore + rollout + '
                   'bookkeeping + backward, results left on the device', 'rows': rows}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
