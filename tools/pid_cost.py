#!/usr/bin/env python3
"""Cost of the PID rollout on one GPU -> profiles/pid_cost.json.  Per shape (4 096 and 65 536 envs, the shipped Quadrotor 2D and 3D
tracking tasks as tests/golden/pid_settings.json holds them, T = 64 steps, float32 and float64), same process, same device, the SAME
library, interleaved repeats, medians of device-event times, per control step:
  (a) scg_rollout_pid, shared and per-env gains;
  (b) scg_rollout_feedback with a constant hover schedule (K = 0, ff = U_EQ): the stateless rollout the PID one is modelled on;
  (c) scg_step_sequence replaying the PID rollout's own actions, with obs / reward / done / flags enabled: the loop without any law.
No env stops early in these 64 steps (asserted), so every launch does all T steps.

usage: pid_cost.py [--out profiles/pid_cost.json] [--reps 7] [--envs 4096 65536]"""
import argparse
import json
import os
import statistics
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from safe_control_gym_amd.registration import make  # noqa: E402

T = 64


def timed(fn):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3            # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pid_cost.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--envs', type=int, nargs='*', default=[4096, 65536])
    a = ap.parse_args()
    with open(os.path.join(ROOT, 'tests', 'golden', 'pid_settings.json')) as f:
        cases = json.load(f)['cases']
    rows = []
    for name in ('quadrotor_2D_track', 'quadrotor_3D_track'):
        env_func = partial(make, cases[name]['env'], **cases[name]['task'])
        for dtype in ('float32', 'float64'):
            for N in a.envs:
                ctrl = make('pid', env_func, num_envs=N, dtype=dtype)
                venv = ctrl._env()
                nx, nu = ctrl.spec.nx, ctrl.spec.nu
                f = dict(dtype=venv.dtype, device=venv.device)
                o = dict(x=torch.zeros(T, nx, N, **f), u=torch.zeros(T, nu, N, **f), final_obs=torch.zeros(nx, N, **f), stats=torch.zeros(4, N, **f),
                         n_steps=torch.zeros(N, dtype=torch.int32, device=venv.device), final_flags=torch.zeros(N, dtype=torch.uint8, device=venv.device))
                g = torch.as_tensor(ctrl.gains, **f)
                gp = g.unsqueeze(-1).expand(18, N).contiguous()
                cfg = ctrl.config_struct()
                state = torch.zeros(9, N, **f)
                K0 = torch.zeros(1, nu, nx, **f)
                ff0 = torch.as_tensor(np.asarray(ctrl.model.U_EQ)[None], **f).contiguous()
                actions = torch.zeros(T, N, nu, **f)
                seq_out = {}

                def pid_shared():
                    ctrl._restart(); state.zero_(); venv.rollout_pid(g, cfg, T, pid_state=state, per_env=False, **o)

                def pid_per_env():
                    ctrl._restart(); state.zero_(); venv.rollout_pid(gp, cfg, T, pid_state=state, per_env=True, **o)

                def feedback():
                    ctrl._restart(); state.zero_(); venv.rollout_feedback(K0, ff0, T, per_env=False, **o)

                def sequence():
                    ctrl._restart(); state.zero_()
                    seq_out['o'] = venv.step_sequence(actions, out=seq_out.get('o'), terminal_obs=False)

                def restart_only():
                    ctrl._restart(); state.zero_()
                feedback()
                assert int(o['n_steps'].min()) == T, 'an env stopped early under the hover schedule'
                pid_shared()
                assert int(o['n_steps'].min()) == T, 'an env stopped early under the PID law'
                actions.copy_(o['u'].permute(0, 2, 1))
                fns = dict(sequence=sequence, feedback=feedback, pid_shared=pid_shared, pid_per_env=pid_per_env, restart=restart_only)
                t = {k: [] for k in fns}
                for _ in range(a.reps):                                  # interleaved
                    for k, fn in fns.items():
                        t[k].append(timed(fn))
                med = {k: statistics.median(v) for k, v in t.items()}
                per = {k: (med[k] - med['restart']) / T for k in fns if k != 'restart'}
                row = dict(task=name, dtype=dtype, envs=N, steps=T, restart_us=med['restart'], reps=a.reps,
                           pid_shared_us_per_step=per['pid_shared'], pid_per_env_us_per_step=per['pid_per_env'],
                           feedback_us_per_step=per['feedback'], step_sequence_us_per_step=per['sequence'],
                           pid_over_sequence=per['pid_shared'] / per['sequence'], pid_over_feedback=per['pid_shared'] / per['feedback'],
                           pid_per_env_over_shared=per['pid_per_env'] / per['pid_shared'])
                print(json.dumps(row), flush=True)
                rows.append(row)
                ctrl.close()
                del ctrl, venv, o, actions, seq_out, gp, state
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'method': 'medians of device-event times, interleaved repeats, same process, same library; '
                   'per-step = (launch incl. state restore - state restore) / steps', 'rows': rows}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
