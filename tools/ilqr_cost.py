#!/usr/bin/env python3
"""Cost of the LQR / iLQR kernels on one GPU -> profiles/ilqr_cost.json.  Per shape (4 096 and 65 536 envs, CartPole and Quadrotor 2D
stabilisation, T = 64, float32 and float64), same process, same device, interleaved repeats, medians of device-event times:
  (a) scg_rollout_feedback per control step, shared and per-env schedule;
  (b) scg_step_sequence per control step with the same outputs enabled (obs, reward, done, flags; the state is the obs here) — a kernel
      this feature does not change;
  (c) one whole iLQR iteration (state restore + rollout + bookkeeping + backward pass) as lqr.iLQR.learn(to_host=False) runs it, and the same iteration built
      from the older entry points only: a step_tensors loop with a torch bmm feedback, and the backward pass as batched torch ops on
      prior_model Jacobians.  That baseline lives here only; it is not shipped.
Envs never stop early here (LQR keeps them in bounds), so every launch does all T steps.

usage: ilqr_cost.py [--out profiles/ilqr_cost.json] [--reps 7]"""
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


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)            # us
    return out


def torch_backward(venv, ctrl, x, u, lamb, gains, ff, eps):
    """iLQR.update_policy as batched torch ops ([N] problems side by side), Jacobians from scg_prior_model (the env's own prior)."""
    nx, nu, N = ctrl.spec.nx, ctrl.spec.nu, x.shape[2]
    f = dict(dtype=x.dtype, device=x.device)
    Q, R = torch.as_tensor(ctrl.Q, **f), torch.as_tensor(ctrl.R, **f)
    goal = torch.as_tensor(np.atleast_2d(ctrl.spec.X_GOAL)[0], **f)
    ueq = torch.as_tensor(ctrl.model.U_EQ, **f)
    dt = float(ctrl.model.dt)
    eye_x, eye_u = torch.eye(nx, **f), torch.eye(nu, **f)
    Sv = (x[T].t() - goal) @ Q
    Sm = Q.expand(N, nx, nx).clone()
    for k in reversed(range(T)):
        xk, uk = x[k].t().contiguous(), u[k].t().contiguous()
        jac = venv.prior_model(xk, uk, want=('A', 'B'), eps=eps)
        Ad, Bd = eye_x + jac['A'] * dt, jac['B'] * dt
        Qv, Rv = (xk - goal) @ Q, (uk - ueq) @ R
        BdT = Bd.transpose(1, 2)
        g = Rv + torch.bmm(BdT, Sv.unsqueeze(-1)).squeeze(-1)
        SA = torch.bmm(Sm, Ad)
        G = torch.bmm(BdT, SA)
        H = R + torch.bmm(BdT, torch.bmm(Sm, Bd))
        H = 0.5 * (H + H.transpose(1, 2))
        ev, V = torch.linalg.eigh(H)
        ev = ev.clamp(min=0) + lamb.unsqueeze(-1)
        Hi = torch.bmm(V / ev.unsqueeze(1), V.transpose(1, 2))
        duff = -torch.bmm(Hi, g.unsqueeze(-1)).squeeze(-1)
        K = -torch.bmm(Hi, G)
        gains[k] = K.permute(1, 2, 0)
        ff[k] = (uk + duff - torch.bmm(K, xk.unsqueeze(-1)).squeeze(-1)).t()
        KT = K.transpose(1, 2)
        Sm = Q + torch.bmm(Ad.transpose(1, 2), SA) + torch.bmm(KT, torch.bmm(H, K)) + torch.bmm(KT, G) + torch.bmm(G.transpose(1, 2), K)
        Sv = Qv + torch.bmm(Ad.transpose(1, 2), Sv.unsqueeze(-1)).squeeze(-1) + torch.bmm(KT, torch.bmm(H, duff.unsqueeze(-1))).squeeze(-1) \
            + torch.bmm(KT, g.unsqueeze(-1)).squeeze(-1) + torch.bmm(G.transpose(1, 2), duff.unsqueeze(-1)).squeeze(-1)
    del eye_u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ilqr_cost.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--envs', type=int, nargs='*', default=[4096, 65536])
    a = ap.parse_args()
    with open(os.path.join(ROOT, 'tests', 'golden', 'ilqr_settings.json')) as f:
        cases = json.load(f)['cases']
    rows = []
    for name in ('cartpole_stab', 'quadrotor_2D_stab'):
        case = cases[name]
        task = dict(case['task'], episode_len_sec=T / case['task']['ctrl_freq'])
        if name == 'quadrotor_2D_stab':
            task['init_state'] = {'init_x': 0.0, 'init_z': 1.0, 'init_theta': 0.05}          # a start LQR holds for all T steps
        env_func = partial(make, case['env'], **task)
        for dtype in ('float32', 'float64'):
            for N in a.envs:
                algo = dict(case['algo'], max_iterations=1)
                ctrl = make('ilqr', env_func, num_envs=N, dtype=dtype, **algo)
                venv = ctrl._env()
                td = venv.dtype
                nx, nu = ctrl.spec.nx, ctrl.spec.nu
                f = dict(dtype=td, device=venv.device)
                K0, ff0 = ctrl._as_schedule(*ctrl.lqr_schedule())
                Kp = K0[:1].expand(T, nu, nx).unsqueeze(-1).expand(T, nu, nx, N).contiguous()
                fp = ff0[:1].expand(T, nu).unsqueeze(-1).expand(T, nu, N).contiguous()
                b = ctrl._buffers()
                assert ctrl.max_steps == T
                actions = torch.zeros(T, N, nu, **f)
                seq_out = {}

                def shared():
                    ctrl._restart(); ctrl._rollout(K0, ff0, False)

                def per_env():
                    ctrl._restart(); ctrl._rollout(Kp, fp, True)

                def sequence():
                    ctrl._restart()
                    seq_out['o'] = venv.step_sequence(actions, out=seq_out.get('o'), terminal_obs=False)

                def restart_only():
                    ctrl._restart()
                shared()
                assert int(b['n_steps'].min()) == T, 'an env stopped early: the shapes would not be comparable'
                actions.copy_(b['u'].permute(0, 2, 1))                  # the sequence kernel replays the same closed loop
                t = {k: [] for k in ('shared', 'per_env', 'sequence', 'restart')}
                for _ in range(a.reps):                                  # interleaved
                    for k, fn in (('sequence', sequence), ('shared', shared), ('per_env', per_env), ('restart', restart_only)):
                        t[k] += timed(fn, 1, warm=1)
                med = {k: statistics.median(v) for k, v in t.items()}
                per_step = {k: (med[k] - med['restart']) / T for k in ('shared', 'per_env', 'sequence')}

                # (c) one whole iteration
                lamb = torch.ones(N, **f)
                unstable = torch.zeros(N, dtype=torch.uint8, device=venv.device)
                model = ctrl.model_struct()

                def iteration_new():
                    ctrl.ite_counter = 0
                    ctrl.learn(to_host=False)

                def backward_only():
                    venv.ilqr_backward(model, T, b['x'], b['u'], b['n_steps'], lamb, None, Kp, fp, unstable)
                gains_t, ff_t = Kp.clone(), fp.clone()
                xbuf, ubuf = torch.zeros(T + 1, nx, N, **f), torch.zeros(T, nu, N, **f)

                def iteration_old():
                    ctrl._restart()
                    obs = None
                    st = venv.get_raw_state  # noqa: F841  (the old path has no device-side restore: ctrl._restart stands in for it)
                    obs = b['x'][0].t().contiguous()
                    cost = torch.zeros(N, **f)
                    for k in range(T):
                        uk = torch.bmm(gains_t[k].permute(2, 0, 1), obs.unsqueeze(-1)).squeeze(-1) + ff_t[k].t()
                        xbuf[k], ubuf[k] = obs.t(), uk.t()
                        o = venv.step_tensors(uk.contiguous())
                        obs = o.obs
                        cost -= o.reward
                    xbuf[T] = obs.t()
                    torch_backward(venv, ctrl, xbuf, ubuf, lamb, gains_t, ff_t, float(model.eps))
                t_new = timed(iteration_new, max(3, a.reps // 2), warm=1)
                t_bw = timed(backward_only, a.reps, warm=1)
                t_old = timed(iteration_old, 3, warm=1)
                row = dict(task=name, dtype=dtype, envs=N, steps=T,
                           rollout_shared_us_per_step=per_step['shared'], rollout_per_env_us_per_step=per_step['per_env'],
                           step_sequence_us_per_step=per_step['sequence'], restart_us=med['restart'],
                           per_env_over_sequence=per_step['per_env'] / per_step['sequence'], shared_over_sequence=per_step['shared'] / per_step['sequence'],
                           backward_us=statistics.median(t_bw), ilqr_iteration_us=statistics.median(t_new),
                           baseline_iteration_us=statistics.median(t_old), speedup=statistics.median(t_old) / statistics.median(t_new),
                           reps=a.reps)
                print(json.dumps(row), flush=True)
                rows.append(row)
                ctrl.close()
                del ctrl, venv, b, Kp, fp, gains_t, ff_t, xbuf, ubuf, actions, seq_out
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'method': 'medians of device-event times, interleaved repeats, same process; '
                   'per-step = (launch incl. state restore - state restore) / steps; ilqr_iteration = learn(max_iterations=1): restore + '
                   'rollout + bookkeeping + backward, results left on the device', 'rows': rows}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
