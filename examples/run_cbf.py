#!/usr/bin/env python3
"""The reference's examples/cbf experiment, batched: the shipped PPO policy on the cartpole (ctrl_freq 25, pyb_freq 1000, quadratic
cost, state limits +-(2, 2, 0.2, 2), randomised initial states), one episode per env on 65 536 envs, without and with the CBF-QP
safety filter — each evaluation ONE kernel launch (scg_rollout_policy / scg_rollout_cbf).  Prints the share of steps that violate the
state constraint, the share of episodes with a violation, the mean return and the filter's correction statistics.

usage: run_cbf.py [--envs 65536] [--seed 42] [--hard] [--check-cbf]"""
import argparse
import copy
import json
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from safe_control_gym_amd import _lib as L  # noqa: E402
from safe_control_gym_amd.ppo import evaluate  # noqa: E402
from safe_control_gym_amd.registration import make  # noqa: E402
from safe_control_gym_amd.vec_env import HipVecEnv  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--hard', action='store_true', help='hard-constrained QP (soft_constrained: False)')
    ap.add_argument('--check-cbf', action='store_true', help='also run CBF.is_cbf() on the default grid')
    a = ap.parse_args()
    S = json.load(open(os.path.join(GOLDEN, 'cbf_settings.json')))                  # the example's task and filter settings
    D = np.load(os.path.join(GOLDEN, 'cbf.npz'))                                    # the example's shipped actor, as arrays
    cfg = copy.deepcopy(S['task_config'])
    cfg.pop('seed', None)
    cfg['randomized_init'] = True
    shape = (S['algo_config']['hidden_dim'], S['algo_config']['activation'])
    env = HipVecEnv(S['task'], a.envs, seed=a.seed, return_numpy=False, policy=shape, cbf=True, **cfg)
    sf = make(S['safety_filter'], partial(make, S['task'], **cfg), **dict(S['sf_config'], soft_constrained=not a.hard)).attach(env)
    parts = [np.asarray(D[f'actor/actor.pi_net.fcs.{i}.{k}'], dtype=np.float32).reshape(-1) for i in range(3) for k in ('weight', 'bias')]
    parts.append(np.asarray(D['actor/actor.logstd'], dtype=np.float32).reshape(-1))
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    flat = torch.tensor(np.concatenate(parts), device=env.device)
    pol = L.Policy(d_params=flat.data_ptr(), W1=int(offs[0]), b1=int(offs[1]), W2=int(offs[2]), b2=int(offs[3]), W3=int(offs[4]), b3=int(offs[5]),
                   logstd_off=int(offs[6]), hidden=shape[0], activation=L.POLICY_ACTS[shape[1]], deterministic=1)
    for name, filt in (('uncertified', None), ('certified', sf)):
        res = evaluate(None, env, policy=pol, safety_filter=filt)
        acc = (env._eval_cbf if filt is not None else env._eval_fused)['acc']
        steps, viol = acc[:, 2].sum().item(), acc[:, 3].sum().item()
        print(f'{name:12s} episodes {int(res["episodes"])}  mean return {res["ep_return"]:.3f}  mean length {res["ep_length"]:.1f}  '
              f'violating steps {viol / steps:.5f}  episodes with a violation {(acc[:, 3] > 0).float().mean().item():.5f}')
        if filt is not None:
            fd = res['safety_filter_data']
            n = fd['steps'].sum().item()
            print(f'{"":12s} corrected steps {fd["corrected_steps"].sum().item() / n:.5f}  infeasible steps (policy action applied) '
                  f'{fd["infeasible_steps"].sum().item() / n:.5f}  mean correction {fd["mean_correction"].mean().item():.4f} N')
    if a.check_cbf:
        valid, bad = sf.is_cbf()
        print(f'is_cbf: valid {valid}, {len(bad)} infeasible grid states')
    env.close()


if __name__ == '__main__':
    main()
