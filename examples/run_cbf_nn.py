#!/usr/bin/env python3
"""The reference's examples/cbf experiment with the learned filter (cbf_experiment.py with safety_filter: cbf_nn), batched: the shipped
PPO(64, tanh) policy on the cartpole (ctrl_freq 25, state limits +-(2, 2, 0.2, 2), randomised initial states) is the uncertified
controller; CBF_NN.learn runs upstream's schedule (num_episodes episodes of max_num_steps steps, blend weight i / (num_episodes - 1),
train_iterations Adam steps after each) with every episode ONE scg_rollout_cbf_nn launch across --learn-envs envs; then one episode
per env on --envs envs without a filter, with the plain CBF filter and with the learned one — each evaluation one launch.  Prints the
share of steps that violate the state constraint, the share of episodes with a violation, the mean return and the corrections.

usage: run_cbf_nn.py [--envs 4096] [--learn-envs 256] [--episodes 20] [--seed 42] [--random-actions] [--load PATH] [--save PATH]"""
import argparse
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
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--learn-envs', type=int, default=256)
    ap.add_argument('--episodes', type=int, default=None, help='num_episodes of learn() (default: the example config\'s 20)')
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--random-actions', action='store_true', help='learn with action_space.sample() instead of the PPO controller')
    ap.add_argument('--load', default=None, help='a checkpoint written by --save: skip learn()')
    ap.add_argument('--save', default=None)
    ap.add_argument('--fused-update', action='store_true', help='the Adam steps in scg_cbf_nn_update, one call per episode (fused_update=True)')
    a = ap.parse_args()
    S = json.load(open(os.path.join(GOLDEN, 'cbf_nn_settings.json')))               # the example's task and filter settings
    D = np.load(os.path.join(GOLDEN, 'cbf.npz'))                                    # the example's shipped actor, as arrays
    cfg = dict(S['task_config'], randomized_init=True)
    cfg.pop('seed', None)
    shape = (S['algo_config']['hidden_dim'], S['algo_config']['activation'])
    dev = torch.device('cuda')
    parts = [np.asarray(D[f'actor/actor.pi_net.fcs.{i}.{k}'], dtype=np.float32).reshape(-1) for i in range(3) for k in ('weight', 'bias')]
    parts.append(np.asarray(D['actor/actor.logstd'], dtype=np.float32).reshape(-1))
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    flat = torch.tensor(np.concatenate(parts), device=dev)
    pol = L.Policy(d_params=flat.data_ptr(), W1=int(offs[0]), b1=int(offs[1]), W2=int(offs[2]), b2=int(offs[3]), W3=int(offs[4]), b3=int(offs[5]),
                   logstd_off=int(offs[6]), hidden=shape[0], activation=L.POLICY_ACTS[shape[1]], deterministic=1)
    sf_config = dict(S['sf_config'])
    if a.episodes is not None:
        sf_config['num_episodes'] = a.episodes
    if a.fused_update:
        sf_config['fused_update'] = True
    env_func = partial(make, S['task'], **cfg)
    sf = make(S['safety_filter'], env_func, seed=a.seed, policy=shape, **sf_config)
    if a.load:
        sf.load(a.load)
        print(f'loaded {a.load}')
    else:
        sf.uncertified_controller = None if a.random_actions else pol
        sf.learn(num_envs=a.learn_envs)
        torch.cuda.synchronize()
        rows = sf.buffer.pos if sf.buffer.buffer_size < sf.buffer.max_size else sf.buffer.max_size
        print(f'learn: {sf.num_episodes} episodes x {sf.max_num_steps} steps x {a.learn_envs} envs, {rows} buffer rows, '
              f'{sf.num_episodes * sf.train_iterations} Adam steps')
    if a.save:
        sf.save(a.save)
    plain = make('cbf', env_func, seed=a.seed, policy=shape, **{k: S['sf_config'][k] for k in ('slope', 'soft_constrained', 'slack_weight',
                                                                                             'slack_tolerance')})
    for name, filt, kw in (('uncertified', None, dict(cbf=True)), ('cbf', plain, dict(cbf=True)), ('cbf_nn', sf, dict(cbf_nn=True))):
        env = HipVecEnv(S['task'], a.envs, seed=a.seed, return_numpy=False, policy=shape, **kw, **cfg)
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
        env.close()
    sf.close()
    del flat


if __name__ == '__main__':
    main()
