#!/usr/bin/env python3
"""RARL through the reference's controller surface with the fused collector: make('rarl', env_func, fused_rollout=True, ...) on
Quadrotor2D trajectory tracking with a `dynamics` adversary — every collection is one scg_rollout_adversarial launch (protagonist and
adversary on the matrix cores inside the env kernel) — trained for a few iterations, then the protagonist is evaluated alone.

    python examples/train_rarl.py [--envs 4096] [--iterations 4] [--algo rarl|rap]

Prints one JSON line per training iteration and the protagonist's evaluation return.
"""
import argparse, functools, json, os, sys, tempfile, time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_control_gym_amd.registration import load_task, make              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--algo', default='rarl', choices=('rarl', 'rap'))
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=100)                       # rarl.yaml rollout_steps
    ap.add_argument('--iterations', type=int, default=4)
    ap.add_argument('--eval-episodes', type=int, default=16)
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    env_id, cfg = load_task('quadrotor_2D_track')
    env_func = functools.partial(make, env_id, **dict(cfg, adversary_disturbance='dynamics', adversary_disturbance_scale=0.1))
    out = tempfile.mkdtemp(prefix='rarl_')
    extra = dict(agent_iterations=1, adversary_iterations=1) if args.algo == 'rarl' else {}
    per_iter = args.envs * args.steps * (2 if args.algo == 'rarl' else 1)
    ctrl = make(args.algo, env_func, training=True, output_dir=out, checkpoint_path=os.path.join(out, 'model_latest.pt'), seed=args.seed,
                fused_rollout=True, rollout_batch_size=args.envs, rollout_steps=args.steps, mini_batch_size=args.envs * args.steps // 4,
                opt_epochs=4, max_env_steps=args.iterations * per_iter, **extra)
    assert ctrl.impl._fused_two_sided, 'the fused collector did not engage'
    ctrl.reset()
    t0 = time.perf_counter()
    while ctrl.total_steps < args.iterations * per_iter:
        res = ctrl.train_step()
        print(json.dumps({'step': ctrl.total_steps, 'policy_loss': res.get('policy_loss'), 'policy_loss_adv': res.get('policy_loss_adv'),
                          'env_steps_per_s': ctrl.total_steps / (time.perf_counter() - t0)}), flush=True)
    torch.cuda.synchronize()
    ev = ctrl.run(n_episodes=args.eval_episodes)
    print(json.dumps({'train_seconds': time.perf_counter() - t0, 'env_steps': ctrl.total_steps,
                      'eval_mean_return': float(np.mean(ev['ep_returns'])), 'eval_mean_length': float(np.mean(ev['ep_lengths']))}))
    ctrl.close()


if __name__ == '__main__':
    main()
