#!/usr/bin/env python3
"""Safe-Explorer PPO through the reference's controller surface with the fused collector: make('safe_explorer_ppo', env_func,
fused_rollout=True, pretraining=False, pretrained=<the shipped pre-trained safety layer>, ...) on Quadrotor2D trajectory tracking with
the shipped shape (hidden_dim 128, constraint_hidden_dim 150) — every collection is one scg_rollout_safe launch (actor, safety layer,
projection, sampling and env step inside the env kernel) — trained for a few iterations, then evaluated with the deterministic kernel.

    python examples/train_safe_explorer.py [--envs 4096] [--iterations 4] [--pretrain-epochs 0]

--pretrain-epochs K > 0 runs upstream's FIRST phase before that, fused as well (fused_pretrain=True: per epoch one scg_collect_constraints
launch for the random-action transitions and one scg_safety_update launch for all minibatches), and hands its checkpoint to the second
phase instead of the shipped one.

Prints one JSON line per pre-training epoch and training iteration, and the evaluation return.
"""
import argparse, functools, json, os, sys, tempfile, time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from safe_control_gym_amd.registration import load_task, make              # noqa: E402

PRETRAINED = os.path.join(ROOT, 'tests', 'golden', 'safe_explorer_ppo', 'safe_explorer_ppo_pretrain_quadrotor_2D_track.pt')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--iterations', type=int, default=4)
    ap.add_argument('--eval-episodes', type=int, default=16)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--pretrain-epochs', type=int, default=0)
    args = ap.parse_args()
    env_id, cfg = load_task('quadrotor_2D_track')
    env_func = functools.partial(make, env_id, **cfg)
    out = tempfile.mkdtemp(prefix='safe_explorer_')
    per_iter = args.envs * args.steps
    shape = dict(hidden_dim=128, constraint_hidden_dim=150, constraint_slack=[0.05, 0.05, 0.05, 0.05, 0.01, 0.01] * 2)
    pretrained = PRETRAINED
    if args.pretrain_epochs > 0:        # safe_explorer_ppo_quadrotor_2D_pretrain.yaml's batch, steps per epoch and learning rate
        pre = make('safe_explorer_ppo', env_func, training=True, output_dir=os.path.join(out, 'pretrain'),
                   checkpoint_path=os.path.join(out, 'pretrain', 'model_latest.pt'), seed=args.seed, pretraining=True, fused_pretrain=True,
                   rollout_batch_size=min(args.envs, 256), constraint_epochs=args.pretrain_epochs, constraint_steps_per_epoch=3000,
                   constraint_batch_size=256, constraint_lr=1e-4, eval_interval=0, log_interval=max(args.pretrain_epochs // 10, 1), **shape)
        assert pre.impl._fused_pretrain, 'the fused pre-training did not engage'
        pre.reset()
        t0 = time.perf_counter()
        for h in pre.learn():
            print(json.dumps({'pretrain_epoch': h['step'], 'mean_constraint_loss': float(np.mean([h[f'constraint_{i}_loss'] for i in range(12)]))}),
                  flush=True)
        print(json.dumps({'pretrain_seconds': time.perf_counter() - t0, 'epochs': pre.total_steps}), flush=True)
        pre.close()
        pretrained = os.path.join(out, 'pretrain')
    ctrl = make('safe_explorer_ppo', env_func, training=True, output_dir=out, checkpoint_path=os.path.join(out, 'model_latest.pt'),
                seed=args.seed, pretraining=False, pretrained=pretrained, fused_rollout=True, **shape, rollout_batch_size=args.envs, rollout_steps=args.steps,
                mini_batch_size=per_iter // 4, opt_epochs=4, max_env_steps=args.iterations * per_iter)
    assert ctrl.impl._fused_safe is not None, 'the fused collector did not engage'
    ctrl.reset()
    t0 = time.perf_counter()
    while ctrl.total_steps < args.iterations * per_iter:
        res = ctrl.train_step()
        print(json.dumps({'step': ctrl.total_steps, 'policy_loss': res.get('policy_loss'),
                          'env_steps_per_s': ctrl.total_steps / (time.perf_counter() - t0)}), flush=True)
    torch.cuda.synchronize()
    ev = ctrl.run(n_episodes=args.eval_episodes)
    print(json.dumps({'train_seconds': time.perf_counter() - t0, 'env_steps': ctrl.total_steps,
                      'eval_mean_return': float(np.mean(ev['ep_returns'])), 'eval_mean_length': float(np.mean(ev['ep_lengths']))}))
    ctrl.close()


if __name__ == '__main__':
    main()
