#!/usr/bin/env python3
"""Evaluate a SAC policy on N CartPole envs in ONE kernel launch (scg_rollout_actor), and once more behind the CBF safety filter
(scg_rollout_cbf_actor).  Loads a checkpoint, or trains briefly when none is given.  Prints the mean return, the share of episodes
that violate a constraint, and the filter's statistics.

usage: run_sac_eval.py [--envs 4096] [--seed 42] [--checkpoint model.pt] [--train-steps 20000] [--hidden 64]"""
import argparse
import copy
import json
import os
import shutil
import sys
import tempfile
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--checkpoint', default=None)
    ap.add_argument('--train-steps', type=int, default=20000)
    ap.add_argument('--hidden', type=int, default=64, help='32, 64, 96, 128 or 256; 256 (upstream\'s default width) implies the controller key wide_actor=True: the agent trains in PyTorch, both '
                         'evaluation legs are still one launch each')
    a = ap.parse_args()
    from safe_control_gym_amd.registration import make
    with open(os.path.join(ROOT, 'tests', 'golden', 'cbf_settings.json')) as f:
        s = json.load(f)                         # the reference's examples/cbf task and filter settings
    cfg = dict(s['task_config'], randomized_init=True)
    cfg.pop('seed', None)
    env_func = partial(make, s['task'], **cfg)
    out = tempfile.mkdtemp()
    wide = dict(wide_actor=True) if a.hidden == 256 else {}
    ctrl = make('sac', env_func, training=True, output_dir=out, checkpoint_path=os.path.join(out, 'model_latest.pt'), seed=a.seed,
                hidden_dim=a.hidden, activation='leaky_relu', fused_rollout=True, max_env_steps=a.train_steps, warm_up_steps=min(1000, a.train_steps // 2), **wide)
    if a.checkpoint:
        ctrl.load(a.checkpoint)
    else:
        ctrl.reset()
        ctrl.learn()
    sf = make('cbf', env_func, **copy.deepcopy(s['sf_config']))
    legs = (('unfiltered', None), ('filtered', sf)) if ctrl.impl._fused_rollout else (('unfiltered', None),)
    for name, filt in legs:
        res = ctrl.run(n_episodes=a.envs, safety_filter=filt)
        line = f"{name}: {a.envs} episodes, mean return {res['ep_returns'].mean():.3f}, mean length {res['ep_lengths'].mean():.1f}, " \
               f"episodes with a violation {(res['constraint_violation'] > 0).mean():.4f}"
        if filt is not None:
            d = res['safety_filter_data']
            line += f", corrected steps {d['corrected_steps'].sum() / d['steps'].sum():.4f}, infeasible steps {d['infeasible_steps'].sum() / d['steps'].sum():.4f}"
        print(line)
    ctrl.close()
    shutil.rmtree(out, ignore_errors=True)


if __name__ == '__main__':
    main()
