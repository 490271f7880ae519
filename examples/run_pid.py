#!/usr/bin/env python3
"""The PID baseline on a batch: the shipped Quadrotor 2D tracking task flown by N envs at once, each with its own (P_z, D_z) pair of
position gains from a grid, in ONE launch; prints the best and the worst tracking RMSE of the grid.

usage: run_pid.py [--envs 1024] [--dtype float64]"""
import argparse
import os
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from safe_control_gym_amd.registration import get_config, load_task, make  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=1024)
    ap.add_argument('--dtype', default='float64')
    a = ap.parse_args()
    env_id, cfg = load_task('quadrotor_2D_track')
    cfg.update(cost='quadratic', normalized_rl_action_space=False, randomized_init=False, done_on_out_of_bound=True, constraints=None,
               init_state={'init_x': 0.0, 'init_z': 1.0})
    ctrl = make('pid', partial(make, env_id, **cfg), num_envs=a.envs, dtype=a.dtype, **get_config('pid'))
    side = int(np.ceil(np.sqrt(a.envs)))
    pz, dz = np.meshgrid(np.linspace(0.4, 3.0, side), np.linspace(0.1, 1.2, side))
    gains = np.tile(ctrl.default_gains(), (a.envs, 1))
    gains[:, 2], gains[:, 8] = pz.reshape(-1)[:a.envs], dz.reshape(-1)[:a.envs]           # P_COEFF_FOR[z], D_COEFF_FOR[z]
    ctrl.set_gains(gains)
    res = ctrl.run()
    rmse = np.sqrt(res['mse'])
    flown = res['ep_lengths'] == ctrl.max_steps
    best, worst = int(np.argmin(np.where(flown, rmse, np.inf))), int(np.argmax(np.where(flown, rmse, -np.inf)))
    print(f'{a.envs} gain sets, {int(flown.sum())} flew the whole {ctrl.max_steps}-step episode')
    for tag, i in (('best', best), ('worst', worst)):
        print(f'{tag}: P_z = {gains[i, 2]:.3f}, D_z = {gains[i, 8]:.3f}: RMSE {rmse[i]:.4f} m, return {res["ep_returns"][i]:.2f}')
    d = int(np.argmin(np.abs(gains[:, 2] - 1.25) + np.abs(gains[:, 8] - 0.5)))
    print(f'nearest to the default (1.25, 0.5): P_z = {gains[d, 2]:.3f}, D_z = {gains[d, 8]:.3f}: RMSE {rmse[d]:.4f} m')
    ctrl.close()


if __name__ == '__main__':
    main()
