#!/usr/bin/env python3
"""Known answers of the reference's DDPG COLLECTOR, produced by running its own class: controllers/ddpg/ddpg.py `DDPG.train_step`
(:271-341) on the reference's Quadrotor (2-D tracking, 10-step episodes so that time-limit truncations occur, `done_on_out_of_bound`
on so that real terminations occur too), 4 envs x 40 vector steps, a warm-up of 8 env steps (two vector steps of
action_space.sample()), no gradient updates (train_interval beyond the run), the default Ornstein-Uhlenbeck noise on.

Upstream's make_action_noise_process calls eval('LinearSchedule') / eval('OrnsteinUhlenbeckProcess') inside ddpg_utils, which imports
neither: DDPG(...) raises NameError with its own default config.  This generator injects both names into ddpg_utils' namespace before
constructing the controller, so the recording shows the intended behaviour.

Recorded: every transition `env.step` returned (tests/replay_env.py replays them), the actions the reference fed (uniform warm-up
draws, then its actor's float32 output + the noise, added in place), the actor's output alone, the N(0, 1) draws the noise process
consumed (in call order: one sample() per env, env order, vector step after vector step), the noise samples, the actor's weights
(hidden width 32, a shape the fused library serves; no update happens, so they are the weights of every step), the process's state
afterwards, and what the reference's DDPGBuffer holds — obs, the noisy UNCLIPPED act, rew, and the TRUE next_obs / mask of the
time-limit fix-up.

    python tests/golden/make_ddpg_collector.py       (build container only: needs the reference checkout) -> ddpg_collector.npz
"""
import functools
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_adversarial as A  # noqa: E402  (stubs, tensorboard stand-in, reference imports)

import torch  # noqa: E402
import yaml  # noqa: E402

OVER = dict(episode_len_sec=0.2, randomized_init=True, done_on_out_of_bound=True)


class _RecordingNumpy:
    """Stands in for `np` inside math_and_models/random_processes.py: every np.random.randn call is recorded."""

    def __init__(self, log):
        self._log = log
        self.random = self

    def randn(self, *size):
        x = np.random.randn(*size)
        self._log.append(np.asarray(x, dtype=np.float64).copy())
        return x

    def __getattr__(self, name):
        return getattr(np, name)


def main():
    from safe_control_gym.controllers.ddpg import ddpg_utils
    from safe_control_gym.math_and_models import random_processes, schedule
    import safe_control_gym.controllers.ddpg.ddpg as mod
    ddpg_utils.LinearSchedule = schedule.LinearSchedule                  # the NameError fix-up (see the docstring)
    ddpg_utils.OrnsteinUhlenbeckProcess = random_processes.OrnsteinUhlenbeckProcess
    draws = []
    random_processes.np = _RecordingNumpy(draws)
    cfg = yaml.safe_load(open(os.path.join(A.REF, 'safe_control_gym/controllers/ddpg/ddpg.yaml')))
    cfg.update(hidden_dim=32, activation='relu', rollout_batch_size=4, warm_up_steps=8, train_interval=10 ** 9, max_buffer_size=120,
               num_workers=1, tensorboard=False)
    tc = yaml.safe_load(open(os.path.join(A.REF, 'examples/rl/config_overrides/quadrotor_2D/quadrotor_2D_track.yaml')))['task_config']
    tc.update(OVER)
    tc.pop('seed', None)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        env_func = functools.partial(A.make, 'quadrotor', output_dir=tmp, **tc)
        torch.manual_seed(4)
        ctrl = mod.DDPG(env_func, training=True, output_dir=tmp, use_gpu=False, seed=6, **cfg)
        raw0 = []
        reset0 = ctrl.env.reset
        ctrl.env.reset = lambda *a, **k: (lambda r: (raw0.append(np.asarray(r[0], dtype=float).copy()), r)[1])(reset0(*a, **k))
        ctrl.reset()
        ctrl.env.reset = reset0
        out['obs0'] = raw0[0]
        out.update(A.flat_sd(ctrl.agent.ac.state_dict(), 'ac'))
        policy, samples = [], []
        act0 = ctrl.agent.ac.act
        ctrl.agent.ac.act = lambda obs, **kw: (lambda a: (policy.append(a.copy()), a)[1])(act0(obs, **kw))
        sample0 = ctrl.noise_process.sample
        ctrl.noise_process.sample = lambda: (lambda x: (samples.append(np.asarray(x, dtype=np.float64).copy()), x)[1])(sample0())
        steps, T = [], 40
        env = ctrl.env
        orig = env.__class__.step

        def rec_step(act):
            nxt, rew, done, info = orig(env, act)
            trunc = np.zeros(len(done), dtype=bool)
            term = np.zeros_like(nxt)
            for i, inf in enumerate(info['n']):
                if 'terminal_info' in inf:
                    term[i] = inf['terminal_observation']
                    trunc[i] = bool(inf['terminal_info'].get('TimeLimit.truncated', False))
            steps.append({'act': np.asarray(act).copy(), 'next_obs': nxt.copy(), 'rew': np.asarray(rew, dtype=float).copy(),
                          'done': np.asarray(done).copy(), 'trunc': trunc, 'term_obs': term})
            return nxt, rew, done, info
        env.step = rec_step
        for _ in range(T):
            ctrl.train_step()
        for k in steps[0]:
            out[f'transitions/{k}'] = np.stack([s[k] for s in steps])
        out['policy_act'] = np.stack(policy)                    # [T - warm-up steps][N][act_dim], float32
        out['noise/draws'] = np.stack(draws)                    # [(T - warm-up) N][act_dim]
        out['noise/samples'] = np.stack(samples)
        sd = ctrl.noise_process.state_dict()
        out['noise/x_prev'], out['noise/std_current'] = np.asarray(sd['x_prev'], np.float64), np.float64(sd['std']['current'])
        b = ctrl.buffer
        for k in ('obs', 'act', 'rew', 'next_obs', 'mask'):
            out[f'buffer/{k}'] = np.asarray(b.__dict__[k], dtype=np.float64).copy()
        out['buffer/pos_size'] = np.array([b.pos, b.buffer_size])
        out['total_steps'] = np.array(ctrl.total_steps)
        out['warm_vector_steps'] = np.array(T - len(policy))
    d, tr = out['transitions/done'], out['transitions/trunc']
    print('vector steps', T, 'warm-up', int(out['warm_vector_steps']), 'dones', int(d.sum()), 'truncations', int(tr.sum()),
          'terminations', int((d & ~tr).sum()), 'buffer pos/size', out['buffer/pos_size'].tolist(), 'act dtype', out['transitions/act'].dtype)
    assert tr.sum() > 0 and (d & ~tr).sum() > 0 and out['noise/draws'].shape[0] == (T - int(out['warm_vector_steps'])) * 4
    np.savez_compressed(os.path.join(HERE, 'ddpg_collector.npz'), **out)
    print('ddpg_collector.npz written,', len(out), 'arrays')


if __name__ == '__main__':
    main()
