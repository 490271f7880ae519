#!/usr/bin/env python3
"""Known answers of the reference's DDPG, produced by running the reference's own classes.

    python tests/golden/make_ddpg.py             (build container only: needs the reference checkout)

controllers/ddpg/ddpg_utils.py (DDPGAgent.update, MLPActorCritic) and math_and_models/random_processes.py / schedule.py are pure
torch / NumPy and import under tests/golden/ref_stubs.py.  Upstream's make_action_noise_process calls eval('LinearSchedule') and
eval('OrnsteinUhlenbeckProcess') inside ddpg_utils, which imports neither (DDPG(...) raises NameError with its own default config);
this generator injects both names into ddpg_utils' namespace before it runs anything, so the fixture records the intended behaviour.

Cases written to tests/golden/ddpg.npz:
  agent/<case>/...   initial ac / ac_targ weights, the three batches fed, the weights, target weights, Adam exp_avg / exp_avg_sq / step
                     and loss statistics after three DDPGAgent.update calls (CPU)
  noise/<kind>/...   the normal draws, the samples over 3 vector steps of 7 envs, reset_states, state_dict
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import ref_stubs  # noqa: E402

ref_stubs.install()

import torch  # noqa: E402
from gymnasium.spaces import Box  # noqa: E402

from safe_control_gym.controllers.ddpg import ddpg_utils  # noqa: E402
from safe_control_gym.math_and_models import random_processes, schedule  # noqa: E402

ddpg_utils.LinearSchedule = schedule.LinearSchedule                                  # the NameError fix-up (see the docstring)
ddpg_utils.OrnsteinUhlenbeckProcess = random_processes.OrnsteinUhlenbeckProcess
ddpg_utils.GaussianProcess = random_processes.GaussianProcess

# (name, obs_dim, act_dim, hidden, activation, low, high, hyper-parameters, batch)
CASES = [('h32_tanh', 6, 1, 32, 'tanh', [-0.5], [2.0], {}, 64),
         ('h64_relu', 10, 4, 64, 'relu', [-1.0] * 4, [1.0] * 4, {'gamma': 0.95, 'tau': 0.02, 'actor_lr': 3e-3, 'critic_lr': 2e-3}, 96)]


def flat_sd(sd, prefix):
    return {f'{prefix}/{k}': v.detach().cpu().numpy().copy() for k, v in sd.items()}


def agent_case(out, name, obs_dim, act_dim, hidden, act, low, high, hp, batch):
    torch.manual_seed(11)
    obs_space = Box(-1, 1, (obs_dim,))
    act_space = Box(np.array(low, np.float32), np.array(high, np.float32))
    agent = ddpg_utils.DDPGAgent(obs_space, act_space, hidden_dim=hidden, activation=act, **hp)
    p = f'agent/{name}'
    out.update(flat_sd(agent.ac.state_dict(), f'{p}/init/ac'))
    out.update(flat_sd(agent.ac_targ.state_dict(), f'{p}/init/ac_targ'))
    rng = np.random.default_rng(7)
    stats = []
    for k in range(3):
        b = {'obs': rng.normal(0, 1, (batch, obs_dim)).astype(np.float32),
             'act': rng.uniform(low, high, (batch, act_dim)).astype(np.float32),
             'rew': rng.normal(0, 1, (batch, 1)).astype(np.float32),
             'next_obs': rng.normal(0, 1, (batch, obs_dim)).astype(np.float32),
             'mask': (rng.uniform(size=(batch, 1)) > 0.2).astype(np.float32)}
        for key, v in b.items():
            out[f'{p}/batch{k}/{key}'] = v
        res = agent.update({key: torch.as_tensor(v) for key, v in b.items()})
        stats.append([res['policy_loss'], res['critic_loss']])
    out[f'{p}/stats'] = np.array(stats, np.float64)
    out.update(flat_sd(agent.ac.state_dict(), f'{p}/final/ac'))
    out.update(flat_sd(agent.ac_targ.state_dict(), f'{p}/final/ac_targ'))
    for oname, opt, module in (('actor_opt', agent.actor_opt, agent.ac.actor), ('critic_opt', agent.critic_opt, agent.ac.q)):
        names = dict((id(t), n) for n, t in module.named_parameters())
        for prm in opt.param_groups[0]['params']:
            st = opt.state[prm]
            n = names[id(prm)]
            out[f'{p}/final/{oname}/{n}/exp_avg'] = st['exp_avg'].numpy().copy()
            out[f'{p}/final/{oname}/{n}/exp_avg_sq'] = st['exp_avg_sq'].numpy().copy()
            out[f'{p}/final/{oname}/{n}/step'] = np.float64(float(st['step']))
    out[f'{p}/meta'] = np.array([obs_dim, act_dim, hidden, batch], np.int64)
    out[f'{p}/act'] = np.array(act)
    out[f'{p}/low'], out[f'{p}/high'] = np.array(low, np.float32), np.array(high, np.float32)
    hpv = dict({'gamma': 0.99, 'tau': 0.005, 'actor_lr': 0.001, 'critic_lr': 0.001}, **hp)
    out[f'{p}/hp'] = np.array([hpv['gamma'], hpv['tau'], hpv['actor_lr'], hpv['critic_lr']], np.float64)


def noise_case(out, kind, config, act_dim=3, n_env=7, n_step=3):
    np.random.seed(23)
    draws = np.random.randn(n_env * n_step + 4, act_dim)          # what the process will draw, recorded first
    np.random.seed(23)
    proc = ddpg_utils.make_action_noise_process(dict(config, std=dict(config['std'])), Box(-np.ones(act_dim), np.ones(act_dim)))
    samples = np.stack([np.stack([proc.sample() for _ in range(n_env)]) for _ in range(n_step)])
    p = f'noise/{kind}'
    out[f'{p}/draws'] = draws[:n_env * n_step]
    out[f'{p}/samples'] = samples
    sd = proc.state_dict()
    if 'x_prev' in sd:
        out[f'{p}/state/x_prev'] = np.asarray(sd['x_prev'], np.float64)
        out[f'{p}/state/std_current'] = np.float64(sd['std']['current'])
        proc.reset_states()
        out[f'{p}/reset/x_prev'] = np.asarray(proc.x_prev, np.float64)
        out[f'{p}/after_reset'] = proc.sample()                   # draw n_env * n_step of the recorded stream
        out[f'{p}/draw_after_reset'] = draws[n_env * n_step]


def main():
    out = {}
    for c in CASES:
        agent_case(out, *c)
    noise_case(out, 'ou', {'func': 'OrnsteinUhlenbeckProcess', 'std': {'func': 'LinearSchedule', 'args': 0.3, 'end': 0.05, 'steps': 50}})
    noise_case(out, 'gaussian', {'func': 'GaussianProcess', 'std': {'func': 'LinearSchedule', 'args': 0.3, 'end': 0.05, 'steps': 50}})
    path = os.path.join(HERE, 'ddpg.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {len(out)} arrays')


if __name__ == '__main__':
    main()
