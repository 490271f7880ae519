#!/usr/bin/env python3
"""The checkpoint schema of the two off-policy trainers -> tests/golden/offpolicy_checkpoint_schema.json.

    python tests/golden/make_offpolicy_checkpoint_schema.py      (CPU only; no reference checkout needed)

Recorded at commit f0d5b96 ("Pin the step kernels off their fast paths; test scg_step_range"), the last one in which sac.py and
ddpg.py each carried their own trainer: the fixture is what THAT code wrote, and tests/test_offpolicy_cpu.py holds the shared
trainer (safe_control_gym_amd/offpolicy.py) to it.  Re-record only from a commit whose checkpoint format is the intended one.

A schema is the nested key tree of a checkpoint file with, per leaf, its type and (tensors, arrays) dtype and shape — no values.
Each case is a trainer of 4 envs, hidden 32 and a ring of 64 over the replayed transitions of tests/golden/ddpg_collector.npz
(tests/replay_env.py), run for 6 vector steps: across the warm-up boundary (8 transitions) and through four updates.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

COMMIT = 'f0d5b96'
OUT = os.path.join(HERE, 'offpolicy_checkpoint_schema.json')
TASK = dict(episode_len_sec=0.2, randomized_init=True, done_on_out_of_bound=True)
NOISE = {'ou': {'func': 'OrnsteinUhlenbeckProcess', 'std': {'func': 'LinearSchedule', 'args': 0.2}},
         'gaussian': {'func': 'GaussianProcess', 'std': {'func': 'LinearSchedule', 'args': 0.3, 'end': 0.05, 'steps': 50}}}
STEPS = 6


def replay_env():
    """4 envs x 40 recorded vector steps; its 'random state' is the replay position, so that a checkpoint resumes the env too."""
    from tests.replay_env import ReplayVecEnv, spec_for
    G = np.load(os.path.join(HERE, 'ddpg_collector.npz'))
    tr = {k: G[f'transitions/{k}'] for k in ('next_obs', 'rew', 'done', 'trunc', 'term_obs')}
    env = ReplayVecEnv(spec_for(TASK), 'cpu', G['obs0'], tr['next_obs'], tr['rew'], tr['done'], tr['trunc'], tr['term_obs'])
    env.get_env_random_state = lambda: {'t': env.t}
    env.set_env_random_state = lambda state: setattr(env, 't', int(state['t']))
    return env


def build_trainer(algo, noise='ou', norm=False, seed=3):
    """algo: 'sac' | 'ddpg'.  The PyTorch collector and the eager update (CPU)."""
    from safe_control_gym_amd import ddpg, sac
    extra = {'cuda_graphs': False, 'updates_per_step': 2}
    if norm:
        extra.update(norm_obs=True, norm_reward=True)
    kw = dict(hidden_dim=32, activation='relu', rollout_batch_size=4, warm_up_steps=8, train_interval=4, train_batch_size=16,
              max_buffer_size=64, extra=extra)
    if algo == 'sac':
        return sac.SAC(replay_env(), sac.SACConfig(use_entropy_tuning=True, **kw), seed=seed)
    return ddpg.DDPG(replay_env(), ddpg.DDPGConfig(random_process=NOISE[noise], **kw), seed=seed)


def schema(x):
    """Containers as {type name: children}; leaves as a string of type, dtype and shape."""
    if torch.is_tensor(x):
        return f'Tensor {x.dtype} {list(x.shape)}'
    if isinstance(x, np.ndarray):
        return f'ndarray {x.dtype} {list(x.shape)}'
    if isinstance(x, dict):
        return {type(x).__name__: {str(k): schema(v) for k, v in x.items()}}
    if isinstance(x, (list, tuple)):
        return {type(x).__name__: [schema(v) for v in x]}
    return type(x).__name__


def cases():
    """(name, algo, trainer keywords, save keywords)"""
    out = []
    for algo, noises in (('sac', (None,)), ('ddpg', ('ou', 'gaussian'))):
        for noise in noises:
            tag = algo if noise is None else f'{algo}-{noise}'
            kw = {} if noise is None else {'noise': noise}
            for training in (True, False):
                for save_buffer in (True, False):
                    out.append((f'{tag}-training{int(training)}-buffer{int(save_buffer)}', algo, kw, dict(training=training, save_buffer=save_buffer)))
            out.append((f'{tag}-normalised', algo, dict(kw, norm=True), dict(training=True, save_buffer=False)))
    return out


def checkpoint_schemas(tmp_dir):
    """{case name: schema of the file `save` wrote}; one trainer per (algo, trainer keywords), saved in every way asked for."""
    trainers, out = {}, {}
    for name, algo, kw, save_kw in cases():
        key = (algo, tuple(sorted(kw.items())))
        if key not in trainers:
            t = trainers[key] = build_trainer(algo, **kw)
            results = [t.train_step() for _ in range(STEPS)]
            assert 'updates' not in results[1] and sum(r.get('updates', 0) for r in results) == 8
        path = os.path.join(tmp_dir, name + '.pt')
        trainers[key].save(path, **save_kw)
        out[name] = schema(torch.load(path, map_location='cpu', weights_only=False))
    return out


if __name__ == '__main__':
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        got = checkpoint_schemas(tmp)
    with open(OUT, 'w') as f:
        json.dump({'recorded_at': COMMIT, 'cases': got}, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{len(got)} cases -> tests/golden/offpolicy_checkpoint_schema.json')
