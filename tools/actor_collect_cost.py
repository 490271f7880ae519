#!/usr/bin/env python3
"""Cost of SAC's fused training collection on one GPU -> profiles/actor_collect_cost.json.  One chunk of 25 policy-mode vector steps
(upstream's sac.yaml: 4 envs, an update every 100 env steps) of SAC hidden 128 relu on Quadrotor 3D tracking as shipped, at 4, 256 and
2 048 envs, same process, same device, alternating runs:
  (a) chunked    ONE scg_rollout_sac_collect launch + its one-thread bookkeeping launch (OffPolicyTrainer._collect_chunk);
  (b) stepwise   the graph-replayed stepwise fused collector doing the same 25 steps (OffPolicyTrainer._collect: 25 replays of the
                 captured scg_sac_sample, env step, scg_sac_push — 100 launches), whose code the chunked path does not touch.
Each has a trainer and an env of its own (same task, same seed).  A sample is the host clock around `--chunks` chunks enqueued back to
back and one device synchronise, divided by the number of chunks: what a training loop that does not read statistics back pays per
chunk.  Reported: the median over `--reps` alternating samples and their (min, max).

usage: actor_collect_cost.py [--out profiles/actor_collect_cost.json] [--reps 15] [--chunks 40] [--envs 4 256 2048]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from safe_control_gym_amd.registration import load_task  # noqa: E402
from safe_control_gym_amd.sac import SAC, SACConfig  # noqa: E402
from safe_control_gym_amd.vec_env import HipVecEnv  # noqa: E402
from tests import actor_collect_cases as acc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'actor_collect_cost.json'))
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--chunks', type=int, default=40)
    ap.add_argument('--envs', type=int, nargs='*', default=list(acc.COST_ENVS))
    a = ap.parse_args()
    env_id, cfg = load_task(acc.COST_TASK)
    hidden, act = acc.COST_SHAPE
    K = acc.COST_STEPS
    rows = []
    for N in a.envs:
        def trainer(policy, **extra):
            env = HipVecEnv(env_id, N, seed=7, return_numpy=False, policy=policy, **cfg)
            scfg = SACConfig(hidden_dim=hidden, activation=act, warm_up_steps=0, train_interval=K * N, max_buffer_size=1_000_000, extra=extra)
            return SAC(env, scfg, seed=7)
        chunked, stepwise = trainer((hidden, act, 'sac'), collect_steps=K), trainer(None)
        assert chunked._collect_k == K and stepwise._fused_collect and stepwise._graph_collect and not stepwise._collect_k

        def run_chunked():
            chunked._collect_chunk(K, False)
            chunked.buffer.advance_host(K * N)

        def run_stepwise():
            for _ in range(K):
                stepwise._collect(False)
                stepwise.buffer.advance_host(N)
        fns = dict(chunked=run_chunked, stepwise=run_stepwise)
        for fn in fns.values():                         # warm-up: kernel attributes, the two eager steps and the graph capture
            fn(); fn()
        torch.cuda.synchronize()
        assert stepwise._collect_graphs and all(g['g'] is not None for g in stepwise._collect_graphs.values())
        t = {k: [] for k in fns}
        for _ in range(a.reps):                         # alternating
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.chunks):
                    fn()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / a.chunks * 1e6)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = dict(task=acc.COST_TASK, hidden=hidden, activation=act, envs=N, steps=K, reps=a.reps, chunks_per_sample=a.chunks,
                   chunked_us=med['chunked'], stepwise_us=med['stepwise'], stepwise_over_chunked=med['stepwise'] / med['chunked'],
                   spread_us={k: [min(v), max(v)] for k, v in t.items()}, ring_rows=dict(chunked=chunked.buffer.size, stepwise=stepwise.buffer.size))
        assert chunked.buffer.size == stepwise.buffer.size and bool(torch.isfinite(chunked.buffer.obs[:chunked.buffer.size]).all())
        print(json.dumps(row), flush=True)
        rows.append(row)
        chunked.env.close()
        stepwise.env.close()
        del chunked, stepwise, fns
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0),
                   'method': 'host clock around `chunks_per_sample` chunks of 25 policy-mode vector steps enqueued back to back and one device '
                             'synchronise, per chunk; medians and (min, max) over alternating samples, same process; each path on a trainer '
                             'and an env of its own', 'rows': rows}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
