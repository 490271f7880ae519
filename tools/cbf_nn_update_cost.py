#!/usr/bin/env python3
"""What training the cbf_nn residual network costs with and without the fused Adam steps (scg_cbf_nn_update), measured, not promised.

  steps     200 Adam steps at batch 64 on a filled buffer: one update_rows() call (fused_update=True) against the eager loop of
            update(buf.gather(idx)) the default path runs — the same indices, the same box, alternating samples
  learn     one whole learn() episode at 256 envs (reset, one 250-step launch, the push, train_iterations = 200 steps) both ways
  kernels   the two kernels' device times from a rocprofv3 --kernel-trace --stats run of their own (a child process that runs
            `--trace-target`: 3 x 200 fused steps and nothing else), against the step's arithmetic (13 M multiply-adds at batch 64) and parameter traffic
            (read p, m, v + write p, m, v of 67 586 words: 1.6 MB; parameters alone 0.8 MB)

Setup: the reference's examples/cbf task (tests/golden/cbf_nn_settings.json) and the fixture's residual weights; the buffer holds
256 x 248 rows of a learn() episode.  Wall clock around each piece with the device synchronised (the eager loop is host-bound: wall
clock is what a caller waits for) and device-event times; medians of --reps alternating repeats after --warmup rounds.  Writes
profiles/cbf_nn_update_cost.json (or --out).

usage: cbf_nn_update_cost.py [--reps 15] [--warmup 2] [--steps 200] [--batch 64] [--envs 256] [--no-trace] [--out profiles/cbf_nn_update_cost.json]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import cbf_nn_cases as CN  # noqa: E402
from tests import cbf_nn_model as NM  # noqa: E402

FMA_PER_ROW = 3 * (4 * 256 + 256 * 256 + 2 * 256)             # forward, data gradient, weight gradient: one multiply-add each per weight
FLOP_PER_ROW = 2 * FMA_PER_ROW
PARAM_WORDS = 67586


def stats(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'all': [float(x) for x in v]}


def make_filter(**over):
    import torch
    from safe_control_gym_amd.registration import make
    S = CN.settings()
    D = np.load(os.path.join(CN.GOLDEN, 'cbf_nn.npz'))
    env_id, cfg = CN.task_config(False)
    sf = make('cbf_nn', partial(make, env_id, **cfg), **dict(S['sf_config'], **over))
    sf.mlp.load_state_dict({k: torch.tensor(D['mlp/' + k]) for k in NM.KEYS})
    return sf


def filled(sf, envs, steps):
    """One learn() episode's rows in the filter's buffer (no training: train_iterations is put back afterwards)."""
    keep, sf.train_iterations = sf.train_iterations, 0
    sf.learn(num_envs=envs)
    sf.train_iterations = keep
    return sf.buffer


def both(fn):
    """(wall ms, device ms) of fn(), the device idle before and after."""
    import torch
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t0 = time.perf_counter()
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, ev[0].elapsed_time(ev[1])


def trace_target(a):
    import torch
    on = make_filter(fused_update=True, num_episodes=1, max_num_steps=a.episode_steps, train_batch_size=a.batch)
    buf = filled(on, a.envs, a.episode_steps)
    idx = np.random.default_rng(0).integers(0, len(buf), size=(a.steps, a.batch))
    for _ in range(3):
        on.update_rows(idx)
    torch.cuda.synchronize()
    on.close()


def kernel_stats(a):
    """The fused step's two kernels under rocprofv3, in a child process of its own; None when the profiler is not installed."""
    if shutil.which('rocprofv3') is None:
        return None
    d = tempfile.mkdtemp(prefix='cbf_nn_update_kt_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'p', '--', sys.executable, os.path.abspath(__file__),
               '--trace-target', '--steps', str(a.steps), '--batch', str(a.batch), '--envs', str(a.envs), '--episode-steps', str(a.episode_steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            return {'error': f'rocprofv3 exit {r.returncode}', 'stderr_tail': r.stderr[-400:]}
        rows = [x for x in csv.DictReader(open(files[0])) if 'phase_a' in x['Name'] or 'phase_b' in x['Name']]
        out = {('phase_a' if 'phase_a' in x['Name'] else 'phase_b'): {'calls': int(x['Calls']), 'avg_us': float(x['AverageNs']) * 1e-3,
                                                                      'total_ms': float(x['TotalDurationNs']) * 1e-6} for x in rows}
        if set(out) == {'phase_a', 'phase_b'}:
            out['step_us'] = out['phase_a']['avg_us'] + out['phase_b']['avg_us']
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--episode-steps', type=int, default=250)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-target', action='store_true', help='run the fused steps only (the program rocprofv3 traces)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cbf_nn_update_cost.json'))
    a = ap.parse_args()
    if a.trace_target:
        return trace_target(a)
    kt = None if a.no_trace else kernel_stats(a)        # (before this process opens the device)
    import torch
    from safe_control_gym_amd import _cbf_nn_update as U
    res = {'steps': a.steps, 'batch': a.batch, 'envs': a.envs, 'reps': a.reps, 'warmup': a.warmup, 'source_hash': f'0x{U.source_hash():016x}',
           'fma_per_step': FMA_PER_ROW * a.batch, 'flop_per_step': FLOP_PER_ROW * a.batch, 'param_bytes': 4 * PARAM_WORDS, 'optimiser_bytes_per_step': 6 * 4 * PARAM_WORDS}
    over = dict(num_episodes=1, max_num_steps=a.episode_steps, train_batch_size=a.batch, train_iterations=a.steps)
    on, off = make_filter(fused_update=True, **over), make_filter(**over)
    bufs = {k: filled(f, a.envs, a.episode_steps) for k, f in (('fused', on), ('eager', off))}
    res['device'] = torch.cuda.get_device_name(0)
    res['buffer_rows'] = len(bufs['fused'])
    idx = np.random.default_rng(0).integers(0, len(bufs['fused']), size=(a.steps, a.batch))

    def eager():
        for i in range(a.steps):
            off.update(bufs['eager'].gather(idx[i]))
    run = {'fused': lambda: on.update_rows(idx), 'eager': eager}
    t = {k: [] for k in run}
    for r in range(a.warmup + a.reps):
        for k in run:                                    # alternating
            v = both(run[k])
            if r >= a.warmup:
                t[k].append(v)
    case = {k + '_wall_ms': stats([w for w, _ in v]) for k, v in t.items()}
    case.update({k + '_device_ms': stats([d for _, d in v]) for k, v in t.items()})
    case['eager_over_fused_wall'] = case['eager_wall_ms']['median'] / case['fused_wall_ms']['median']
    case['fused_us_per_step_wall'] = case['fused_wall_ms']['median'] * 1e3 / a.steps
    case['fused_us_per_step_device'] = case['fused_device_ms']['median'] * 1e3 / a.steps
    case['eager_us_per_step_wall'] = case['eager_wall_ms']['median'] * 1e3 / a.steps
    res['steps_case'] = case
    print(f"{a.steps} Adam steps at batch {a.batch}: fused {case['fused_wall_ms']['median']:.2f} ms wall ({case['fused_device_ms']['median']:.2f} ms device), "
          f"eager {case['eager_wall_ms']['median']:.2f} ms wall: x{case['eager_over_fused_wall']:.1f}")
    t = {'fused': [], 'eager': []}
    for r in range(a.warmup + a.reps):
        for k, f in (('fused', on), ('eager', off)):
            v = both(lambda: f.learn(num_envs=a.envs))
            if r >= a.warmup:
                t[k].append(v[0])
    learn = {k + '_episode_wall_ms': stats(v) for k, v in t.items()}
    learn['eager_over_fused'] = learn['eager_episode_wall_ms']['median'] / learn['fused_episode_wall_ms']['median']
    res['learn_case'] = learn
    print(f"learn episode, {a.envs} envs, {a.steps} steps: fused {learn['fused_episode_wall_ms']['median']:.1f} ms, eager "
          f"{learn['eager_episode_wall_ms']['median']:.1f} ms: x{learn['eager_over_fused']:.1f}")
    res['kernels'] = kt if kt is not None else 'not measured (--no-trace, or rocprofv3 is not installed)'
    if isinstance(kt, dict) and 'step_us' in kt:
        kt['gflops_on_kernel_time'] = res['flop_per_step'] / (kt['step_us'] * 1e-6) * 1e-9
        kt['optimiser_gb_per_s_on_phase_b'] = res['optimiser_bytes_per_step'] / (kt['phase_b']['avg_us'] * 1e-6) * 1e-9
        print(f"kernels: phase_a {kt['phase_a']['avg_us']:.1f} us + phase_b {kt['phase_b']['avg_us']:.1f} us = {kt['step_us']:.1f} us per step "
              f"({kt['gflops_on_kernel_time']:.0f} GFLOP/s; phase_b moves its 1.6 MB at {kt['optimiser_gb_per_s_on_phase_b']:.0f} GB/s)")
    for f in (on, off):
        f.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fjson:
        json.dump(res, fjson, indent=1)
        fjson.write('\n')


if __name__ == '__main__':
    main()
