"""bench.py on one GPU: --steps is the number of timed steps (also when it is not a multiple of --graph-len), and --dump-outputs
writes the last timed step's outputs, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(dump, steps, graph_len, envs=4096):
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', '7', '--graph-len', str(graph_len),
           '--envs', str(envs), '--no-secondary', '--no-cpu-baseline', '--dump-outputs', str(dump)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def test_bench_times_exactly_steps_and_dumps_the_same_outputs_twice(tmp_path):
    envs = 4096
    runs = [_bench(tmp_path / 'a', 1500, 1000, envs), _bench(tmp_path / 'b', 1500, 1000, envs)]
    for r in runs:
        assert r['steps'] == 1500 and r['ms_per_step'] > 0 and r['config']['finite_outputs'] is True
        assert r['value'] == pytest.approx(envs * 1500 / (r['ms_per_step'] * 1e-3 * 1500), rel=1e-9)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert {'obs.npy', 'reward.npy', 'done.npy', 'flags.npy', 'terminal_obs.npy', 'fin_stats.npy'} <= set(names)
    assert names == sorted(os.listdir(tmp_path / 'b'))
    for f in names:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64) and envs in a.shape, (f, a.dtype, a.shape)        # (c_values: [rows, envs])
        assert np.isfinite(a).all(), f
        np.testing.assert_array_equal(a, b, err_msg=f)
    # a different number of steps leaves different outputs: the dump is the state after the timed steps, not after set-up
    _bench(tmp_path / 'c', 1499, 1000, envs)
    assert not np.array_equal(np.load(tmp_path / 'a' / 'obs.npy'), np.load(tmp_path / 'c' / 'obs.npy'))
