"""bench.py on one GPU: --steps is the number of timed steps (also when it is not a multiple of --graph-len), and --dump-outputs
writes the last timed step's outputs, identical from run to run and with or without --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(dump, steps, graph_len, envs=4096, extra=('--full', '--no-secondary', '--no-cpu-baseline')):
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', '7', '--graph-len', str(graph_len),
           '--envs', str(envs), *extra, '--dump-outputs', str(dump)]
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


def test_plain_bench_is_the_headline_alone_and_dumps_what_full_dumps(tmp_path):
    """Without --full the line is the headline alone, whatever the other options ask for (no roofline, output check, legs or CPU
    baseline), and the dumped outputs are those of a --full run: what --full adds runs after the dump."""
    envs = 4096
    full = _bench(tmp_path / 'full', 1200, 500, envs)
    plain = _bench(tmp_path / 'plain', 1200, 500, envs, extra=())
    assert set(plain) == {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                          'vs_baseline', 'dtype', 'data', 'config'}
    assert set(full) - set(plain) == {'roofline'} and set(full['config']) - set(plain['config']) == {'finite_outputs'}
    for k in ('metric', 'unit', 'n_gpus', 'steps', 'warmup', 'higher_is_better', 'dtype'):
        assert plain[k] == full[k], k
    assert plain['steps'] == 1200 and plain['ms_per_step'] > 0
    assert plain['value'] == pytest.approx(envs * 1200 / (plain['ms_per_step'] * 1e-3 * 1200), rel=1e-9)
    names = sorted(os.listdir(tmp_path / 'full'))
    assert names == sorted(os.listdir(tmp_path / 'plain')) and 'obs.npy' in names
    for f in names:
        np.testing.assert_array_equal(np.load(tmp_path / 'plain' / f), np.load(tmp_path / 'full' / f), err_msg=f)
