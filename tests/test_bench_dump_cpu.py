"""bench.py --dump-outputs, host side: what the writer puts on disk (no kernel launches)."""
import os

import numpy as np
import torch

import bench


def _outputs(n):
    g = torch.Generator().manual_seed(0)
    return {'obs': torch.randn(n, 12, generator=g), 'reward': torch.randn(n, generator=g, dtype=torch.float64),
            'done': torch.rand(n, generator=g) > 0.5, 'flags': torch.randint(0, 32, (n,), generator=g, dtype=torch.uint8),
            'c_values': torch.randn(16, n, generator=g), 'fin_stats': torch.randn(n, 4, generator=g)}


def test_dump_writes_every_output_as_float32_or_float64(tmp_path):
    t = _outputs(1000)
    bench.dump_outputs(str(tmp_path), t, 1000)
    assert sorted(os.listdir(tmp_path)) == sorted(f'{k}.npy' for k in t)
    for k, v in t.items():
        a = np.load(tmp_path / f'{k}.npy')
        assert a.dtype == (np.float64 if v.dtype == torch.float64 else np.float32)
        np.testing.assert_array_equal(a, v.numpy().astype(a.dtype))


def test_dump_over_the_limit_writes_one_fixed_seeded_sample_of_envs(tmp_path):
    t = _outputs(20000)
    limit = 200_000
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), t, 20000, limit=limit)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted([f'{k}.npy' for k in t] + ['env_index.npy'])
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= limit
    idx = np.load(tmp_path / 'a' / 'env_index.npy')
    assert idx.dtype == np.float64 and len(idx) > 100 and np.all(np.diff(idx) > 0)
    rows = idx.astype(np.int64)
    for k, v in t.items():
        a = np.load(tmp_path / 'a' / f'{k}.npy')
        np.testing.assert_array_equal(a, np.take(v.numpy(), rows, axis=1 if k == 'c_values' else 0).astype(a.dtype))
        np.testing.assert_array_equal(a, np.load(tmp_path / 'b' / f'{k}.npy'))     # same sample run to run
