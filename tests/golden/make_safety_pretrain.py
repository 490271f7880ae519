#!/usr/bin/env python3
"""Known answers of the reference's SafetyLayer.update (controllers/safe_explorer/safe_explorer_utils.py:86-118), produced by running the
reference's own class.

    python tests/golden/make_safety_pretrain.py     (build container only: needs /root/reference)

Two shapes (the library shapes the GPU tests already build), seeded synthetic transitions in a small ring, a fixed list of ring rows per
minibatch.  The reference's SafetyLayer runs the minibatches in float32 on the CPU, and once more in float64 from the same initial
parameters and data; per case the fixture holds, in scg_safety_update's flat layout (per constraint W1 | b1 | W2 | b2):

    <case>/dims            obs, A, C, Hc, batch, minibatches, ring rows
    <case>/lr
    <case>/init            [C, P] float32 initial parameters
    <case>/obs|act|c|c_next  the ring, float32
    <case>/rows            [minibatches, batch] int32 ring rows
    <case>/loss64, final64, m64, v64, grad64     the float64 run: per-minibatch losses, final parameters, Adam moments, the LAST
                                                  minibatch's gradients
    <case>/loss32          the float32 run's losses
    <case>/final32_d, m32_d, v32_d, grad32_d       the float32 run as int32 bit-pattern differences to float32(<float64 result>): small
                                                  integers (the two runs agree to a few units in the last place), which is what keeps the
                                                  file small; tests/safety_pretrain_model.py::load_case undoes it exactly.

tests/test_safety_pretrain_cpu.py holds the NumPy restatement (tests/safety_pretrain_model.py) to it; tests/test_gpu_safe_pretrain.py the
fused kernel.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import ref_stubs  # noqa: E402

ref_stubs.install()

from gymnasium.spaces import Box  # noqa: E402
from safe_control_gym.controllers.safe_explorer.safe_explorer_utils import SafetyLayer  # noqa: E402

# name: (obs, A, C, Hc, batch, minibatches, lr, ring rows, seed)
CASES = {'cartpole_stab': (4, 1, 8, 100, 33, 5, 1e-3, 40, 3), 'quadrotor_2D_track': (6, 2, 12, 16, 257, 4, 1e-3, 264, 4)}


def flat(tensors_of_model):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors_of_model])


def run(dims, init_sd, data, rows, lr, dtype):
    obs, A, C, Hc = dims
    layer = SafetyLayer(Box(-1, 1, (obs,)), Box(-1, 1, (A,)), hidden_dim=Hc, num_constraints=C, lr=lr, slack=0.05)
    layer.constraint_models.load_state_dict(init_sd)
    layer.constraint_models.to(dtype)
    layer.optimizers = [torch.optim.Adam(m.parameters(), lr=lr) for m in layer.constraint_models]
    losses = []
    for idx in rows:
        res = layer.update({k: torch.as_tensor(v[idx], dtype=dtype) for k, v in data.items()})
        losses.append([res[f'constraint_{i}_loss'] for i in range(C)])
    models, opts = layer.constraint_models, layer.optimizers
    return {'loss': np.array(losses, dtype=np.float64),
            'final': np.stack([flat(m.parameters()) for m in models]),
            'm': np.stack([flat(o.state[p]['exp_avg'] for p in m.parameters()) for m, o in zip(models, opts)]),
            'v': np.stack([flat(o.state[p]['exp_avg_sq'] for p in m.parameters()) for m, o in zip(models, opts)]),
            'grad': np.stack([flat(p.grad for p in m.parameters()) for m in models])}


def main():
    out = {}
    for name, (obs, A, C, Hc, batch, nb, lr, cap, seed) in CASES.items():
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        init = SafetyLayer(Box(-1, 1, (obs,)), Box(-1, 1, (A,)), hidden_dim=Hc, num_constraints=C, lr=lr, slack=0.05)
        # (PyTorch's default initialisation and the transitions below are rounded to short binary fractions: exact in float32 either
        #  way, and the file stays under its size limit next to the float64 results, which do not compress)
        with torch.no_grad():
            for p in init.constraint_models.parameters():
                p.copy_(torch.round(p * 1024) / 1024)
        init_sd = {k: v.clone() for k, v in init.constraint_models.state_dict().items()}
        data = {'obs': rng.normal(0, 1, (cap, obs)), 'act': rng.uniform(-1, 1, (cap, A)), 'c': rng.normal(-0.3, 0.3, (cap, C))}
        # c_next = c + (a smooth function of obs) . act + noise: something a one-hidden-layer model can fit
        mix = rng.normal(0, 0.5, (C, obs, A))
        data['c_next'] = data['c'] + np.einsum('bo,coa,ba->bc', np.tanh(data['obs']), mix, data['act']) + rng.normal(0, 0.02, (cap, C))
        data = {k: (np.round(v * 256) / 256).astype(np.float32) for k, v in data.items()}
        rows = np.stack([rng.permutation(cap)[:batch] for _ in range(nb)]).astype(np.int32)
        r32 = run((obs, A, C, Hc), init_sd, data, rows, lr, torch.float32)
        r64 = run((obs, A, C, Hc), init_sd, data, rows, lr, torch.float64)
        out[f'{name}/dims'] = np.array([obs, A, C, Hc, batch, nb, cap], dtype=np.int32)
        out[f'{name}/lr'] = np.float64(lr)
        out[f'{name}/init'] = np.stack([flat(m.parameters()) for m in init.constraint_models]).astype(np.float32)
        for k, v in data.items():
            out[f'{name}/{k}'] = v
        out[f'{name}/rows'] = rows
        out[f'{name}/loss32'] = r32['loss'].astype(np.float32)
        for k in ('loss', 'final', 'm', 'v', 'grad'):
            assert r64[k].dtype == np.float64
            out[f'{name}/{k}64'] = r64[k]
        for k in ('final', 'm', 'v', 'grad'):
            assert r32[k].dtype == np.float32
            out[f'{name}/{k}32_d'] = r32[k].view(np.int32) - r64[k].astype(np.float32).view(np.int32)
        print(name, 'loss32', r32['loss'][:, 0], 'max |final32 - final64|', np.abs(r32['final'] - r64['final']).max(),
              'max |grad32 - grad64|', np.abs(r32['grad'] - r64['grad']).max(), 'max |grad|', np.abs(r64['grad']).max())
    path = os.path.join(HERE, 'safety_pretrain.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 256 * 1024


if __name__ == '__main__':
    main()
