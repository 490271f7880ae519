"""CPU side of the cbf_nn residual network's fused Adam steps (include/scg_cbf_nn_update.h): the float64 model the GPU tests lean on
(tests/cbf_nn_update_model.py) is pinned to the reference-generated fixture, the fixture is shown to need no exclusions, and the host
logic (the struct, the build, the library's file name, the facade's argument checks) is checked without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys
from functools import partial

import numpy as np
import pytest

from tests import cbf_nn_cases as CN
from tests import cbf_nn_update_model as UM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def replay():
    """The fixture's three recorded updates through the float64 model: (fixture, final weights, losses, gradients, loss after)."""
    fx = UM.fixture()
    w0, batch = fx[0], fx[1]
    b = (batch['state'], batch['act'], batch['barrier_dot'], batch['barrier_dot_approx'])
    w, losses, grads = UM.train(w0, [b, b, b])
    return fx, w, losses, grads, UM.loss_and_grad(w, *b)[0]


def test_model_reproduces_the_reference_fixture(replay):
    """Bounds.  Parameters after the three recorded updates: 2e-7 absolute on every stored one — three times the worst gap measured
    between this float64 model and the reference's float32 run (W3 6.5e-8, W1 4.0e-8, b1 3.5e-8, b3 1.4e-8, W2's stored rows 8.4e-9, b2
    4.7e-9); the bound only says that the model is the reference's arithmetic.  train/loss is a float32 evaluation under the same
    weights: 1e-6 relative, tests/test_cbf_nn_cpu.py's bound for that evaluation (measured 1.8e-7, two float32 places at 40.7).
    train/loss_after is a float32 evaluation under the reference's float32 weights, which differ from the model's by the gaps above:
    the same 1e-6 plus the first-order effect of those gaps, sum over tensors of |gradient|_1 x the tensor's measured gap (measured
    9.1e-7 relative in all)."""
    (w0, batch, after, loss, loss_after, _), w, losses, _, la = replay
    assert abs(losses[0] - loss) <= 1e-6 * abs(loss)
    worst = {}
    for k, got in zip(UM.KEYS, w):
        if k == 'fcs.1.weight':
            worst[k] = float(np.abs(got[::8] - after[k + '/rows']).max())
            sums = after[k + '/sums']
            # (the float64 sum and sum of squares of the float32 W2: 65 536 terms, each within the bound)
            assert abs(got.sum() - sums[0]) <= 2e-7 * got.size and abs((got * got).sum() - sums[1]) <= 2e-7 * 2 * np.abs(got).sum()
        else:
            worst[k] = float(np.abs(got - after[k]).max())
        assert worst[k] <= 2e-7, (k, worst[k])
    print('float64 model vs fixture, worst absolute gap per tensor:', worst)
    b = (batch['state'], batch['act'], batch['barrier_dot'], batch['barrier_dot_approx'])
    first_order = sum(float(np.abs(g).sum()) * worst[k] for k, g in zip(UM.KEYS, UM.loss_and_grad(w, *b)[1]))
    print(f'loss_after: model {la!r} fixture {loss_after!r} first-order bound {first_order:.3e}')
    assert abs(la - loss_after) <= 1e-6 * abs(loss_after) + first_order
    assert any(not np.array_equal(np.asarray(a, dtype=np.float64), b) for a, b in zip(w0, w))


def test_fixture_needs_no_exclusions(replay):
    """In all three recorded steps every gradient element is exactly zero (a dead unit) or far above Adam's eps = 1e-8, where
    g / (|g| + eps) would turn a last-place difference into a full lr.  Of the elements the fixture stores and the tests compare (every
    tensor but W2 whole, W2's every-8th rows) none has 0 < |g| <= 1e-6 (the smallest is above 1e-5).  Of the 65 536 elements of W2 two
    lie below 1e-6 (row 33 in step 1, 6.3e-7; row 161 in step 3, 2.0e-7), in rows the fixture does not store; W2 enters the comparison
    through its sum and sum of squares only.  For them and for any later fixture: no element at all within 10 eps, where the step's
    relative sensitivity to the gradient's relative error, eps / (|g| + eps), is at most 9 %."""
    _, _, _, grads, _ = replay
    for step, gs in enumerate(grads):
        stored = np.abs(np.concatenate([(g[::8] if k == 'fcs.1.weight' else g).reshape(-1) for k, g in zip(UM.KEYS, gs)]))
        assert np.count_nonzero((stored > 0) & (stored <= 1e-6)) == 0, step
        assert np.count_nonzero(stored == 0) > 0 and stored[stored > 0].min() > 1e-5
        flat = np.abs(np.concatenate([g.reshape(-1) for g in gs]))
        assert np.count_nonzero((flat > 0) & (flat <= 10 * UM.EPS)) == 0, step
        print(f'step {step}: {np.count_nonzero((flat > 0) & (flat <= 1e-6))} of {flat.size} elements with 0 < |g| <= 1e-6, smallest nonzero {flat[flat > 0].min():.3e}')
        dead_w2 = np.count_nonzero(gs[2] == 0) / gs[2].size
        assert 0.05 < dead_w2 < 0.5, dead_w2                              # dead units exist: the keeps-its-bits contract is exercised


def test_model_gradient_is_the_derivative(replay):
    """The model's gradient against a central difference of its own loss, in float64, on a few elements of every tensor."""
    (w0, batch, *_), *_ = replay
    b = (batch['state'], batch['act'], batch['barrier_dot'], batch['barrier_dot_approx'])
    _, grads = UM.loss_and_grad(w0, *b)
    rng = np.random.default_rng(0)
    for ti, g in enumerate(grads):
        live = np.flatnonzero(g.reshape(-1) != 0)
        for e in rng.choice(live, size=min(3, live.size), replace=False):
            hi = [np.array(w, dtype=np.float64) for w in w0]
            lo = [np.array(w, dtype=np.float64) for w in w0]
            hi[ti].reshape(-1)[e] += 1e-6
            lo[ti].reshape(-1)[e] -= 1e-6
            fd = (UM.loss_and_grad(hi, *b)[0] - UM.loss_and_grad(lo, *b)[0]) / 2e-6
            assert abs(fd - g.reshape(-1)[e]) <= 1e-5 * max(1.0, abs(fd)), (ti, e, fd, g.reshape(-1)[e])


def test_struct_matches_the_header(tmp_path):
    """The ctypes struct against the header, through the compiler: size and every field's offset."""
    from safe_control_gym_amd import _cbf_nn_update as U
    names = [f[0] for f in U.UpdateArgs._fields_]
    hdr = re.sub(r'/\*.*?\*/', '', open(U.HEADER).read(), flags=re.S)
    fields = re.search(r'typedef struct scg_cbf_nn_update_args \{(.*?)\}', hdr, re.S).group(1)
    declared = [n.strip().lstrip('*') for line in fields.split(';') if line.strip() for n in re.sub(r'^\s*(const\s+)?\w+\s*\*?', '', line.strip()).split(',')]
    assert declared == names
    src = tmp_path / 'layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "scg_cbf_nn_update.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(scg_cbf_nn_update_args));\n'
                   + ''.join(f'  printf(" %zu", offsetof(scg_cbf_nn_update_args, {n}));\n' for n in names)
                   + f'  printf(" %d %d", SCG_CBF_NN_UPDATE_PARAMS, SCG_CBF_NN_UPDATE_MAX_BATCH);\n  return 0;\n}}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(U.UpdateArgs) == 112
    assert out[1:-2] == [getattr(U.UpdateArgs, n).offset for n in names]
    assert out[-2:] == [U.N_PARAMS, U.MAX_BATCH] and U.N_PARAMS == 67586 == sum(UM.SIZES) and U.MAX_BATCH >= 256


def test_library_builds_and_its_name_resolves():
    """hipcc cross-compiles the library for gfx950; build()'s stale-library sweep finds the new family's hash under its file name and does
    not mistake it for a cbf_nn library."""
    import __graft_entry__ as G
    from safe_control_gym_amd import _cbf_nn, _cbf_nn_update as U, _lib as L
    if not os.path.exists(L._hipcc()):
        pytest.skip('hipcc is not installed')
    so = U.build()
    assert os.path.basename(so).startswith(U.PREFIX) and not os.path.basename(so).startswith(_cbf_nn.PREFIX)
    assert not U.PREFIX.startswith(_cbf_nn.PREFIX) and not _cbf_nn.PREFIX.startswith(U.PREFIX)
    assert L._lib_source_hash(so) == U.source_hash() == G.expected_source_hash(os.path.basename(so))
    assert U.source_hash() != _cbf_nn.source_hash()
    # the existing cbf_nn libraries keep their sources: the new translation unit is none of their dependencies
    assert U.SRC not in _cbf_nn.DEPS and U.HEADER not in _cbf_nn.DEPS
    with open(so, 'rb') as f:
        blob = f.read()
    for sym in (b'scg_cbf_nn_update', b'scg_cbf_nn_update_work_bytes', b'scg_cbf_nn_update_shape'):
        assert sym in blob


def _make(**over):
    from safe_control_gym_amd.registration import make
    env_id, cfg = CN.task_config(False)
    return make('cbf_nn', partial(make, env_id, **cfg), **dict(CN.settings()['sf_config'], **over))


def test_fused_update_is_off_by_default_and_checks_its_batch():
    pytest.importorskip('torch')
    from safe_control_gym_amd import _cbf_nn_update as U
    from safe_control_gym_amd.cbf_nn import CBF_NN_DEFAULTS
    assert 'fused_update' not in CBF_NN_DEFAULTS                         # an extension key, not a YAML default
    sf = _make()
    assert sf.fused_update is False and sf.opt is not None
    on = _make(fused_update=True, train_batch_size=U.MAX_BATCH)
    assert on.fused_update is True and on.opt is None and on.last_losses is None
    with pytest.raises(ValueError, match='train_batch_size'):
        _make(fused_update=True, train_batch_size=U.MAX_BATCH + 1)
    _make(train_batch_size=U.MAX_BATCH + 1)                              # the default path serves any batch, as before


def test_update_rows_refuses_indices_outside_the_buffer():
    """The index check runs on the host before anything is launched: no GPU is needed to see it refuse."""
    torch = pytest.importorskip('torch')
    from safe_control_gym_amd.cbf_nn import DeviceCBFBuffer

    class _OnDevice(DeviceCBFBuffer):                                    # a filled buffer that claims to be on the device
        def reset(self):
            super().reset()
            self.state = _Claims(self.state)

    class _Claims:
        is_cuda = True

        def __init__(self, t):
            self.t = t

    on = _make(fused_update=True)
    on.buffer = _OnDevice(4, 1, 32, 'cpu', 8)
    on.buffer.buffer_size = 10
    on._fused_call = lambda *a, **k: pytest.fail('an invalid index reached the launch')
    for bad in ([[0, 10]], [[-1, 3]], [[0, 1], [2, 1 << 20]]):
        with pytest.raises(ValueError, match='indices'):
            on.update_rows(np.asarray(bad))
    with pytest.raises(ValueError):
        on.update_rows(np.zeros((0, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        on.update_rows(np.zeros((2, 4)))                                 # not an int array
    off = _make()
    from safe_control_gym_amd import _lib as L
    with pytest.raises(L.ScgError):
        off.update_rows(np.zeros((1, 4), dtype=np.int64))
    assert torch is not None


if __name__ == '__main__':
    sys.exit(pytest.main([__file__, '-q']))
