"""scg_cbf_nn_update (include/scg_cbf_nn_update.h) on the device: the residual network's loss, gradient and Adam steps against the float64
model of tests/cbf_nn_update_model.py (pinned to the reference fixture by tests/test_cbf_nn_update_cpu.py), the header's bit contracts,
the gather, and the filter's fused_update key.

Tolerances are computed in the tests from measurements that do not involve the kernels:
  gradient (per tensor)   4 x the largest deviation of float32 PyTorch-on-CPU autograd from the float64 model on the same batch, floor 4
                          float32 places of the tensor's largest gradient magnitude (the factor 4: another, equally long float32
                          summation order; tests/golden/make_cbf_nn.py's margin for float32-vs-float64 bounds)
  losses                  4 x the float64 model's relative deviation from the recorded / PyTorch value, floor 1e-6 relative
  parameters (per tensor) 4 x the float64 model's deviation from the fixture's train/after/* tensor, floor 4 float32 places of the
                          tensor's largest magnitude (the facade test, whose batches no fixture records: the same rule with float32
                          PyTorch Adam on the CPU, run on the same batches, as the reference's float32 result)
Every test prints the figures it computed before it asserts."""
import copy
import ctypes as C
from functools import partial

import numpy as np
import pytest

from tests import cbf_nn_cases as CN
from tests import cbf_nn_update_model as UM

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
RING = 101                      # rows of the test ring: no multiple of the row tile


def _lib():
    from safe_control_gym_amd import _cbf_nn_update as U
    return U, U.lib()


class Net:
    """Device state of one network under training: params, both moments, the step count and the scratch."""

    def __init__(self, weights):
        U, D = _lib()
        self.p = torch.tensor(UM.pack(weights), device=DEV)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.step = torch.zeros(1, dtype=torch.float32, device=DEV)
        self.work = torch.empty(U.work_bytes(D, U.MAX_BATCH) // 4, dtype=torch.float32, device=DEV)

    def snapshot(self):
        return [t.clone() for t in (self.p, self.m, self.v, self.step)]

    def restore(self, snap):
        for t, s in zip((self.p, self.m, self.v, self.step), snap):
            t.copy_(s)

    def same_bits(self, snap):
        return all(torch.equal(t.view(torch.int32), s.view(torch.int32)) for t, s in zip((self.p, self.m, self.v, self.step), snap))


class Ring:
    def __init__(self, state, act, bd, bda):
        self.np = (np.ascontiguousarray(state, dtype=np.float32).reshape(-1, 4), np.ascontiguousarray(act, dtype=np.float32).reshape(-1),
                   np.ascontiguousarray(bd, dtype=np.float64).reshape(-1), np.ascontiguousarray(bda, dtype=np.float64).reshape(-1))
        self.t = [torch.tensor(a, device=DEV) for a in self.np]

    def rows(self, idx):
        """What the float64 model sees of these rows: the float64 columns rounded to float32, as .to(float32)."""
        s, a, bd, bda = self.np
        return s[idx], a[idx], bd[idx].astype(np.float32), bda[idx].astype(np.float32)


def call(net, ring, rows, lr=UM.LR, train=True, grad=False, expect=0):
    """One scg_cbf_nn_update call; rows int [n, batch].  Returns (losses [n], gradient [67586] or None) as NumPy."""
    U, D = _lib()
    rows = np.asarray(rows, dtype=np.int32)
    assert rows.ndim == 2 and rows.min() >= 0 and rows.max() < ring.np[0].shape[0]
    d_rows = torch.tensor(rows, device=DEV)
    loss = torch.full((rows.shape[0],), float('nan'), dtype=torch.float32, device=DEV)
    g = torch.full((U.N_PARAMS,), float('nan'), dtype=torch.float32, device=DEV) if grad else None
    a = U.UpdateArgs(d_params=net.p.data_ptr(), d_m=net.m.data_ptr(), d_v=net.v.data_ptr(), d_step=net.step.data_ptr(), d_state=ring.t[0].data_ptr(),
                     d_act=ring.t[1].data_ptr(), d_barrier_dot=ring.t[2].data_ptr(), d_barrier_dot_approx=ring.t[3].data_ptr(),
                     d_rows=d_rows.data_ptr(), n_batches=rows.shape[0], batch=rows.shape[1], lr=lr, train=int(train), d_loss=loss.data_ptr(),
                     d_grad=g.data_ptr() if grad else None, d_work=net.work.data_ptr())
    rc = D.scg_cbf_nn_update(C.byref(a), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))
    assert rc == expect, (rc, D.scg_cbf_nn_update_last_error())
    torch.cuda.synchronize()
    return loss.cpu().numpy(), (g.cpu().numpy() if grad else None)


@pytest.fixture(scope='module')
def fx():
    w0, batch, after, loss, loss_after, states = UM.fixture()
    rng = np.random.default_rng(5)
    # a ring of fixture states whose float64 columns are not representable in float32
    ring = Ring(states[:RING], rng.uniform(-10.0, 10.0, RING), rng.normal(0.0, 2.0, RING) + 1e-9, rng.normal(0.0, 2.0, RING) + 1e-9)
    assert np.any(ring.np[2] != ring.np[2].astype(np.float32)) and np.any(ring.np[3] != ring.np[3].astype(np.float32))
    fixture_ring = Ring(batch['state'], batch['act'], batch['barrier_dot'], batch['barrier_dot_approx'])
    return dict(w0=w0, batch=batch, after=after, loss=loss, loss_after=loss_after, ring=ring, fixture_ring=fixture_ring)


def torch_f32(weights, state, act, bd, bda):
    """CBF_NN.compute_loss and its autograd gradient in float32 PyTorch on the CPU."""
    W = [torch.tensor(np.asarray(w, dtype=np.float32), requires_grad=True) for w in weights]
    s, a, d, p = (torch.tensor(np.asarray(x, dtype=np.float32)) for x in (state, act, bd, bda))
    h = torch.relu(torch.nn.functional.linear(s.reshape(-1, 4), W[0], W[1]))
    h = torch.relu(torch.nn.functional.linear(h, W[2], W[3]))
    a_b = torch.nn.functional.linear(h, W[4], W[5])
    est = d.reshape(-1, 1) + torch.unsqueeze(a_b[:, 0], 1) * a.reshape(-1, 1) + torch.unsqueeze(a_b[:, 1], 1)
    loss = (est - p.reshape(-1, 1)).pow(2).mean()
    loss.backward()
    return float(loss.detach()), [w.grad.numpy().astype(np.float64) for w in W]


@pytest.mark.parametrize('case', ['fixture', 1, 5, 37, 64, 100, 256])
def test_gradient_and_loss(fx, case):
    """train = 0 with d_grad: the fixture's own batch, and batches of 1, 5 (a masked tail in the second 4-row tile), 37, 64, 100 and
    max_batch rows drawn from a 101-row ring with a duplicated index (from 5 rows on)."""
    U, _ = _lib()
    assert U.MAX_BATCH == 256
    if case == 'fixture':
        ring, idx = fx['fixture_ring'], np.arange(64)
    else:
        ring = fx['ring']
        idx = np.random.default_rng(100 + case).integers(0, RING, size=case)
        if case >= 5:
            idx[-1] = idx[1]                                              # a duplicate, in another tile than its twin
            assert len(set(idx.tolist())) < case
    rows = ring.rows(idx)
    want_loss, want = UM.loss_and_grad(fx['w0'], *rows)
    t_loss, t_grad = torch_f32(fx['w0'], *rows)
    net = Net(fx['w0'])
    snap = net.snapshot()
    loss, g = call(net, ring, idx.reshape(1, -1), train=False, grad=True)
    assert net.same_bits(snap)                                            # train = 0 writes nothing but the loss and the gradient
    got = UM.unpack(g.astype(np.float64))
    tol_loss = max(4 * abs(t_loss - want_loss) / abs(want_loss), 1e-6)
    print(f'case {case}: loss {loss[0]!r} model {want_loss!r} torch {t_loss!r} rel tol {tol_loss:.2e}')
    assert abs(float(loss[0]) - want_loss) <= tol_loss * abs(want_loss)
    for k, a, b, t in zip(UM.KEYS, got, want, t_grad):
        big = float(np.abs(b).max())
        tol = max(4 * float(np.abs(t - b).max()), 4 * UM.ulp(big))
        dev = float(np.abs(a - b).max())
        print(f'  {k}: max |g| {big:.3e}  torch-f32 dev {np.abs(t - b).max():.3e}  tol {tol:.3e}  kernel dev {dev:.3e}  zeros {np.count_nonzero(b == 0)}')
        assert dev <= tol, (k, dev, tol)
        assert np.all(a[b == 0] == 0), k                                  # dead units: exactly zero


def _param_check(got_flat, fxd, label):
    """Parameters against train/after/* with test 2's tolerance rule; returns the figures."""
    model_w, _, _ = UM.train(fxd['w0'], [fxd['fixture_ring'].rows(np.arange(64))] * 3)
    got = UM.unpack(np.asarray(got_flat, dtype=np.float64))
    after = fxd['after']
    for k, a, mw in zip(UM.KEYS, got, model_w):
        if k == 'fcs.1.weight':
            want, a_cmp, m_cmp = after[k + '/rows'].astype(np.float64), a[::8], mw[::8]
        else:
            want, a_cmp, m_cmp = after[k].astype(np.float64), a, mw
        model_dev = float(np.abs(m_cmp - want).max())
        tol = max(4 * model_dev, 4 * UM.ulp(float(np.abs(want).max())))
        dev = float(np.abs(a_cmp - want).max())
        print(f'{label} {k}: model dev {model_dev:.3e}  tol {tol:.3e}  kernel dev {dev:.3e}')
        assert dev <= tol, (k, dev, tol)
        if k == 'fcs.1.weight':                                            # the rows the fixture does not store: through the two sums
            sums, f32 = after[k + '/sums'], a.astype(np.float32).astype(np.float64)
            d_sum, d_sq = abs(f32.sum() - sums[0]), abs((f32 * f32).sum() - sums[1])
            print(f'{label} {k}: sum dev {d_sum:.3e} (bound {a.size * tol:.3e})  sum of squares dev {d_sq:.3e} (bound {2 * np.abs(a).sum() * tol:.3e})')
            assert d_sum <= a.size * tol and d_sq <= 2 * np.abs(a).sum() * tol


def test_the_references_three_updates(fx):
    """From mlp/*, zero moments and step 0: three minibatches of the fixture batch at lr = 0.001 in one call."""
    ring, rows = fx['fixture_ring'], np.tile(np.arange(64), (3, 1))
    b = ring.rows(np.arange(64))
    model_w, model_losses, model_grads = UM.train(fx['w0'], [b] * 3)
    model_after = UM.loss_and_grad(model_w, *b)[0]
    net = Net(fx['w0'])
    before = net.p.cpu().numpy().copy()
    losses, _ = call(net, ring, rows)
    assert float(net.step.cpu()) == 3.0
    la, _ = call(net, ring, rows[:1], train=False)
    for name, got, want, model in (('loss', losses[0], fx['loss'], model_losses[0]), ('loss_after', la[0], fx['loss_after'], model_after)):
        tol = max(4 * abs(model - want) / abs(want), 1e-6)
        print(f'{name}: kernel {got!r} fixture {want!r} model {model!r} rel tol {tol:.2e} rel dev {abs(float(got) - want) / abs(want):.2e}')
        assert abs(float(got) - want) <= tol * abs(want)
    after = net.p.cpu().numpy()
    _param_check(after, fx, 'three updates')
    # a parameter whose gradient was exactly zero in all three steps (a dead unit) keeps its bits; the others moved
    dead = np.all([UM.pack(g, np.float64) == 0 for g in model_grads], axis=0)
    assert 0.05 < dead.mean() < 0.5
    assert np.array_equal(after.view(np.int32)[dead], before.view(np.int32)[dead])
    live = np.all([UM.pack(g, np.float64) != 0 for g in model_grads], axis=0)
    assert np.all(after[live] != before[live])
    assert np.all(net.m.cpu().numpy()[dead] == 0) and np.all(net.v.cpu().numpy()[dead] == 0)


def test_bit_contracts(fx):
    ring = fx['ring']
    rng = np.random.default_rng(9)
    rows = rng.integers(0, RING, size=(3, 37))
    net = Net(fx['w0'])
    start = net.snapshot()
    l3, _ = call(net, ring, rows)
    one_call = net.snapshot()
    assert float(net.step.cpu()) == 3.0                                   # d_step advances by n_batches
    # three calls of one minibatch
    net.restore(start)
    l1 = np.concatenate([call(net, ring, rows[i:i + 1])[0] for i in range(3)])
    assert net.same_bits(one_call) and np.array_equal(l1.view(np.int32), l3.view(np.int32))
    # the same call again from the same state
    net.restore(start)
    l3b, _ = call(net, ring, rows)
    assert net.same_bits(one_call) and np.array_equal(l3b.view(np.int32), l3.view(np.int32))
    assert not torch.equal(one_call[0], start[0])
    # train = 0 from a state with non-zero moments: nothing but the losses (and the gradient) is written
    l0, g0 = call(net, ring, rows, train=False, grad=True)
    assert net.same_bits(one_call) and np.all(np.isfinite(l0)) and np.all(np.isfinite(g0))
    l0b, _ = call(net, ring, rows, train=False)
    assert net.same_bits(one_call) and np.array_equal(l0b.view(np.int32), l0.view(np.int32))
    # the gradient is the LAST minibatch's
    _, g_last = call(net, ring, rows[2:], train=False, grad=True)
    assert np.array_equal(g_last.view(np.int32), g0.view(np.int32))
    # arguments it does not serve: refused, nothing written
    U, D = _lib()
    for bad in (np.zeros((1, U.MAX_BATCH + 1), dtype=np.int32),):
        call(net, ring, bad, expect=-1)
        assert net.same_bits(one_call)
    v = C.c_int64(-7)
    assert D.scg_cbf_nn_update_work_bytes(0, C.byref(v)) == -1 and D.scg_cbf_nn_update_work_bytes(U.MAX_BATCH + 1, C.byref(v)) == -1 and v.value == -7


def test_gather(fx):
    """Indexed rows of a ring with float64 columns against the same rows pre-rounded to float32 and laid out contiguously; a batch that is
    one row 64 times against that row alone."""
    ring = fx['ring']
    idx = np.random.default_rng(21).permutation(RING)[:64]
    idx[7] = idx[50]
    s, a, bd, bda = ring.rows(idx)
    dense = Ring(s, a, bd.astype(np.float64), bda.astype(np.float64))
    assert np.any(ring.np[2][idx] != bd)                                  # the rounding is not a no-op
    outs = []
    for r, rows in ((ring, idx.reshape(1, -1)), (dense, np.arange(64).reshape(1, -1))):
        net = Net(fx['w0'])
        l, g = call(net, r, np.tile(rows, (2, 1)), grad=True)             # two steps: the second one's gradient depends on the first step
        outs.append((l, g, net.snapshot()))
    assert np.array_equal(outs[0][0].view(np.int32), outs[1][0].view(np.int32))
    assert np.array_equal(outs[0][1].view(np.int32), outs[1][1].view(np.int32))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs[0][2], outs[1][2]))
    # one row, 64 times: the mean of 64 equal terms is the term and the gradient that row's, up to the rounding of the partial sums
    # (3 x is not exact): both calls are held to the model's single-row loss and gradient at the gradient test's tolerance
    row = int(idx[3])
    net = Net(fx['w0'])
    l64, g64 = call(net, ring, np.full((1, 64), row), train=False, grad=True)
    l1, g1 = call(net, ring, np.full((1, 1), row), train=False, grad=True)
    want_loss, want = UM.loss_and_grad(fx['w0'], *ring.rows(np.array([row])))
    t_loss, t_grad = torch_f32(fx['w0'], *ring.rows(np.array([row])))
    for l in (l64[0], l1[0]):
        assert abs(float(l) - want_loss) <= max(4 * abs(t_loss - want_loss) / abs(want_loss), 1e-6) * abs(want_loss)
    for k, a64, a1, b, t in zip(UM.KEYS, UM.unpack(g64.astype(np.float64)), UM.unpack(g1.astype(np.float64)), want, t_grad):
        tol = max(4 * float(np.abs(t - b).max()), 4 * UM.ulp(float(np.abs(b).max())))
        print(f'one row x 64, {k}: tol {tol:.3e}  dev {np.abs(a64 - b).max():.3e}  against the 1-row call {np.abs(a64 - a1).max():.3e}')
        assert np.abs(a64 - b).max() <= tol and np.abs(a1 - b).max() <= tol
        assert np.array_equal(a64 == 0, a1 == 0)


# ---------------------------------------------------------------------------------------------------------------- the facade
SF_OVER = dict(num_episodes=2, max_num_steps=12, train_iterations=5, train_batch_size=64, max_buffer_size=4096, seed=4)


def _filter(**over):
    from safe_control_gym_amd.registration import make
    env_id, cfg = CN.task_config(False)
    sf = make('cbf_nn', partial(make, env_id, **cfg), **dict(copy.deepcopy(CN.settings()['sf_config']), **dict(SF_OVER, **over)))
    w0 = UM.fixture()[0]
    sf.mlp.load_state_dict({k: torch.tensor(np.asarray(w, dtype=np.float32)) for k, w in zip(UM.KEYS, w0)})
    return sf


def _learn_with_snapshots(sf, n):
    """learn(num_envs=n) with the buffer rebuilt episode by episode from the launches' traces (the buffer's zero rows of episode 1 are
    overwritten in episode 2: the final buffer does not show what episode 1 sampled): returns the per-episode snapshot buffers."""
    from safe_control_gym_amd import cbf_nn
    traces, orig = [], sf.rollout

    def spy(*a, **kw):
        o = orig(*a, **kw)
        traces.append({k: o[k].clone() for k in ('obs', 'applied')})
        return o
    sf.rollout = spy
    sf.learn(num_envs=n)
    torch.cuda.synchronize()
    sf.rollout = orig
    env, buf = sf._learn_env, sf.buffer
    prior = (sf.model.params['length'], sf.model.params['m'], sf.model.params['M'], sf.model.params['g'])
    snap = type(buf)(4, 1, buf.max_size, env.device, buf.batch_size)
    snaps = []
    for o in traces:
        st, ac, bd, ap = cbf_nn.pushed_arrays(o['obs'][1:, :, :4], o['applied'].double(), sf.state_limits, prior, float(env.spec.CTRL_FREQ))
        snap.push({'state': st, 'act': ac, 'barrier_dot': bd, 'barrier_dot_approx': ap})
        snaps.append({k: getattr(snap, k).clone() for k in snap.KEYS})
    for k in buf.KEYS:
        assert torch.equal(getattr(buf, k), snaps[-1][k]), k
    return snaps


def test_facade(fx, tmp_path):
    from safe_control_gym_amd import _cbf_nn
    n, iters = 4, SF_OVER['train_iterations']
    w0 = fx['w0']
    on = _filter(fused_update=True)
    assert on.opt is None
    ptr0 = on.residual().d_params
    assert on.mlp.fcs[0].weight.data_ptr() == ptr0 == on._flat.data_ptr()                        # the parameters are views into the master vector
    snaps = _learn_with_snapshots(on, n)
    assert on.residual().d_params == ptr0 == on._flat.data_ptr()                                 # a stable pointer, nothing re-packed
    assert on.last_losses.shape == (iters,) and bool(torch.isfinite(on.last_losses).all())
    assert float(on._upd['step'].cpu()) == 2 * iters
    assert len(on.sampled_indices) == 2 * iters and all(len(i) == 64 for i in on.sampled_indices)
    # the default path at the same seed draws the same indices, and is bit for bit an eager replay of update(buf.gather(idx))
    off = _filter()
    snaps_off = _learn_with_snapshots(off, n)
    assert all(np.array_equal(a, b) for a, b in zip(on.sampled_indices, off.sampled_indices))
    from safe_control_gym_amd.ppo import MLP
    ref = MLP(4, 2, [256, 256], 'relu').to(off._learn_env.device)
    ref.load_state_dict({k: torch.tensor(np.asarray(w, dtype=np.float32)) for k, w in zip(UM.KEYS, w0)})
    opt = torch.optim.Adam(ref.parameters(), off.learning_rate)
    for ep in range(2):
        for idx in off.sampled_indices[ep * iters:(ep + 1) * iters]:
            i = torch.as_tensor(np.asarray(idx), device=ref.fcs[0].weight.device, dtype=torch.long)
            b = {k: snaps_off[ep][k][i].to(torch.float32) for k in snaps_off[ep]}
            a_b = ref(b['state'])
            loss = (b['barrier_dot'] + torch.unsqueeze(a_b[:, 0], 1) * b['act'] + torch.unsqueeze(a_b[:, 1], 1) - b['barrier_dot_approx']).pow(2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
    for k in UM.KEYS:
        assert torch.equal(ref.state_dict()[k], off.mlp.state_dict()[k]), k
    # the fused path's weights: the same indices on the same rows through the float64 model, to the three-updates test's tolerance RULE:
    # per tensor 4 x the float64 model's deviation from the reference's float32 result, floor 4 float32 places.  There the reference's
    # float32 result is the fixture; for these batches it is the reference's own arithmetic, float32 PyTorch Adam on the CPU (which
    # reproduces the fixture exactly), run on the same batches.  (The fixture's NUMBERS do not carry over: Adam's step is invariant to
    # the gradient's scale, so a parameter moves by the gradient's RELATIVE float32 error x lr, and these rows — the buffer's zero rows and
    # states far outside the limits — have elements whose |g| is small against their summands.  Measured on MI355X: W2 deviates from
    # the model by 4.4e-7 after the 10 steps against 3.4e-8 = 4 x the fixture's 8.4e-9.)
    batches = []
    for ep in range(2):
        host = {k: v.cpu().numpy() for k, v in snaps[ep].items()}
        for idx in on.sampled_indices[ep * iters:(ep + 1) * iters]:
            batches.append((host['state'][idx], host['act'][idx].astype(np.float32), host['barrier_dot'][idx].astype(np.float32),
                            host['barrier_dot_approx'][idx].astype(np.float32)))
    model_w, model_losses, _ = UM.train(w0, batches, lr=on.learning_rate)
    cpu = MLP(4, 2, [256, 256], 'relu')
    cpu.load_state_dict({k: torch.tensor(np.asarray(w, dtype=np.float32)) for k, w in zip(UM.KEYS, w0)})
    cpu_opt = torch.optim.Adam(cpu.parameters(), on.learning_rate)
    for st, ac, bd, ap in batches:
        a_b = cpu(torch.tensor(st))
        loss = (torch.tensor(bd) + torch.unsqueeze(a_b[:, 0], 1) * torch.tensor(ac) + torch.unsqueeze(a_b[:, 1], 1) - torch.tensor(ap)).pow(2).mean()
        cpu_opt.zero_grad()
        loss.backward()
        cpu_opt.step()
    torch_w = [cpu.state_dict()[k].numpy().astype(np.float64) for k in UM.KEYS]
    torch.cuda.synchronize()
    got = UM.unpack(on._flat.cpu().numpy().astype(np.float64))
    for k, a, b, tw in zip(UM.KEYS, got, model_w, torch_w):
        model_dev = float(np.abs(tw - b).max())
        tol = max(4 * model_dev, 4 * UM.ulp(float(np.abs(b).max())))
        dev = float(np.abs(a - b).max())
        print(f'facade {k}: float32 PyTorch dev from the model {model_dev:.3e}  tol {tol:.3e}  kernel dev from the model after {len(batches)} steps {dev:.3e}')
        assert dev <= tol, (k, dev, tol)
        assert torch.equal(dict(zip(UM.KEYS, on._tensors()))[k].detach().cpu(), torch.tensor(a.astype(np.float32)))
    last = on.last_losses.cpu().numpy()
    # (weights within ~1e-7 of the model's, |gradient|_1 of order 1e4 at most: 1e-3 on losses of order 30)
    assert np.allclose(last, model_losses[-iters:], rtol=1e-4)
    # certify launches read the master vector as it is: no refresh between the step and the launch
    venv = on._env()
    states = torch.tensor(np.asarray(UM.fixture()[5][:67], dtype=np.float32), device=venv.device)
    acts = torch.linspace(-8.0, 8.0, 67, device=venv.device)
    mine = on.certify_tensors(states, acts, with_ab=True)
    direct = venv.certify_nn_tensors(on.params(), _cbf_nn.residual_of(on._flat), states, acts)
    assert all(torch.equal(x, y) for x, y in zip(mine, direct))
    # update(batch) keeps working (the same kernels on the batch as a ring of its own) and certify sees the step at once
    before = on._flat.clone()
    on.update(on.buffer.gather(on.sampled_indices[-1]))
    torch.cuda.synchronize()
    assert not torch.equal(before, on._flat) and float(on._upd['step'].cpu()) == 2 * iters + 1
    assert not torch.equal(on.certify_tensors(states, acts, with_ab=True)[3], mine[3])
    assert float(on.compute_loss(on.buffer.gather(on.sampled_indices[-1])).detach()) > 0
    # save, then load into a fresh filter: extract_a_b bit for bit, the optimiser state untouched
    path = str(tmp_path / 'cbf_nn_fused.pt')
    on.save(path)
    fresh = _filter(fused_update=True)
    fresh.load(path)
    x = UM.fixture()[5][:33]
    a0, b0 = on.extract_a_b(x)
    a1, b1 = fresh.extract_a_b(x)
    assert np.array_equal(a0.view(np.int32), a1.view(np.int32)) and np.array_equal(b0.view(np.int32), b1.view(np.int32))
    assert fresh._upd is None                                             # (not checkpointed, as upstream's optimiser is not)
    m_before = on._upd['m'].clone()
    fresh.buffer = on.buffer
    with pytest.raises(ValueError, match='indices'):
        fresh.update_rows(np.array([[0, len(on.buffer)]]))
    on.load(path)
    on.reset()
    assert torch.equal(on._upd['m'], m_before) and on.residual().d_params == ptr0
    for f in (on, off, fresh):
        f.close()
