"""The cbf_nn safety filter without a GPU: tests/cbf_nn_model.py (the NumPy restatement the kernels are compared against) pinned to the
reference-generated fixture (tests/golden/cbf_nn.npz, make_cbf_nn.py), the float32 cost of the closed form with the learned row (where
the kernels' tolerance comes from), the product's loss / update / pushed arrays / buffer against the reference's, and the host-side
surface: registry entry and defaults, refusals, `supported()` and the LDS arithmetic.

Forward-pass bound.  |a_b32 - a_b64| <= TAU S per output, TAU = 1e-5 and S = |b3| + sum |W3| |h2| the magnitude of the output layer's
dot-product terms in float64 (tests/test_gpu_offpolicy_collector.py's bound for a float32 forward pass of this depth).

Closed-form bounds.  bound_u / bound_s = 4 x the largest deviation of the float32 model from the float64 one on the fixture rows, both
fed the reference's float32 (a_nn, b_nn): the factor tests/test_gpu_cbf.py uses (other sin / cos, other contraction).  Rows whose
float64 r(u0) lies within bound_s of 0, or whose s* lies within it of slack_tolerance, may take either branch in float32; they are left
out of flag and value comparisons and must be at most 1 % of the fixture (a condition on the fixture, asserted here and in the
generator)."""
import copy
import json
import os
import re
from functools import partial

import numpy as np
import pytest

from tests import cbf_nn_model as NM

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
D = np.load(os.path.join(GOLDEN, 'cbf_nn.npz'))
S = json.load(open(os.path.join(GOLDEN, 'cbf_nn_settings.json')))
SF = S['sf_config']
LO, HI = (float(v) for v in D['action_bounds'])
TAU = 1e-5
WEIGHTS = [D['mlp/' + k] for k in NM.KEYS]


def env_func(**over):
    from safe_control_gym_amd.registration import make
    cfg = copy.deepcopy(S['task_config'])
    cfg.pop('seed', None)
    cfg.update(over)
    return partial(make, S['task'], **cfg)


def bounds(soft, ab=None):
    """(r64, r32, bound_u, bound_s, boundary rows) on the fixture rows with the reference's float32 a_b."""
    ab = D['a_b'] if ab is None else ab
    args = (D['states'], D['actions'], ab, D['limits'], D['prior'], SF['slope'], SF['slack_weight'], SF['slack_tolerance'], LO, HI)
    r64, r32 = NM.certify(*args, soft=soft), NM.certify(*args, soft=soft, dtype=np.float32)
    bound_u = 4 * np.abs(r32['u'].astype(np.float64) - r64['u']).max()
    bound_s = 4 * np.abs(r32['s'].astype(np.float64) - r64['s']).max()
    near = np.abs(r64['r0']) <= bound_s
    if soft:
        near |= np.abs(r64['s'] - SF['slack_tolerance']) <= bound_s
    return r64, r32, bound_u, bound_s, near


def test_forward_matches_the_reference():
    a_b64, mag = NM.forward(WEIGHTS, D['states'], with_magnitude=True)
    np.testing.assert_array_equal(a_b64, D['a_b64'])
    ratio = np.abs(D['a_b'].astype(np.float64) - a_b64) / (TAU * mag)
    print(f'reference float32 forward vs float64: worst error / (TAU S) {ratio.max():.3f}; |a_nn| median {np.median(np.abs(a_b64[:, 0])):.3f}, '
          f'|b_nn| median {np.median(np.abs(a_b64[:, 1])):.3f}')
    assert ratio.max() <= 1.0
    a_b32 = NM.forward(WEIGHTS, D['states'], dtype=np.float32)
    assert (np.abs(a_b32.astype(np.float64) - a_b64) <= TAU * mag).all()


@pytest.mark.parametrize('mode', ['soft', 'hard'])
def test_model_matches_the_reference_minimisers(mode):
    soft = mode == 'soft'
    r = NM.certify(D['states'], D['actions'], D['a_b64'], D['limits'], D['prior'], SF['slope'], SF['slack_weight'], SF['slack_tolerance'], LO, HI,
                   soft=soft)
    acc = D[f'{mode}/accepted']
    assert acc.mean() >= 0.99
    if soft:
        np.testing.assert_allclose(r['u'][acc], D['soft/u'][acc], rtol=0, atol=1e-8)
        np.testing.assert_allclose(r['s'][acc], D['soft/s'][acc], rtol=0, atol=1e-8)
        assert (r['feasible'][acc] == (D['soft/s'][acc] <= SF['slack_tolerance'])).all()
    else:
        ne = D['hard/nonempty']
        assert (r['feasible'] == ne)[acc].all() and 0 < ne.mean() < 1
        np.testing.assert_allclose(r['u'][acc & ne], D['hard/u'][acc & ne], rtol=0, atol=1e-8)
    # the residual matters on this fixture: the plain filter's answer differs on at least a quarter of the rows
    plain = NM.certify(D['states'], D['actions'], np.zeros_like(D['a_b64']), D['limits'], D['prior'], SF['slope'], SF['slack_weight'],
                       SF['slack_tolerance'], LO, HI, soft=soft)
    _, _, bound_u, _, _ = bounds(soft)
    assert (np.abs(plain['u'] - r['u']) > 100 * bound_u).mean() >= 0.25


@pytest.mark.parametrize('mode', ['soft', 'hard'])
def test_float32_cost_of_the_closed_form(mode):
    r64, r32, bound_u, bound_s, near = bounds(mode == 'soft')
    print(f'{mode}: bound_u {bound_u:.3e} bound_s {bound_s:.3e}; boundary rows {int(near.sum())} / {len(near)}; float32 flag mismatches outside '
          f'them {int((r32["feasible"] != r64["feasible"])[~near].sum())}')
    assert near.mean() <= 0.01
    assert (r32['feasible'] == r64['feasible'])[~near].all()
    assert 0 < bound_u < 1e-3 and bound_s < 1e-3


def _filter(**over):
    from safe_control_gym_amd.registration import make
    return make('cbf_nn', env_func(), **dict(copy.deepcopy(SF), **over))


def _load_weights(sf):
    sf.mlp.load_state_dict({k: torch.tensor(D['mlp/' + k]) for k in NM.KEYS})


def test_loss_and_three_updates_match_the_reference():
    sf = _filter()
    _load_weights(sf)
    batch = {k: torch.tensor(D['train/batch/' + k]) for k in ('state', 'act', 'barrier_dot', 'barrier_dot_approx')}
    loss = float(sf.compute_loss(batch).detach())
    assert abs(loss - float(D['train/loss'])) <= 1e-6 * abs(float(D['train/loss']))
    m64 = NM.loss(WEIGHTS, *[D['train/batch/' + k] for k in ('state', 'act', 'barrier_dot', 'barrier_dot_approx')])
    assert abs(m64 - float(D['train/loss'])) <= 1e-5 * abs(m64)
    for _ in range(S['n_updates']):
        sf.update(batch)
    assert abs(float(sf.compute_loss(batch).detach()) - float(D['train/loss_after'])) <= 1e-6 * abs(float(D['train/loss_after']))
    after = {k: v.detach().numpy() for k, v in sf.mlp.state_dict().items()}
    assert list(after) == list(NM.KEYS)                                     # upstream's state-dict keys
    for k in NM.KEYS:
        if k == 'fcs.1.weight':
            want, got = D['train/after/' + k + '/rows'], after[k][::S['w2_row_stride']]
            sums = np.array([after[k].astype(np.float64).sum(), (after[k].astype(np.float64) ** 2).sum()])
            np.testing.assert_allclose(sums, D['train/after/' + k + '/sums'], rtol=1e-6)
        else:
            want, got = D['train/after/' + k], after[k]
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), k
        assert np.abs(want - D['mlp/' + k][::S['w2_row_stride']] if k == 'fcs.1.weight' else want - D['mlp/' + k]).max() > 0, k


def test_pushed_arrays_and_buffer_match_the_reference():
    from safe_control_gym_amd import cbf_nn
    obs_after, inputs, freq = D['traj/obs_after'], D['traj/inputs'], float(D['traj/ctrl_freq'])
    model = NM.pushed_arrays(obs_after, inputs, D['limits'], D['prior'], freq)
    for k, v in model.items():
        want = D['traj/pushed/' + k]
        assert v.shape == want.shape == (S['traj_steps'] - 2, want.shape[1])
        np.testing.assert_allclose(v, want, rtol=1e-12, atol=1e-12)
    # the product's device function (here on the CPU), one env and three envs side by side
    st = torch.tensor(obs_after).unsqueeze(1)
    got = cbf_nn.pushed_arrays(st, torch.tensor(inputs).unsqueeze(1), D['limits'], D['prior'], freq)
    for k, v in zip(('state', 'act', 'barrier_dot', 'barrier_dot_approx'), got):
        np.testing.assert_allclose(v.numpy(), D['traj/pushed/' + k], rtol=1e-12, atol=1e-12)
    got3 = cbf_nn.pushed_arrays(st.repeat(1, 3, 1), torch.tensor(inputs).unsqueeze(1).repeat(1, 3), D['limits'], D['prior'], freq)
    for k, v in zip(('state', 'act', 'barrier_dot', 'barrier_dot_approx'), got3):
        np.testing.assert_allclose(v.numpy(), np.concatenate([D['traj/pushed/' + k]] * 3), rtol=1e-12, atol=1e-12)      # env after env
    # CBFBuffer's bookkeeping, including the wrap-around push
    buf = cbf_nn.DeviceCBFBuffer(4, 1, S['buffer_size'], 'cpu', S['batch_rows'])
    push = dict(zip(('state', 'act', 'barrier_dot', 'barrier_dot_approx'), got))
    buf.push(push)
    assert (buf.pos, buf.buffer_size) == (int(D['traj/pos1']), int(D['traj/size1']))
    buf.push(push)
    sd = buf.state_dict()
    assert list(sd) == ['pos', 'buffer_size', 'state', 'act', 'barrier_dot', 'barrier_dot_approx']
    assert (sd['pos'], sd['buffer_size']) == (int(D['traj/pos2']), int(D['traj/size2']))
    for k in ('state', 'act', 'barrier_dot', 'barrier_dot_approx'):
        np.testing.assert_allclose(sd[k].astype(np.float32), D['traj/buffer/' + k], rtol=0, atol=0)
    again = cbf_nn.DeviceCBFBuffer(4, 1, S['buffer_size'], 'cpu', S['batch_rows'])
    again.load_state_dict(sd)
    assert (again.pos, again.buffer_size) == (buf.pos, buf.buffer_size) and torch.equal(again.barrier_dot, buf.barrier_dot)
    idx = buf.sample_indices(5)
    assert idx.shape == (5,) and (idx >= 0).all() and (idx < len(buf)).all()
    assert buf.gather(idx)['state'].dtype == torch.float32


def test_registry_entry_defaults_and_settings():
    from safe_control_gym_amd.cbf import CBF
    from safe_control_gym_amd.cbf_nn import CBF_NN, CBF_NN_DEFAULTS
    from safe_control_gym_amd.registration import get_config
    assert get_config('cbf_nn') == S['sf_defaults'] == CBF_NN_DEFAULTS
    assert S['safety_filter'] == 'cbf_nn' and SF['hidden_dims'] == [256, 256]
    sf = _filter()
    assert isinstance(sf, CBF_NN) and isinstance(sf, CBF)
    assert (sf.max_num_steps, sf.num_episodes, sf.train_batch_size, sf.train_iterations, sf.learning_rate) == \
        tuple(SF[k] for k in ('max_num_steps', 'num_episodes', 'train_batch_size', 'train_iterations', 'learning_rate'))
    assert [tuple(t.shape) for t in sf._tensors()] == [(256, 4), (256,), (256, 256), (256,), (2, 256), (2,)]
    assert isinstance(sf.opt, torch.optim.Adam) and sf.opt.defaults['lr'] == SF['learning_rate']
    assert sf.uncertified_controller is None
    text = open(os.path.join(ROOT, 'safe_control_gym_amd', 'registration.py')).read()
    assert not re.search(r"cbf_nn'[^\n]*out of scope", text)


def test_checkpoint_keys_round_trip(tmp_path):
    sf = _filter()
    _load_weights(sf)
    path = str(tmp_path / 'ckpt' / 'model.pt')
    sf.save(path)
    state = torch.load(path, weights_only=False)
    assert set(state) == {'agent', 'buffer'} and list(state['agent']) == list(NM.KEYS)
    assert list(state['buffer']) == ['pos', 'buffer_size', 'state', 'act', 'barrier_dot', 'barrier_dot_approx']
    other = _filter(training=False)
    other.save(str(tmp_path / 'eval.pt'))
    assert set(torch.load(str(tmp_path / 'eval.pt'), weights_only=False)) == {'agent'}
    other.load(path)
    for k in NM.KEYS:
        assert torch.equal(other.mlp.state_dict()[k], sf.mlp.state_dict()[k])


def test_refusals():
    from safe_control_gym_amd import _cbf_nn
    from safe_control_gym_amd import _lib as L
    from safe_control_gym_amd.registration import load_task, make
    with pytest.raises(NotImplementedError, match=re.escape('cbf_nn serves hidden_dims = [256, 256]')):
        _filter(hidden_dims=[64, 64])
    env_id, cfg = load_task('quadrotor_2D_track')
    cfg = dict(cfg, constraints=[{'constraint_form': 'default_constraint', 'constrained_variable': 'state'},
                                 {'constraint_form': 'default_constraint', 'constrained_variable': 'input'}])
    with pytest.raises(NotImplementedError, match=re.escape('[Error] Currently CBF is only implemented for the cartpole system.')):
        make('cbf_nn', partial(make, env_id, **cfg))
    # actor kinds and shapes
    assert _cbf_nn.supported('cartpole', 4, 64, 1, 'tanh') and _cbf_nn.supported('cartpole', 8, 128, 1, 'relu')
    assert not _cbf_nn.supported('cartpole', 4, 64, 1, 'tanh', kind='sac') and not _cbf_nn.supported('cartpole', 4, 256, 1, 'relu', kind='ddpg')
    assert not _cbf_nn.supported('cartpole', 4, 256, 1, 'relu')              # PPO's tuple has no width 256
    assert not _cbf_nn.supported('quadrotor', 6, 64, 2, 'tanh') and not _cbf_nn.supported('cartpole', 4, 64, 1, 'gelu')
    sf = _filter()

    class NotPpo:
        impl = object()
    with pytest.raises(L.ScgError, match='no SAC / DDPG'):
        sf._actor_of(NotPpo())


def test_lds_arithmetic():
    """The host's LDS arithmetic restates csrc/scg_mlp_rows.h (MlpRowsLds<4, 2, G>) and csrc/scg_mlp.h (MlpLds<obs, H, 1, 16>): the row-split
    image alone is what DESIGN's wide-kernel table lists for 6-float rows' L1Q = 4 sibling; with the actor image the 160 KiB limit
    decides the geometry."""
    from safe_control_gym_amd import _cbf_nn
    assert _cbf_nn.rows_image_bytes(1) == 4 * (3076 + 256 + 16384 + 512) and _cbf_nn.rows_image_bytes(8) == 4 * (3076 + 2048 + 16384 + 4096)
    # MlpLds<4, 64, 1, 16>: W1F 2 x 4 x 64, W2F 4 tiles x 1024, W3 64, biases 128, b3 1 -> 4 804 words (rounded up to 16-byte granules)
    assert _cbf_nn.actor_image_bytes(4, 64) == 4 * 4804
    for obs in (4, 8):
        for hidden in (32, 64, 96, 128):
            b1, b8 = _cbf_nn.rollout_lds_bytes(obs, hidden, 1), _cbf_nn.rollout_lds_bytes(obs, hidden, 8)
            assert b1 <= _cbf_nn.LDS_LIMIT
            assert _cbf_nn.rollout_tiles(obs, hidden, 100) == 1
            assert _cbf_nn.rollout_tiles(obs, hidden, 65536) == (8 if b8 <= _cbf_nn.LDS_LIMIT else 1)
    assert _cbf_nn.rollout_lds_bytes(4, 128, 8) > _cbf_nn.LDS_LIMIT          # G = 1 at every N
    assert _cbf_nn.rollout_lds_bytes(4, 96, 8) <= _cbf_nn.LDS_LIMIT
    assert _cbf_nn.rollout_tiles(4, 160, 1) is None                          # an actor that does not fit at G = 1 either: refused
    assert _cbf_nn.residual_sizes() == [1024, 256, 65536, 256, 512, 2]


def test_header_and_binding_agree():
    import ctypes as C
    from safe_control_gym_amd import _cbf_nn
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'scg_cbf_nn.h')).read(), flags=re.S)
    names = set(re.findall(r'\b(scg_[a-z_0-9]+)\s*\(', hdr))
    assert {'scg_cbf_nn_certify', 'scg_rollout_cbf_nn', 'scg_cbf_nn_shape', 'scg_cbf_nn_lds'} <= names
    for struct, cls in (('scg_cbf_residual', _cbf_nn.Residual), ('scg_cbf_nn_mode', _cbf_nn.Mode)):
        fields = re.search(r'typedef struct %s \{(.*?)\}' % struct, hdr, re.S).group(1)
        declared = [n.split()[-1].lstrip('*') for line in fields.split(';') if line.strip() for n in line.strip().split(None, 1)[1].split(',')]
        assert declared == [f[0] for f in cls._fields_], struct
    assert C.sizeof(_cbf_nn.Residual) == 8 + 6 * 4 + 4 + 4 and C.sizeof(_cbf_nn.Mode) == 5 * 4
    # ONE copy of the closed form: the nn variant adds the residual to the row and calls the same solve
    core = open(os.path.join(ROOT, 'safe_control_gym_amd', 'csrc', 'scg_cbf_core.h')).read()
    for fn in ('cbf_row', 'cbf_solve', 'cbf_certify', 'cbf_nn_certify'):
        assert len(re.findall(r'__forceinline__ \w+ %s\(' % fn, core)) == 1, fn
    assert '#include "scg_cbf_core.h"' in open(os.path.join(ROOT, 'safe_control_gym_amd', 'csrc', 'scg_cbf_nn.hip')).read()
