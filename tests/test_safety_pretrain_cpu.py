"""The Safe-Explorer pre-training update on the CPU: the NumPy float64 restatement (tests/safety_pretrain_model.py) against the reference's
own SafetyLayer runs (tests/golden/make_safety_pretrain.py -> safety_pretrain.npz), the fixture's shape, and SafetyLayer's flat storage
(what scg_safety_update works on) against the plain layer: same state_dict, moments and step counts intact across save / load."""
import copy
import os

import numpy as np
import pytest

from tests import safety_pretrain_model as M

torch = pytest.importorskip('torch')


def test_fixture_is_small_and_has_the_two_shapes():
    assert os.path.getsize(M.GOLDEN) < 256 * 1024
    a, b = (M.load_case(n) for n in M.CASES)
    assert (a['obs_dim'], a['act_dim'], a['C'], a['Hc'], a['batch'], a['n_batches'], a['lr']) == (4, 1, 8, 100, 33, 5, 1e-3)
    assert (b['obs_dim'], b['act_dim'], b['C'], b['Hc'], b['batch'], b['n_batches'], b['lr']) == (6, 2, 12, 16, 257, 4, 1e-3)
    for g in (a, b):
        P = g['Hc'] * (g['obs_dim'] + 1 + g['act_dim']) + g['act_dim']
        assert g['init'].shape == (g['C'], P) and g['init'].dtype == np.float32
        assert g['rows'].shape == (g['n_batches'], g['batch']) and g['rows'].min() >= 0 and g['rows'].max() < g['capacity']
        assert g['final32'].dtype == np.float32 and np.isfinite(g['final32']).all()
        assert np.abs(g['final64'] - g['init']).max() > 1e-3                 # the run moved the parameters
        assert np.abs(g['grad64']).max() > 0.1


@pytest.mark.parametrize('name', M.CASES)
def test_model_reproduces_the_float64_run(name):
    g = M.load_case(name)
    r = M.run(g['init'], g['data'], g['rows'], g['lr'])
    for k in ('loss', 'final', 'm', 'v', 'grad'):
        err = np.abs(r[k] - g[k + '64']).max()
        print(f'{name} {k}: max |model - reference float64| = {err:.3g}')
        np.testing.assert_allclose(r[k], g[k + '64'], rtol=1e-12, atol=1e-12, err_msg=k)
    assert r['steps'] == g['n_batches']


@pytest.mark.parametrize('name', M.CASES)
def test_model_is_within_the_references_own_float32_distance(name):
    """|model - reference float32| <= 4 x max |reference float32 - reference float64|, per quantity."""
    g = M.load_case(name)
    r = M.run(g['init'], g['data'], g['rows'], g['lr'])
    for k in ('loss', 'final', 'm', 'v', 'grad'):
        own = np.abs(g[k + '32'].astype(np.float64) - g[k + '64']).max()
        err = np.abs(r[k] - g[k + '32']).max()
        print(f'{name} {k}: reference f32-f64 {own:.3g}, model-f32 {err:.3g}')
        assert own > 0 and err <= 4 * own, (k, err, own)


def test_loss_only_mode_and_ring_rows():
    g = M.load_case('cartpole_stab')
    r = M.run(g['init'], g['data'], g['rows'], g['lr'], train=False)
    assert np.array_equal(r['final'], g['init'].astype(np.float64)) and r['steps'] == 0
    np.testing.assert_allclose(r['loss'][0], g['loss64'][0], rtol=1e-12)
    rows = M.ring_rows(pos=13 * 7 + 6, k_steps=4, n_envs=7, capacity=30)      # wraps inside the launch
    assert rows.shape == (4, 7) and rows[0, 0] == 97 % 30 and rows[1, 0] == (97 + 7) % 30 and rows[3, 6] == (97 + 27) % 30
    assert len(set(rows.reshape(-1).tolist())) == 28                          # k * N <= capacity: no row twice


def _layer(seed, flat):
    from safe_control_gym_amd.safe_explorer import SafetyLayer
    torch.manual_seed(seed)
    layer = SafetyLayer(5, 2, 3, hidden_dim=7, lr=3e-3, slack=[0.05, 0.0, 0.1])
    return layer.flatten() if flat else layer


def _batch(seed, n=20):
    g = torch.Generator().manual_seed(seed)
    return {'obs': torch.randn(n, 5, generator=g), 'act': torch.randn(n, 2, generator=g), 'c': torch.randn(n, 3, generator=g),
            'c_next': torch.randn(n, 3, generator=g)}


def _assert_same_state(a, b):
    assert list(a['constraint_models']) == list(b['constraint_models'])
    for k in a['constraint_models']:
        assert torch.equal(a['constraint_models'][k], b['constraint_models'][k]), k
    assert len(a['optimizers']) == len(b['optimizers'])
    for oa, ob in zip(a['optimizers'], b['optimizers']):
        assert oa['param_groups'] == ob['param_groups'] and set(oa['state']) == set(ob['state'])
        for i in oa['state']:
            assert set(oa['state'][i]) == set(ob['state'][i]) == {'step', 'exp_avg', 'exp_avg_sq'}
            for k in oa['state'][i]:
                assert torch.equal(torch.as_tensor(oa['state'][i][k]), torch.as_tensor(ob['state'][i][k])), (i, k)


def test_flat_storage_has_the_unflattened_layers_state_dict():
    plain, flat = _layer(3, False), _layer(3, True)
    fl = flat._flat
    assert fl['p'].shape == (3, 7 * (5 + 1 + 2) + 2)
    for m in flat.constraint_models:                                         # the parameters are views into the one buffer
        for p in m.parameters():
            assert p.data_ptr() >= fl['p'].data_ptr() and p.data_ptr() < fl['p'].data_ptr() + fl['p'].numel() * 4
    W1, b1, W2, b2 = M.split(fl['p'].numpy(), 5, 2, 7)
    assert np.array_equal(W1[1], flat.constraint_models[1].fcs[0].weight.detach().numpy())
    assert np.array_equal(b2[2], flat.constraint_models[2].fcs[1].bias.detach().numpy())
    _assert_same_state(plain.state_dict(), flat.state_dict())                # never stepped: empty optimiser states on both
    for s in (11, 12):                                                       # eager updates act on the flat buffer through the views
        assert torch.equal(plain.update(_batch(s)), flat.update(_batch(s)))
    _assert_same_state(plain.state_dict(), flat.state_dict())
    assert np.array_equal(M.split(fl['p'].numpy(), 5, 2, 7)[2][0], flat.constraint_models[0].fcs[1].weight.detach().numpy())


def test_flat_moments_travel_in_torch_optims_layout_both_ways():
    """A state dict saved from the flat moments (as after fused updates) loads into an eager layer and back: moments and step counts
    intact, and both layers then take the same eager step."""
    flat = _layer(5, True)
    fl = flat._flat
    g = torch.Generator().manual_seed(9)
    fl['m'].copy_(torch.randn(fl['m'].shape, generator=g) * 1e-2)
    fl['v'].copy_(torch.rand(fl['v'].shape, generator=g) * 1e-3)
    fl['steps'].copy_(torch.tensor([4.0, 4.0, 4.0]))
    fl['moments'] = 'flat'                                                   # what update_fused(train=True) leaves
    sd = copy.deepcopy(flat.state_dict())
    assert set(sd) == {'constraint_models', 'optimizers'} and '2.fcs.1.weight' in sd['constraint_models']
    st = sd['optimizers'][1]['state']
    assert sorted(st) == [0, 1, 2, 3] and float(st[0]['step']) == 4.0
    assert torch.equal(st[0]['exp_avg'].reshape(-1), fl['m'][1, :35]) and torch.equal(st[3]['exp_avg_sq'].reshape(-1), fl['v'][1, -2:])
    eager = _layer(6, False)
    eager.load_state_dict(sd)
    _assert_same_state(eager.state_dict(), sd)
    back = _layer(7, True)
    back.load_state_dict(copy.deepcopy(eager.state_dict()))
    assert back._flat['moments'] == 'opt'
    back._moments_from_optimizers()
    for k in ('p', 'm', 'v', 'steps'):
        assert torch.equal(back._flat[k], fl[k]), k
    assert torch.equal(eager.update(_batch(21)), flat.update(_batch(21)))     # flat: the optimisers continue from the flat moments
    _assert_same_state(eager.state_dict(), flat.state_dict())
    assert float(flat.state_dict()['optimizers'][0]['state'][0]['step']) == 5.0
