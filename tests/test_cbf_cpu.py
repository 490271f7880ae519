"""The CBF safety filter without a GPU: the float64 restatement (tests/cbf_model.py) against the reference-generated fixture
(tests/golden/cbf.npz, made by tests/golden/make_cbf.py from the reference's own cbf_cartpole / get_lie_derivative expressions and a
general-purpose QP solve), the registry id and its defaults, the constructor's errors, the C header."""
import copy
import json
import os
import re
from functools import partial

import numpy as np
import pytest

from tests import cbf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
D = np.load(os.path.join(GOLDEN, 'cbf.npz'))
S = json.load(open(os.path.join(GOLDEN, 'cbf_settings.json')))
SF = S['sf_config']
LO, HI = (float(v) for v in D['action_bounds'])


def env_func(**over):
    from safe_control_gym_amd.registration import make
    cfg = copy.deepcopy(S['task_config'])
    cfg.update(over)
    return partial(make, S['task'], **cfg)


def restated(tag, soft, dtype=np.float64):
    return M.certify(D['states'], D['actions'], D['limits'], D[f'{tag}/prior'], SF['slope'], SF['slack_weight'], SF['slack_tolerance'], LO, HI,
                     soft=soft, dtype=dtype)


@pytest.mark.parametrize('tag', ['default', 'alt'])
def test_barrier_and_lie_derivative_equal_the_reference_expressions(tag):
    """h, LfV(X, 0), LfV(X, 1) of the reference's expression graph, 1e-12 relative; b against the difference of the two Lie derivatives,
    relative to the larger of them (the subtraction cancels: the fixture's difference carries their rounding, not b's)."""
    assert len(D['states']) >= 2000 and np.abs(D['states'] / D['limits']).max() > 1.05
    h, a, b = M.barrier_terms(D['states'], D['limits'], D[f'{tag}/prior'])
    np.testing.assert_allclose(h, D[f'{tag}/h'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(a, D[f'{tag}/LfV0'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(a + b, D[f'{tag}/LfV1'], rtol=1e-12, atol=0)
    scale = np.maximum(np.abs(D[f'{tag}/LfV0']), np.abs(D[f'{tag}/LfV1']))
    assert (np.abs(b - (D[f'{tag}/LfV1'] - D[f'{tag}/LfV0'])) <= 1e-12 * scale).all()


@pytest.mark.parametrize('tag', ['default', 'alt'])
@pytest.mark.parametrize('mode', ['soft', 'hard'])
def test_closed_form_equals_the_solver_minimisers(tag, mode):
    r = restated(tag, mode == 'soft')
    acc, nonempty = D[f'{tag}/{mode}/accepted'], D[f'{tag}/{mode}/nonempty']
    rows = acc & nonempty
    assert rows.sum() >= 2000 and D[f'{tag}/{mode}/kkt'][acc].max() < S['kkt_tol']
    du = np.abs(r['u'] - D[f'{tag}/{mode}/u'])[rows].max()
    ds = np.abs(r['s'] - D[f'{tag}/{mode}/s'])[rows].max()
    corrected = (np.abs(r['u'] - r['u0']) > 1e-9)[rows].mean()
    print(f'{tag} {mode}: rows {int(rows.sum())}, |du| <= {du:.3e}, |ds| <= {ds:.3e}, corrected {corrected:.3f}, feasible {r["feasible"].mean():.3f}')
    assert du <= 1e-6 and ds <= 1e-6
    assert corrected > 0.2 and (np.abs(D['actions']) > HI).any()            # the correction and the input clip are exercised
    if mode == 'hard':                                                      # empty feasible set: the flag only
        assert (r['feasible'] == nonempty).all() and (~nonempty).sum() > 0
        assert (r['u'][~nonempty] == r['u0'][~nonempty]).all()


@pytest.mark.parametrize('tag', ['default', 'alt'])
@pytest.mark.parametrize('mode', ['soft', 'hard'])
def test_closed_form_satisfies_the_kkt_conditions(tag, mode):
    """Stationarity, primal and dual feasibility, complementarity of the restatement's own minimiser, with the multipliers the closed
    form implies (lam = 2 w s for the barrier row of the soft problem; (u - u0) / b for the hard one)."""
    soft = mode == 'soft'
    r = restated(tag, soft)
    h, a, b = M.barrier_terms(D['states'], D['limits'], D[f'{tag}/prior'])
    k = SF['slope'] * h + a
    u, u0, s = r['u'], r['u0'], r['s']
    rows = r['feasible'] if not soft else np.ones(len(u), bool)
    g = k + b * u + s                                                       # barrier row, >= 0
    assert (g[rows] >= -1e-9).all() and (s >= 0).all() and (u >= LO).all() and (u <= HI).all()
    with np.errstate(divide='ignore', invalid='ignore'):
        lam = 2 * SF['slack_weight'] * s if soft else np.where(np.abs(u - u0) > 0, (u - u0) / b, 0.0)
    assert (lam[rows] >= -1e-9).all()
    assert (np.abs(lam * g)[rows] <= 1e-9 * np.maximum(1.0, np.abs(lam))[rows]).all()                   # complementarity
    ru = (u - u0) - lam * b                                                 # = mu_lo - mu_hi: zero inside the box, signed on its faces
    inside = (u > LO) & (u < HI)
    assert (np.abs(ru)[rows & inside] <= 1e-9 * np.maximum(1.0, np.abs(lam * b))[rows & inside]).all()
    assert (ru[rows & (u <= LO)] >= -1e-9).all() and (ru[rows & (u >= HI)] <= 1e-9).all()


def test_registry_id_and_defaults():
    from safe_control_gym_amd.cbf import CBF, CBF_DEFAULTS
    from safe_control_gym_amd.registration import get_config, make
    assert get_config('cbf') == S['sf_defaults'] == CBF_DEFAULTS
    sf = make('cbf', env_func(), **copy.deepcopy(SF))
    assert isinstance(sf, CBF)
    assert (sf.slope, sf.soft_constrained, sf.slack_weight, sf.slack_tolerance) == tuple(S['sf_defaults'][k] for k in
                                                                                       ('slope', 'soft_constrained', 'slack_weight', 'slack_tolerance'))
    assert sf.state_limits == list(D['limits']) and set(sf.results_dict) == {'feasible', 'uncertified_action', 'certified_action', 'correction'}
    p = sf.params()
    assert list(p.L) == [np.float32(v) for v in D['limits']] and (p.lo, p.hi, p.soft) == (LO, HI, 1)
    np.testing.assert_allclose([p.l, p.m, p.M, p.g], D['default/prior'], rtol=1e-7)
    alt = make('cbf', env_func(), prior_info={'prior_prop': S['non_default_prior_prop']}).params()
    np.testing.assert_allclose([alt.l, alt.m, alt.M, alt.g], D['alt/prior'], rtol=1e-7)
    with pytest.raises(NotImplementedError, match='select_action is not and will not be implemented'):
        sf.select_action(np.zeros(4))


def test_constructor_errors_match_the_reference():
    """cbf.py:49-70: exception types and texts."""
    from safe_control_gym_amd.registration import make
    state = copy.deepcopy(S['task_config']['constraints'][0])
    inp = copy.deepcopy(S['task_config']['constraints'][1])
    with pytest.raises(NotImplementedError, match="CBF currently can't handle more than 1 constraint"):
        make('cbf', env_func(constraints=[state, state, inp]))
    with pytest.raises(NotImplementedError, match="CBF currently can't handle more than 1 constraint"):
        make('cbf', env_func(constraints=[state, inp, inp]))
    with pytest.raises(Exception, match='CBF requires at least 1 input constraint') as e:
        make('cbf', env_func(constraints=[state]))
    assert type(e.value) is Exception
    with pytest.raises(Exception, match='CBF requires at least 1 state constraint') as e:
        make('cbf', env_func(constraints=[inp]))
    assert type(e.value) is Exception
    from safe_control_gym_amd.registration import load_task
    env_id, cfg = load_task('quadrotor_2D_track')
    cfg = dict(cfg, constraints=[{'constraint_form': 'default_constraint', 'constrained_variable': 'state'},
                                 {'constraint_form': 'default_constraint', 'constrained_variable': 'input'}])
    with pytest.raises(NotImplementedError, match=re.escape('[Error] Currently CBF is only implemented for the cartpole system.')):
        make('cbf', partial(make, env_id, **cfg))


def test_grid_is_the_reference_grid():
    """cbf.py:243-259: 100 points -> 104 -> 26 per dimension, +-(limits + tolerance), first dimension slowest."""
    from safe_control_gym_amd.cbf import grid_points_per_dim, state_grid
    assert grid_points_per_dim(100, 4) == 26 and grid_points_per_dim(3, 4) == 2
    g = state_grid(D['limits'], 100, 0.01)
    assert g.shape == (26 ** 4, 4)
    np.testing.assert_allclose(g[0], -(D['limits'] + 0.01))
    np.testing.assert_allclose(g[-1], D['limits'] + 0.01)
    assert (g[1, :3] == g[0, :3]).all() and g[1, 3] > g[0, 3]


def test_header_declares_both_entry_points():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'scg_cbf.h')).read(), flags=re.S)
    names = set(re.findall(r'\b(scg_[a-z_0-9]+)\s*\(', hdr))
    assert {'scg_cbf_certify', 'scg_rollout_cbf', 'scg_cbf_shape'} <= names
    from safe_control_gym_amd import _cbf
    fields = re.search(r'typedef struct scg_cbf_params \{(.*?)\}', hdr, re.S).group(1)
    declared = [n.strip().split('[')[0] for line in fields.split(';') if line.strip() for n in line.strip().split(None, 1)[1].split(',')]
    assert declared == [f[0] for f in _cbf.CbfParams._fields_]
    import ctypes as C
    assert C.sizeof(_cbf.CbfParams) == 14 * 4
    # ONE device function in all of csrc/, in the header both CBF translation units include
    csrc = os.path.join(ROOT, 'safe_control_gym_amd', 'csrc')
    defs = [n for n in sorted(os.listdir(csrc)) if n.endswith(('.h', '.hip'))
            and re.search(r'CbfResult\s+cbf_certify\s*\(', open(os.path.join(csrc, n)).read())]
    assert defs == ['scg_cbf_core.h']
    assert len(re.findall(r'CbfResult\s+cbf_certify\s*\(', open(os.path.join(csrc, defs[0])).read())) == 1
    for unit in ('scg_cbf.hip', 'scg_cbf_wide.hip'):
        assert '#include "scg_cbf_core.h"' in open(os.path.join(csrc, unit)).read()
