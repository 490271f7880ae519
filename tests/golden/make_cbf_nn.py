#!/usr/bin/env python3
"""Golden vectors of the reference's cbf_nn safety filter (safety_filters/cbf/cbf_nn.py).

    python tests/golden/make_cbf_nn.py            (build container only: needs /root/reference and SciPy)

What is evaluated is the reference's OWN code, on tests/golden/ref_stubs.py and casadi_numeric.py (as make_cbf.py does):
    math_and_models/neural_networks.py   MLP(4, 2, [256, 256], 'relu')                       the residual network and its initial weights
    safety_filters/cbf/cbf_nn.py         CBF_NN.extract_a_b, compute_loss, update            called on a holder of `mlp`, `opt`, `model`
    safety_filters/cbf/cbf_utils.py      cbf_cartpole, CBFBuffer                             the barrier, the buffer (with a wrap-around push)
    safety_filters/cbf/cbf.py            CBF.get_lie_derivative                              LfV(X, u)
    envs/gym_control/cartpole.py         the env of the recorded trajectory and the prior model

The QP minimisers come from make_cbf.solve_row (SciPy SLSQP, float64) fed the learned row: cbf_nn.py:104-124 is
    -slope h - LfV(X, u) - (a_nn u + b_nn) <= s,   LfV = a + b u    =>    the plain problem with a' = a + b_nn, b' = b + a_nn,
and a row enters the fixture only when its KKT residual (make_cbf.kkt_residual) is below 1e-9 (the minimiser is unique, make_cbf.py's
docstring).  About a fifth of the soft rows stay above that with SLSQP and kkt_residual (in cbf.npz too: 79-83 % accepted: the rows
with a large slack, where the non-negative least squares inside kkt_residual is itself only good to ~1e-7); those rows are solved
again by `active_set_row`, an exact enumeration of the active sets of the same two-variable QP (one linear solve each), and are held
to the same residual with the multipliers of that solve.  `soft/polished` marks them.  Neither solver is the closed form the kernels evaluate.

The slicing of learn() (cbf_nn.py:357-380) is restated in `pushed_by_the_reference` with its line numbers; the Functions it calls are
the reference's.

Output: tests/golden/cbf_nn.npz, tests/golden/cbf_nn_settings.json.  States and actions are float32 values (stored as such): the
kernels read float32, and the reference is evaluated on exactly those numbers.  Of the parameters after the three updates the five
small tensors are stored whole and W2 as every 8th row plus the float64 sum and sum of squares of the whole tensor (the file stays
below the largest committed fixture).
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_cbf  # noqa: E402  (installs the stubs, defines cs.gradient / cs.dot)
from tests.golden.make_cbf import KKT_TOL, solve_row  # noqa: E402

import torch  # noqa: E402
import yaml  # noqa: E402
from safe_control_gym.envs.gym_control.cartpole import CartPole  # noqa: E402
from safe_control_gym.math_and_models.neural_networks import MLP  # noqa: E402
from safe_control_gym.safety_filters.cbf.cbf_utils import CBFBuffer, cbf_cartpole  # noqa: E402

from tests import cbf_nn_model as NM  # noqa: E402
from tests.golden.make_golden import REF, load_task_config  # noqa: E402

N_STATES = 3000
TORCH_SEED = 20261021
W3_SCALE, B3_SCALE = 10.0, 5.0          # the output layer of the freshly initialised network, scaled so that the residual matters
TRAJ_STEPS, BATCH_ROWS, N_UPDATES = 12, 64, 3
W2_ROW_STRIDE = 8
BUFFER_SIZE = 16                         # two pushes of TRAJ_STEPS - 2 = 10 rows: the second wraps around


def reference_cbf_nn():
    from safe_control_gym.safety_filters.cbf.cbf_nn import CBF_NN
    return CBF_NN


def active_set_row(k, b, u0, w, lo, hi):
    """The soft QP in (u, z = sqrt(2 w) s):  min 1/2 (u - u0)^2 + 1/2 z^2  s.t.  G x + d >= 0  with rows (b, 1 / c), (0, 1), (1, 0),
    (-1, 0).  For every subset of rows taken as equalities the KKT system is linear; the subset whose solution is primal and dual
    feasible is the minimiser.  Returns (u, s, True, KKT residual) of the best subset, as solve_row does.  The residual is the largest of
    the stationarity components, the complementarity products m_i g_i and the primal infeasibilities, as make_cbf.kkt_residual's, but
    with the multipliers of the subset's own linear solve: kkt_residual finds its multipliers by non-negative least squares, whose own
    accuracy (~1e-7 where z = sqrt(2 w) s is in the hundreds, i.e. on every row whose slack is large) is above the 1e-9 asked of the
    point.  A point that passes here has multipliers m >= 0 with every KKT component below the tolerance, which bounds the least-squares
    optimum too."""
    import itertools
    c = np.sqrt(2.0 * w)
    G = np.array([[b, 1.0 / c], [0.0, 1.0], [1.0, 0.0], [-1.0, 0.0]])
    d = np.array([k, 0.0, -lo, hi])
    x0 = np.array([u0, 0.0])
    best = None
    for r in range(0, 3):
        for act in itertools.combinations(range(4), r):
            A = G[list(act)]
            n = len(act)
            K = np.block([[np.eye(2), -A.T], [A, np.zeros((n, n))]]) if n else np.eye(2)
            rhs = np.concatenate([x0, -d[list(act)]])
            sol = np.linalg.lstsq(K, rhs, rcond=None)[0]
            for _ in range(3):                       # iterative refinement, the defect in extended precision (cond(K) ~ 2 w)
                defect = (rhs.astype(np.longdouble) - K.astype(np.longdouble) @ sol.astype(np.longdouble)).astype(np.float64)
                sol = sol + np.linalg.lstsq(K, defect, rcond=None)[0]
            u, z = float(min(max(sol[0], lo), hi)), float(max(sol[1], 0.0))
            m = np.zeros(4)
            m[list(act)] = sol[2:]
            if (m < 0.0).any():                      # not dual feasible: not the minimiser
                continue
            g = np.array([k + b * u + z / c, z, u - lo, hi - u])
            res = float(max(np.abs(np.array([u - u0, z]) - G.T @ m).max(), np.abs(m * g).max(), np.maximum(0.0, -g).max()))
            if best is None or res < best[3]:
                best = (u, z / c, True, res)
    return best


def pushed_by_the_reference(cbf, lie_derivative, obs_after, inputs, ctrl_freq):
    """cbf_nn.py:357-380 for one recorded episode: obs_after[c] is `obs` after env.step(blended_input) of step c, inputs[c] that input."""
    n = len(inputs)
    states = np.zeros((n, 4))
    inp = np.zeros((n, 1))
    barrier_values = np.zeros((n, 1))
    lie_derivative_values = np.zeros((n, 1))
    for counter in range(n):
        obs, blended_input = obs_after[counter], inputs[counter]
        states[counter, :] = obs                                                                       # :357
        inp[counter, :] = blended_input                                                                # :358
        barrier_values[counter, :] = cbf(X=obs)['cbf']                                                 # :359
        lie_derivative_values[counter, :] = lie_derivative(X=obs, u=blended_input)['LfV']              # :360
    barrier_dot_approx = (barrier_values[2:] - barrier_values[:-2]) / (2 * 1 / ctrl_freq)              # :372
    return {'state': states[1:-1, :], 'act': inp[1:-1, :], 'barrier_dot': lie_derivative_values[1:-1, :],        # :375-380
            'barrier_dot_approx': barrier_dot_approx}


def main():
    CBF_NN = reference_cbf_nn()
    with open(os.path.join(REF, 'examples/cbf/config_overrides/cbf_nn_config.yaml')) as f:
        sf = yaml.safe_load(f)
    with open(os.path.join(REF, 'safe_control_gym/safety_filters/cbf/cbf_nn.yaml')) as f:
        sf_defaults = yaml.safe_load(f)
    with open(os.path.join(REF, 'examples/cbf/config_overrides/ppo_config.yaml')) as f:
        algo = yaml.safe_load(f)
    task_cfg = load_task_config('cartpole', 'examples/cbf/config_overrides/cartpole_config.yaml')
    cfg = dict(task_cfg)
    cfg.pop('seed', None)
    cfg['output_dir'] = '/tmp'
    env = CartPole(**cfg)
    sc = env.constraints.state_constraints[0]
    limits = [min(abs(sc.upper_bounds[i]), abs(sc.lower_bounds[i])) for i in range(4)]
    lo, hi = float(env.physical_action_bounds[0][0]), float(env.physical_action_bounds[1][0])
    c = sf['sf_config']
    slope, w, tol = c['slope'], c['slack_weight'], c['slack_tolerance']
    env._setup_symbolic(prior_prop={})
    model = env.symbolic
    holder = types.SimpleNamespace(X=model.x_sym, u=model.u_sym, model=model, cbf=cbf_cartpole(model.x_sym, limits))
    lie = make_cbf.reference_lie_derivative()(holder)
    prior = np.array([env.EFFECTIVE_POLE_LENGTH, env.POLE_MASS, env.CART_MASS, env.GRAVITY_ACC])          # l, m, M, g

    # ---- the residual network: the reference's MLP at a fixed seed, output layer scaled
    torch.manual_seed(TORCH_SEED)
    mlp = MLP(model.nx, model.nu + 1, hidden_dims=list(c['hidden_dims']), activation='relu')
    with torch.no_grad():
        mlp.fcs[-1].weight.mul_(W3_SCALE)
        mlp.fcs[-1].bias.mul_(B3_SCALE)
    weights = [mlp.state_dict()[k].detach().numpy().copy() for k in NM.KEYS]

    class Holder:                          # what CBF_NN's methods read of `self`
        extract_a_b, compute_loss, update = CBF_NN.extract_a_b, CBF_NN.compute_loss, CBF_NN.update

    hold = Holder()
    hold.mlp, hold.model = mlp, types.SimpleNamespace(nu=model.nu)

    # ---- rows: drawn as in make_cbf.py, rounded to float32; the seed is redrawn until the float64 answers alone keep the share of
    #      boundary rows (|r(u0)| or |s* - tolerance| within the slack bound) at or below 1 %
    for seed in range(20261021, 20261041):
        rng = np.random.default_rng(seed)
        states = (rng.uniform(-1.1, 1.1, size=(N_STATES, 4)) * np.asarray(limits)).astype(np.float32)
        actions = rng.uniform(-12.0, 12.0, size=N_STATES).astype(np.float32)
        a_b = np.stack([np.concatenate([np.atleast_1d(v) for v in hold.extract_a_b(np.asarray(x, dtype=np.float64))]) for x in states]).astype(np.float32)
        a_b64 = NM.forward(weights, states.astype(np.float64))
        args = (states.astype(np.float64), actions.astype(np.float64), a_b, limits, prior, slope, w, tol, lo, hi)
        share = {}
        for mode, soft in (('soft', True), ('hard', False)):
            r64, r32 = NM.certify(*args, soft=soft), NM.certify(*args, soft=soft, dtype=np.float32)
            bound_u = 4 * np.abs(r32['u'].astype(np.float64) - r64['u']).max()
            bound_s = 4 * np.abs(r32['s'].astype(np.float64) - r64['s']).max()
            near = np.abs(r64['r0']) <= bound_s
            if soft:
                near |= np.abs(r64['s'] - tol) <= bound_s
            plain = NM.certify(*args[:2], np.zeros_like(a_b), *args[3:], soft=soft)
            share[mode] = (near.mean(), (np.abs(plain['u'] - r64['u']) > 100 * bound_u).mean(), bound_u, bound_s)
        print(f'seed {seed}: ' + ', '.join(f'{m}: boundary share {v[0]:.4f}, residual matters on {v[1]:.3f}, bounds {v[2]:.2e} / {v[3]:.2e}'
                                           for m, v in share.items()))
        if all(v[0] <= 0.01 for v in share.values()):
            break
    else:
        raise SystemExit('no seed keeps the boundary rows at or below 1 %')
    assert all(v[1] >= 0.25 for v in share.values()), 'the residual must move u* on at least a quarter of the rows'
    assert np.abs(a_b64 - a_b).max() <= 1e-5 * np.abs(a_b64).max() + 1e-5, 'float64 forward disagrees with the reference'
    out = {'states': states, 'actions': actions, 'limits': np.asarray(limits, dtype=np.float64), 'action_bounds': np.array([lo, hi]),
           'prior': prior, 'a_b': a_b, 'a_b64': a_b64, 'row_seed': np.array(seed)}
    for k, v in zip(NM.KEYS, weights):
        out['mlp/' + k] = v

    # ---- minimisers of the learned row: the reference's h and LfV Functions + the float64 forward, make_cbf.solve_row
    X64 = states.astype(np.float64)
    h = np.array([float(np.asarray(holder.cbf(X=x)['cbf']).reshape(-1)[0]) for x in X64])
    l0 = np.array([float(np.asarray(lie(X=x, u=np.zeros(1))['LfV']).reshape(-1)[0]) for x in X64])
    l1 = np.array([float(np.asarray(lie(X=x, u=np.ones(1))['LfV']).reshape(-1)[0]) for x in X64])
    for mode, soft in (('soft', True), ('hard', False)):
        rows = [solve_row(h[i], l0[i] + a_b64[i, 1], (l1[i] - l0[i]) + a_b64[i, 0], float(actions[i]), slope, w, lo, hi, soft) for i in range(N_STATES)]
        polished = np.zeros(N_STATES, bool)
        if soft:
            for i, r in enumerate(rows):
                if not r[3] < KKT_TOL:
                    rows[i] = active_set_row(slope * h[i] + l0[i] + a_b64[i, 1], (l1[i] - l0[i]) + a_b64[i, 0],
                                             min(max(float(actions[i]), lo), hi), w, lo, hi)
                    polished[i] = True
            out['soft/polished'] = polished
        u, s = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        nonempty, kkt = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
        accepted = kkt < KKT_TOL
        out[f'{mode}/u'], out[f'{mode}/s'], out[f'{mode}/nonempty'], out[f'{mode}/accepted'] = u, s, nonempty, accepted
        print(f'{mode}: accepted {int(accepted.sum())} / {N_STATES} ({int(polished.sum())} by the active-set enumeration), worst accepted KKT residual {kkt[accepted].max():.2e}, empty feasible set '
              f'{int((~nonempty).sum())}')
        assert accepted.mean() >= 0.99

    # ---- the recorded trajectory and what learn() pushes for it, through the reference's CBFBuffer (second push wraps around)
    obs, _ = env.reset(seed=7)
    trng = np.random.default_rng(5)
    obs_after, inputs = [], []
    for _ in range(TRAJ_STEPS):
        u_in = trng.uniform(lo, hi, size=1)
        obs, _, _, _ = env.step(u_in)
        obs_after.append(np.asarray(obs, dtype=np.float64)[:4].copy())
        inputs.append(u_in.copy())
    obs_after, inputs = np.asarray(obs_after), np.asarray(inputs)
    pushed = pushed_by_the_reference(holder.cbf, lie, obs_after, inputs, env.CTRL_FREQ)
    buf = CBFBuffer(env.observation_space, env.action_space, BUFFER_SIZE, 'cpu', BATCH_ROWS)
    buf.push(pushed)
    out['traj/pos1'], out['traj/size1'] = np.array(buf.pos), np.array(buf.buffer_size)
    buf.push(pushed)
    out['traj/obs_after'], out['traj/inputs'], out['traj/ctrl_freq'] = obs_after, inputs.reshape(-1), np.array(float(env.CTRL_FREQ))
    for k, v in pushed.items():
        out['traj/pushed/' + k] = np.asarray(v, dtype=np.float64)
    bs = buf.state_dict()
    out['traj/pos2'], out['traj/size2'] = np.array(bs['pos']), np.array(bs['buffer_size'])
    for k in ('state', 'act', 'barrier_dot', 'barrier_dot_approx'):
        out['traj/buffer/' + k] = np.asarray(bs[k])

    # ---- loss and three updates on a 64-row batch (the reference's compute_loss / update, Adam at the YAML's learning rate)
    brng = np.random.default_rng(11)
    idx = brng.choice(N_STATES, BATCH_ROWS, replace=False)
    batch = {'state': states[idx], 'act': brng.uniform(lo, hi, size=(BATCH_ROWS, 1)).astype(np.float32),
             'barrier_dot': brng.normal(0.0, 2.0, size=(BATCH_ROWS, 1)).astype(np.float32),
             'barrier_dot_approx': brng.normal(0.0, 2.0, size=(BATCH_ROWS, 1)).astype(np.float32)}
    tb = {k: torch.as_tensor(v) for k, v in batch.items()}
    hold.opt = torch.optim.Adam(mlp.parameters(), c['learning_rate'])
    out['train/loss'] = np.array(float(hold.compute_loss(tb).detach()))
    for _ in range(N_UPDATES):
        hold.update(tb)
    out['train/loss_after'] = np.array(float(hold.compute_loss(tb).detach()))
    for k, v in batch.items():
        out['train/batch/' + k] = v
    after = {k: mlp.state_dict()[k].detach().numpy().copy() for k in NM.KEYS}
    for k, v in after.items():
        if k == 'fcs.1.weight':
            out['train/after/' + k + '/rows'] = v[::W2_ROW_STRIDE]
            out['train/after/' + k + '/sums'] = np.array([v.astype(np.float64).sum(), (v.astype(np.float64) ** 2).sum()])
        else:
            out['train/after/' + k] = v
    path = os.path.join(HERE, 'cbf_nn.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < 778012
    settings = {'task': 'cartpole', 'task_config': task_cfg, 'safety_filter': sf['safety_filter'], 'sf_config': sf['sf_config'],
                'sf_defaults': sf_defaults, 'algo_config': {k: algo['algo_config'][k] for k in ('hidden_dim', 'activation')},
                'n_states': N_STATES, 'kkt_tol': KKT_TOL, 'torch_seed': TORCH_SEED, 'w3_scale': W3_SCALE, 'b3_scale': B3_SCALE,
                'traj_steps': TRAJ_STEPS, 'batch_rows': BATCH_ROWS, 'n_updates': N_UPDATES, 'w2_row_stride': W2_ROW_STRIDE,
                'buffer_size': BUFFER_SIZE}
    with open(os.path.join(HERE, 'cbf_nn_settings.json'), 'w') as f:
        json.dump(settings, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
