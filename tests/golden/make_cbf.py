#!/usr/bin/env python3
"""Golden vectors of the reference's CBF safety filter (safety_filters/cbf/cbf.py).

    python tests/golden/make_cbf.py            (build container only: needs /root/reference and SciPy)

What is evaluated is the reference's OWN code, on tests/golden/casadi_numeric.py (the expression-graph stand-in for CasADi):
    safety_filters/cbf/cbf_utils.py  cbf_cartpole(X, state_limits)                  -> h
    safety_filters/cbf/cbf.py        CBF.get_lie_derivative (called on a holder of X, u, model, cbf)   -> LfV(X, u)
    envs/gym_control/cartpole.py     _setup_symbolic: the x_dot the Lie derivative is taken along
The stand-in lacks two CasADi calls cbf.py makes, `gradient` and `dot`; both are defined below from its `jacobian`.

The QP minimisers do NOT come from qpOASES: qpOASES (and CasADi's Opti stack that drives it) is not available here.  The reference's
problem (cbf.py:94-147) is      minimise 1/2 (u - u0)^2 + w s^2   s.t.  -slope h - LfV(X, u) <= s,  s >= 0,  lo <= u <= hi     (soft)
                                minimise 1/2 (u - u0)^2           s.t.  -slope h - LfV(X, u) <= 0,          lo <= u <= hi     (hard)
with LfV affine in u.  The soft objective is strictly convex in (u, s), the hard one in u, and the feasible sets are convex, so the
minimiser is UNIQUE: any exact solver returns what the reference's solver returns.  Here a general-purpose solver (SciPy SLSQP,
float64, ftol 1e-16, started from several points) solves each row, and a row enters the fixture only after its KKT residuals —
stationarity, primal feasibility and complementarity (multipliers >= 0 by non-negative least squares), evaluated in the scaled
variable z = sqrt(2 w) s in which the objective is 1/2 |.|^2 — are below 1e-9.  Hard-constrained rows whose feasible set is empty carry the flag only.

Output: tests/golden/cbf.npz (arrays), tests/golden/cbf_settings.json (the example's task and filter settings, the filter's default
YAML, the sampling parameters).  The actor of examples/cbf/models/ppo_model_cartpole.pt is stored as plain arrays.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import ref_stubs  # noqa: E402

ref_stubs.install()

import casadi as cs  # noqa: E402  (the stand-in)

# the two CasADi calls cbf.py makes that the stand-in lacks, from its jacobian
cs.gradient = lambda expr, var: cs.transpose(cs.jacobian(expr, var))      # noqa: E731  column vector of d expr / d var
cs.dot = lambda a, b: cs.mtimes(cs.transpose(a), b)                         # noqa: E731
if 'gymnasium.spaces' in sys.modules and not hasattr(sys.modules['gymnasium.spaces'], 'box'):       # cbf_utils imports the submodule name
    sys.modules['gymnasium.spaces'].box = sys.modules['gymnasium.spaces']

import yaml  # noqa: E402
from safe_control_gym.envs.gym_control.cartpole import CartPole  # noqa: E402
from safe_control_gym.safety_filters.cbf.cbf_utils import cbf_cartpole  # noqa: E402

from tests.golden.make_golden import REF, load_task_config  # noqa: E402

N_STATES = 3000
KKT_TOL = 1e-9
NON_DEFAULT_PRIOR = {'pole_length': 0.62, 'pole_mass': 0.14, 'cart_mass': 1.3}


def reference_lie_derivative():
    """cbf.py's get_lie_derivative, the function object itself (imported lazily: the module pulls in the controller base class)."""
    from safe_control_gym.safety_filters.cbf.cbf import CBF
    return CBF.get_lie_derivative


def kkt_residual(grad_f, grads, values):
    """Largest KKT residual of a point of  min f  s.t.  g_i >= 0:  multipliers m >= 0 by non-negative least squares on
    [grad g_i ...; diag(g_i)] m = [grad f; 0] (stationarity and complementarity together); returned: the largest of the stationarity
    components, the complementarity products m_i g_i and the primal infeasibilities max(0, -g_i).  Dual feasibility holds by construction."""
    from scipy.optimize import nnls
    G = np.asarray(grads, dtype=float).T                    # [n_var, n_con]
    g = np.asarray(values, dtype=float)
    A = np.vstack([G, np.diag(g)])
    rhs = np.concatenate([np.asarray(grad_f, dtype=float), np.zeros(len(g))])
    m, _ = nnls(A, rhs)
    return float(max(np.abs(A @ m - rhs).max(), np.maximum(0.0, -g).max()))


def solve_row(h, a, b, u_raw, slope, w, lo, hi, soft):
    """(u*, s*, feasible set non-empty, largest KKT residual) of one row by SLSQP; LfV(X, u) = a + b u."""
    from scipy.optimize import minimize
    k = slope * h + a
    u0 = min(max(u_raw, lo), hi)
    opts = {'ftol': 1e-16, 'maxiter': 500}
    best = None
    if soft:
        c = np.sqrt(2.0 * w)                         # z = c s: the objective becomes 1/2 (u - u0)^2 + 1/2 z^2
        fun = lambda v: 0.5 * (v[0] - u0) ** 2 + 0.5 * v[1] ** 2            # noqa: E731
        jac = lambda v: np.array([v[0] - u0, v[1]])                        # noqa: E731
        cons = [{'type': 'ineq', 'fun': lambda v: k + b * v[0] + v[1] / c, 'jac': lambda v: np.array([b, 1.0 / c])}]
        for start in ((u0, 0.0), (u0, max(0.0, -k - b * u0) * c), (lo, 0.0), (hi, 0.0), (0.0, 1.0)):
            r = minimize(fun, np.array(start, dtype=float), jac=jac, constraints=cons, bounds=[(lo, hi), (0.0, None)], method='SLSQP',
                         options=opts)
            u, z = float(min(max(r.x[0], lo), hi)), float(max(r.x[1], 0.0))
            res = kkt_residual([u - u0, z], [[b, 1.0 / c], [0.0, 1.0], [1.0, 0.0], [-1.0, 0.0]], [k + b * u + z / c, z, u - lo, hi - u])
            if best is None or res < best[3]:
                best = (u, z / c, True, res)
        for _ in range(3):                           # restart from the best point: SLSQP's own stopping rule leaves ~1e-9
            if best[3] < 0.1 * KKT_TOL:
                break
            r = minimize(fun, np.array([best[0], best[1] * c]), jac=jac, constraints=cons, bounds=[(lo, hi), (0.0, None)], method='SLSQP',
                         options=opts)
            u, z = float(min(max(r.x[0], lo), hi)), float(max(r.x[1], 0.0))
            res = kkt_residual([u - u0, z], [[b, 1.0 / c], [0.0, 1.0], [1.0, 0.0], [-1.0, 0.0]], [k + b * u + z / c, z, u - lo, hi - u])
            if res < best[3]:
                best = (u, z / c, True, res)
        return best
    if max(k + b * lo, k + b * hi) < 0.0:            # hard and no input satisfies the row: the flag only
        return (np.nan, 0.0, False, 0.0)
    fun = lambda v: 0.5 * (v[0] - u0) ** 2                                  # noqa: E731
    jac = lambda v: np.array([v[0] - u0])                                   # noqa: E731
    cons = [{'type': 'ineq', 'fun': lambda v: k + b * v[0], 'jac': lambda v: np.array([b])}]
    for start in (u0, lo, hi, 0.5 * (lo + hi)):
        r = minimize(fun, np.array([start], dtype=float), jac=jac, constraints=cons, bounds=[(lo, hi)], method='SLSQP', options=opts)
        u = float(min(max(r.x[0], lo), hi))
        res = kkt_residual([u - u0], [[b], [1.0], [-1.0]], [k + b * u, u - lo, hi - u])
        if best is None or res < best[3]:
            best = (u, 0.0, True, res)
    return best


def main():
    with open(os.path.join(REF, 'examples/cbf/config_overrides/cbf_config.yaml')) as f:
        sf = yaml.safe_load(f)
    with open(os.path.join(REF, 'safe_control_gym/safety_filters/cbf/cbf.yaml')) as f:
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
    slope, w, tol = sf['sf_config']['slope'], sf['sf_config']['slack_weight'], sf['sf_config']['slack_tolerance']

    rng = np.random.default_rng(20261016)
    states = rng.uniform(-1.1, 1.1, size=(N_STATES, 4)) * np.asarray(limits)
    actions = rng.uniform(-12.0, 12.0, size=N_STATES)
    out = {'states': states, 'actions': actions, 'limits': np.asarray(limits, dtype=np.float64), 'action_bounds': np.array([lo, hi])}
    get_lie = reference_lie_derivative()
    priors = {'default': {}, 'alt': NON_DEFAULT_PRIOR}
    for tag, prior_prop in priors.items():
        env._setup_symbolic(prior_prop=prior_prop)
        model = env.symbolic
        holder = types.SimpleNamespace(X=model.x_sym, u=model.u_sym, model=model, cbf=cbf_cartpole(model.x_sym, limits))
        lie = get_lie(holder)
        h = np.array([float(np.asarray(holder.cbf(X=x)['cbf']).reshape(-1)[0]) for x in states])
        l0 = np.array([float(np.asarray(lie(X=x, u=np.zeros(1))['LfV']).reshape(-1)[0]) for x in states])
        l1 = np.array([float(np.asarray(lie(X=x, u=np.ones(1))['LfV']).reshape(-1)[0]) for x in states])
        out[f'{tag}/h'], out[f'{tag}/LfV0'], out[f'{tag}/LfV1'] = h, l0, l1
        out[f'{tag}/prior'] = np.array([prior_prop.get('pole_length', env.EFFECTIVE_POLE_LENGTH), prior_prop.get('pole_mass', env.POLE_MASS),
                                        prior_prop.get('cart_mass', env.CART_MASS), env.GRAVITY_ACC])          # l, m, M, g
        for mode, soft in (('soft', True), ('hard', False)):
            rows = [solve_row(h[i], l0[i], l1[i] - l0[i], actions[i], slope, w, lo, hi, soft) for i in range(N_STATES)]
            u = np.array([r[0] for r in rows])
            s = np.array([r[1] for r in rows])
            nonempty = np.array([r[2] for r in rows])
            kkt = np.array([r[3] for r in rows])
            accepted = kkt < KKT_TOL
            out[f'{tag}/{mode}/u'], out[f'{tag}/{mode}/s'] = u, s
            out[f'{tag}/{mode}/nonempty'], out[f'{tag}/{mode}/accepted'], out[f'{tag}/{mode}/kkt'] = nonempty, accepted, kkt
            print(f'{tag} {mode}: accepted {int(accepted.sum())} / {N_STATES}, worst accepted KKT residual {kkt[accepted].max():.2e}, '
                  f'empty feasible set {int((~nonempty).sum())}, corrected {int((np.abs(u - np.clip(actions, lo, hi)) > 1e-9).sum())}')

    import torch
    sd = torch.load(os.path.join(REF, 'examples/cbf/models/ppo_model_cartpole.pt'), map_location='cpu', weights_only=False)['agent']['ac']
    for k, v in sd.items():
        if k.startswith('actor.'):
            out['actor/' + k] = v.detach().cpu().numpy()
    np.savez_compressed(os.path.join(HERE, 'cbf.npz'), **out)
    settings = {'task': 'cartpole', 'task_config': task_cfg, 'safety_filter': sf['safety_filter'], 'sf_config': sf['sf_config'],
                'sf_defaults': sf_defaults, 'algo_config': {k: algo['algo_config'][k] for k in ('hidden_dim', 'activation')},
                'non_default_prior_prop': NON_DEFAULT_PRIOR, 'n_states': N_STATES, 'kkt_tol': KKT_TOL}
    with open(os.path.join(HERE, 'cbf_settings.json'), 'w') as f:
        json.dump(settings, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
