"""NumPy restatement of the reference's cbf_nn safety filter (safety_filters/cbf/cbf_nn.py), built on tests/cbf_model.py: the residual
network's forward pass, the QP's closed-form minimiser with the learned row (k' = k + b_nn, b' = b + a_nn), the loss, and the arrays
learn() pushes.  `dtype` selects the arithmetic (float64: the yardstick; float32: the CPU measurement of what single precision costs,
which sets the kernels' tolerance).  tests/test_cbf_nn_cpu.py pins this file to the reference-generated fixture."""
import numpy as np

from tests import cbf_model as M

KEYS = ('fcs.0.weight', 'fcs.0.bias', 'fcs.1.weight', 'fcs.1.bias', 'fcs.2.weight', 'fcs.2.bias')


def forward(weights, X, dtype=np.float64, with_magnitude=False):
    """a_b [n, 2] = MLP(4 -> 256 -> 256 -> 2)(X), relu on both hidden layers; weights: the six tensors in KEYS' order (torch layout).
    with_magnitude: also S [n, 2] = |b3| + sum |W3| |h2|, the magnitude of the output layer's dot-product terms."""
    W1, b1, W2, b2, W3, b3 = (np.asarray(w, dtype=dtype) for w in weights)
    x = np.asarray(X, dtype=dtype).reshape(-1, 4)
    h1 = np.maximum(x @ W1.T + b1, dtype(0))
    h2 = np.maximum(h1 @ W2.T + b2, dtype(0))
    out = h2 @ W3.T + b3
    if with_magnitude:
        return out, np.abs(h2) @ np.abs(W3).T + np.abs(b3)
    return out


def certify(X, u, ab, limits, prior, slope, slack_weight, slack_tolerance, lo, hi, soft=True, dtype=np.float64):
    """cbf_model.certify with the learned row: dict(u0, u, s, feasible, r0, k, b) — k, b the row's k' and b'."""
    h, a, b = M.barrier_terms(X, limits, prior, dtype)
    ab = np.asarray(ab, dtype=dtype).reshape(-1, 2)
    u = np.asarray(u, dtype=dtype).reshape(-1)
    slope, w, tol, lo, hi = dtype(slope), dtype(slack_weight), dtype(slack_tolerance), dtype(lo), dtype(hi)
    k = (slope * h + a) + ab[:, 1]
    b = b + ab[:, 0]
    u0 = np.clip(u, lo, hi)
    r0 = -k - b * u0
    ok = r0 <= 0
    with np.errstate(divide='ignore', invalid='ignore'):
        if soft:
            wb2 = dtype(2.0) * w * b
            u1 = np.clip((u0 - wb2 * k) / (dtype(1.0) + wb2 * b), lo, hi)
            us = np.where(ok, u0, u1)
            s = np.where(ok, dtype(0.0), np.maximum(dtype(0.0), -k - b * us))
            feasible = s <= tol
        else:
            ub = -k / b
            inside = (b != 0) & (ub >= lo) & (ub <= hi)
            us = np.where(ok | ~inside, u0, ub)
            s = np.zeros_like(u0)
            feasible = ok | inside
    return {'u0': u0, 'u': us.astype(dtype), 's': s.astype(dtype), 'feasible': feasible, 'r0': r0, 'k': k, 'b': b}


def sensitivity(r, slack_weight, lo, hi, soft=True):
    """First-order effect of an error (dk, db) of the row on the float64 minimiser `r` (certify's dict): the absolute values of
    (du/dk, du/db, ds/dk, ds/db).  u* does not depend on the row where r0 <= 0 or where the result is clipped; s* = -k - b u* where
    positive, so ds/dk = -1 - b du/dk and ds/db = -u* - b du/db (signed: in the unclipped soft case they shrink to -1 / (1 + 2 w b^2)
    and its companion, which is why s* is far better conditioned than -k - b u* term by term)."""
    k, b, u0, u = r['k'], r['b'], r['u0'], r['u']
    w = float(slack_weight)
    corrected = r['r0'] > 0
    free = corrected & (u > lo) & (u < hi)
    with np.errstate(divide='ignore', invalid='ignore'):
        if soft:
            den = 1.0 + 2.0 * w * b * b
            du_dk = -2.0 * w * b / den
            du_db = (-2.0 * w * k * den - (u0 - 2.0 * w * b * k) * 4.0 * w * b) / (den * den)
        else:
            du_dk = -1.0 / b
            du_db = k / (b * b)
    du_dk, du_db = np.where(free, du_dk, 0.0), np.where(free, du_db, 0.0)
    positive = corrected & (r['s'] > 0)
    ds_dk = np.where(positive, -1.0 - b * du_dk, 0.0)
    ds_db = np.where(positive, -u - b * du_db, 0.0)
    return np.abs(du_dk), np.abs(du_db), np.abs(ds_dk), np.abs(ds_db)


def loss(weights, state, act, barrier_dot, barrier_dot_approx, dtype=np.float64):
    """cbf_nn.py:227-251 with upstream's column reading a = a_b[:, 0], b = a_b[:, 1]."""
    a_b = forward(weights, state, dtype)
    est = np.asarray(barrier_dot, dtype=dtype).reshape(-1) + a_b[:, 0] * np.asarray(act, dtype=dtype).reshape(-1) + a_b[:, 1]
    return float(((est - np.asarray(barrier_dot_approx, dtype=dtype).reshape(-1)) ** 2).mean())


def pushed_arrays(states, inputs, limits, prior, ctrl_freq):
    """The four arrays cbf_nn.py:357-380 push for one env's trace, float64: states [K, 4] the state AFTER each step, inputs [K] the
    input that produced it.  h and LfV are the prior model's; the first and the last step are dropped."""
    states = np.asarray(states, dtype=np.float64).reshape(-1, 4)
    inputs = np.asarray(inputs, dtype=np.float64).reshape(-1)
    h, a, b = M.barrier_terms(states, limits, prior)
    lie = a + b * inputs
    approx = (h[2:] - h[:-2]) / (2 * 1 / ctrl_freq)
    return {'state': states[1:-1], 'act': inputs[1:-1, None], 'barrier_dot': lie[1:-1, None], 'barrier_dot_approx': approx[:, None]}
