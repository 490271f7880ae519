"""Float64 restatement of the reference's CBF-QP safety filter (safety_filters/cbf/cbf.py, cbf_utils.cbf_cartpole, the cartpole prior
model of envs/gym_control/cartpole.py:409-414) and of its closed-form minimiser: what the HIP kernels are compared against.  NumPy
only, vectorised over rows; `dtype` selects the arithmetic (float64: the yardstick; float32: the CPU measurement of what single
precision costs, which sets the kernels' tolerance).  tests/test_cbf_cpu.py pins this file to the reference-generated fixture."""
import numpy as np


def barrier_terms(X, limits, prior, dtype=np.float64):
    """(h, a, b): the barrier, LfV(X, 0) and LfV(X, 1) - LfV(X, 0); prior = (l, m, M, g)."""
    X = np.asarray(X, dtype=dtype).reshape(-1, 4)
    L = np.asarray(limits, dtype=dtype)
    l, m, M, g = (dtype(v) for v in prior)
    one, two = dtype(1.0), dtype(2.0)
    q = X / L
    h = one - (q * q).sum(axis=1, dtype=dtype)
    gr = -two * X / (L * L)
    sn, cs = np.sin(X[:, 2]), np.cos(X[:, 2])
    Mm, ml = m + M, m * l
    tmp0 = ml * X[:, 3] * X[:, 3] * sn / Mm
    den = l * (dtype(4.0) / dtype(3.0) - m * cs * cs / Mm)
    thdd0 = (g * sn - cs * tmp0) / den
    xdd0 = tmp0 - ml * thdd0 * cs / Mm
    dtmp = one / Mm
    dthdd = -cs * dtmp / den
    dxdd = dtmp - ml * dthdd * cs / Mm
    a = gr[:, 0] * X[:, 1] + gr[:, 1] * xdd0 + gr[:, 2] * X[:, 3] + gr[:, 3] * thdd0
    b = gr[:, 1] * dxdd + gr[:, 3] * dthdd
    return h, a, b


def certify(X, u, limits, prior, slope, slack_weight, slack_tolerance, lo, hi, soft=True, dtype=np.float64):
    """The CBF-QP's minimiser per row: dict(u0, u, s, feasible, r0) — u0 the clipped action, r0 = r(u0) the slack the barrier row needs
    at u0.  Hard-constrained rows whose feasible set is empty return u0 with feasible False."""
    h, a, b = barrier_terms(X, limits, prior, dtype)
    u = np.asarray(u, dtype=dtype).reshape(-1)
    slope, w, tol, lo, hi = dtype(slope), dtype(slack_weight), dtype(slack_tolerance), dtype(lo), dtype(hi)
    k = slope * h + a
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
    return {'u0': u0, 'u': us.astype(dtype), 's': s.astype(dtype), 'feasible': feasible, 'r0': r0}
