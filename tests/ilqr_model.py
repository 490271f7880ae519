"""Float64 NumPy restatement of iLQR's backward pass and of its accept / reject bookkeeping (include/scg_ilqr.h states the equations;
controllers/lqr/ilqr.py:117-278 of the reference is what they restate).  A test model, not product code: tests/test_ilqr_cpu.py holds
it against the reference-generated fixture, tests/test_gpu_ilqr.py holds the kernels against it where the fixture has no case."""
import numpy as np

EPS_F64 = 1e-6              # the central-difference step of the float64 kernel (HipVecEnv.prior_model's default)
EPS_F32 = 1e-3              # ... and of the float32 kernel


def jacobians(f, x, u, eps, dtype=np.float64):
    """Central differences of f at (x, u), step eps, scaled as the kernel does: (f(+) - f(-)) * (0.5 / eps).  With dtype float32 every
    operand and every result of f is rounded to float32 (f itself is evaluated in float64 and rounded: the kernel's f is float32
    throughout, so this is a lower estimate of its rounding)."""
    nx, nu = len(x), len(u)
    A, B = np.zeros((nx, nx), dtype=dtype), np.zeros((nx, nu), dtype=dtype)
    eps = dtype(eps)
    inv2 = dtype(0.5) / eps
    ff = lambda a, b: np.asarray(f(a, b)).astype(dtype)        # noqa: E731
    for c in range(nx):
        d = np.zeros(nx, dtype=dtype); d[c] = eps
        A[:, c] = (ff(x + d, u) - ff(x - d, u)) * inv2
    for c in range(nu):
        d = np.zeros(nu, dtype=dtype); d[c] = eps
        B[:, c] = (ff(x, u + d) - ff(x, u - d)) * inv2
    return A, B


def sym2_inverse(H, lamb):
    """Closed form for a symmetric 2 x 2 H: V diag(1 / (max(l, 0) + lamb)) V'.  Works in H's dtype."""
    t = H.dtype.type
    a, b, d = H[0, 0], H[0, 1], H[1, 1]
    mean, diff = t(0.5) * (a + d), t(0.5) * (a - d)
    rad = np.sqrt(diff * diff + b * b)
    l1, l2 = mean + rad, mean - rad
    px, py = (diff + rad, b) if diff >= 0 else (b, rad - diff)
    nrm = np.sqrt(px * px + py * py)
    vx, vy = (px / nrm, py / nrm) if nrm > 0 else (t(1), t(0))
    i1, i2 = t(1) / (max(l1, t(0)) + t(lamb)), t(1) / (max(l2, t(0)) + t(lamb))
    return np.array([[vx * vx * i1 + vy * vy * i2, vx * vy * (i1 - i2)], [vx * vy * (i1 - i2), vy * vy * i1 + vx * vx * i2]], dtype=H.dtype)


def regularised_inverse(H, lamb, eig='closed'):
    t = H.dtype.type
    if eig == 'numpy' or H.shape[0] > 2:
        ev, evec = np.linalg.eig(H)
        ev = np.where(ev < 0, t(0), ev) + t(lamb)
        return (evec @ np.diag(t(1) / ev) @ evec.T).astype(H.dtype)
    if H.shape[0] == 1:
        return np.array([[t(1) / (max(H[0, 0], t(0)) + t(lamb))]], dtype=H.dtype)
    return sym2_inverse(H, lamb)


def backward(f, xs, us, n, lamb, goal, tracking, Q, R, u_eq, dt, gains, ff, eps=None, eig='closed', dtype=np.float64, trace=None):
    """xs [>= n + 1, nx] (row n = the final observation), us [>= n, nu]; goal [rows, nx]; gains [T, nu, nx] and ff [T, nu] are updated in
    place for k < n.  Returns unstable (bool).  dtype float32: the whole recursion in float32 with the float32 kernel's step.
    trace (a list): receives the smallest eigenvalue of the symmetrised H of every step, before the clip."""
    if eps is None:
        eps = EPS_F64 if dtype == np.float64 else EPS_F32
    c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)      # noqa: E731
    goal, xs, us, Q, R, u_eq, dt = c(np.atleast_2d(goal)), c(xs), c(us), c(Q), c(R), c(u_eq), dtype(dt)
    nx = xs.shape[1]
    eye = np.eye(nx, dtype=dtype)
    Sv = Q @ (xs[n] - (goal[-1] if tracking else goal[0]))
    Sm = Q.copy()
    unstable = False
    for k in reversed(range(n)):
        x, u = xs[k], us[k]
        Ac, Bc = jacobians(f, x, u, eps, dtype)
        Ad, Bd = eye + Ac * dt, Bc * dt
        xr = goal[min(k, goal.shape[0] - 1)] if tracking else goal[0]
        Qv, Rv = Q @ (x - xr), R @ (u - u_eq)
        g = Rv + Bd.T @ Sv
        G = Bd.T @ (Sm @ Ad)
        H = R + Bd.T @ (Sm @ Bd)
        if not np.isfinite(np.sum(H)):
            unstable = True
            continue
        H = dtype(0.5) * (H + H.T)
        if trace is not None:
            trace.append(float(np.linalg.eigvalsh(H.astype(np.float64)).min()))
        Hi = regularised_inverse(H, lamb, eig)
        duff, K = -Hi @ g, -Hi @ G
        gains[k] = K
        ff[k] = u + duff - K @ x
        Sm = Q + Ad.T @ (Sm @ Ad) + K.T @ (H @ K) + K.T @ G + G.T @ K
        Sv = Qv + Ad.T @ Sv + K.T @ (H @ duff) + K.T @ g + G.T @ duff
        assert Sm.dtype == dtype and Sv.dtype == dtype
    return unstable


class Bookkeeping:
    """ilqr.py:117-181 for one env, one call per iteration; `step` returns the branch taken and whether the backward pass runs."""
    INIT, ACCEPT, REJECT, CONVERGED, OOB = 'init', 'accept', 'reject', 'converged', 'oob'

    def __init__(self, lamb_factor, lamb_max, epsilon):
        self.lamb_factor, self.lamb_max, self.epsilon = lamb_factor, lamb_max, epsilon
        self.lamb, self.prev_cost, self.improved, self.best_iteration, self.it, self.finished = 1.0, -np.inf, False, None, 0, False

    def step(self, cost, out_of_bounds, unstable):
        it = self.it
        self.it += 1
        if it == 0:
            if out_of_bounds:
                self.finished = True
                return self.OOB, False
            self.best_iteration, self.prev_cost, self.improved = 0, cost, False
            return self.INIT, True
        delta = cost - self.prev_cost
        if delta > 0.0 or unstable:
            self.lamb = min(self.lamb * self.lamb_factor, self.lamb_max)
            self.improved = False
            return self.REJECT, False
        self.best_iteration, self.prev_cost = it, cost
        if abs(delta) < self.epsilon and self.improved:
            self.finished = True
            return self.CONVERGED, False
        self.improved = True
        return self.ACCEPT, True
