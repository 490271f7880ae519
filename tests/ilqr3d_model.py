"""tests/ilqr_model.py's backward pass with the regularised inverse pluggable, for the four-input Hessian of Quadrotor 3D
(include/scg_ilqr_wide.h).  Two inverses: `eigh` (np.linalg.eigh: orthonormal eigenvectors whatever the eigenvalues) and `jacobi`, a
NumPy restatement of the kernel's cyclic Jacobi eigen-solve (csrc/scg_ilqr_wide.h: sym4_jacobi_inverse), rotation for rotation.
`eig` is upstream's np.linalg.eig path (ilqr.py:254-257), kept to measure what it does on a repeated eigenvalue.  A test model, not
product code."""
import numpy as np

from tests.ilqr_model import EPS_F32, EPS_F64, jacobians

JACOBI_SWEEPS = 8            # SCG_ILQR_JACOBI_SWEEPS (include/scg_ilqr_wide.h)


def jacobi_eig(H, sweeps=JACOBI_SWEEPS):
    """Eigenvalues and eigenvectors (columns) of a symmetric H by cyclic Jacobi in H's dtype: a fixed number of sweeps over
    (0,1) (0,2) .. (n-2,n-1), a rotation skipped where its off-diagonal element is exactly 0."""
    t = H.dtype.type
    n = H.shape[0]
    A, V = H.copy(), np.eye(n, dtype=H.dtype)
    with np.errstate(over='ignore'):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[p, q]
                    if apq == 0:
                        continue
                    theta = (A[q, q] - A[p, p]) / (t(2) * apq)
                    tt = t(1) / (abs(theta) + np.sqrt(theta * theta + t(1)))
                    tn = -tt if theta < 0 else tt
                    cs = t(1) / np.sqrt(tn * tn + t(1))
                    sn = tn * cs
                    A[p, p] -= tn * apq
                    A[q, q] += tn * apq
                    A[p, q] = A[q, p] = t(0)
                    for k in range(n):
                        if k != p and k != q:
                            akp, akq = A[k, p], A[k, q]
                            A[k, p] = A[p, k] = cs * akp - sn * akq
                            A[k, q] = A[q, k] = sn * akp + cs * akq
                    for k in range(n):
                        vkp, vkq = V[k, p], V[k, q]
                        V[k, p] = cs * vkp - sn * vkq
                        V[k, q] = sn * vkp + cs * vkq
    return np.diag(A).copy(), V


def inverse_jacobi(H, lamb):
    t = H.dtype.type
    ev, V = jacobi_eig(H)
    il = t(1) / (np.where(ev < 0, t(0), ev) + t(lamb))
    return ((V * il) @ V.T).astype(H.dtype)


def inverse_eigh(H, lamb):
    t = H.dtype.type
    ev, V = np.linalg.eigh(H)
    il = t(1) / (np.where(ev < 0, t(0), ev) + t(lamb))
    return ((V * il) @ V.T).astype(H.dtype)


def inverse_eig(H, lamb):
    """ilqr.py:254-257: the NON-symmetric solver's eigenvectors, used as if they were orthonormal."""
    t = H.dtype.type
    ev, V = np.linalg.eig(H)
    ev = np.where(ev < 0, t(0), ev) + t(lamb)
    return (V @ np.diag(t(1) / ev) @ V.T).astype(H.dtype)


def eig_defect(H):
    """max |V'V - I| of np.linalg.eig's eigenvectors: 0 (to rounding) when they are orthonormal."""
    _, V = np.linalg.eig(H)
    return float(np.abs(V.T @ V - np.eye(H.shape[0])).max())


INVERSES = {'eigh': inverse_eigh, 'jacobi': inverse_jacobi, 'eig': inverse_eig}


def backward(f, xs, us, n, lamb, goal, tracking, Q, R, u_eq, dt, gains, ff, inverse='jacobi', eps=None, dtype=np.float64, hessians=None):
    """ilqr_model.backward with `inverse` (a key of INVERSES or a callable (H, lamb) -> Hinv).  hessians (a list): receives the
    symmetrised H of every step."""
    inv = INVERSES[inverse] if isinstance(inverse, str) else inverse
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
        if hessians is not None:
            hessians.append(H.copy())
        Hi = inv(H, lamb)
        duff, K = -Hi @ g, -Hi @ G
        gains[k] = K
        ff[k] = u + duff - K @ x
        Sm = Q + Ad.T @ (Sm @ Ad) + K.T @ (H @ K) + K.T @ G + G.T @ K
        Sv = Qv + Ad.T @ Sv + K.T @ (H @ duff) + K.T @ g + G.T @ duff
        assert Sm.dtype == dtype and Sv.dtype == dtype
    return unstable


def deviation(K, ff, Kr, fr):
    """The fixture's figure: max relative deviation of K / ff from a reference pair."""
    return float(max(np.abs(K - Kr).max() / np.abs(Kr).max(), np.abs(ff - fr).max() / np.abs(fr).max()))
