"""The filters' algebra on the host, for a caller-supplied measurement object.

The filters of kalman.py take their steps through the verbs of renderer.Renderer (``cov_predict``,
``project_mask``, ``update_begin`` / ``update_step`` / ``step_error`` / ``update_cov``).  A caller may hand the
constructors its own measurement object instead (``renderer=``; the CPU tests of the host logic do, with the oracle
behind it).  Such an object offers ``measure`` and ``error`` only; ``HostAlgebra`` wraps it and gives the filters the
same verbs in NumPy / SciPy, with the signatures and return shapes of the native ones.
"""
import contextlib
import os
import time

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

# A default-sized BLAS thread team on a many-core host with a small CPU quota (a container, the GPU box) is slower than
# a handful of threads by orders of magnitude, so the team is capped (HYDRA_MI_BLAS_THREADS overrides the cap).
try:
    from threadpoolctl import ThreadpoolController as _ThreadpoolController
except ImportError:                                   # pragma: no cover
    _ThreadpoolController = None
_BLAS_THREADS = int(os.environ.get("HYDRA_MI_BLAS_THREADS", "8"))


_controller = []


def _blas_cap():
    """Cap the BLAS / OpenMP pools for the host algebra of one filter step.  The pools are looked up
    once (threadpoolctl scans the loaded libraries, ~0.5 ms)."""
    if _ThreadpoolController is None:
        return contextlib.nullcontext()
    if not _controller:
        _controller.append(_ThreadpoolController())
    return _controller[0].limit(limits=_BLAS_THREADS)


def _spd_solve(A, b):
    """A x = b through the Cholesky factor of the information matrix, or an LU factor if it is not positive definite
    (the finite-difference HTH is symmetric but only approximately positive semi-definite)."""
    try:
        return sla.cho_solve(sla.cho_factor(A, lower=True, check_finite=False), b, check_finite=False)
    except np.linalg.LinAlgError:
        return sla.lu_solve(sla.lu_factor(A, check_finite=False), b, check_finite=False)


def _spd_inverse(A):
    """inv(A) for a symmetric matrix: through the Cholesky factor when A is positive definite."""
    try:
        c, info = sla.lapack.dpotrf(A, lower=1, clean=0, overwrite_a=0)
        if info == 0:
            inv, info = sla.lapack.dpotri(c, lower=1, overwrite_c=1)
            if info == 0:
                low = np.tril(inv)
                return low + np.tril(inv, -1).T
    except Exception:
        pass
    return np.linalg.inv(A)


def _spring_jacobian(n2, bars, blocks):
    """d f / d y of the spring force (reference kalman.py:865-902), sparse, from the per-spring blocks.

    The reference forms  -K [diag(kappa (1 - l0/l)) x I2] K^T - K diag(d) [dk x 1_2]  with
    dk_i = kappa l0_i / l_i^3 * d_i^T (K^T)_i and d = K^T y, as dense products.  Bar i between
    vertices a and b contributes the symmetric 2x2 block  B_i = k_i I + c_i d_i d_i^T  (k_i = kappa (1 - l0_i/l_i),
    c_i = kappa l0_i / l_i^3; blocks[i] = (Bxx, Bxy, Byy), IteratedMSKalmanFilter._spring_blocks) with sign - on
    (a,a), (b,b) and + on (a,b), (b,a); assembled here directly from those blocks."""
    if bars is None or len(bars) == 0:
        return sp.csr_matrix((n2, n2))
    bars = np.asarray(bars, np.int64)
    blocks = np.asarray(blocks, np.float64)
    Bm = blocks[:, [0, 1, 1, 2]].reshape(-1, 2, 2)
    vals = np.concatenate((-Bm, -Bm, Bm, Bm)).reshape(-1)
    a, b = bars[:, 0], bars[:, 1]
    al = np.arange(2)
    rows, cols = [], []
    for (p, q) in ((a, a), (b, b), (a, b), (b, a)):
        rows.append((2 * p[:, None, None] + al[None, :, None]) + 0 * al[None, None, :])
        cols.append((2 * q[:, None, None] + al[None, None, :]) + 0 * al[None, :, None])
    return sp.csr_matrix((vals, (np.concatenate(rows).reshape(-1), np.concatenate(cols).reshape(-1))), shape=(n2, n2))


def _fwft(A, a, W):
    """F W F^T for F = [[I, a I], [A, I]] with A sparse (2N x 2N), by blocks."""
    n2 = A.shape[0]
    W11, W12, W21, W22 = W[:n2, :n2], W[:n2, n2:], W[n2:, :n2], W[n2:, n2:]
    P11 = W11 + a * W21
    P12 = W12 + a * W22
    P21 = A.dot(np.ascontiguousarray(W11)) + W21
    P22 = A.dot(np.ascontiguousarray(W12)) + W22
    out = np.empty_like(W)
    out[:n2, :n2] = P11 + a * P12
    out[:n2, n2:] = A.dot(np.ascontiguousarray(P11.T)).T + P12
    out[n2:, :n2] = P21 + a * P22
    out[n2:, n2:] = A.dot(np.ascontiguousarray(P21.T)).T + P22
    return out


def _inside(y_m, p):
    """Per vertex: do the four pixels around it all belong to the mask (then its distance is <= 0)."""
    m = np.asarray(y_m)
    H, W = m.shape
    x0 = np.floor(p[:, 0]).astype(int)
    y0 = np.floor(p[:, 1]).astype(int)
    ok = (x0 >= 0) & (y0 >= 0) & (x0 + 1 < W) & (y0 + 1 < H)
    xs, ys = np.clip(x0, 0, W - 2), np.clip(y0, 0, H - 2)
    return ok & (m[ys, xs] > 0.5) & (m[ys, xs + 1] > 0.5) & (m[ys + 1, xs] > 0.5) & (m[ys + 1, xs + 1] > 0.5)


def _mask_distance(y_m):
    """Signed distance to the object's outline: positive outside the mask, negative inside -- the reference's fd
    (imgproc.py:195-235: -cv2.pointPolygonTest of the contour through the object's border pixels), restated in
    imgproc.outline_distance; what hm_project_mask evaluates on the device."""
    from .imgproc import outline_distance
    return outline_distance(y_m)


class HostAlgebra:
    """The step-wise verbs of renderer.Renderer on the host, around a measurement object with ``measure`` and ``error``."""

    blas_cap = staticmethod(_blas_cap)

    def __init__(self, measurement):
        self.measurement = measurement
        self._W0 = self._invW0 = self._X0 = None
        self._A = self._A_old = None          # information matrices of the last step and of the one before (None: the prior)

    def update_frame(self, y_im, y_flow, y_m):
        """The next observation: handed on to a measurement object that wants to see it."""
        seen = getattr(self.measurement, "update_frame", None)
        if seen is not None:
            seen(y_im, y_flow, y_m)

    def cov_predict(self, W, bars, blocks, a, s, eps_F, fetch=True):
        """F W F^T + Weps for F = [[I, a I], [s A, I]], A the spring Jacobian of `bars` / `blocks` (bars=None: A = 0),
        Weps = eps_F [[I/4, I/2], [I/2, I]] (reference kalman.py:184)."""
        n2 = W.shape[0] // 2
        out = _fwft(_spring_jacobian(n2, bars, blocks) * s, a, W)
        i = np.arange(n2)
        out[i, i] += eps_F / 4
        out[i, n2 + i] += eps_F / 2
        out[n2 + i, i] += eps_F / 2
        out[n2 + i, n2 + i] += eps_F
        return out

    def project_mask(self, X, y_m):
        """KalmanFilter.projectmask (reference kalman.py:724-742) -> (X projected, number of vertices more than 1 px
        outside).  Steps, step size and the stale d / index set follow the reference."""
        if y_m is None:
            raise ValueError("project_mask on the host needs the mask itself")
        X = np.array(X, np.float64)
        n2 = X.shape[0] // 2
        p = X[:n2].reshape(-1, 2)
        near = ~_inside(y_m, p)           # vertices whose four surrounding pixels are not all object
        if not near.any():
            return X, 0                   # d <= 0 everywhere: nothing to project
        fd = _mask_distance(y_m)
        ddeps = 1e-1
        p_orig = p.copy()
        d = np.zeros(len(p))              # surely-inside vertices have d <= 0: never selected below
        d[near] = fd(p[near])
        ix = d > 1
        for _ in range(10):
            if ix.any():
                gx = (fd(p[ix] + [ddeps, 0]) - d[ix]) / ddeps
                gy = (fd(p[ix] + [0, ddeps]) - d[ix]) / ddeps
                g2 = gx ** 2 + gy ** 2
                with np.errstate(divide="ignore", invalid="ignore"):
                    step = np.where(g2 > 0, d[ix] / g2, 0.0)
                p[ix] -= (step * np.vstack((gx, gy))).T
        X[n2:] += (p - p_orig).reshape(X[n2:].shape)
        return X, int(ix.sum())

    def update_begin(self, W_prior, X0):
        """Keep the prior, inv(W) and X0 for the steps that follow."""
        self._W0 = W_prior
        self._invW0 = _spd_inverse(W_prior)
        self._X0 = np.asarray(X0, np.float64).reshape(-1, 1)
        self._A = self._A_old = None

    def update_step(self, state, y_im, y_flow, y_m, want_error=True):
        """Measurement at state.X and the solve -> (step [4N,1], Hz_components [4N,4], None): the new iterate
        X0 + step is not rendered here, step_error does that once the caller has kept it."""
        t0 = time.time()
        Hz, HTH, Hzc = self.measurement.measure(state, y_im, y_flow, y_m)
        state.count_renders(time.time() - t0)
        self._A_old, self._A = self._A, self._invW0 + HTH
        step = _spd_solve(self._A, Hz - HTH.dot(self._X0 - state.X))
        return step, Hzc, None

    def step_error(self, state, y_im, y_flow, y_m):
        """(e_im, e_fx, e_fy, e_m) of the iterate just stepped to (state.X)."""
        return self.measurement.error(state, y_im, y_flow, y_m, want_flow=False)[:4]

    def update_cov(self, which=0, fetch=True):
        """Covariance of the last step (0), of the one before (1) or the prior (-1)."""
        A = {0: self._A, 1: self._A_old, -1: None}[which]
        return self._W0 if A is None else _spd_inverse(A)
