"""Rauch-Tung-Striebel smoothing of a recorded track.

The tracker is a filter: frame k's state uses the frames up to k.  Every workflow here is offline (a recorded video in,
the states of all frames out), so each frame's estimate may as well use the frames after it too.  The smoother records,
after every ``kf.compute()``, what the update kept on the device -- the posterior covariance P_k, the prior mean m_k the
update started from -- and the posterior mean x_k; ``run()`` then goes backward over the record on the device
(hm_smooth_* in include/hydra_mi.h, csrc/smooth_kernels.h):

    G_k  = P_k F_k^T Pp_{k+1}^-1,   Pp_{k+1} = F_k P_k F_k^T + Weps (recomputed, the forward prediction's bits;
                                    G_k through the Cholesky factor of Pp_{k+1}, its inverse is never formed)
    xs_k = x_k + G_k (xs_{k+1} - m_{k+1})
    Ps_k = P_k + G_k (Ps_{k+1} - Pp_{k+1}) G_k^T      (covariances=True)

    with RTSSmoother(kf, capacity=len(frames)) as sm:
        for each frame: kf.compute(...); sm.record()
        xs, var = sm.run()          # K x 4N each; var = diag(Ps_k)
        Ps3 = sm.cov(3)

FlowEKFPipeline.run(smoother=sm) records after every step.
"""
import ctypes

import numpy as np

from . import _lib

WORK_MATRICES = 7          # the backward step's n x n work matrices (hm_smooth_create)


def record_bytes(n_vertices, capacity):
    """Device memory of a smoother: per frame one 4N x 4N slot and four 4N vectors, plus the work matrices."""
    n4 = 4 * int(n_vertices)
    return int(capacity) * (n4 * n4 + 4 * n4) * 8 + WORK_MATRICES * n4 * n4 * 8


def check_budget(n_vertices, capacity, max_bytes):
    """ValueError when a record of `capacity` frames of a mesh of `n_vertices` would need more than max_bytes."""
    need = record_bytes(n_vertices, capacity)
    if need > max_bytes:
        raise ValueError("RTSSmoother: a record of %d frames at %d vertices needs %d bytes of device memory "
                         "(%.2f MB per frame), more than max_bytes = %d" %
                         (int(capacity), int(n_vertices), need, 8.0 * (4 * n_vertices) ** 2 / 1e6, int(max_bytes)))
    return need


def _model(kf):
    """(bars, l0, kappa, a, s, eps_F) of the filter's prediction, as its predict() hands them to the device."""
    st = kf.state
    if hasattr(kf, "_bars") and hasattr(kf, "kappa"):          # IteratedMSKalmanFilter
        bars = np.ascontiguousarray(kf._bars, np.int32).reshape(-1, 2)
        l0 = np.ascontiguousarray(np.asarray(st.l0, np.float64)[:, 0])
        return bars, l0, float(kf.kappa), float(kf.deltat), float(kf.deltat / kf.M), float(st.eps_F)
    # the constant-velocity model of KalmanFilter.predict: F = [[I, I], [0, I]]
    return np.zeros((0, 2), np.int32), np.zeros(0), 0.0, 1.0, 0.0, float(st.eps_F)


class RTSSmoother:
    """The record and the backward pass of one filter (KalmanFilter, IteratedKalmanFilter, IteratedMSKalmanFilter).

    capacity: frames the record holds; covariances: run() also forms every Ps_k (var, cov(k)) -- otherwise the means
    only, with matrix-vector products; max_bytes: the device memory the record may take (ValueError beyond it)."""

    def __init__(self, kf, capacity, covariances=True, max_bytes=8 << 30):
        self._h = None
        self.N = int(kf.N)
        self.capacity = int(capacity)
        if self.capacity < 2:
            raise ValueError("RTSSmoother: capacity %d: a record needs at least 2 frames" % self.capacity)
        self.bytes = check_budget(self.N, self.capacity, max_bytes)
        self.covariances = bool(covariances)
        self.kf = kf
        self._model = _model(kf)
        bars, l0, kappa, a, s, eps_F = self._model
        r = kf.state.renderer
        h = _lib.c_vp()
        _lib.check(_lib.lib().hm_smooth_create(r._h, self.capacity, int(bars.shape[0]), _lib.ptr(bars), _lib.ptr(l0),
                                               kappa, a, s, eps_F, ctypes.byref(h)), "hm_smooth_create")
        self._h = h
        self._renderer = r
        self._smoothed = False
        _lib.register(self, 1)

    # -- lifetime -------------------------------------------------------------------------------------
    def close(self):
        if self._h is not None:
            _lib.lib().hm_smooth_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self, who):
        if self._h is None:
            raise RuntimeError("RTSSmoother.%s: the smoother is closed" % who)
        if self._renderer._h is None:
            raise RuntimeError("RTSSmoother.%s: the filter it records has been closed" % who)
        return self._h

    # -- the record -----------------------------------------------------------------------------------
    def __len__(self):
        if self._h is None:
            return 0
        k = ctypes.c_int32()
        _lib.check(_lib.lib().hm_smooth_count(self._h, ctypes.byref(k), None), "hm_smooth_count")
        return k.value

    def _check_model(self):
        now = _model(self.kf)
        same = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(now, self._model))
        if not same or self.kf.state.renderer is not self._renderer:
            raise RuntimeError("RTSSmoother.record: the filter's springs or parameters changed since the smoother was "
                               "created (one record holds one model)")

    def record(self, X=None):
        """After kf.compute(): frame k's posterior covariance and prior mean (on the device) and its state X (default:
        the filter's).  RuntimeError when the record is full; the record stays as it was."""
        h = self._handle("record")
        self._check_model()
        x = np.ascontiguousarray(np.asarray(self.kf.state.X if X is None else X, np.float64).reshape(-1))
        if x.shape[0] != 4 * self.N:
            raise ValueError("RTSSmoother.record: state of %d entries for %d vertices" % (x.shape[0], self.N))
        _lib.check(_lib.lib().hm_smooth_record(h, _lib.ptr(x)), "hm_smooth_record")

    # -- the backward pass ----------------------------------------------------------------------------
    def run(self, covariances=None):
        """-> (xs, var): xs (K x 4N) the smoothed means, var (K x 4N) the diagonals of Ps_k or None (covariances off).
        With covariances the record is consumed: cov(k) then gives Ps_k, and nothing more can be recorded."""
        h = self._handle("run")
        want = self.covariances if covariances is None else bool(covariances)
        K = len(self)
        xs = np.empty((K, 4 * self.N))
        var = np.empty((K, 4 * self.N)) if want else None
        rc = _lib.lib().hm_smooth_run(h, 1 if want else 0, _lib.ptr(xs), _lib.ptr(var))
        if want:
            self._smoothed = True
        if rc == _lib.HM_ERR_NUMERIC:
            raise FloatingPointError(_lib.lib().hm_last_error().decode())
        _lib.check(rc, "hm_smooth_run")
        return xs, var

    def cov(self, k):
        """Slot k: the smoothed covariance Ps_k after run() with covariances (before it: the filtered P_k)."""
        return self.fetch(k)[0]

    def fetch(self, k):
        """-> (slot k (4N x 4N), x_k, m_k) as recorded (the slot holds Ps_k after a run with covariances)."""
        h = self._handle("fetch")
        n4 = 4 * self.N
        P, x, m = np.empty((n4, n4)), np.empty(n4), np.empty(n4)
        _lib.check(_lib.lib().hm_smooth_fetch(h, int(k), _lib.ptr(P), _lib.ptr(x), _lib.ptr(m)), "hm_smooth_fetch")
        return P, x, m

    def prior(self, k):
        """Pp_k (k >= 1) recomputed from slot k-1 as the backward pass forms it (before a run with covariances)."""
        h = self._handle("prior")
        n4 = 4 * self.N
        Pp = np.empty((n4, n4))
        _lib.check(_lib.lib().hm_smooth_prior(h, int(k), _lib.ptr(Pp)), "hm_smooth_prior")
        return Pp

    def model(self):
        """(bars, l0, kappa, a, s, eps_F) of the record."""
        return self._model


def gemm(which, A, B, C=None, device=0):
    """hm_op_smooth_gemm: the backward step's products on host arrays (tests).  which: "tn" A^T B, "nnd" A (B - C),
    "sym" C + A B^T (lower triangle, mirrored), "ln" tril(A) B, "tl" A^T tril(B) (what lies right of the diagonal of the
    triangular operand is not read)."""
    code = {"tn": 0, "nnd": 1, "sym": 2, "ln": 3, "tl": 4}[which]
    A = np.ascontiguousarray(A, np.float64)
    B = np.ascontiguousarray(B, np.float64)
    C = None if C is None else np.ascontiguousarray(C, np.float64)
    n = A.shape[0]
    for M in (A, B) + (() if C is None else (C,)):
        if M.shape != (n, n):
            raise ValueError("gemm: square n x n operands expected")
    out = np.empty((n, n))
    _lib.check(_lib.lib().hm_op_smooth_gemm(int(device), code, n, _lib.ptr(A), _lib.ptr(B), _lib.ptr(C), _lib.ptr(out)),
               "hm_op_smooth_gemm")
    return out
