"""The two seams of kalman.py on the CPU: the host algebra behind a caller-supplied measurement object
(kalman_host.HostAlgebra) and the owner of the state prediction started ahead (kalman.PredictionAhead, on the worker's
host thread).  The 48 x 48 case of test_host_cpu.py."""
import ctypes
import types

import numpy as np

from oracle import ekf_ref
from test_host_cpu import OracleRenderer, _tiny_case


class Counting(OracleRenderer):
    def __init__(self, *a):
        OracleRenderer.__init__(self, *a)
        self.calls = dict(measure=0, error=0)

    def measure(self, *a, **k):
        self.calls["measure"] += 1
        return OracleRenderer.measure(self, *a, **k)

    def error(self, *a, **k):
        self.calls["error"] += 1
        return OracleRenderer.error(self, *a, **k)


def test_call_counts_on_the_measurement_seam(hm):
    """Per compute(): measure once per iteration, error once per iterate that is kept and once more for the result; an
    iterate that is reverted is never rendered."""
    from hydra_mi import kalman
    video, flow, dm = _tiny_case(hm)
    r = Counting(dm, video[:, :, 0], (1e-3, 1.0, 1.0))
    kf = kalman.IteratedMSKalmanFilter(dm, video[:, :, 0], flow[:, :, :, 0], True, nI=2, renderer=r)
    assert kf.state.renderer is r and kf.state.algebra.measurement is r and not kf.state.native
    for k in (1, 2):
        before = dict(r.calls)
        frame = video[:, :, k]
        kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
        accepted = kf.niter - (1 if kf.reverted else 0)
        assert 1 <= kf.niter <= 2
        assert r.calls["measure"] - before["measure"] == kf.niter
        assert r.calls["error"] - before["error"] == accepted + 1

    class Exploding(Counting):
        def measure(self, state, y_im, y_flow, y_m, deltaX=2.0):
            Hz, HTH, Hzc = Counting.measure(self, state, y_im, y_flow, y_m, deltaX)
            Hz = Hz.copy()
            Hz[0] = 1e9                                   # throws vertex 0 far away
            return Hz, HTH, Hzc

    video, flow, dm = _tiny_case(hm)
    r = Exploding(dm, video[:, :, 0], (1e-3, 1e-3, 1e10))
    kf = kalman.IteratedKalmanFilter(dm, video[:, :, 0], flow[:, :, :, 0], True, renderer=r)
    kf.update(video[:, :, 0], flow[:, :, :, 0], (video[:, :, 0] > 0).astype(np.uint8))
    assert kf.reverted and kf.niter == 1 and r.calls == dict(measure=1, error=0)


def _rel(got, want):
    return np.linalg.norm(got - want) / np.linalg.norm(want)


def test_host_cov_predict_against_the_definition(hm):
    """HostAlgebra.cov_predict is F W F^T + Weps for F = [[I, a I], [s A, I]], A assembled densely here from the same
    per-spring blocks.  The block form and the dense product differ by rounding only: the host path of the commit before
    this module existed (_fwft of a sparse A, plus Weps) gave 3.2e-17 .. 4.6e-17 for the relative difference in the
    Frobenius norm on these inputs (4N = 40, seeds 0 .. 4); the bound is that times nine, for the order of operations."""
    from hydra_mi import kalman
    video, flow, dm = _tiny_case(hm)
    kf = kalman.IteratedMSKalmanFilter(dm, video[:, :, 0], flow[:, :, :, 0], True, nI=2,
                                       renderer=OracleRenderer(dm, video[:, :, 0], (1e-3, 1.0, 1.0)))
    st, alg = kf.state, kf.state.algebra
    N = st.N
    rng = np.random.default_rng(0)
    st.X = st.X + rng.normal(0, 0.3, st.X.shape)
    B = rng.normal(size=(4 * N, 4 * N))
    W = B @ B.T / (4 * N) + 0.1 * np.eye(4 * N)
    blocks = kf._spring_blocks()
    a, s = kf.deltat, kf.deltat / kf.M
    A = np.zeros((2 * N, 2 * N))
    for (i, j), (bxx, bxy, byy) in zip(kf._bars, blocks):
        Bm = np.array([[bxx, bxy], [bxy, byy]])
        A[2 * i:2 * i + 2, 2 * i:2 * i + 2] -= Bm
        A[2 * j:2 * j + 2, 2 * j:2 * j + 2] -= Bm
        A[2 * i:2 * i + 2, 2 * j:2 * j + 2] += Bm
        A[2 * j:2 * j + 2, 2 * i:2 * i + 2] += Bm
    # (the blocks are the spring Jacobian of the reference, restated in the oracle: a rounding or two per entry)
    assert np.abs(A - ekf_ref.ms_dfdy(st.K, st.l0[:, 0], st.X[:2 * N], kf.kappa)).max() < 1e-14 * np.abs(A).max()
    e = np.eye(2 * N)
    F = np.block([[e, a * e], [s * A, e]])
    W_in = W.copy()
    got = alg.cov_predict(W, kf._bars, blocks, a, s, st.eps_F, fetch=False)
    d = _rel(got, F @ W @ F.T + st.Weps)
    print("cov_predict, springs: relative difference %.3g" % d)
    assert d < 4e-16 and np.array_equal(W, W_in)
    # the constant-velocity filter: no springs, a = 1, s = 0
    F1, Weps1, _ = ekf_ref.initial_covariances(N, 0.25)
    d = _rel(alg.cov_predict(W, None, None, 1.0, 0.0, 0.25), F1 @ W @ F1.T + Weps1)
    print("cov_predict, constant velocity: relative difference %.3g" % d)
    assert d < 4e-16


def test_host_update_cov_names_the_step(hm):
    """HostAlgebra.update_cov(which): 0 the last step's covariance inv(inv(W0) + HTH), 1 the one before, -1 the prior --
    the very array that was given in, also before any step.  W0 has eigenvalues in [0.5, 1.5] and the HTH are Gram matrices
    of norm ~ 1, so the systems have condition numbers below 10: inverses agree with numpy's to ~ 40 x 10 x 1e-16."""
    from hydra_mi import kalman_host
    n4 = 40
    rng = np.random.default_rng(3)
    Q = np.linalg.qr(rng.normal(size=(n4, n4)))[0]
    W0 = (Q * rng.uniform(0.5, 1.5, n4)) @ Q.T
    W0 = (W0 + W0.T) / 2
    X0 = rng.normal(size=(n4, 1))
    lin = []

    def measure(state, y_im, y_flow, y_m):
        G = rng.normal(size=(n4, 6)) / np.sqrt(n4)
        lin.append((rng.normal(size=(n4, 1)), G @ G.T, rng.normal(size=(n4, 4))))
        return lin[-1]

    alg = kalman_host.HostAlgebra(types.SimpleNamespace(measure=measure))
    state = types.SimpleNamespace(X=X0.copy(), count_renders=lambda dt: None)
    alg.update_begin(W0, X0)
    assert alg.update_cov(-1) is W0 and alg.update_cov(-1, fetch=False) is W0
    assert alg.update_cov(0) is W0 and alg.update_cov(1) is W0           # no step yet: the prior
    invW0 = np.linalg.inv(W0)
    for k in range(2):
        step, Hzc, err = alg.update_step(state, None, None, None)
        Hz, HTH, Hzc_k = lin[k]
        assert err is None and Hzc is Hzc_k
        assert _rel(step, np.linalg.solve(invW0 + HTH, Hz - HTH @ (X0 - state.X))) < 1e-12
        state.X = X0 + step
    assert alg.update_cov(-1) is W0
    assert _rel(alg.update_cov(0), np.linalg.inv(invW0 + lin[1][1])) < 1e-12
    assert _rel(alg.update_cov(1, fetch=False), np.linalg.inv(invW0 + lin[0][1])) < 1e-12
    assert not np.allclose(alg.update_cov(0), alg.update_cov(1))


def _newton_now(kf):
    """hm_ms_newton, synchronously, from the filter's state, springs and parameters as they are."""
    from hydra_mi import _lib
    st = kf.state
    X = np.ascontiguousarray(st.X.reshape(-1), np.float64).copy()
    bars = np.ascontiguousarray(kf._bars, np.int32)
    l0 = np.ascontiguousarray(st.l0[:, 0], np.float64)
    its = ctypes.c_int()
    _lib.check(_lib.lib().hm_ms_newton(int(st.N), len(bars), _lib.ptr(bars), _lib.ptr(l0), float(kf.kappa), float(kf.M),
                                       float(kf.deltat), int(kf.maxiter), float(kf.tol), _lib.ptr(X), ctypes.byref(its)),
               "hm_ms_newton")
    return X, its.value


def test_prediction_ahead_on_the_host_worker(hm):
    """kalman.PredictionAhead with the worker on its host thread: a job taken from unchanged inputs is hm_ms_newton bit
    for bit; one whose state, springs or parameters changed meanwhile is waited for and dropped; after a failed update
    the worker is drained and usable; close() twice is harmless."""
    from hydra_mi import _lib, kalman
    video, flow, dm = _tiny_case(hm)
    kf = kalman.IteratedMSKalmanFilter(dm, video[:, :, 0], flow[:, :, :, 0], True, nI=2,
                                       renderer=OracleRenderer(dm, video[:, :, 0], (1e-3, 1.0, 1.0)))
    ahead = kf._ahead
    rng = np.random.default_rng(1)
    kf.state.X = kf.state.X + rng.normal(0, 0.3, kf.state.X.shape)

    def taken_equals_synchronous():
        ahead.start()
        assert ahead.matches() and ahead.attached is False
        X, its = ahead.take()
        Xs, its_s = _newton_now(kf)
        assert np.array_equal(X, Xs) and its == its_s and its >= 20 and not np.array_equal(X, kf.state.X.reshape(-1))
        assert not ahead.matches() and ahead.take() is None                 # nothing in flight any more

    assert ahead.take() is None and not ahead.matches()                     # nothing started yet
    taken_equals_synchronous()
    for change in ("state", "spring", "parameter"):
        ahead.start()
        if change == "state":
            kf.state.X[3, 0] += 1e-3
        elif change == "spring":
            kf.state.l0[2, 0] *= 1.01
        else:
            kf.tol = 1e-5
        assert not ahead.matches()
        assert ahead.take() is None and ahead.take() is None
        taken_equals_synchronous()                                          # the worker is idle and takes the next job
    # an update that was armed and failed: whether its job was started is not known
    for started in (False, True):
        ahead._armed, ahead.cov_armed = ahead.inputs(), True                # (what arm() leaves behind)
        if started:
            bars, l0, par = ahead._armed
            X = np.ascontiguousarray(kf.state.X.reshape(-1))
            _lib.check(_lib.lib().hm_ms_newton_start(ahead.worker(), int(kf.state.N), len(bars), _lib.ptr(bars), _lib.ptr(l0),
                                                     *par, _lib.ptr(X)), "hm_ms_newton_start")
        ahead.drain()
        assert ahead._armed is None and not ahead.cov_armed and not ahead.adopt() and ahead.take() is None
        taken_equals_synchronous()
    # ... and on a worker that has never had a job
    fresh = kalman.PredictionAhead(kf)
    fresh.worker()
    fresh._armed = fresh.inputs()
    fresh.drain()
    fresh.close()
    fresh.close()
    kf.close()
    assert ahead._worker is None
    kf.close()
