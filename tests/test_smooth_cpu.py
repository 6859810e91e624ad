"""The RTS smoother without a GPU: the NumPy restatement (tests/smooth_ref.py) against the direct solution of the joint
least-squares problem over all frames, argument errors of hm_smooth_*, and RTSSmoother's memory budget."""
import ctypes
import types

import numpy as np
import pytest

import smooth_ref


def _spd(rng, n, scale=1.0):
    A = rng.standard_normal((n, n))
    return scale * (A @ A.T / n + np.eye(n))


def _linear_gaussian(rng, N, K, springs):
    """A linear-Gaussian track of K frames of 4N states: x_0 ~ N(m_0, Pp_0), x_{k+1} = F_k x_k + w (Q), y_k = H_k x_k
    + v (R_k).  -> the filter's P_k, x_k, m_k, F_k, Q and the joint least-squares solution (means, covariances)."""
    n = 4 * N
    if springs:
        bars = np.array([[i, (i + 1) % N] for i in range(N)], np.int32)
        Fs = []
        for k in range(K - 1):
            blk = rng.standard_normal((N, 3)) * 0.3
            Fs.append(smooth_ref.F_matrix(N, 0.05, 0.05, smooth_ref.dfdy(N, bars, blk)))
    else:
        Fs = [smooth_ref.F_matrix(N, 1.0, 0.0) for _ in range(K - 1)]
    Q = _spd(rng, n, 0.1)            # (the filter's Weps is singular: the joint problem needs Q^-1)
    m0, Pp0 = rng.standard_normal(n), _spd(rng, n)
    Hs = [rng.standard_normal((n // 2 + 1, n)) for _ in range(K)]
    Rs = [_spd(rng, n // 2 + 1, 0.5) for _ in range(K)]
    ys = [rng.standard_normal(n // 2 + 1) * 3 for _ in range(K)]
    # the filter
    P, x, m = [], [], []
    mk, Ppk = m0, Pp0
    for k in range(K):
        H, R, y = Hs[k], Rs[k], ys[k]
        Pk = np.linalg.inv(np.linalg.inv(Ppk) + H.T @ np.linalg.solve(R, H))
        Pk = (Pk + Pk.T) / 2
        xk = mk + Pk @ H.T @ np.linalg.solve(R, y - H @ mk)
        P.append(Pk); x.append(xk); m.append(mk)
        if k < K - 1:
            mk = Fs[k] @ xk
            Ppk = Fs[k] @ Pk @ Fs[k].T + Q
    # the joint problem: minimise |x_0 - m_0|^2_{Pp0^-1} + sum |y_k - H_k x_k|^2_{R_k^-1} + sum |x_{k+1} - F_k x_k|^2_{Q^-1}
    A = np.zeros((K * n, K * n))
    b = np.zeros(K * n)
    Pi, Qi = np.linalg.inv(Pp0), np.linalg.inv(Q)
    A[:n, :n] += Pi
    b[:n] += Pi @ m0
    for k in range(K):
        s = slice(k * n, (k + 1) * n)
        A[s, s] += Hs[k].T @ np.linalg.solve(Rs[k], Hs[k])
        b[s] += Hs[k].T @ np.linalg.solve(Rs[k], ys[k])
    for k in range(K - 1):
        s, t = slice(k * n, (k + 1) * n), slice((k + 1) * n, (k + 2) * n)
        F = Fs[k]
        A[s, s] += F.T @ Qi @ F
        A[t, t] += Qi
        A[s, t] -= F.T @ Qi
        A[t, s] -= Qi @ F
    sol = np.linalg.solve(A, b).reshape(K, n)
    cov = np.linalg.inv(A)
    covs = [cov[k * n:(k + 1) * n, k * n:(k + 1) * n] for k in range(K)]
    return P, np.array(x), np.array(m), Fs, Q, sol, covs


@pytest.mark.parametrize("springs", [False, True])
@pytest.mark.parametrize("N,K", [(1, 2), (2, 5), (3, 7)])
def test_restatement_is_the_joint_least_squares_solution(springs, N, K):
    """Pins tests/smooth_ref.py independently of its own formulas: on linear-Gaussian systems the smoothed means and
    covariances are the solution of the joint problem over all frames and the blocks of its inverse Hessian."""
    rng = np.random.default_rng(17 * N + K + (100 if springs else 0))
    P, x, m, Fs, Q, sol, covs = _linear_gaussian(rng, N, K, springs)
    xs, Ps, _ = smooth_ref.smooth(P, x, m, Fs, Q)
    for k in range(K):
        assert np.linalg.norm(xs[k] - sol[k]) <= 1e-10 * max(1.0, np.linalg.norm(sol[k]))
        assert np.linalg.norm(Ps[k] - covs[k]) <= 1e-10 * max(1.0, np.linalg.norm(covs[k]))
    xs0, Ps0, _ = smooth_ref.smooth(P, x, m, Fs, Q, want_cov=False)
    assert Ps0 is None and np.array_equal(xs0, xs)


def test_restated_model_matrices():
    """F = [[I, a I], [s dfdy, I]] with dfdy assembled from the spring blocks, Weps = eps [[I/4, I/2], [I/2, I]]."""
    N = 3
    bars = np.array([[0, 1], [1, 2]], np.int32)
    X = np.array([0.0, 0.0, 3.0, 0.0, 3.0, 4.0] + [0.0] * 6)
    blk = smooth_ref.spring_blocks(bars, np.array([2.0, 5.0]), -1.0, X)
    # bar 0 along x, l = 3, l0 = 2: k = -(1 - 2/3), c = -2/27; Bxx = k + c 9, Bxy = 0, Byy = k
    assert np.allclose(blk[0], [-1 / 3 - 2 / 3, 0.0, -1 / 3])
    D = smooth_ref.dfdy(N, bars, blk)
    assert np.allclose(D, D.T) and np.allclose(D.sum(axis=1).reshape(N, 2).sum(axis=0), 0.0)
    F = smooth_ref.model_F(N, bars, np.array([2.0, 5.0]), -1.0, 0.05, 0.05, X)
    assert np.allclose(F[6:, :6], 0.05 * D) and np.allclose(F[:6, 6:], 0.05 * np.eye(6))
    W = smooth_ref.Weps(N, 0.2)
    assert np.allclose(W[:6, :6], 0.05 * np.eye(6)) and np.allclose(W[:6, 6:], 0.1 * np.eye(6))


def test_argument_errors_do_not_need_a_gpu(hm):
    from hydra_mi import _lib
    L = _lib.lib()
    h = _lib.c_vp()
    assert L.hm_smooth_create(None, 1, 0, None, None, 0.0, 1.0, 0.0, 1.0, ctypes.byref(h)) == -1
    assert b"capacity 1" in L.hm_last_error()
    assert L.hm_smooth_create(None, 8, 0, None, None, 0.0, 1.0, 0.0, 1.0, ctypes.byref(h)) == -1
    assert b"NULL filter handle" in L.hm_last_error()
    assert L.hm_smooth_create(None, 8, 0, None, None, 0.0, 1.0, 0.0, 1.0, None) == -1
    x = np.zeros(16)
    assert L.hm_smooth_record(None, _lib.ptr(x)) == -1
    assert L.hm_smooth_run(None, 1, _lib.ptr(x), _lib.ptr(x)) == -1
    assert L.hm_smooth_fetch(None, 0, None, None, None) == -1
    assert L.hm_smooth_prior(None, 1, _lib.ptr(x)) == -1
    assert L.hm_smooth_count(None, None, None) == -1
    assert L.hm_smooth_destroy(None) == 0
    a = np.zeros((4, 4))
    assert L.hm_op_smooth_gemm(0, 5, 4, _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), _lib.ptr(a)) == -1
    assert b"which 5" in L.hm_last_error()
    assert L.hm_op_smooth_gemm(0, -1, 4, _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), _lib.ptr(a)) == -1
    assert b"which -1" in L.hm_last_error()
    assert L.hm_op_smooth_gemm(0, 2, 4, _lib.ptr(a), _lib.ptr(a), None, _lib.ptr(a)) == -1
    assert L.hm_op_smooth_gemm(0, 1, 4, _lib.ptr(a), _lib.ptr(a), None, _lib.ptr(a)) == -1
    assert L.hm_op_smooth_gemm(0, 0, 0, _lib.ptr(a), _lib.ptr(a), None, _lib.ptr(a)) == -1


def test_budget_is_refused_with_its_numbers(hm):
    from hydra_mi import smooth
    n4 = 4 * 201
    per_frame = (n4 * n4 + 4 * n4) * 8
    assert smooth.record_bytes(201, 64) == 64 * per_frame + 7 * n4 * n4 * 8
    assert smooth.check_budget(201, 64, 8 << 30) == smooth.record_bytes(201, 64)
    with pytest.raises(ValueError, match=r"a record of 2000 frames at 201 vertices needs %d bytes .*5\.17 MB per frame.*"
                                         r"max_bytes = %d" % (smooth.record_bytes(201, 2000), 8 << 30)):
        smooth.check_budget(201, 2000, 8 << 30)
    # the constructor checks before it touches the filter's device handle
    kf = types.SimpleNamespace(N=201)
    with pytest.raises(ValueError, match="a record of 100 frames at 201 vertices"):
        smooth.RTSSmoother(kf, 100, max_bytes=100 * per_frame)
    with pytest.raises(ValueError, match="capacity 1"):
        smooth.RTSSmoother(kf, 1)
