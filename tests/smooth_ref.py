"""NumPy f64 restatement of the Rauch-Tung-Striebel smoother (hydra_mi.smooth, csrc/smooth_kernels.h).

From the recorded P_k (posterior covariances), x_k (posterior means), m_k (the prior means the updates started from)
and the model F_k, Weps, backward for k = K-2 .. 0:

    Pp_{k+1} = F_k P_k F_k^T + Weps
    G_k      = P_k F_k^T Pp_{k+1}^-1
    xs_k     = x_k + G_k (xs_{k+1} - m_{k+1})
    Ps_k     = P_k + G_k (Ps_{k+1} - Pp_{k+1}) G_k^T

with xs_{K-1} = x_{K-1}, Ps_{K-1} = P_{K-1}.  Test infrastructure: the package does not import it.
"""
import numpy as np


def spring_blocks(bars, l0, kappa, X):
    """Per spring (Bxx, Bxy, Byy) of dfdy at the vertices of X (csrc/ekf.hip spring_blocks)."""
    X = np.asarray(X, np.float64).reshape(-1)
    bars = np.asarray(bars).reshape(-1, 2)
    a, b = bars[:, 0], bars[:, 1]
    dx = X[2 * a] - X[2 * b]
    dy = X[2 * a + 1] - X[2 * b + 1]
    l = np.sqrt(dx * dx + dy * dy)
    k = kappa * (1.0 - l0 / l)
    c = kappa * l0 / (l * l * l)
    return np.column_stack((k + c * dx * dx, c * dx * dy, k + c * dy * dy))


def dfdy(N, bars, blocks):
    """2N x 2N: bar i between a and b adds -B_i at (a, a), (b, b) and +B_i at (a, b), (b, a)."""
    D = np.zeros((2 * N, 2 * N))
    for (a, b), (bxx, bxy, byy) in zip(np.asarray(bars).reshape(-1, 2), np.asarray(blocks).reshape(-1, 3)):
        B = np.array([[bxx, bxy], [bxy, byy]])
        for p, q, sg in ((a, a, -1), (b, b, -1), (a, b, 1), (b, a, 1)):
            D[2 * p:2 * p + 2, 2 * q:2 * q + 2] += sg * B
    return D


def F_matrix(N, a, s, D=None):
    """F = [[I, a I], [s D, I]] (4N x 4N); D = dfdy (2N x 2N) or None (the constant-velocity model)."""
    e = np.eye(2 * N)
    A = np.zeros((2 * N, 2 * N)) if D is None else s * np.asarray(D)
    return np.block([[e, a * e], [A, e]])


def Weps(N, eps_F):
    e = np.eye(2 * N)
    return eps_F * np.block([[e / 4, e / 2], [e / 2, e]])


def model_F(N, bars, l0, kappa, a, s, X):
    """F_k of the filter's prediction at state X_k: the spring blocks at X_k, or constant velocity without springs."""
    if len(bars) == 0:
        return F_matrix(N, a, s)
    return F_matrix(N, a, s, dfdy(N, bars, spring_blocks(bars, l0, kappa, X)))


def smooth(P, x, m, F, Q, want_cov=True):
    """P: K covariances, x / m: K x n, F: K-1 transition matrices (F[k] from frame k to k+1), Q: n x n (or a list).
    -> (xs K x n, Ps list of K or None, steps: per k the dict of Pp, G of that step)."""
    K = len(P)
    x = np.asarray(x, np.float64).reshape(K, -1)
    m = np.asarray(m, np.float64).reshape(K, -1)
    xs = np.empty_like(x)
    xs[K - 1] = x[K - 1]
    Ps = [None] * K
    Ps[K - 1] = np.array(P[K - 1])
    steps = [None] * K
    for k in range(K - 2, -1, -1):
        Qk = Q[k] if isinstance(Q, (list, tuple)) else Q
        FP = F[k] @ P[k]
        Pp = FP @ F[k].T + Qk
        G = np.linalg.solve(Pp, FP).T          # P F^T Pp^-1 = (Pp^-1 F P)^T (P, Pp symmetric)
        xs[k] = x[k] + G @ (xs[k + 1] - m[k + 1])
        if want_cov:
            Ps[k] = P[k] + G @ (Ps[k + 1] - Pp) @ G.T
        steps[k] = dict(Pp=Pp, G=G)
    return xs, (Ps if want_cov else None), steps
