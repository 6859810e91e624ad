"""NumPy f64 restatement of the Rauch-Tung-Striebel smoother (hydra_mi.smooth, csrc/smooth_kernels.h).

From the recorded P_k (posterior covariances), x_k (posterior means), m_k (the prior means the updates started from)
and the model F_k, Weps, backward for k = K-2 .. 0:

    Pp_{k+1} = F_k P_k F_k^T + Weps
    G_k      = P_k F_k^T Pp_{k+1}^-1
    xs_k     = x_k + G_k (xs_{k+1} - m_{k+1})
    Ps_k     = P_k + G_k (Ps_{k+1} - Pp_{k+1}) G_k^T

with xs_{K-1} = x_{K-1}, Ps_{K-1} = P_{K-1}.  Test infrastructure: the package does not import it.

smooth_ld is the same recursion in numpy.longdouble (the reference of tests/test_smooth_precision_*.py, with the
inverse of tests/dense_ref.py), and the error measures next to it are taken where the smoother works: on the correction
xs_k - x_k, a fraction of a pixel behind positions of tens of pixels, and on Ps_k scaled to a unit diagonal.
"""
import numpy as np

LD = np.longdouble


def spring_blocks(bars, l0, kappa, X):
    """Per spring (Bxx, Bxy, Byy) of dfdy at the vertices of X (csrc/ctx.h spring_blocks)."""
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


# ---- the extended-precision reference and its error measures ------------------------------------------------------------
def smooth_ld(P, x, m, F, Q, refine=2):
    """The recursion of smooth() in numpy.longdouble, from the same binary64 inputs (F[k]: model_F at the recorded x_k,
    promoted).  Pp = F P F^T + Q symmetrised, inv(Pp) from dense_ref.chol_inverse_ld, G = (inv(Pp) F P)^T.

    -> dict: xs (K x n), Ps, Pp (lists of K; Pp[0] is None): the refined result (`refine` Newton-Schulz steps on every
    inverse); xs_raw, Ps_raw: the whole recursion again with the raw inverses T^T T, for the reference's own
    uncertainty (as dense_ref.reference does); kappas: per step k the kappa_2 of Pp_{k+1} scaled to a unit diagonal
    (None for k = K-1); kappa: the largest of them.  FloatingPointError where a Pp has no Cholesky factor."""
    import dense_ref
    K = len(P)
    xl = np.asarray(x, LD).reshape(K, -1)
    ml = np.asarray(m, LD).reshape(K, -1)
    out = dict(xs=np.empty_like(xl), xs_raw=np.empty_like(xl), Ps=[None] * K, Ps_raw=[None] * K, Pp=[None] * K,
               kappas=[None] * K)
    for key in ("xs", "xs_raw"):
        out[key][K - 1] = xl[K - 1]
    for key in ("Ps", "Ps_raw"):
        out[key][K - 1] = np.asarray(P[K - 1], LD)
    for k in range(K - 2, -1, -1):
        Fk, Pk = np.asarray(F[k], LD), np.asarray(P[k], LD)
        Qk = np.asarray(Q[k] if isinstance(Q, (list, tuple)) else Q, LD)
        FP = Fk @ Pk
        Pp = FP @ Fk.T + Qk
        Pp = (Pp + Pp.T) / 2
        raw, fine = dense_ref.chol_inverse_ld(Pp, refine)
        out["Pp"][k + 1] = Pp
        out["kappas"][k] = dense_ref._kappa_scaled(Pp, fine)
        for inv, xs, Ps in ((fine, out["xs"], out["Ps"]), (raw, out["xs_raw"], out["Ps_raw"])):
            G = (inv @ FP).T
            xs[k] = xl[k] + G @ (xs[k + 1] - ml[k + 1])
            Ps[k] = Pk + G @ (Ps[k + 1] - Pp) @ G.T
    out["kappa"] = max(kp for kp in out["kappas"] if kp is not None)
    return out


def cov_err(C, Cref):
    """max over i, j of |C - Cref|_ij / sqrt(Cref_ii Cref_jj): one frame's Ps_k, or a Pp_k"""
    Cr = np.asarray(Cref, LD)
    d = np.sqrt(np.diag(Cr))
    return float(np.max(np.abs(np.asarray(C, LD) - Cr) / np.outer(d, d)))


def mean_err(xs, x, xs_ref, Ps_ref):
    """(position half, velocity half) of |d (c - c_ref)|_2 / |d c_ref|_2 for one frame: c = xs - x the correction the
    smoother computes, c_ref = xs_ref - x, d = 1 / sqrt(diag Ps_ref)"""
    xl = np.asarray(x, LD).reshape(-1)
    d = 1 / np.sqrt(np.diag(np.asarray(Ps_ref, LD)))
    cr = d * (np.asarray(xs_ref, LD).reshape(-1) - xl)
    dc = d * (np.asarray(xs, LD).reshape(-1) - xl) - cr
    h = xl.size // 2
    return tuple(float(np.sqrt(dc[s] @ dc[s]) / np.sqrt(cr[s] @ cr[s])) for s in (slice(0, h), slice(h, None)))


def whitened_correction_rms(x, xs_ref, Ps_ref):
    """RMS of (xs_ref - x) / sqrt(diag Ps_ref) over one frame: what the relative mean measure divides by"""
    c = (np.asarray(xs_ref, LD).reshape(-1) - np.asarray(x, LD).reshape(-1)) / np.sqrt(np.diag(np.asarray(Ps_ref, LD)))
    return float(np.sqrt(np.mean(c * c)))


def errors(xs, Ps, x, ref):
    """per frame k = 0 .. K-2 the triple (mean error of the positions, of the velocities, covariance error) of a result
    xs (K x n), Ps (K matrices) against smooth_ld's dict -> (K-1) x 3 array"""
    K = len(ref["Ps"])
    return np.array([mean_err(xs[k], x[k], ref["xs"][k], ref["Ps"][k]) + (cov_err(Ps[k], ref["Ps"][k]),)
                     for k in range(K - 1)])


def uncertainty(x, ref):
    """the reference's own: its raw recursion against its refined one, in the same measures"""
    return errors(ref["xs_raw"], ref["Ps_raw"], x, ref)
