"""Extended-precision reference of the dense update, its priors, its error measures and its case table, shared by
tests/test_dense_ref_cpu.py (the reference alone), tests/test_dense_precision_gpu.py (the device against it) and
tools/dense_precision_table.py (the record under profiles/dense_precision.md).

The update solves, in binary64 on the device (csrc/dense_kernels.h, chol_flow_kernels.h),

    invW = inv(W)        A = invW + HTH        cov = inv(A)        step = cov (Hz - HTH (X0 - X))

Here the same is written out in numpy's longdouble (x87 extended, 64 bits of significand, u = 2^-64): a column Cholesky,
the inverse of its triangle, and Newton-Schulz steps on top.  The reference returns its raw result next to the refined
one, so that a test can state how uncertain the reference itself is and hold that far below its bound.

Errors are taken in the scaling that gives A a unit diagonal (D = sqrt(diag A)): a block of small variances cannot hide
inside the norm of a block of large ones.

The bound of the device (BOUND_FACTOR): 8 x max(e_lapack, u kappa_2(A^)), e_lapack the error of numpy.linalg in binary64
against the same reference in the same measure, u = 2^-53, A^ = D^-1 A D^-1.  Three bits for another elimination order,
32-wide accumulation on the matrix cores and the 0.62-ulp reciprocal square root."""
import zlib

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
BOUND_FACTOR = 8.0
SIDE = 64
DNB = 32            # block size of the factorisation (dense_kernels.h)
TV_ROWS = 128       # row groups of k_tvec
TTT_PF = 3          # block products in flight in k_ttt
EKF_MAX_STAR = 24


def available():
    """the reference needs a longdouble with at least the 64-bit significand of x87 extended"""
    return np.finfo(LD).nmant >= 63


SKIP_REASON = "numpy.longdouble has a %d-bit mantissa here; the reference needs 63" % np.finfo(LD).nmant


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- the reference ------------------------------------------------------------------------------------------------
def chol_inverse_ld(A, refine=2):
    """-> (raw, refined) inverse of the symmetric positive definite A in longdouble.  raw = T^T T with T = L^-1 from a
    column Cholesky A = L L^T and a forward substitution; refined = raw after `refine` Newton-Schulz steps
    X <- X (2 I - A X), symmetrised.  The steps form their residual in the same longdouble, so both results are good to
    about 2^-64 kappa(A); they are two estimates with differently structured errors, and their distance is what the
    reference states as its own uncertainty.  FloatingPointError on a pivot that is not positive (or not finite)."""
    A = np.asarray(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0 or not np.isfinite(d):
            raise FloatingPointError("pivot %d of %d is %g: the matrix is not positive definite" % (j, n, float(d)))
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    T = np.zeros((n, n), LD)
    for i in range(n):
        e = np.zeros(n, LD)
        e[i] = 1
        T[i] = (e - L[i, :i] @ T[:i]) / L[i, i]
    raw = T.T @ T
    X = raw
    two = 2 * np.eye(n, dtype=LD)
    for _ in range(refine):
        X = X @ (two - A @ X)
        X = (X + X.T) / 2
    return raw, X


def _kappa_scaled(A, cov):
    """kappa_2 of A^ = D^-1 A D^-1, D = sqrt(diag A), from the largest eigenvalues of A^ and of its inverse D cov D (each
    accurate in binary64 however small the other end of the spectrum is)"""
    d = np.sqrt(np.diag(A))
    Ah = np.asarray(A / np.outer(d, d), np.float64)
    Ch = np.asarray(cov * np.outer(d, d), np.float64)
    return float(np.linalg.eigvalsh((Ah + Ah.T) / 2)[-1] * np.linalg.eigvalsh((Ch + Ch.T) / 2)[-1])


def reference(W, HTH, Hz, X0, X, refine=2):
    """-> dict, all longdouble: invW, A, cov, step (4N), kappa (kappa_2 of A scaled to unit diagonal, a float), and
    cov_raw, step_raw: the same chain without any Newton-Schulz step, for the reference's own uncertainty.
    refine=0 (the near-singular priors only): no Newton-Schulz step at all.  A step's own rounding is about
    n 2^-64 kappa(W) |inv(W)| in every entry, unstructured; from kappa(W) = 1e15 on that swamps the small eigenvalues
    of inv(W), the ones HTH is added to, where the Cholesky inverse keeps them."""
    H = np.asarray(HTH, LD)
    rhs = np.asarray(Hz, LD).reshape(-1) - H @ (np.asarray(X0, LD).reshape(-1) - np.asarray(X, LD).reshape(-1))
    invW_raw, invW = chol_inverse_ld(W, refine)
    A = invW + H
    _, cov = chol_inverse_ld(A, refine)
    cov_raw, _ = chol_inverse_ld(invW_raw + H, refine=0)
    return dict(invW=invW, A=A, cov=cov, step=cov @ rhs, kappa=_kappa_scaled(A, cov), cov_raw=cov_raw,
                step_raw=cov_raw @ rhs)


def lapack(W, HTH, Hz, X0, X):
    """the comparator: the same two stages with numpy.linalg in binary64 -> dict cov, step (4N)"""
    W, H = np.asarray(W, np.float64), np.asarray(HTH, np.float64)
    rhs = np.asarray(Hz, np.float64).reshape(-1) - H @ (np.asarray(X0, np.float64).reshape(-1) -
                                                         np.asarray(X, np.float64).reshape(-1))
    cov = np.linalg.inv(np.linalg.inv(W) + H)
    return dict(cov=cov, step=cov @ rhs)


# ---- error measures -----------------------------------------------------------------------------------------------
def cov_err(C, ref):
    """max over i, j of |C - Cref|_ij / sqrt(Cref_ii Cref_jj)"""
    Cr = ref["cov"]
    d = np.sqrt(np.diag(Cr))
    return float(np.max(np.abs(np.asarray(C, LD) - Cr) / np.outer(d, d)))


def step_err(x, ref):
    """(position half, velocity half) of |D (x - xref)|_2 / |D xref|_2 with D = sqrt(diag A)"""
    xr = ref["step"]
    D = np.sqrt(np.diag(ref["A"]))
    dx = D * (np.asarray(x, LD).reshape(-1) - xr)
    h = xr.size // 2
    return tuple(float(np.sqrt(dx[s] @ dx[s]) / np.sqrt((D[s] * xr[s]) @ (D[s] * xr[s]))) for s in (slice(0, h), slice(h, None)))


def errors(got, ref):
    """-> (step error of the positions, of the velocities, covariance error) of a dict with step, cov"""
    return step_err(got["step"], ref) + (cov_err(got["cov"], ref),)


def uncertainty(ref):
    """the reference's own: its raw result against its refined one, in the three measures"""
    return errors(dict(step=ref["step_raw"], cov=ref["cov_raw"]), ref)


def bounds(ref, e_lapack):
    """what the device may be wrong by, per measure: BOUND_FACTOR x max(e_lapack, u kappa)"""
    return tuple(BOUND_FACTOR * max(e, U * ref["kappa"]) for e in e_lapack)


# ---- priors ---------------------------------------------------------------------------------------------------------
def spectrum(n, kappa):
    """Q diag(logspace(0, -log10 kappa)) Q^T, Q from the QR of a normal matrix seeded by (n, kappa); symmetric"""
    Q, _ = np.linalg.qr(_rng("spectrum:%d:%g" % (n, kappa)).normal(size=(n, n)))
    W = (Q * np.logspace(0.0, -np.log10(kappa), n)) @ Q.T
    return (W + W.T) / 2


def scaled(n, kappa, s):
    """D spectrum(n, kappa) D with D = 1 on the positions (first half) and s on the velocities"""
    d = np.concatenate((np.ones(n // 2), np.full(n - n // 2, float(s))))
    W = spectrum(n, kappa) * np.outer(d, d)
    return (W + W.T) / 2


def filter_like(N, side=SIDE, eps_F=1e-1):
    """the filter's initial covariance diag(1e-2 positions, 1 velocities) after two mass-spring predictions
    F W F^T + Weps (oracle ekf_ref.ms_predict on mesh_n(N, side), slightly off rest): dense, positions and velocities
    coupled"""
    from oracle import ekf_ref
    m = mesh_n(N, side)
    _, Weps, W = ekf_ref.initial_covariances(N, eps_F)
    K = ekf_ref.incidence(N, m.bars)
    X = np.concatenate((m.p.reshape(-1) + _rng("filter_like:%d" % N).normal(0, 0.3, 2 * N), np.zeros(2 * N)))
    for _ in range(2):
        X, W = ekf_ref.ms_predict(X, W, Weps, K, m.L)
    return (W + W.T) / 2


def pair_indefinite(n, i, j):
    """the identity with entries (i, j) and (j, i) set to 2: eigenvalues 3 and -1 behind a diagonal of ones"""
    W = np.eye(n)
    W[i, j] = W[j, i] = 2.0
    return W


def negated_spectrum(n, kappa=1e4):
    """spectrum(n, kappa) with its smallest eigenvalue negated (the diagonal stays positive)"""
    w, V = np.linalg.eigh(spectrum(n, kappa))
    w[0] = -w[0]
    W = (V * w) @ V.T
    return (W + W.T) / 2


# ---- meshes ---------------------------------------------------------------------------------------------------------
_MESHES = {}


def mesh_n(N, side=SIDE):
    """a valid mesh of exactly N vertices inside a side-px frame: the first N points of a jittered grid, Delaunay
    (slivers along the hull dropped), one orientation.  Every vertex is used, no star reaches EKF_MAX_STAR."""
    if (N, side) in _MESHES:
        return _MESHES[(N, side)]
    from scipy.spatial import Delaunay
    from hydra_mi import mesh
    import update_cases
    cols = int(np.ceil(np.sqrt(N)))
    rows = int(np.ceil(N / cols))
    lo, hi = 0.17 * side, 0.80 * side
    h = (hi - lo) / max(cols - 1, rows - 1, 1)
    g = np.array([(lo + h * (k % cols), lo + h * (k // cols)) for k in range(N)])
    p = g + _rng("mesh_n:%d:%d" % (N, side)).uniform(-0.18 * h, 0.18 * h, g.shape)
    t = Delaunay(p).simplices
    keep = np.abs(update_cases.doubled_areas(p.reshape(-1), t)) > 0.2 * h * h
    m = update_cases.oriented(mesh.Mesh(p, t[keep], h))
    star = np.bincount(m.t.reshape(-1), minlength=N)
    if m.size() != N or star.min() < 1 or star.max() >= EKF_MAX_STAR:
        raise AssertionError("mesh_n(%d, %d): stars of %d..%d triangles" % (N, side, star.min(), star.max()))
    _MESHES[(N, side)] = m
    return m


# ---- the case table -------------------------------------------------------------------------------------------------
# N -> (4N, remainder of 4N in the 32-row block, what the size exercises)
SIZES = {5: (20, 20, "one partial block"),
         8: (32, 0, "one full block, no padding"),
         9: (36, 4, "last block is one 4-row strip"),
         16: (64, 0, "two full blocks"),
         17: (68, 4, "last block is one 4-row strip"),
         24: (96, 0, "k_ttt with exactly TTT_PF steps"),
         32: (128, 0, "at the TV_ROWS boundary of k_tvec"),
         33: (132, 4, "past the TV_ROWS boundary of k_tvec"),
         50: (200, 8, "step grid large enough for the workgroup-id remap of k_chol_step")}

PRIORS = ("spectrum_1", "spectrum_1e4", "spectrum_1e8", "spectrum_1e11", "filter_like", "scaled_1e4_1e-4",
          "scaled_1e4_1e4")
MOVED_PRIOR = "spectrum_1e4"        # the prior that also runs with X0 = X + N(0, 0.3)
FLOW_PRIOR = "spectrum_1e8"         # the prior of the chol_flow 0 / 1 comparison
GOOD_PRIOR = "spectrum_1e4"         # the prior of the update that follows a refused one
NEAR_SINGULAR = ("spectrum_1e15", "spectrum_1e16")
NEAR_SINGULAR_N = 9

# indefinite priors with a positive diagonal: name -> (N, builder of the 4N x 4N matrix)
INDEFINITE = {"pair_first_block": (9, lambda n: pair_indefinite(n, 3, 21)),
              "pair_middle_block": (33, lambda n: pair_indefinite(n, 66, 90)),
              "pair_last_strip_36": (9, lambda n: pair_indefinite(n, n - 2, n - 1)),
              "pair_last_strip_68": (17, lambda n: pair_indefinite(n, n - 2, n - 1)),
              "negated_eigenvalue": (17, lambda n: negated_spectrum(n, 1e4))}


def prior(name, N):
    n = 4 * N
    if name == "filter_like":
        return filter_like(N)
    kind, *a = name.split("_")
    if kind == "spectrum":
        return spectrum(n, float(a[0]))
    if kind == "scaled":
        return scaled(n, float(a[0]), float(a[1]))
    raise KeyError(name)


def cases():
    """every (N, prior name, moved) of the accuracy table: each prior with X0 = X, one per size with X0 moved as well"""
    out = []
    for N in SIZES:
        out += [(N, p, False) for p in PRIORS] + [(N, MOVED_PRIOR, True)]
    return out


def states(N, moved):
    """-> (X, X0): the state the measurement is taken at and the prior mean (X itself unless moved)"""
    m = mesh_n(N)
    r = _rng("state:%d" % N)
    X = np.concatenate((m.p.reshape(-1) + r.normal(0, 0.3, 2 * N), r.normal(0, 1.0, 2 * N)))
    return X, (X + r.normal(0, 0.3, X.size) if moved else X.copy())


def synthetic_hth(N):
    """a stand-in for HTH and Hz where there is no device: a sum of outer products, each over the twelve state entries
    of one triangle (positions weighted 30, velocities 1, as image and flow terms are), so sparse with the mesh's own
    pattern and positive semi-definite -> (HTH, Hz)"""
    m = mesh_n(N)
    r = _rng("hth:%d" % N)
    n = 4 * N
    H = np.zeros((n, n))
    for tr in m.t:
        idx = np.concatenate([(2 * v, 2 * v + 1, 2 * N + 2 * v, 2 * N + 2 * v + 1) for v in tr])
        G = r.normal(size=(12, 8)) * np.tile((30.0, 30.0, 1.0, 1.0), 3)[:, None]
        H[np.ix_(idx, idx)] += G @ G.T
    H = (H + H.T) / 2
    return H, H @ r.normal(0, 0.5, n)


# ---- the device side (GPU test and table tool) ------------------------------------------------------------------------
class _State:
    pass


class Device:
    """one Renderer on mesh_n(N) with an observation in place, as tests/test_ekf_gpu._setup / _observation build them"""

    def __init__(self, N, side=SIDE):
        from hydra_mi import renderer, synth
        from oracle import ekf_ref
        self.N, self.side, self.m = N, side, mesh_n(N, side)
        m, eps = self.m, (1e-3, 1.0, 1.0)
        tex = synth.noise_texture(side, 8).astype(np.uint8)
        self.R = renderer.Renderer(m, np.zeros((N, 2)), np.zeros((side, side, 2), np.float32), side, tex, True, *eps)
        meas = ekf_ref.Measurement(N, m.t, m.p, tex, *eps)
        Xobs = np.concatenate((m.p.reshape(-1) + 1.5, np.full(2 * N, 0.5)))
        y_im, yfx, yfy, ym = meas.render(Xobs)
        noise = _rng("obs:%d" % N).normal(0, 0.05, (side, side, 2))
        self.obs = (y_im, (np.dstack((yfx, -yfy)) + noise).astype(np.float32), (ym // 255).astype(np.uint8))
        self._measured = {}

    def measure(self, X):
        """(Hz, HTH) of k_hth_scatter at X: the arithmetic k_solve_prep promises to repeat, so the system's true input"""
        key = X.tobytes()
        if key not in self._measured:
            st = _State()
            st.X = X.reshape(-1, 1)
            Hz, HTH, _ = self.R.measure(st, *self.obs)
            self._measured[key] = (Hz.reshape(-1).copy(), HTH.copy())
        return self._measured[key]

    def update(self, W, X, X0):
        """update_begin + update_step at X -> dict step (4N), cov, prior (update_cov(-1))"""
        st = _State()
        st.X = X.reshape(-1, 1)
        self.R.update_begin(W, X0)
        step, _, _ = self.R.update_step(st, *self.obs, want_error=False)
        return dict(step=step.reshape(-1), cov=self.R.update_cov(0), prior=self.R.update_cov(-1))


def measured_case(dev, name, moved, W=None, refine=2):
    """one case on the device -> (reference, device result, errors of the comparator, errors of the device)"""
    X, X0 = states(dev.N, moved)
    W = prior(name, dev.N) if W is None else W
    Hz, HTH = dev.measure(X)
    ref = reference(W, HTH, Hz, X0, X, refine)
    got = dev.update(W, X, X0)
    return ref, got, errors(lapack(W, HTH, Hz, X0, X), ref), errors(got, ref)
