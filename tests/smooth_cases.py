"""The case table of the smoother's precision tests, shared by tests/test_smooth_precision_cpu.py (the reference alone),
tests/test_smooth_precision_gpu.py (the device against it) and tools/smooth_precision_table.py (the record under
profiles/smooth_precision.md).

A case is a track of K = 4 frames on dense_ref.mesh_n(N), its forward filter run on the host:

    Pp_0 = dense_ref.prior(name, N)          P_k = inv(inv(Pp_k) + h HTH)   (longdouble, rounded once, symmetrised)
    x_k  = m_k + noise of the posterior's scale                              (so that the corrections are not small)
    m_{k+1} = F_k x_k                        Pp_{k+1} = F_k P_k F_k^T + Weps

with HTH from dense_ref.synthetic_hth(N), h a strong (1) or a weak (1e-6) measurement, F_k the mass-spring model
(kappa = -1, a = s = 0.05, the bars of the mesh) or constant velocity (no bars, a = 1, s = 0), eps_F 1e-1 or 1e-6.  The
recorded doubles P_k, x_k, m_k are the input of the device, of the comparator (smooth_ref.smooth in binary64) and of
the reference (smooth_ref.smooth_ld) alike.

The bar of a case, per frame and per measure (smooth_ref.errors): BOUND_FACTOR x max(e_numpy, u kappa) -- e_numpy the
comparator's error against the same reference in the same measure, u = 2^-53, kappa the largest kappa_2 over the steps
of Pp scaled to a unit diagonal, BOUND_FACTOR = dense_ref.BOUND_FACTOR for the reasons written there (the smoother runs
the same factorisation and the same kind of product).  What accumulates over the three backward steps is carried by the
comparator, which runs the same recursion."""
import collections

import numpy as np

import dense_ref as dr
import smooth_ref

LD = np.longdouble
K = 4
KAPPA, DELTAT, MASS = -1.0, 0.05, 1.0       # the mass-spring model: a = DELTAT, s = DELTAT / MASS

# N -> what 4N exercises in the backward step: the smallest size at which each structure first appears
SIZES = {5: "one partial 32-block",
         8: "exactly one block",
         9: "a last block of one 4-row strip",
         17: "two blocks and a strip",
         24: "three full blocks (TTT_PF: the products through the factor have a slab wholly left of the diagonal)",
         33: "past TV_ROWS",
         50: "enough blocks for the task scheduling of k_chol_flow to matter",
         65: "past 256 in k_sm_trmv / k_sm_mvt: a second pass of the j loop, a second workgroup"}

Case = collections.namedtuple("Case", "N prior h eps_F springs")

# Every size has spectrum_1e4 and one ill-conditioned prior (spectrum_1e8 or spectrum_1e11); the other priors, the weak
# measurement, the small eps_F and the constant-velocity model are spread so that each appears at least twice.
# N = 50 and N = 65 have two cases each: their longdouble reference takes seconds.
# Not in the table: (33, spectrum_1e8, h = 1e-6, eps_F = 1e-6, constant velocity) -- the reference's own uncertainty
# reaches 1/8 of the bar in the mean measure there, over the cap of 1/16 (test_smooth_precision_cpu.py); N = 33 has the
# same prior and measurement with eps_F = 1e-1 instead, which lowers kappa.
CASES = (
    Case(5, "spectrum_1e4", 1.0, 1e-1, True),
    Case(5, "spectrum_1e11", 1e-6, 1e-1, True),
    Case(5, "spectrum_1", 1.0, 1e-1, False),
    Case(8, "spectrum_1e4", 1e-6, 1e-1, False),
    Case(8, "spectrum_1e8", 1.0, 1e-6, True),
    Case(8, "scaled_1e4_1e4", 1.0, 1e-1, False),
    Case(9, "spectrum_1e4", 1.0, 1e-6, True),
    Case(9, "spectrum_1e11", 1.0, 1e-6, True),
    Case(9, "filter_like", 1e-6, 1e-1, True),
    Case(17, "spectrum_1e4", 1.0, 1e-1, False),
    Case(17, "spectrum_1e8", 1e-6, 1e-1, True),
    Case(17, "scaled_1e4_1e4", 1.0, 1e-1, True),
    Case(17, "filter_like", 1.0, 1e-1, True),
    Case(17, "scaled_1e4_1e-4", 1.0, 1e-6, True),
    Case(24, "spectrum_1e4", 1e-6, 1e-6, True),
    Case(24, "spectrum_1e11", 1.0, 1e-1, False),
    Case(24, "spectrum_1", 1e-6, 1e-1, True),
    Case(33, "spectrum_1e4", 1.0, 1e-1, True),
    Case(33, "spectrum_1e8", 1e-6, 1e-1, False),
    Case(33, "scaled_1e4_1e-4", 1e-6, 1e-1, False),
    Case(50, "spectrum_1e4", 1.0, 1e-1, True),
    Case(50, "spectrum_1e8", 1.0, 1e-6, True),
    Case(65, "spectrum_1e4", 1e-6, 1e-1, True),
    Case(65, "spectrum_1e8", 1.0, 1e-1, True),
)
BENIGN = Case(9, "spectrum_1e4", 1.0, 1e-6, True)       # kappa of a few hundred: the consistency and planted-error case
ILL = ("spectrum_1e8", "spectrum_1e11")
WHAT = ("mean positions", "mean velocities", "covariance")


def label(c):
    return "N=%d %s h=%g eps_F=%g %s" % (c.N, c.prior, c.h, c.eps_F, "springs" if c.springs else "constant velocity")


def cases_of(N):
    return [c for c in CASES if c.N == N]


def model(c):
    """(bars, l0, kappa, a, s, eps_F) as hydra_mi.smooth._model hands them to hm_smooth_create"""
    if not c.springs:
        return np.zeros((0, 2), np.int32), np.zeros(0), 0.0, 1.0, 0.0, float(c.eps_F)
    m = dr.mesh_n(c.N)
    return (np.ascontiguousarray(m.bars, np.int32).reshape(-1, 2), np.ascontiguousarray(m.L, np.float64), KAPPA, DELTAT,
            DELTAT / MASS, float(c.eps_F))


def max_degree(c):
    """the largest number of springs at one vertex: the length of the longest sum in k_fw_rows / k_pft_cols"""
    bars = model(c)[0]
    return int(np.bincount(bars.reshape(-1), minlength=c.N).max()) if len(bars) else 0


def transition(c, xk):
    bars, l0, kappa, a, s, _ = model(c)
    return smooth_ref.model_F(c.N, bars, l0, kappa, a, s, xk)


_TRACKS, _REFS = {}, {}


def track(c):
    """-> dict P (K matrices), x, m (K x 4N), F (K-1 matrices), Q: the record of the case, in binary64; computed once"""
    if c in _TRACKS:
        return _TRACKS[c]
    N, n = c.N, 4 * c.N
    rng = dr._rng("smooth:%d:%s:%g:%g:%d" % (c.N, c.prior, c.h, c.eps_F, c.springs))
    mesh = dr.mesh_n(N)
    Q = smooth_ref.Weps(N, c.eps_F)
    H = (dr.synthetic_hth(N)[0] * c.h).astype(LD)
    Pp = dr.prior(c.prior, N)
    mk = np.concatenate((mesh.p.reshape(-1), rng.normal(0, 1.0, 2 * N)))
    P, x, ms, F = [], [], [], []
    for k in range(K):
        Pk = dr.chol_inverse_ld(dr.chol_inverse_ld(Pp, refine=0)[0] + H, refine=0)[0]      # (input data: no refinement)
        Pk = np.asarray(Pk, np.float64)
        Pk = (Pk + Pk.T) / 2
        # the posterior's own scale, at most a pixel (or a pixel per frame) so that the mesh stays a mesh
        xk = mk + rng.normal(0, 0.3, n) * np.sqrt(np.diag(Pk)).clip(0, 1)
        P.append(Pk); x.append(xk); ms.append(mk)
        if k < K - 1:
            Fk = transition(c, xk)
            F.append(Fk)
            mk = Fk @ xk
            Pp = Fk @ Pk @ Fk.T + Q
            Pp = (Pp + Pp.T) / 2
    _TRACKS[c] = dict(P=P, x=np.array(x), m=np.array(ms), F=F, Q=Q)
    return _TRACKS[c]


def measured(P, x, m, F, Q):
    """reference, comparator errors and bars of one record -> dict ref (smooth_ld), e_numpy, unc, bound ((K-1) x 3 each:
    per frame the mean error of the positions, of the velocities, the covariance error), base = bound / BOUND_FACTOR"""
    ref = smooth_ref.smooth_ld(P, x, m, F, Q)
    xs, Ps, _ = smooth_ref.smooth(P, x, m, F, Q)
    e_numpy = smooth_ref.errors(xs, Ps, x, ref)
    base = np.maximum(e_numpy, dr.U * ref["kappa"])
    return dict(ref=ref, e_numpy=e_numpy, unc=smooth_ref.uncertainty(x, ref), base=base, bound=dr.BOUND_FACTOR * base,
                numpy=(xs, Ps))


def reference(c):
    """measured() of the case's own track; computed once"""
    if c not in _REFS:
        t = track(c)
        _REFS[c] = measured(t["P"], t["x"], t["m"], t["F"], t["Q"])
    return _REFS[c]


def prior_bound(c, xk, P, Q):
    """What hm_smooth_prior may be wrong by, componentwise: c_p u (|F| |P| |F|^T + Weps)_ij, with |F| taken term by term.

    Pp = F P F^T + Weps is a product with no inverse in it, so no kappa.  The device forms it in two passes of the same
    shape (k_fw_rows: F P by rows; k_pft_cols: (F P) F^T by columns).  In a pass, a term of the longest sum -- a velocity
    row, over the d springs of its vertex -- goes through: the difference of the two ends (1 rounding), the product with
    the block entry (1), the sum of the block's two products (1), the running sum over the springs (d), the product with
    s (1), the sum with the velocity entry (1): d + 5 roundings, so a relative error of at most (d + 5) u of the sum of
    the terms' magnitudes (the build keeps product and sum apart: -ffp-contract=off).  Two passes, one more rounding
    where Weps is added: c_p = 2 (d_max + 5) + 1 = 2 d_max + 11, d_max the largest vertex degree of the mesh (0 for
    constant velocity).  The spring blocks add nothing: the host evaluates them by the expression of
    smooth_ref.spring_blocks, operation by operation.  (1 + u)^c_p - 1 <= 1.01 c_p u at these sizes.

    The terms' magnitudes: the kernels never assemble F.  They sum s B_q (P_v - P_u) spring by spring, so what bounds
    their terms is the matrix with sum_q |B_q| in the diagonal block of vertex v and |B_q| off it -- not |sum_q B_q|,
    the diagonal block of the assembled F, which is smaller wherever the xy entries of a vertex's springs cancel (on these
    meshes they do).  A bound with the assembled |F| is not a bound of this
    arithmetic, nor of the reference's own assembly of dfdy in binary64.  -> (c_p, the 4N x 4N array of bounds)"""
    bars, l0, kappa, a, s, _ = model(c)
    cp = 2 * max_degree(c) + 11
    if len(bars):
        blocks = np.abs(smooth_ref.spring_blocks(bars, l0, kappa, xk))
        Fa = np.abs(smooth_ref.F_matrix(c.N, a, s, smooth_ref.dfdy(c.N, bars, blocks))).astype(LD)
    else:
        Fa = np.asarray(smooth_ref.F_matrix(c.N, a, s), LD)
    return cp, 1.01 * cp * dr.U * (Fa @ np.abs(np.asarray(P, LD)) @ Fa.T + np.asarray(Q, LD))


# ---- the device side (GPU test and table tool) ------------------------------------------------------------------------
class _Namespace:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def filter_stand_in(c, renderer):
    """what RTSSmoother reads of a filter object (hydra_mi.smooth._model): N, state.renderer / l0 / eps_F, and for the
    mass-spring model _bars, kappa, deltat, M (left out: the constant-velocity model)"""
    bars, l0, kappa, a, s, eps_F = model(c)
    kf = _Namespace(N=c.N, state=_Namespace(renderer=renderer, l0=l0.reshape(-1, 1), eps_F=eps_F, X=None))
    if c.springs:
        kf._bars, kf.kappa, kf.deltat, kf.M = bars, KAPPA, DELTAT, MASS
    return kf


def record(dev, sm, P, x, m):
    """Put a chosen record on the device: an update_run without iterations keeps the prior as the resident covariance
    and its X0 as the prior mean (test_ekf_gpu.test_update_run_without_iterations_keeps_the_prior), which is what
    hm_smooth_record copies."""
    dev.R.update_frame(*dev.obs)
    for k in range(len(P)):
        dev.R.update_run(np.ascontiguousarray(P[k]), m[k], *dev.obs, 0, 1e-4)
        sm.record(x[k])


def run_on_device(dev, c, on_recorded=None):
    """the case on dev (a dense_ref.Device of c.N) -> dict: fetched (what sm.fetch returns per frame, before the runs;
    on_recorded(fetched) is called before anything is computed from the record), prior (Pp_k of sm.prior, k = 1 .. K-1),
    xs0 (run without covariances), xs, var, Ps (run with)"""
    from hydra_mi.smooth import RTSSmoother
    t = track(c)
    with RTSSmoother(filter_stand_in(c, dev.R), K) as sm:
        record(dev, sm, t["P"], t["x"], t["m"])
        fetched = [sm.fetch(k) for k in range(K)]
        if on_recorded is not None:
            on_recorded(fetched)
        prior = [None] + [sm.prior(k) for k in range(1, K)]
        xs0, var0 = sm.run(covariances=False)
        xs, var = sm.run(covariances=True)
        Ps = [sm.cov(k) for k in range(K)]
    return dict(fetched=fetched, prior=prior, xs0=xs0, var0=var0, xs=xs, var=var, Ps=Ps)


def prior_errors(c, got):
    """per k = 1 .. K-1: (the largest |Pp_device - Pp_ref|_ij over its componentwise bar, the same difference in the scaled
    covariance measure), and c_p"""
    t, ref = track(c), reference(c)["ref"]
    out = []
    for k in range(1, K):
        cp, B = prior_bound(c, t["x"][k - 1], t["P"][k - 1], t["Q"])
        diff = np.abs(np.asarray(got["prior"][k], LD) - ref["Pp"][k])
        out.append((float(np.max(diff / B)), smooth_ref.cov_err(got["prior"][k], ref["Pp"][k])))
    return out, cp


def device_errors(c, got):
    """(K-1) x 3: the device's errors per frame in the measures of smooth_ref.errors"""
    return smooth_ref.errors(got["xs"], got["Ps"], track(c)["x"], reference(c)["ref"])
