"""The dense update on the device (blocked Cholesky in both forms, chol32_strip*, k_tvec, k_ttt, the prior inverse and
the assembly of k_solve_prep) against the extended-precision reference of tests/dense_ref.py: at the block-structure
edges of 4N, with ill-conditioned, correlated and badly scaled priors, in measures scaled so that a block of small
variances cannot hide.

The bar, per case and per measure: 8 x max(e_lapack, u kappa_2(A^)) -- e_lapack the error of numpy.linalg in binary64
against the same reference, u = 2^-53, A^ the information matrix scaled to a unit diagonal (dense_ref.bounds).  What the
device measured against it is recorded in profiles/dense_precision.md (tools/dense_precision_table.py).

HTH and Hz are read back with Renderer.measure at the same state: k_solve_prep promises the arithmetic of
k_hth_scatter, so those arrays are the system's true input."""
import numpy as np
import pytest

import dense_ref as dr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not dr.available(), reason=dr.SKIP_REASON)]

WHAT = ("step positions", "step velocities", "covariance")


@pytest.fixture(scope="module")
def devices(hm):
    """one Renderer per mesh, shared by the tests of that size and closed with the module"""
    made = {}

    def get(N):
        if N not in made:
            made[N] = dr.Device(N)
        made[N].R.tune("chol_flow", 1)
        return made[N]
    yield get
    for d in made.values():
        d.R.close()


def _check(dev, name, moved, W=None, refine=2):
    """one case against the bar; -> the device's result"""
    ref, got, e_lapack, e_dev = dr.measured_case(dev, name, moved, W, refine)
    bound = dr.bounds(ref, e_lapack)
    print("N=%d %s%s kappa %.2e  lapack %s  device %s  ratio %s" % (
        dev.N, name, " moved" if moved else "", ref["kappa"], " ".join("%.2e" % e for e in e_lapack),
        " ".join("%.2e" % e for e in e_dev), " ".join("%.2f" % (e / (b / dr.BOUND_FACTOR)) for e, b in zip(e_dev, bound))))
    assert np.isfinite(got["step"]).all() and np.isfinite(got["cov"]).all(), (dev.N, name)
    for what, e, b in zip(WHAT, e_dev, bound):
        assert e <= b, (dev.N, name, moved, what, e, b)
    return got


@pytest.mark.parametrize("N", sorted(dr.SIZES))
def test_device_dense_update_matches_extended_reference(devices, N):
    dev = devices(N)
    for n_, name, moved in dr.cases():
        if n_ != N:
            continue
        W = dr.prior(name, N)
        got = _check(dev, name, moved, W)
        cov = got["cov"]
        assert np.array_equal(cov, cov.T), (N, name)                  # k_ttt stores both mirror images
        assert (np.diag(cov) > 0).all(), (N, name)
        assert np.array_equal(got["prior"], W), (N, name)


@pytest.mark.parametrize("N", sorted(dr.SIZES))
def test_both_factorisation_forms_give_the_same_bits(devices, N):
    """chol_flow 0 and 1 at the new sizes, with the kappa = 1e8 prior"""
    dev = devices(N)
    W = dr.prior(dr.FLOW_PRIOR, N)
    X, X0 = dr.states(N, True)
    out = []
    for mode in (1, 0):
        dev.R.tune("chol_flow", mode)
        out.append(dev.update(W, X, X0))
    dev.R.tune("chol_flow", 1)
    assert np.isfinite(out[0]["step"]).all()
    assert np.array_equal(out[0]["step"], out[1]["step"]) and np.array_equal(out[0]["cov"], out[1]["cov"])


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", sorted(dr.INDEFINITE))
def test_indefinite_prior_with_positive_diagonal_is_refused(devices, name, mode):
    """Only the elimination can notice these (dense_ref.INDEFINITE): update_run raises, the step-wise calls never return
    a finite step, and the handle then does an ordinary update to the bar."""
    N, make = dr.INDEFINITE[name]
    dev = devices(N)
    R = dev.R
    R.tune("chol_flow", mode)
    try:
        bad = make(4 * N)
        X, X0 = dr.states(N, False)
        R.update_frame(*dev.obs)
        with pytest.raises(FloatingPointError):
            R.update_run(bad, X0, *dev.obs, 3, 1e-4)
        try:
            step = dev.update(bad, X, X0)["step"]
        except FloatingPointError:
            step = None
        assert step is None or not np.isfinite(step).all()
        _check(dev, dr.GOOD_PRIOR, False)
    finally:
        R.tune("chol_flow", 1)


@pytest.mark.parametrize("name", dr.NEAR_SINGULAR)
def test_near_singular_prior_is_refused_or_solved_to_the_bar(devices, name):
    """kappa(W) = 1e15, 1e16, positive definite as stored: either FloatingPointError, or finite numbers inside the bar;
    never non-finite numbers handed back as a result."""
    N = dr.NEAR_SINGULAR_N
    dev = devices(N)
    W = dr.prior(name, N)
    X, X0 = dr.states(N, False)
    dev.R.update_frame(*dev.obs)
    try:
        Xk, info, errs, Hzc, gains, tok = dev.R.update_run(W, X0, *dev.obs, 1, 1e-4)
    except FloatingPointError:
        return
    assert np.isfinite(Xk).all() and np.isfinite(tok.fetch()).all()
    _check(dev, name, False, W, refine=0)          # see dense_ref.reference
