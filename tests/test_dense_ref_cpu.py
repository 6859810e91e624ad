"""The extended-precision reference of the dense update (tests/dense_ref.py) on its own, and the conditions its case
table has to meet before tests/test_dense_precision_gpu.py may hold the device to it.  Synthetic sparse positive
semi-definite matrices stand in for HTH (dense_ref.synthetic_hth); no GPU."""
import numpy as np
import pytest

import dense_ref as dr

pytestmark = pytest.mark.skipif(not dr.available(), reason=dr.SKIP_REASON)

_REF = {}


def _case(N, name, moved):
    """reference, comparator errors, bounds of one case of the table; computed once"""
    key = (N, name, moved)
    if key not in _REF:
        HTH, Hz = dr.synthetic_hth(N)
        X, X0 = dr.states(N, moved)
        W = dr.prior(name, N)
        ref = dr.reference(W, HTH, Hz, X0, X)
        e_lapack = dr.errors(dr.lapack(W, HTH, Hz, X0, X), ref)
        _REF[key] = (ref, e_lapack, dr.bounds(ref, e_lapack))
    return _REF[key]


def _kappa(W):
    """kappa_2 of a symmetric positive definite W: its largest eigenvalue times the largest of its longdouble inverse"""
    inv = np.asarray(dr.chol_inverse_ld(W)[0], np.float64)
    return np.linalg.eigvalsh(W)[-1] * np.linalg.eigvalsh((inv + inv.T) / 2)[-1]


def test_table_covers_what_the_issue_lists():
    assert sorted(dr.SIZES) == [5, 8, 9, 16, 17, 24, 32, 33, 50]
    assert len(dr.cases()) == len(dr.SIZES) * (len(dr.PRIORS) + 1)
    assert sum(1 for c in dr.cases() if c[2]) == len(dr.SIZES)
    assert dr.MOVED_PRIOR in dr.PRIORS and dr.FLOW_PRIOR in dr.PRIORS and dr.GOOD_PRIOR in dr.PRIORS


@pytest.mark.parametrize("N", sorted(dr.SIZES))
def test_sizes_have_the_block_structure_they_claim(N):
    n4, rem, _ = dr.SIZES[N]
    assert n4 == 4 * N and n4 % dr.DNB == rem
    m = dr.mesh_n(N)
    assert m.size() == N and m.p.shape == (N, 2)
    assert np.array_equal(np.unique(m.t), np.arange(N))                       # every vertex is used
    assert np.bincount(m.t.reshape(-1)).max() < dr.EKF_MAX_STAR
    assert m.p.min() > 2.0 and m.p.max() < dr.SIDE - 4.0                      # inside the frame, the observation's shift too
    import update_cases
    assert (update_cases.doubled_areas(m.p.reshape(-1), m.t) > 1.0).all()    # one orientation, no sliver
    assert dr.mesh_n(N) is m
    if N == 24:
        assert n4 // dr.DNB == dr.TTT_PF
    if N == 32:
        assert n4 == dr.TV_ROWS
    if N == 33:
        assert dr.TV_ROWS < n4 <= dr.TV_ROWS + 4


@pytest.mark.parametrize("N", [5, 17, 50])
@pytest.mark.parametrize("kappa", [1.0, 1e4, 1e8, 1e11])
def test_spectrum_has_the_condition_number_asked_for(N, kappa):
    W = dr.spectrum(4 * N, kappa)
    assert np.array_equal(W, W.T) and np.array_equal(W, dr.spectrum(4 * N, kappa))
    assert abs(_kappa(W) / kappa - 1.0) <= 0.01


@pytest.mark.parametrize("s", [1e-4, 1e4])
def test_scaled_prior_is_the_spectrum_between_two_scalings(s):
    n = 68
    W, S = dr.scaled(n, 1e4, s), dr.spectrum(n, 1e4)
    d = np.concatenate((np.ones(n // 2), np.full(n // 2, s)))
    assert np.array_equal(W, W.T)
    assert np.allclose(W / np.outer(d, d), S, rtol=1e-14, atol=0.0)
    assert np.diag(W)[n // 2:].mean() / np.diag(W)[:n // 2].mean() == pytest.approx(s * s, rel=0.5)


@pytest.mark.parametrize("N", [5, 33])
def test_filter_like_prior_is_dense_and_couples_positions_with_velocities(N):
    W = dr.filter_like(N)
    n2 = 2 * N
    assert np.array_equal(W, W.T) and np.linalg.eigvalsh(W)[0] > 0
    assert np.count_nonzero(W[:n2, n2:]) > n2                                  # more than a diagonal of couplings
    c = W[:n2, n2:] / np.sqrt(np.outer(np.diag(W)[:n2], np.diag(W)[n2:]))
    assert np.abs(np.diag(c)).min() > 0.3                                      # a vertex's position follows its velocity
    off = W - np.diag(np.diag(W))
    assert np.count_nonzero(off[:n2, :n2]) > 0                                 # and the springs tie vertices together


def test_chol_inverse_is_an_inverse_and_refines():
    W = dr.spectrum(68, 1e8)
    raw, fine = dr.chol_inverse_ld(W)
    assert raw.dtype == np.longdouble and fine.dtype == np.longdouble
    eye = np.eye(68, dtype=np.longdouble)
    Wl = W.astype(np.longdouble)
    assert np.abs(Wl @ raw - eye).max() <= 2.0 ** -64 * 1e8 * 68
    # a Newton-Schulz step forms its residual in the same longdouble, so it cannot beat u kappa either: the refined
    # inverse is a second estimate at that level, and the distance between the two is the reference's uncertainty
    assert 0 < np.abs(fine - raw).max() <= 2.0 ** -64 * 1e8 * 68 * np.abs(raw).max()
    assert np.array_equal(fine, fine.T)
    # against binary64 LAPACK: agreement at binary64's own level, u kappa
    assert np.abs(np.asarray(fine, np.float64) - np.linalg.inv(W)).max() <= 68 * dr.U * 1e8 * np.abs(np.linalg.inv(W)).max()


def test_reference_solves_what_it_says():
    N = 9
    HTH, Hz = dr.synthetic_hth(N)
    X, X0 = dr.states(N, True)
    W = dr.prior("spectrum_1e4", N)
    ref = dr.reference(W, HTH, Hz, X0, X)
    A = np.asarray(ref["A"], np.float64)
    assert np.allclose(A, np.linalg.inv(W) + HTH, rtol=1e-9)
    assert np.allclose(A @ np.asarray(ref["step"], np.float64), Hz - HTH @ (X0 - X), rtol=1e-8, atol=1e-8 * np.abs(Hz).max())
    d = np.sqrt(np.diag(A))
    assert ref["kappa"] == pytest.approx(np.linalg.cond(A / np.outer(d, d)), rel=1e-6)
    # the measures: zero for the reference itself, and a planted error comes out at its size in the small block too
    assert dr.errors(dict(step=ref["step"], cov=ref["cov"]), ref) == (0.0, 0.0, 0.0)
    x = np.asarray(ref["step"], np.float64).copy()
    x[2 * N:] *= 1 + 1e-6
    ep, ev = dr.step_err(x, ref)
    assert ep <= 1e-15 and ev == pytest.approx(1e-6, rel=1e-3)
    C = np.asarray(ref["cov"], np.float64).copy()
    k = int(np.argmin(np.diag(C)))
    C[k, k] *= 1 + 1e-6
    assert dr.cov_err(C, ref) == pytest.approx(1e-6, rel=1e-3)


@pytest.mark.parametrize("N", sorted(dr.SIZES))
def test_reference_is_a_hundred_times_surer_than_the_bound(N):
    """A condition on the case table: the reference's own uncertainty (raw against refined) is at most 1/100 of the
    bound the GPU test applies, in every measure, and the comparator is inside that bound."""
    for n_, name, moved in dr.cases():
        if n_ != N:
            continue
        ref, e_lapack, bound = _case(N, name, moved)
        for what, unc, e, b in zip(("step positions", "step velocities", "covariance"), dr.uncertainty(ref), e_lapack, bound):
            assert np.isfinite(b) and b > 0
            assert unc <= b / 100.0, (N, name, moved, what, unc, b)
            assert e <= b, (N, name, moved, what, e, b)


@pytest.mark.parametrize("name", sorted(dr.INDEFINITE))
def test_indefinite_priors_have_a_positive_diagonal_and_no_factor(name):
    N, make = dr.INDEFINITE[name]
    W = make(4 * N)
    assert np.array_equal(W, W.T) and np.diag(W).min() > 0 and np.linalg.eigvalsh(W)[0] < 0
    with pytest.raises(FloatingPointError):
        dr.chol_inverse_ld(W)
    if name.startswith("pair"):
        i, j = np.argwhere(np.triu(W, 1) != 0)[0]
        nb = -(-4 * N // dr.DNB)
        block = {"pair_first_block": 0, "pair_middle_block": nb // 2}.get(name, nb - 1)
        assert i // dr.DNB == block and j // dr.DNB == block and 0 < block + 1 <= nb
        if "last_strip" in name:
            assert (i, j) == (4 * N - 2, 4 * N - 1) and 4 * N % dr.DNB == 4


@pytest.mark.parametrize("name", dr.NEAR_SINGULAR)
def test_near_singular_priors_are_definite_as_stored(name):
    """what the device is given is still positive definite in extended precision, so a reference exists"""
    W = dr.prior(name, dr.NEAR_SINGULAR_N)
    assert np.diag(W).min() > 0
    assert _kappa(W) > 1e14
    dr.chol_inverse_ld(W)


def test_non_finite_matrix_is_refused():
    W = np.eye(8)
    W[7, 7] = np.nan
    with pytest.raises(FloatingPointError):
        dr.chol_inverse_ld(W)
