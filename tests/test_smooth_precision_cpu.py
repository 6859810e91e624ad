"""The extended-precision reference of the RTS smoother (smooth_ref.smooth_ld) on its own, and the conditions the case
table of tests/smooth_cases.py has to meet before tests/test_smooth_precision_gpu.py may hold the device to it.  No GPU."""
import numpy as np
import pytest

import dense_ref as dr
import smooth_cases as sc
import smooth_ref

pytestmark = pytest.mark.skipif(not dr.available(), reason=dr.SKIP_REASON)

LD = np.longdouble
TOL_STEP = 1e-10        # the Frobenius bound of tests/test_smooth_gpu.py, which the planted error has to pass


def _rel(a, b):
    """the measure of tests/test_smooth_gpu.py"""
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def test_table_covers_what_the_issue_lists():
    assert sorted(sc.SIZES) == [5, 8, 9, 17, 24, 33, 50, 65]
    assert len(set(sc.CASES)) == len(sc.CASES) and sc.BENIGN in sc.CASES
    for N in sc.SIZES:
        mine = sc.cases_of(N)
        assert any(c.prior == "spectrum_1e4" for c in mine), N
        assert any(c.prior in sc.ILL for c in mine), N
    assert len(sc.cases_of(50)) == 2 and len(sc.cases_of(65)) == 2
    for p in dr.PRIORS:
        assert sum(c.prior == p for c in sc.CASES) >= 2, p
    for h in (1.0, 1e-6):
        assert sum(c.h == h for c in sc.CASES) >= 2, h
    for e in (1e-1, 1e-6):
        assert sum(c.eps_F == e for c in sc.CASES) >= 2, e
    for s in (True, False):
        assert sum(c.springs == s for c in sc.CASES) >= 2, s
    assert all(c.h in (1.0, 1e-6) and c.eps_F in (1e-1, 1e-6) and c.prior in dr.PRIORS for c in sc.CASES)


def test_sizes_have_the_structure_they_claim():
    n4 = {N: 4 * N for N in sc.SIZES}
    assert n4[5] < dr.DNB and n4[8] == dr.DNB and n4[9] == dr.DNB + 4
    assert n4[17] == 2 * dr.DNB + 4 and n4[24] == dr.TTT_PF * dr.DNB
    assert dr.TV_ROWS < n4[33] <= dr.TV_ROWS + 4
    assert n4[50] // dr.DNB >= 6
    assert 256 < n4[65] <= 256 + 4                    # k_sm_trmv: j = t + 256 exists for t < 4; k_sm_mvt: 2 workgroups
    m = dr.mesh_n(65)
    assert m.size() == 65 and np.array_equal(np.unique(m.t), np.arange(65))
    for N in sc.SIZES:
        bars = sc.model(sc.Case(N, "spectrum_1", 1.0, 1e-1, True))[0]
        assert bars.min() == 0 and bars.max() == N - 1 and np.all(bars[:, 0] != bars[:, 1])


@pytest.mark.parametrize("N", sorted(sc.SIZES))
def test_records_are_what_a_filter_would_leave(N):
    """every stored P_k is symmetric with a positive diagonal, every Pp_k has a longdouble Cholesky factor, and the model
    the comparator and the reference use is the one the device is given"""
    for c in sc.cases_of(N):
        t = sc.track(c)
        bars, l0, kappa, a, s, eps_F = sc.model(c)
        assert t["x"].shape == t["m"].shape == (sc.K, 4 * N) and len(t["P"]) == sc.K and len(t["F"]) == sc.K - 1
        for k in range(sc.K):
            P = t["P"][k]
            assert P.dtype == np.float64 and np.array_equal(P, P.T) and np.diag(P).min() > 0, (sc.label(c), k)
            assert np.isfinite(t["x"][k]).all() and np.isfinite(t["m"][k]).all()
        for k in range(sc.K - 1):
            assert np.array_equal(t["F"][k], smooth_ref.model_F(N, bars, l0, kappa, a, s, t["x"][k]))
            assert np.array_equal(t["m"][k + 1], t["F"][k] @ t["x"][k])
            Pp = sc.reference(c)["ref"]["Pp"][k + 1]
            dr.chol_inverse_ld(Pp, refine=0)           # FloatingPointError where there is no factor
        assert np.array_equal(t["Q"], smooth_ref.Weps(N, eps_F))
        if not c.springs:
            assert len(bars) == 0 and (a, s) == (1.0, 0.0)
            assert np.array_equal(t["F"][0], smooth_ref.F_matrix(N, 1.0, 0.0))


@pytest.mark.parametrize("N", sorted(sc.SIZES))
def test_reference_is_sixteen_times_surer_than_the_bar(N):
    """A condition on the case table: the reference's own uncertainty (its raw recursion against its refined one) is at
    most 1/16 of the bar, per frame and in every measure; the comparator is inside the bar by construction.  A case that
    misses this is replaced in the table (smooth_cases.CASES names the one that was); the cap stays."""
    for c in sc.cases_of(N):
        r = sc.reference(c)
        assert np.isfinite(r["bound"]).all() and (r["bound"] > 0).all()
        assert r["ref"]["kappa"] == max(r["ref"]["kappas"][:sc.K - 1]) and r["ref"]["kappas"][sc.K - 1] is None
        for k in range(sc.K - 1):
            for what, unc, e, b in zip(sc.WHAT, r["unc"][k], r["e_numpy"][k], r["bound"][k]):
                assert unc <= b / 16.0, (sc.label(c), k, what, unc, b)
                assert e <= b, (sc.label(c), k, what, e, b)


@pytest.mark.parametrize("N", sorted(sc.SIZES))
def test_corrections_are_not_small(N):
    """the relative mean measure divides by the whitened correction: its RMS is at least 1e-2 in every frame k < K-1"""
    for c in sc.cases_of(N):
        t, ref = sc.track(c), sc.reference(c)["ref"]
        for k in range(sc.K - 1):
            rms = smooth_ref.whitened_correction_rms(t["x"][k], ref["xs"][k], ref["Ps"][k])
            assert rms >= 1e-2, (sc.label(c), k, rms)


def test_measures_are_zero_for_the_reference_and_see_a_planted_error_at_its_size():
    t, r = sc.track(sc.BENIGN), sc.reference(sc.BENIGN)
    ref = r["ref"]
    assert np.array_equal(smooth_ref.errors(ref["xs"], ref["Ps"], t["x"], ref), np.zeros((sc.K - 1, 3)))
    n = t["x"].shape[1]
    k = 1
    C = np.asarray(ref["Ps"][k], np.float64).copy()
    i = int(np.argmin(np.diag(C)))
    C[i, i] *= 1 + 1e-6
    assert smooth_ref.cov_err(C, ref["Ps"][k]) == pytest.approx(1e-6, rel=1e-3)
    xs = ref["xs"][k].copy()
    xs[:n // 2] += 1e-6 * (ref["xs"][k][:n // 2] - t["x"][k][:n // 2])
    ep, ev = smooth_ref.mean_err(xs, t["x"][k], ref["xs"][k], ref["Ps"][k])
    assert ep == pytest.approx(1e-6, rel=1e-6) and ev == 0.0


def test_new_mean_measure_sees_what_the_frobenius_norm_does_not():
    """The reference result with a relative perturbation of 1e-9 planted in the velocity half of the correction, rounded
    to binary64 as a device would hand it back: it fails the bar of the mean measure in every frame and passes today's
    check of tests/test_smooth_gpu.py, _rel(xs, xs_ref) <= TOL_STEP, with room to spare."""
    t, r = sc.track(sc.BENIGN), sc.reference(sc.BENIGN)
    ref, (xs_np, _) = r["ref"], r["numpy"]
    n = t["x"].shape[1]
    for k in range(sc.K - 1):
        xl = np.asarray(t["x"][k], LD)
        c = ref["xs"][k] - xl
        c[n // 2:] *= 1 + LD(1e-9)
        planted = np.asarray(xl + c, np.float64)
        ep, ev = smooth_ref.mean_err(planted, t["x"][k], ref["xs"][k], ref["Ps"][k])
        assert ev > r["bound"][k][1], (k, ev, r["bound"][k][1])          # fails the new bar ...
        assert ev == pytest.approx(1e-9, rel=0.05)
        assert ep <= r["bound"][k][0]                                      # ... in the half it was planted in only
        old = _rel(planted, xs_np[k])
        assert old <= TOL_STEP / 10, (k, old)                              # ... and passes the old one with room


def test_smooth_ld_agrees_with_the_binary64_restatement_on_the_benign_case():
    """A consistency check of smooth_ld against smooth_ref.smooth (pinned by tests/test_smooth_cpu.py): in the Frobenius
    measure to n u kappa; in the new measures to n (u kappa + the rounding of xs_k itself to binary64, which in the
    measure of the correction is u |d x_k| / |d c_k|) -- the level e_numpy sits at."""
    c = sc.BENIGN
    t, r = sc.track(c), sc.reference(c)
    ref, (xs, Ps) = r["ref"], r["numpy"]
    n = 4 * c.N
    assert ref["xs"].dtype == LD and all(p.dtype == LD for p in ref["Ps"])
    assert ref["kappa"] < 1e5
    assert np.array_equal(np.asarray(ref["xs"][sc.K - 1], np.float64), t["x"][sc.K - 1])
    assert np.array_equal(np.asarray(ref["Ps"][sc.K - 1], np.float64), t["P"][sc.K - 1])
    for k in range(sc.K - 1):
        assert _rel(xs[k], np.asarray(ref["xs"][k], np.float64)) <= n * dr.U * ref["kappa"]
        assert _rel(Ps[k], np.asarray(ref["Ps"][k], np.float64)) <= n * dr.U * ref["kappa"]
        d = 1 / np.sqrt(np.diag(ref["Ps"][k]))
        xl = np.asarray(t["x"][k], LD)
        for half, e in zip((slice(0, n // 2), slice(n // 2, None)), r["e_numpy"][k][:2]):
            floor = float(np.linalg.norm(np.asarray(d[half] * xl[half], np.float64)) /
                          np.linalg.norm(np.asarray(d[half] * (ref["xs"][k][half] - xl[half]), np.float64)))
            assert e <= n * dr.U * (ref["kappa"] + floor), (k, e, floor)
        assert r["e_numpy"][k][2] <= n * dr.U * ref["kappa"]
        # the steps the reference reports are the ones the comparator took
        Pp = np.asarray(ref["Pp"][k + 1], np.float64)
        assert _rel(smooth_ref.smooth(t["P"], t["x"], t["m"], t["F"], t["Q"])[2][k]["Pp"], Pp) <= n * dr.U


def test_prior_bound_holds_for_the_comparator():
    """the componentwise bar of hm_smooth_prior (smooth_cases.prior_bound) against binary64 numpy's F P F^T + Weps, whose
    sums are longer than the device's (two products of 4N terms each: 2 x 4N u in place of c_p u): inside it with the
    mass-spring model and without"""
    for c in (sc.BENIGN, sc.Case(8, "scaled_1e4_1e4", 1.0, 1e-1, False)):
        t, ref = sc.track(c), sc.reference(c)["ref"]
        cp, B = sc.prior_bound(c, t["x"][0], t["P"][0], t["Q"])
        assert cp == 2 * sc.max_degree(c) + 11 and (B > 0).all()
        Pp = t["F"][0] @ t["P"][0] @ t["F"][0].T + t["Q"]
        assert np.all(np.abs(np.asarray(Pp, LD) - ref["Pp"][1]) <= 2 * 4 * c.N * B / cp)
