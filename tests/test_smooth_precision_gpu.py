"""The backward pass of the RTS smoother on the device (hm_smooth_run: k_fw_rows / k_pft_cols, k_flow_fill / k_chol_flow,
k_sm_trmv / k_sm_mvt, the four k_sm_gemm products) against the extended-precision reference
smooth_ref.smooth_ld: at the block-structure edges of 4N, with ill-conditioned and badly scaled priors, weak measurements
and a small eps_F, in measures taken where the smoother works -- the correction xs_k - x_k whitened by sqrt(diag Ps_k), by
halves, and Ps_k scaled to a unit diagonal (tests/smooth_cases.py: the table, the records and the bar).

The bar, per case, frame and measure: 8 x max(e_numpy, u kappa) -- e_numpy the error of tests/smooth_ref.smooth in
binary64 against the same reference, u = 2^-53, kappa the largest kappa_2 over the steps of Pp scaled to a unit diagonal.
hm_smooth_prior, a product, has the componentwise bar of smooth_cases.prior_bound, c_p u (|F| |P| |F|^T + Weps) with
c_p = 2 d_max + 11 (d_max the largest vertex degree of the mesh, the length of the longest sum in k_fw_rows /
k_pft_cols) and |F| taken spring by spring, as the kernels sum it; both derived there.  What the device
measured against both is recorded in profiles/smooth_precision.md (tools/smooth_precision_table.py).

A chosen record is put on the device with Renderer.update_run(P_k, m_k, ..., max_iter = 0), which keeps the prior as the
resident covariance and m_k as the prior mean, then RTSSmoother.record(x_k); every test first checks that fetch() hands
back P_k, x_k, m_k bit for bit."""
import numpy as np
import pytest

import dense_ref as dr
import smooth_cases as sc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not dr.available(), reason=dr.SKIP_REASON)]


@pytest.fixture(scope="module")
def devices(hm):
    """one Renderer per mesh, shared by the tests of that size and closed with the module"""
    made = {}

    def get(N):
        if N not in made:
            made[N] = dr.Device(N)
        return made[N]
    yield get
    for d in made.values():
        d.R.close()


def _recorded_bit_for_bit(c):
    t = sc.track(c)

    def check(fetched):
        for k, (P, x, m) in enumerate(fetched):
            assert np.array_equal(P, t["P"][k]), (sc.label(c), k)
            assert np.array_equal(x, t["x"][k]) and np.array_equal(m, t["m"][k]), (sc.label(c), k)
    return check


def _check(dev, c):
    """one case against its bars"""
    K = sc.K
    t, r = sc.track(c), sc.reference(c)
    ref, bound = r["ref"], r["bound"]
    got = sc.run_on_device(dev, c, _recorded_bit_for_bit(c))
    e_prior, cp = sc.prior_errors(c, got)
    e_dev = sc.device_errors(c, got)
    print("%s kappa %.2e  numpy %s  device %s  ratio %s  prior (c_p = %d) %.2f of its bar, %.1e scaled" % (
        sc.label(c), ref["kappa"], " ".join("%.2e" % e for e in r["e_numpy"].max(axis=0)),
        " ".join("%.2e" % e for e in e_dev.max(axis=0)), " ".join("%.2f" % v for v in (e_dev / r["base"]).max(axis=0)),
        cp, max(e[0] for e in e_prior), max(e[1] for e in e_prior)))
    # the prediction: a product, componentwise
    for k in range(1, K):
        assert np.isfinite(got["prior"][k]).all(), (sc.label(c), k)
        assert e_prior[k - 1][0] <= 1.0, (sc.label(c), "Pp", k, e_prior[k - 1])
    # the invariants of the two runs
    xs, var, Ps = got["xs"], got["var"], got["Ps"]
    assert got["var0"] is None and np.isfinite(xs).all() and np.isfinite(var).all()
    assert np.array_equal(got["xs0"], xs), sc.label(c)                       # mean-only and full runs: the same bits
    assert np.array_equal(xs[K - 1], t["x"][K - 1]), sc.label(c)             # the last frame is the filter's
    assert np.array_equal(Ps[K - 1], t["P"][K - 1]), sc.label(c)
    for k in range(K):
        assert np.array_equal(Ps[k], Ps[k].T), (sc.label(c), k)              # exactly symmetric
        assert np.array_equal(np.diag(Ps[k]), var[k]), (sc.label(c), k)
    # accuracy, per frame
    for k in range(K - 1):
        for what, e, b in zip(sc.WHAT, e_dev[k], bound[k]):
            assert e <= b, (sc.label(c), k, what, e, b)
        b = bound[k][2]
        d = 1 / np.asarray(np.sqrt(np.diag(ref["Ps"][k])), np.float64)
        lam = np.linalg.eigvalsh(Ps[k] * np.outer(d, d))[0]
        assert lam >= -b, (sc.label(c), k, lam, b)                           # positive semi-definite to the bar
        assert np.all(np.diag(Ps[k]) <= np.diag(t["P"][k]) * (1 + b)), (sc.label(c), k)   # smoothing adds no uncertainty
    return got


@pytest.mark.parametrize("N", sorted(sc.SIZES))
def test_device_smoother_matches_extended_reference(devices, N):
    dev = devices(N)
    for c in sc.cases_of(N):
        _check(dev, c)


def test_non_finite_prediction_fails_loudly_and_leaves_record_and_renderer_usable(devices):
    """A mass-spring record whose last-but-one frame has two vertices joined by a bar in one place: that spring's block
    is not finite, so Pp of the last frame is not.  run() raises FloatingPointError naming the last frame; without
    covariances it leaves the record as it was and the Renderer usable (an update, and a second smoother on it that
    meets its bar); with covariances it raises as well, and the record is then consumed as include/hydra_mi.h says:
    record, run and prior are refused, fetch still hands back x_k and m_k.

    Why no wait of k_chol_flow can hang on a non-finite Pp: a consumer waits for the fill pattern to go away, a quiet NaN
    with a payload no arithmetic produces (a computed NaN is the canonical one or carries the payload of an operand, and
    the operands here are canonical), so every block the chain or a task stores ends the wait for it whatever its
    values; and every wait counts its polls and gives up (ctl[1], HM_ERR_HIP)."""
    from hydra_mi.smooth import RTSSmoother
    c = sc.BENIGN
    K, N = sc.K, c.N
    dev = devices(N)
    t = sc.track(c)
    bars = sc.model(c)[0]
    a, b = (int(v) for v in bars[0])
    x_bad = t["x"].copy()
    x_bad[K - 2, 2 * b:2 * b + 2] = x_bad[K - 2, 2 * a:2 * a + 2]
    named = "frame %d " % (K - 1)
    with RTSSmoother(sc.filter_stand_in(c, dev.R), K) as sm:
        sc.record(dev, sm, t["P"], x_bad, t["m"])
        before = [sm.fetch(k) for k in range(K)]
        for k in range(K):
            assert np.array_equal(before[k][0], t["P"][k]) and np.array_equal(before[k][1], x_bad[k])
            assert np.array_equal(before[k][2], t["m"][k])
        with pytest.raises(FloatingPointError, match=named):
            sm.run(covariances=False)
        assert len(sm) == K
        for k in range(K):
            assert all(np.array_equal(u, v) for u, v in zip(sm.fetch(k), before[k])), k
        # the Renderer: an ordinary update with a good prior
        X, X0 = dr.states(N, False)
        Xk, info, errs, Hzc, gains, tok = dev.R.update_run(dr.prior(dr.GOOD_PRIOR, N), X0, *dev.obs, 3, 1e-4)
        assert info["niter"] >= 1 and np.isfinite(Xk).all() and np.isfinite(tok.fetch()).all()
        # a second smoother on the same Renderer, a good record: to its bar
        _check(dev, c)
        # the first one is still what it was, and fails the same way with covariances
        for k in range(K):
            assert all(np.array_equal(u, v) for u, v in zip(sm.fetch(k), before[k])), k
        with pytest.raises(FloatingPointError, match=named):
            sm.run(covariances=True)
        # consumed
        assert len(sm) == K
        with pytest.raises(RuntimeError, match="smoothed with covariances"):
            sm.record(t["x"][0])
        with pytest.raises(RuntimeError, match="smoothed with covariances"):
            sm.run(covariances=False)
        with pytest.raises(RuntimeError, match="smoothed with covariances"):
            sm.prior(1)
        for k in range(K):
            P, x, m = sm.fetch(k)
            assert np.array_equal(x, x_bad[k]) and np.array_equal(m, t["m"][k]), k
        assert np.array_equal(sm.fetch(K - 1)[0], t["P"][K - 1])             # (the last slot is never written)
