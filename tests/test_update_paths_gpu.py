"""hm_update_run at each of its four doors (tests/update_cases.py) against oracle/ekf_ref.iekf_update, whose results
tests/golden/update_paths.npz holds (tools/make_update_golden.py; tests/test_update_cases_cpu.py holds the cases to their
names and their decisions to margins far wider than the ~1e-9 by which device and oracle iterates differ).

Three kinds of statement:
  * against the oracle: the decisions exactly, the integer error sums exactly, flow sums to 1e-10, state and covariance
    kept in the relative 2-norm, the gains componentwise against W_kept @ Hzc in extended precision;
  * exact identities between device runs: what a door keeps, bit for bit, is what a shorter run of the same case keeps;
    no knob, and no way of fetching a result, changes a bit;
  * the handle afterwards: a second update on the same handle equals that update on a fresh handle, bit for bit -- what a
    reference render, iterate buffer or factor slot left swapped by a speculative measurement taken back would break.
"""
import ctypes
import os

import numpy as np
import pytest

import update_cases as uc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
GOLD = uc.load_golden(os.path.join(os.path.dirname(__file__), "golden", uc.GOLDEN))
U = 2.0 ** -53

# Relative 2-norm bounds of the state and the covariance kept: the bars of one update
# (test_plain_kalman_filter_update_on_device).  No case needs more: measured on the MI355X, the worst case of
# tests/update_cases.py is 2.2e-16 for the state and 1.6e-15 for the covariance (condition numbers up to 1959).
STATE_TOL = 1e-8
COV_TOL = 1e-7


class _State:
    def __init__(self, X):
        self.X = np.asarray(X, np.float64).reshape(-1, 1)


def _renderer(case):
    from hydra_mi import renderer
    m, n = case["mesh"], case["n"]
    return renderer.Renderer(m, np.zeros((m.size(), 2)), np.zeros((n, n, 2), np.float32), n, case["tex"], True,
                             *case["eps"])


def _flow_arg(case, flow, y_m):
    from hydra_mi import renderer
    return renderer.MaskedFlow(flow, y_m) if case["masked"] else flow


def _last_error(R, X):
    """hm_update_last_error -> (return code, the four sums)"""
    from hydra_mi import _lib
    err = (ctypes.c_double * 4)()
    x = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
    rc = _lib.lib().hm_update_last_error(R._h, _lib.ptr(x), err)
    assert rc in (0, 1), rc
    return rc, np.array(err[:])


def _run(case, R, W=None, X0=None, obs=None, max_iter=None, reltol=None, how="tail"):
    """One hm_update_run -> dict(X, info, errs, Hzc, gains, W, last).  how: 'tail' (gains with the call, covariance left on
    the device and fetched), 'lazy' (tail=False + update_tail()), 'w_out' (the C call with a W_out buffer)."""
    from hydra_mi import _lib
    y_im, flow, y_m = obs if obs is not None else (case["y_im"], case["flow"], case["y_m"])
    W = case["W"] if W is None else W
    X0 = case["X0"] if X0 is None else X0
    max_iter = case["max_iter"] if max_iter is None else max_iter
    reltol = case["reltol"] if reltol is None else reltol
    fa = _flow_arg(case, flow, y_m)
    if how == "w_out":
        n4 = 4 * R.n
        masked = R._masked_flag(y_im, fa, y_m)
        Wp = R._cov_arg(W, "update_run")
        X = np.ascontiguousarray(np.asarray(X0, np.float64).reshape(-1)).copy()
        info = (ctypes.c_int * 4)()
        errs = np.zeros((max(max_iter, 1), 4))
        Hzc, gains, Wk = np.empty((n4, 4)), np.empty((3, n4)), np.empty((n4, n4))
        _lib.check(_lib.lib().hm_update_run(R._h, _lib.ptr(Wp), _lib.ptr(X), float(case["deltaX"]), masked, int(max_iter),
                                            float(reltol), info, _lib.ptr(errs), _lib.ptr(Hzc), _lib.ptr(gains),
                                            _lib.ptr(Wk)), "hm_update_run")
        R._cov_serial += 1
        inf = dict(niter=info[0], accepted=info[1], reverted=bool(info[2]), converged=bool(info[3]))
        last = _last_error(R, X)
        return dict(X=X, info=inf, errs=errs[:info[0]].copy(), Hzc=Hzc, gains=gains, W=Wk, W_dev=R.cov_fetch(), last=last)
    X, info, errs, Hzc, gains, tok = R.update_run(W, X0, y_im, fa, y_m, max_iter, reltol, deltaX=case["deltaX"],
                                                  fetch=False, tail=(how != "lazy"))
    last = _last_error(R, X)
    if how == "lazy":
        Hzc, gains = R.update_tail()
    Wk = tok.fetch()
    return dict(X=X.reshape(-1), info=info, errs=errs.copy(), Hzc=Hzc, gains=gains, W=Wk, W_dev=R.cov_fetch(), last=last,
                tok=tok)


def _same_bits(a, b, what=""):
    assert a["info"] == b["info"], what
    for k in ("X", "errs", "W", "Hzc", "gains"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["last"][0] == b["last"][0] and np.array_equal(a["last"][1], b["last"][1]), what


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


@pytest.mark.parametrize("name", uc.NAMES)
def test_door_against_the_oracle(hm, name):
    case, g = uc.build(name), GOLD[name]
    R = _renderer(case)
    n4 = 4 * R.n
    r = _run(case, R)
    niter, accepted, reverted, converged = (int(v) for v in g["info"])
    # the decisions
    assert r["info"] == dict(niter=niter, accepted=accepted, reverted=bool(reverted), converged=bool(converged))
    # the error sums of the accepted rounds: image and mask sums whole numbers, flow sums reductions of binary32 terms
    e = r["errs"][:accepted]
    assert np.array_equal(e[:, [0, 3]], g["errs"][:, [0, 3]])
    if accepted:
        flow_rel = float(np.max(np.abs(e[:, 1:3] - g["errs"][:, 1:3]) / g["errs"][:, 1:3]))
        print("%s: flow sums rel %.3g" % (name, flow_rel))
        assert flow_rel <= 1e-10
    # state and covariance kept
    sx, sw = _rel(r["X"], g["X_kept"]), _rel(r["W"], g["W_kept"])
    cond = float(max(g["cond_A"].max(), g["cond_prior"]))
    print("%s: state rel %.3g  covariance rel %.3g  cond %.4g  cond * 2^-53 %.3g" % (name, sx, sw, cond, cond * U))
    assert sx <= STATE_TOL
    assert sw <= COV_TOL
    # read back after the run: the resident covariance is the one kept
    assert np.array_equal(r["W_dev"], r["W"])
    # Hz components: those of the oracle's last measurement (the flipped round's on a revert, kalman.py:826-830)
    hz_rel = _rel(r["Hzc"], g["Hzc_last"])
    print("%s: Hzc rel %.3g" % (name, hz_rel))
    assert hz_rel <= 1e-9
    # gains: k_gains alone, against the device's own covariance and components in extended precision; the bound is the
    # textbook one for a dot product of length 4N in any order (and one more rounding for c1 + c2)
    Wl, c = r["W"].astype(np.longdouble), r["Hzc"].astype(np.longdouble)
    cols = (c[:, 0], r["Hzc"][:, 1].astype(np.longdouble) + c[:, 2], c[:, 3])
    for k, ck in enumerate(cols):
        ref = Wl @ ck
        bound = 2 * n4 * U * (np.abs(Wl) @ np.abs(ck))
        assert np.all(np.abs(r["gains"][k].astype(np.longdouble) - ref) <= bound), (name, k)
        assert np.any(r["gains"][k] != 0)
    assert _rel(r["gains"], g["gains"]) <= 1e-6            # (and they are the oracle's gains: the right W, the right c)
    # Renderer.error of the state kept without another render: not at hand after a revert, else hm_error's numbers
    rc, err = r["last"]
    if reverted:
        assert rc == 1
    else:
        assert rc == 0
        assert err[0] == g["last_error"][0] and err[3] == g["last_error"][3]
        assert np.all(np.abs(err[1:3] - g["last_error"][1:3]) <= 1e-10 * g["last_error"][1:3])
        ref = R.error(_State(r["X"]), case["y_im"], case["flow"], case["y_m"])       # the raw flow, also when masked
        assert tuple(err) == tuple(float(v) for v in ref[:4])
        if case["masked"]:
            assert err[1] != r["errs"][-1, 1] and err[2] != r["errs"][-1, 2]


def test_revert_in_round_one_keeps_the_prior_bit_for_bit(hm):
    case = uc.build("revert_first")
    for how in ("tail", "lazy", "w_out"):
        r = _run(case, _renderer(case), how=how)
        assert r["info"] == dict(niter=1, accepted=0, reverted=True, converged=False), how
        assert np.array_equal(r["X"], case["X0"]), how
        assert np.array_equal(r["W"], case["W"]) and np.array_equal(r["W_dev"], case["W"]), how


@pytest.mark.parametrize("name", ["revert_later", "revert_later_6"])
def test_later_revert_keeps_what_the_shorter_run_keeps(hm, name):
    case = uc.build(name)
    k = case["round"]
    a = _run(case, _renderer(case))
    b = _run(case, _renderer(case), max_iter=k - 1)
    assert a["info"] == dict(niter=k, accepted=k - 1, reverted=True, converged=False)
    assert b["info"] == dict(niter=k - 1, accepted=k - 1, reverted=False, converged=False)
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["W"], b["W"]) and np.array_equal(a["W_dev"], b["W"])
    assert np.array_equal(a["errs"][:k - 1], b["errs"])


@pytest.mark.parametrize("name", ["converge_early", "masked"])
def test_early_convergence_equals_the_run_that_stops_there(hm, name):
    case = uc.build(name)
    k = case["round"]
    a = _run(case, _renderer(case))
    b = _run(case, _renderer(case), max_iter=k)
    assert a["info"] == dict(niter=k, accepted=k, reverted=False, converged=True)
    assert b["info"] == a["info"]
    _same_bits(a, b)


KNOBS = [("speculate", 0), ("tail_async", 0), ("tail_split", 0), ("chol_flow", 0), ("result_delay", 500)]


@pytest.mark.parametrize("name", uc.NAMES)
def test_no_knob_and_no_way_of_fetching_changes_a_bit(hm, name):
    """each setting against the default (speculate, tail_async, tail_split, chol_flow on, result_delay 0; gains with the
    call, covariance fetched from the device)"""
    case = uc.build(name)
    base = _run(case, _renderer(case))
    for key, value in KNOBS:
        for how in (("tail", "lazy") if key in ("tail_async", "tail_split") else ("tail",)):
            R = _renderer(case)
            R.tune(key, value)
            _same_bits(base, _run(case, R, how=how), (key, value, how))
    for how in ("lazy", "w_out"):
        _same_bits(base, _run(case, _renderer(case), how=how), how)


@pytest.mark.parametrize("spec", [1, 0])
@pytest.mark.parametrize("name", uc.NAMES)
def test_the_handle_afterwards(hm, name, spec):
    """A second, ordinary update (another frame, the posterior as the prior through the device token) on the handle that
    took the door, and on a fresh handle that was only given the state and the covariance kept."""
    from hydra_mi import _lib
    case = uc.build(name)
    y_im, flow, y_m, max_iter, reltol = case["second"]
    obs = (y_im, flow, y_m)
    R = _renderer(case)
    R.tune("speculate", spec)
    first = _run(case, R)
    # the reference render the run leaves behind (hm_jz / hm_j go on from it) is that of the state kept: after a revert the
    # point of the flipped round's measurement, at max_iter the last iterate, whose render has become the reference.
    # (After a convergence it is the point of the last measurement, which the call does not hand out.)
    Xm = None if first["info"]["converged"] else first["X"]
    F = _renderer(case)
    F.tune("speculate", spec)
    if Xm is not None:
        Xp = np.ascontiguousarray(Xm + 0.37)
        masked = 1 if case["masked"] else 0
        out = []
        for Q, init in ((R, False), (F, True)):
            if init:
                Q.update_vertex_buffer(Xm[:2 * Q.n].reshape(-1, 2), Xm[2 * Q.n:].reshape(-1, 2))
                Q.initjacobian(case["y_im"], _flow_arg(case, case["flow"], case["y_m"]), case["y_m"])
            tot, comp = ctypes.c_double(), (ctypes.c_double * 4)()
            _lib.check(_lib.lib().hm_jz(Q._h, _lib.ptr(Xp), masked, ctypes.byref(tot), comp), "hm_jz")
            out.append((tot.value,) + tuple(comp[:]))
        assert out[0] == out[1]
    a = _run(case, R, W=first["tok"], X0=first["X"], obs=obs, max_iter=max_iter, reltol=reltol)
    b = _run(case, F, W=first["W"], X0=first["X"], obs=obs, max_iter=max_iter, reltol=reltol)
    assert a["info"]["niter"] >= 1
    _same_bits(a, b)
    # and the single operators at the state now kept
    Xk = a["X"]
    st = _State(Xk)
    Xq = _State(Xk + 0.21)
    got = []
    for Q in (R, F):
        Q.update_vertex_buffer(Xk[:2 * Q.n].reshape(-1, 2), Xk[2 * Q.n:].reshape(-1, 2))
        Q.initjacobian(y_im, _flow_arg(case, flow, y_m), y_m)
        jz, comp = Q.jz(Xq)
        got.append((jz,) + tuple(comp) + (Q.j(st, case["deltaX"], 0, 1), Q.j(st, case["deltaX"], 2 * Q.n + 1, 3)))
    assert got[0] == got[1] and np.all(np.isfinite(got[0])) and got[0][0] != 0.0


@pytest.mark.parametrize("name", ["revert_later", "revert_later_6", "converge_early"])
def test_doors_through_the_python_filter(hm, name):
    """IteratedMSKalmanFilter.compute (predict -> projectmask -> update) on the inputs of a case, with the fused update and
    with the same loop in Python over hm_update_begin / _step / _cov: the door is really taken (the oracle's tracker,
    ekf_ref.Tracker, takes it on these inputs: a fold in round 2 resp. 7, convergence in round 6), and both ways agree as
    in test_fused_update_equals_stepwise_loop.  The fold cases run with the springs off (kappa = 0): with them the
    prediction pulls the sliver back to its rest shape before the update sees it."""
    from hydra_mi import kalman
    case = uc.build(name)
    m, n = case["mesh"], case["n"]
    kfs, out = [], []
    for fused in (True, False):
        kf = kalman.IteratedMSKalmanFilter(m, case["tex"], np.zeros((n, n, 2), np.float32), True, nI=case["max_iter"])
        kf.fused_update = fused
        kf.reltol = case["reltol"]
        if case["door"] == "revert_later":
            kf.kappa = 0
        kf.state.X = case["X0"].reshape(-1, 1).copy()
        kf.state.W = case["W"].copy()
        out.append(kf.compute(case["y_im"], case["flow"], case["y_m"]))
        kfs.append(kf)
    a, b = kfs
    if case["door"] == "revert_later":
        assert a.reverted and not a.converged and a.niter >= 2
    else:
        assert a.converged and not a.reverted and 2 <= a.niter < case["max_iter"]
    assert (a.niter, a.reverted, a.converged) == (b.niter, b.reverted, b.converged)
    assert np.array_equal(a.state.X, b.state.X)
    assert out[0][:4] == out[1][:4]
    assert np.array_equal(a.state.W, b.state.W)
    assert np.allclose(a.tv, b.tv, rtol=1e-9, atol=1e-12) and np.allclose(a.fv, b.fv, rtol=1e-9, atol=1e-12)
    assert np.allclose(a.mv, b.mv, rtol=1e-9, atol=1e-12)
    assert np.any(a.tv != 0)
