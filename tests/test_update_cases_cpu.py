"""The cases of tests/update_cases.py hold what their names promise -- for the oracle alone, without a GPU.

tests/test_update_paths_gpu.py holds the device to the oracle's results in tests/golden/update_paths.npz; that only means
something if every case really leaves the loop by the door in its name, and if no decision of the loop (a fold, a
convergence, the pixel a vertex lands in) sits so close to its threshold that the ~1e-9 by which device iterates differ
from the oracle's could tip it.  Conditions, not measurements."""
import os

import numpy as np
import pytest

import update_cases as uc
from oracle import ekf_c, ekf_ref

GOLD = uc.load_golden(os.path.join(os.path.dirname(__file__), "golden", uc.GOLDEN))


def test_every_case_is_stored():
    assert set(GOLD) == set(uc.NAMES)


@pytest.mark.parametrize("name", uc.NAMES)
def test_case_takes_its_door_at_its_round(name):
    c, g = uc.build(name), GOLD[name]
    niter, accepted, reverted, converged = (int(v) for v in g["info"])
    assert str(g["door"]) == c["door"]
    assert niter == c["round"]
    assert reverted == (c["door"] in ("revert_first", "revert_later"))
    assert converged == (c["door"] == "converge")
    if c["door"] == "revert_first":
        assert (niter, accepted) == (1, 0)
        assert np.array_equal(g["X_kept"], c["X0"]) and np.array_equal(g["W_kept"], c["W"])
    elif c["door"] == "revert_later":
        assert accepted == niter - 1 >= 1
        assert np.array_equal(g["X_kept"], g["iterates"][niter - 2])
    elif c["door"] == "converge":
        assert 2 <= niter < c["max_iter"] and accepted == niter       # a speculative measurement is in flight at the end
        assert np.array_equal(g["X_kept"], g["iterates"][-1])
    else:
        assert niter == accepted == c["max_iter"]
        assert np.array_equal(g["X_kept"], g["iterates"][-1])
    assert g["errs"].shape == (accepted, 4) and g["iterates"].shape == (niter, 4 * c["mesh"].size())


def test_the_cases_cover_the_shapes_and_limits():
    cases = {n: uc.build(n) for n in uc.NAMES}
    n4 = {n: 4 * c["mesh"].size() for n, c in cases.items()}
    assert any(v % 32 != 0 and -(-v // 32) >= 3 for v in n4.values())      # a partial third block column
    assert any(v <= 32 for v in n4.values())                               # a system inside one block
    assert all(10 <= c["mesh"].size() <= 40 or n4[n] <= 32 for n, c in cases.items())
    assert all(c["n"] <= 96 for c in cases.values())
    assert cases["limit_1"]["max_iter"] == 1 and cases["limit"]["max_iter"] >= 3
    assert any(c["door"] == "revert_later" and c["round"] >= 3 for c in cases.values())   # both factor slots reused
    m = cases["masked"]
    assert m["masked"] and np.any(m["flow"][m["y_m"] == 0] != 0)
    assert not np.array_equal(uc.update_flow(m), m["flow"])


@pytest.mark.parametrize("name", uc.NAMES)
def test_decision_margins(name):
    c, g = uc.build(name), GOLD[name]
    N, tri = c["mesh"].size(), c["mesh"].t
    niter, accepted, reverted, _ = (int(v) for v in g["info"])
    # convergence: no figure within a factor 2 of reltol
    for k, r in enumerate(g["ratios"]):
        assert not (c["reltol"] / 2 <= r <= 2 * c["reltol"]), (k, r)
        assert (r < c["reltol"]) == (c["door"] == "converge" and k == niter - 1), (k, r)
    assert g["ratios"][0] == 1.0 if accepted else True                     # (e_old = 0: round 1 cannot converge)
    # folds: every accepted iterate (and the prior mean) clear of a fold, the flipped one clearly folded
    assert uc.state_areas(c["X0"], N, tri).min() >= uc.AREA_MARGIN
    for k in range(accepted):
        assert uc.state_areas(g["iterates"][k], N, tri).min() >= uc.AREA_MARGIN, k
    if reverted:
        assert uc.state_areas(g["iterates"][niter - 1], N, tri).min() <= -uc.AREA_MARGIN
    # pixels: no vertex of a state that is rendered or measured, nor its +-deltaX positions, on a snap boundary
    for k, X in enumerate([c["X0"]] + list(g["iterates"])):
        assert uc.snap_distance(X, N, c["deltaX"]) >= uc.SNAP_MARGIN, k
    # the systems: positive definite, their condition numbers on file (the GPU bounds scale with them)
    assert np.linalg.eigvalsh(c["W"]).min() > 0
    assert np.isclose(float(g["cond_prior"]), np.linalg.cond(c["W"]), rtol=1e-6)
    assert g["cond_A"].shape == (niter,) and np.all(g["min_eig_A"] > 0) and np.all(g["cond_A"] < 1e6)


@pytest.mark.parametrize("name", ["revert_later", "masked", "small"])
def test_stored_results_are_what_the_builders_give(name):
    """the file cannot drift from the builders: the case run again (the C twin of the oracle, as the tool does)"""
    c, g = uc.build(name), GOLD[name]
    r = uc.run_oracle(c, ekf_c.Measurement)
    assert str(r["door"]) == str(g["door"]) and np.array_equal(r["info"], g["info"])
    assert np.array_equal(r["errs"][:, [0, 3]], g["errs"][:, [0, 3]])
    assert np.allclose(r["errs"], g["errs"], rtol=1e-9, atol=0)
    for k in ("iterates", "X_kept", "W_kept", "gains", "Hzc_last"):
        assert np.linalg.norm(r[k] - g[k]) <= 1e-9 * np.linalg.norm(g[k]), k
    assert np.allclose(r["cond_A"], g["cond_A"], rtol=1e-6)
    if "last_error" in g:
        assert np.allclose(r["last_error"], g["last_error"], rtol=1e-9, atol=0)


def test_c_twin_stands_in_for_the_numpy_oracle():
    """the whole small case through ekf_ref.Measurement (NumPy) and through its C twin: same door, same iterates"""
    c, g = uc.build("small"), GOLD["small"]
    r = uc.run_oracle(c, ekf_ref.Measurement)
    assert str(r["door"]) == str(g["door"]) and np.array_equal(r["info"], g["info"])
    assert np.array_equal(r["errs"][:, [0, 3]], g["errs"][:, [0, 3]])
    for k in ("iterates", "W_kept", "gains", "Hzc_last"):
        assert np.linalg.norm(r[k] - g[k]) <= 1e-9 * np.linalg.norm(g[k]), k


def test_numpy_oracle_reverts_the_sliver_in_round_one():
    """one round of the fold case through the NumPy oracle: it flips the sliver exactly as the stored run says"""
    c, g = uc.build("revert_first"), GOLD["revert_first"]
    r = uc.run_oracle(c, ekf_ref.Measurement)
    assert str(r["door"]) == "revert_first" and np.array_equal(r["info"], g["info"])
    assert np.linalg.norm(r["iterates"] - g["iterates"]) <= 1e-9 * np.linalg.norm(g["iterates"])
    assert np.linalg.norm(r["Hzc_last"] - g["Hzc_last"]) <= 1e-9 * np.linalg.norm(g["Hzc_last"])
