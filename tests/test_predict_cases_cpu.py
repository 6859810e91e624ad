"""The topologies of tests/predict_cases.py and the host Newton loop on them, pinned before the device kernels are held
against both (tests/test_predict_shapes_gpu.py): the builders give the intended vertex counts, spring counts, degrees
and LDS sides, and hm_ms_newton (csrc/predict.cpp: block-eliminated system, conjugate gradients) equals the oracle's
dense inverse per Newton iteration (oracle/ekf_ref.ms_predict) to 1e-9 on every case small enough for the oracle."""
import numpy as np
import pytest

import predict_cases as pc
from predict_cases import host_newton, oracle_newton

# 1/dt = 8.33: nine sub-steps, the last one past t = 1 as in the reference (ceil).  (dt = 0.3 sends every case here to
# 1e154 within the frame, for the oracle and the host alike: no reference for anything.)
PARAMS = {"defaults": pc.DEFAULTS, "dt_0.12": dict(pc.DEFAULTS, dt=0.12), "maxiter_2": dict(pc.DEFAULTS, maxiter=2)}


def small_cases():
    """every case with N <= 129 (the oracle takes seconds there, minutes at 256)"""
    cs = [c for c in pc.grid_cases() if c["N"] <= 129]
    return cs + [pc.wheel_case(k) for k in sorted(pc.WHEELS)] + pc.graph_cases()


def _orientation(c):
    p, t = c["p"], c["t"]
    a, b = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    return a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]


def test_grid_cases_shape():
    cs = {c["name"]: c for c in pc.grid_cases()}
    want = {"grid_8x8": 64, "grid_5x13": 65, "grid_8x16": 128, "grid_3x43": 129, "grid_12x16": 192, "grid_12x16_fan": 193,
            "config4": 201, "grid_15x17": 255, "grid_16x16": 256, "grid_16x16_fan": 257, "grid_15x20": 300}
    assert {k: c["N"] for k, c in cs.items()} == want
    for name, c in cs.items():
        N, I = c["N"], c["I"]
        assert (_orientation(c) > 0).all(), name                          # no fold, no degenerate triangle
        assert N - I + len(c["t"]) == 1, name                              # Euler: one simply connected piece
        assert np.array_equal(c["bars"], pc.bars_of(c["t"])) and c["bars"].dtype == np.int32
        deg = pc.degrees(N, c["bars"])
        assert deg.min() >= 2 and deg.max() == (7 if name == "config4" else 8), name
        if name.startswith("grid") and not name.endswith("fan"):
            r, cc = map(int, name[5:].split("x"))
            assert I == r * (cc - 1) + (r - 1) * cc + (r - 1) * (cc - 1)
            # alternating diagonals: the inner vertices with i + j even have 8 springs, the other inner ones 4
            assert (deg == 8).sum() == sum((i + j) % 2 == 0 for i in range(1, r - 1) for j in range(1, cc - 1))
        assert pc.lds_newton4(I) <= pc.NEWTON4_LDS_MAX and pc.lds_newton(N, I) <= pc.NEWTON_LDS_MAX, name
        d = c["X"][:2 * N] - c["p"].reshape(-1)
        assert 0.3 < d.std() < 0.5 and 1.2 < c["X"][2 * N:].std() < 1.8
    assert cs["grid_15x20"]["I"] == 831
    for name in ("grid_12x16_fan", "grid_16x16_fan"):                     # the fan vertex: 3 springs onto the border
        assert pc.degrees(cs[name]["N"], cs[name]["bars"])[-1] == 3


@pytest.mark.parametrize("k", sorted(pc.WHEELS))
def test_wheel_cases_shape(k):
    c = pc.wheel_case(k)
    deg = pc.degrees(c["N"], c["bars"])
    assert (_orientation(c) > 0).all() and c["N"] - c["I"] + len(c["t"]) == 1
    assert deg.max() == k and deg.min() >= 2
    if k > 8:
        assert (deg == k).sum() == 1 and np.sort(deg)[-2] == 8              # the hub alone, everything else <= 8
    # the neighbour slots k_ms_newton4 would take: DEG = 8 full; 12 with three padding slots; 12 full; refused
    assert {8: 8, 9: 12, 12: 12, 13: 0}[k] == (8 if deg.max() <= 8 else 12 if deg.max() <= 12 else 0)


def test_graph_cases_shape():
    circ, pend, iso = pc.graph_cases()
    assert circ["N"] == 64 and circ["I"] == 384 and (pc.degrees(64, circ["bars"]) == 12).all()
    assert len({tuple(sorted(b)) for b in circ["bars"]}) == 384                # no spring twice
    dp, di = pc.degrees(65, pend["bars"]), pc.degrees(65, iso["bars"])
    assert pend["N"] == iso["N"] == 65 and dp[64] == 1 and di[64] == 0 and (di[:64] >= 2).all()
    for c in (circ, pend, iso):
        assert c["t"] is None and pc.handle_mesh(c["N"])[0].shape[0] == c["N"]


def test_lds_limit_cases():
    a, b = pc.newton4_lds_case(1327), pc.newton4_lds_case(1328)
    for c in (a, b):
        assert c["N"] == 256 and pc.degrees(256, c["bars"]).max() == 12
        assert len({tuple(sorted(x)) for x in c["bars"]}) == c["I"]
    assert pc.lds_newton4(a["I"]) <= pc.NEWTON4_LDS_MAX < pc.lds_newton4(b["I"])
    a, b = pc.newton_lds_case(1124), pc.newton_lds_case(1125)
    for c in (a, b):
        assert c["N"] == 300 and len({tuple(sorted(x)) for x in c["bars"]}) == c["I"]
    assert pc.lds_newton(300, a["I"]) <= pc.NEWTON_LDS_MAX < pc.lds_newton(300, b["I"])


def test_lds_formulas_are_the_layouts():
    """the footprints, summed from the kernels' LDS layouts (csrc/predict_kernels.h)"""
    for N, I in ((18, 40), (256, 1327), (300, 1124)):
        assert pc.lds_newton4(I) == (6 * 256 + 4 * (I + 1) + 4 * 4) * 8 + 2 * I * 4
        assert pc.lds_newton(N, I) == (5 * 4 * N + 7 * 2 * N + 6 * I + 8 + I) * 8 + (N + 1 + 2 * I + 2 * I) * 4


@pytest.mark.parametrize("param", sorted(PARAMS))
def test_host_loop_matches_oracle(hm, param):
    par = PARAMS[param]
    steps = int(np.ceil(1.0 / par["dt"]))
    for c in small_cases():
        X, its = host_newton(c, **par)
        ref = oracle_newton(c, **par)
        assert np.abs(X - ref).max() <= 1e-9 * np.abs(ref).max(), (c["name"], np.abs(X - ref).max())
        assert np.abs(X - c["X"]).max() > 1.0, c["name"]                    # the state did move
        if par["maxiter"] == 2:
            assert its == 2 * steps, (c["name"], its)                       # every sub-step hits the cap
        else:
            assert 2 * steps <= its <= 10 * steps, (c["name"], its)
