"""The NumPy restatement of the deformation readout (tests/strain_ref.py) against mathematics, and the host side of
hydra_mi.strain: no GPU.

The tolerance of the binary64 restatement against np.linalg.svd is 8 x the largest difference between the restatement
run in binary64 and in np.longdouble over strain_ref.random_triangles(SEED, 100000) -- 10^5 triangles, every angle
>= 20 degrees, sides of 4 .. 64 px, uv rounded to binary32, stretches in [0.25, 4].  Measured with SEED = 20261019
(x86-64, 80-bit long double):
    J, l1, l2        largest relative difference 2.34e-15  (J 2.34e-15, l1 4.11e-16, l2 2.26e-15)
    c2, s2           largest absolute difference 5.35e-12  (the axis of a nearly isotropic stretch is ill-conditioned:
                     d / r with r = (l1^2 - l2^2) / 2 near 0; the draw has stretch pairs within 1e-5 of each other)
    rc, rs           largest absolute difference 3.35e-16
test_tolerance_is_what_was_measured holds the three figures; the margin of 8 covers that the SVD's rounding is not ours.
"""
import numpy as np
import pytest

import body_ref
import strain_ref

SEED = 20261019
MEASURED = {"stretch": 2.34e-15, "axis": 5.35e-12, "rotation": 3.35e-16}
TOL = {k: 8.0 * v for k, v in MEASURED.items()}
WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def _differences(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return {"stretch": float(np.abs((a[..., :3] - b[..., :3]) / b[..., :3]).max()),
            "axis": float(np.abs(a[..., 3:5] - b[..., 3:5]).max()),
            "rotation": float(np.abs(a[..., 5:] - b[..., 5:]).max())}


def test_tolerance_is_what_was_measured():
    assert WIDER, "np.longdouble is no wider than binary64 here: the measurement needs an extended format"
    U, x = strain_ref.random_triangles(SEED, 100000)
    got = strain_ref.deform(U, x)
    ref = strain_ref.deform(U.astype(np.longdouble), x.astype(np.longdouble))
    assert got.dtype == np.float64 and ref.dtype == np.longdouble and not np.isnan(got).any()
    seen = _differences(got, ref)
    print("binary64 against long double over 1e5 triangles:", seen)
    for k, v in seen.items():
        assert 0.5 * MEASURED[k] <= v <= MEASURED[k], (k, v, MEASURED[k])


def _svd_truth(A):
    """J, l1, l2, (c2, s2), (rc, rs) of x = A u from np.linalg.svd"""
    Uo, s, Vt = np.linalg.svd(A)
    v = Vt[0]                                            # the first right singular vector: the l1 axis in the body frame
    R = Uo @ Vt                                          # the polar factor (a reflection when det A < 0)
    n = np.hypot(R[0, 0] + R[1, 1], R[1, 0] - R[0, 1])
    rc, rs = ((R[0, 0] + R[1, 1]) / n, (R[1, 0] - R[0, 1]) / n) if n > 1e-8 else (np.nan, np.nan)
    return np.linalg.det(A), s[0], s[1], (v[0] * v[0] - v[1] * v[1], 2 * v[0] * v[1]), (rc, rs)


AFFINE = {
    "stretch x": np.array([[1.5, 0.0], [0.0, 0.8]]),
    "stretch y": np.array([[0.7, 0.0], [0.0, 2.5]]),
    "shear": np.array([[1.0, 0.6], [0.0, 1.0]]),
    "rotated stretch": strain_ref.rot(0.7)[()] @ np.diag([2.0, 0.5]) @ strain_ref.rot(-1.1)[()].T,
    "general": np.array([[1.3, -0.4], [0.9, 0.75]]),
    "quarter": strain_ref.rot(2.6)[()] @ np.diag([0.31, 0.25]) @ strain_ref.rot(0.3)[()].T,
    "four": strain_ref.rot(-2.0)[()] @ np.diag([4.0, 3.2]) @ strain_ref.rot(1.9)[()].T,
}


@pytest.fixture(scope="module")
def mesh():
    p, t = strain_ref.grid_mesh(5, 4, 6.3, 5.1, 9.0, 8.0, seed=4)
    W, H = 56, 40
    tri_of, l1, l2, ids = body_ref.body_map(p, t, W, H)
    assert (ids != t).any(axis=1).any() and (ids == t).all(axis=1).any()        # the swap fires for some, not for others
    return {"p": p, "t": t, "W": W, "H": H, "tri_of": tri_of, "ids": ids}


def _apply(A, p, c=(3.25, -7.5)):
    return p @ np.asarray(A).T + np.asarray(c)


@pytest.mark.parametrize("name", sorted(AFFINE))
def test_an_affine_map_gives_its_svd_in_every_triangle(mesh, name):
    A = AFFINE[name]
    x = _apply(A, mesh["p"])
    v = strain_ref.strain_tri(x.reshape(1, -1), mesh["p"], mesh["ids"])[0]
    J, l1, l2, (c2, s2), (rc, rs) = _svd_truth(A)
    assert np.abs(v[:, 0] / J - 1).max() <= TOL["stretch"]
    assert np.abs(v[:, 1] / l1 - 1).max() <= TOL["stretch"] and np.abs(v[:, 2] / l2 - 1).max() <= TOL["stretch"]
    assert (v[:, 1] >= v[:, 2]).all()
    # the axis modulo pi: its double angle
    assert np.abs(v[:, 3] - c2).max() <= TOL["axis"] and np.abs(v[:, 4] - s2).max() <= TOL["axis"]
    assert np.abs(v[:, 5] - rc).max() <= TOL["rotation"] and np.abs(v[:, 6] - rs).max() <= TOL["rotation"]
    # the same whichever way round a triangle is listed
    w = strain_ref.strain_tri(x.reshape(1, -1), mesh["p"], mesh["t"])[0]
    assert np.abs(w[:, :3] / v[:, :3] - 1).max() <= TOL["stretch"]


@pytest.mark.parametrize("angle", [0.0, 0.3, np.pi / 2, 2.5, -3.0])
def test_a_rigid_motion_stretches_nothing(mesh, angle):
    x = _apply(strain_ref.rot(angle)[()], mesh["p"], (11.0, 2.5))
    v = strain_ref.strain_tri(x.reshape(1, -1), mesh["p"], mesh["ids"])[0]
    assert np.abs(v[:, :3] - 1).max() <= TOL["stretch"]
    assert np.abs(v[:, 5] - np.cos(angle)).max() <= TOL["rotation"] and np.abs(v[:, 6] - np.sin(angle)).max() <= TOL["rotation"]


def test_a_translation_is_exactly_the_identity(mesh):
    x = mesh["p"] + (16.0, -8.0)                         # (a power of two: the shifted positions are exact)
    v = strain_ref.strain_tri(x.reshape(1, -1), mesh["p"], mesh["ids"])[0]
    assert np.array_equal(v, np.tile([1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0], (len(mesh["t"]), 1)))


def test_a_reflection_has_a_negative_area_ratio_and_positive_stretches(mesh):
    A = np.array([[-1.25, 0.0], [0.0, 0.8]])
    v = strain_ref.strain_tri(_apply(A, mesh["p"]).reshape(1, -1), mesh["p"], mesh["ids"])[0]
    assert (v[:, 0] < 0).all() and (v[:, 2] > 0).all()
    assert np.abs(v[:, 0] / -1.0 - 1).max() <= TOL["stretch"]
    assert np.abs(v[:, 1] / 1.25 - 1).max() <= TOL["stretch"] and np.abs(v[:, 2] / 0.8 - 1).max() <= TOL["stretch"]


@pytest.mark.parametrize("k", [0.25, 1.0, 3.0])
def test_an_isotropic_scale_has_no_axis(mesh, k):
    # exactly isotropic in binary64: a power of two, or 3, times body coordinates of few bits
    p = np.rint(mesh["p"] * 4) / 4
    v = strain_ref.strain_tri((k * p).reshape(1, -1), p, mesh["ids"])[0]
    assert np.array_equal(v[:, 3:5], np.tile([1.0, 0.0], (len(v), 1)))
    assert np.abs(v[:, 0] / (k * k) - 1).max() <= TOL["stretch"] and np.abs(v[:, 1:3] / k - 1).max() <= TOL["stretch"]


def test_a_collapsed_rest_triangle_and_a_nan_vertex_are_nan():
    p = np.array([[2.0, 2.0], [10.0, 2.0], [6.0, 2.0], [6.0, 9.0], [12.0, 9.0]])        # 0, 1, 2 on a line
    ids = np.array([[0, 1, 2], [0, 1, 3], [1, 4, 3]])
    x = p * 1.5
    v = strain_ref.strain_tri(x.reshape(1, -1), p, ids)[0]
    assert np.isnan(v[0]).all() and np.isfinite(v[1:]).all()
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[4, 1] = bad
        v = strain_ref.strain_tri(y.reshape(1, -1), p, ids)[0]
        assert np.isnan(v[0]).all() and np.isfinite(v[1]).all() and np.isnan(v[2]).all()


def test_label_traces_are_the_mean_over_the_pixels(mesh):
    rng = np.random.default_rng(8)
    W, H, T, tri_of = mesh["W"], mesh["H"], len(mesh["t"]), mesh["tri_of"]
    L = 9
    lab = np.kron(rng.integers(-1, L - 1, (H // 8, W // 8)), np.ones((8, 8), np.int64))     # label L - 1 owns no pixel
    lab[10:30, 12:40][tri_of[10:30, 12:40] >= 0] = 3                                         # a label over many triangles
    states = [_apply(A, mesh["p"]) + rng.normal(0, 0.4, mesh["p"].shape) for A in AFFINE.values()]
    v = strain_ref.strain_tri(np.array(states).reshape(len(states), -1), mesh["p"], mesh["ids"])
    cnt = strain_ref.label_counts(tri_of, lab, L, T)
    assert (cnt[3] > 0).sum() >= 3 and cnt[L - 1].sum() == 0
    got = strain_ref.label_traces(v, cnt)
    on = tri_of >= 0
    for s in range(L):
        px = on & (lab == s)
        if not px.any():
            assert np.isnan(got[:, s]).all()
            continue
        want = v.astype(np.longdouble)[:, tri_of[px], :3].sum(axis=1) / np.longdouble(px.sum())
        assert float(np.abs((got[:, s] - want) / want).max()) <= 1e-12
    # a triangle that is NaN in one frame: the labels over it are NaN in that frame alone
    v[2, 5] = np.nan
    got = strain_ref.label_traces(v, cnt)
    over = cnt[:, 5] > 0
    assert over.any() and np.isnan(got[2, over]).all() and np.isfinite(got[[0, 1, 3], :][:, over]).all()
    assert np.isfinite(got[2, ~over & (cnt.sum(axis=1) > 0)]).all()


def test_levels_round_half_to_even_and_clamp():
    lv, keep = strain_ref.levels(np.array([1.0, 1.5, 0.5, 1.0 + 0.5 / 64, 1.0 + 1.5 / 64, 1.0 - 0.5 / 64, 9.0, -9.0, np.nan, np.inf]), 64.0)
    assert lv[:8].tolist() == [128, 160, 96, 128, 130, 128, 255, 0] and keep.tolist() == [False] * 8 + [True, False] and lv[9] == 255


def test_artifact_score(hm):
    from hydra_mi import strain
    t = np.linspace(0, 1, 50)
    a = 1.0 + 0.1 * np.sin(7 * t)
    J = np.stack((a, a, a, np.ones(50), a, a), axis=1)
    even = np.tile([1.0, -1.0], 24)                       # +-1 alternating ...
    slow = np.repeat([1.0, -1.0], 24)                     # ... against a step: both mean 0, their product sums to 0
    dff = np.stack((3 * a - 1, 2 - 5 * a, np.full(50, 0.3), a, a, a), axis=1)
    r = strain.artifact_score(J, dff)
    assert abs(r[0] - 1) <= 1e-12 and abs(r[1] + 1) <= 1e-12 and np.isnan(r[2]) and np.isnan(r[3])
    assert strain.artifact_score(even[:, None], slow[:, None])[0] == 0.0
    dff[::7, 4] = np.nan                                  # frames that are not finite are left out
    assert abs(strain.artifact_score(J, dff)[4] - 1) <= 1e-12
    dff[1:, 5] = np.nan
    assert np.isnan(strain.artifact_score(J, dff)[5])
    with pytest.raises(ValueError):
        strain.artifact_score(J, dff[:, :2])


def test_default_lut_and_the_body_order_on_the_host(hm, mesh):
    from hydra_mi import strain
    lut = strain.default_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0].tolist() == [255, 0, 0] and lut[128].tolist() == [255, 255, 255] and lut[255].tolist() == [0, 0, 255]
    assert (np.diff(lut[:129, 2].astype(int)) >= 0).all() and (np.diff(lut[128:, 0].astype(int)) <= 0).all()
    assert np.array_equal(strain.body_order(mesh["p"], mesh["t"]), mesh["ids"])
    a0 = strain.rest_area(mesh["p"], mesh["t"])
    assert (a0 > 0).all() and abs(a0.sum() - 4 * 3 * 72.0) < 0.5 * 72.0
