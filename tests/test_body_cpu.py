"""The body-frame readout without a GPU: the body map of the NumPy restatement (tests/body_ref.py) against the render's
coverage, the host point code of hydra_mi.body (locate, track, discs, files), argument errors of hm_body_*, and the
physical sense of the readout on the committed golden tracks."""
import ctypes
import os

import numpy as np
import pytest

import body_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _meshes():
    from hydra_mi import mesh
    g1 = np.load(os.path.join(GOLD, "config1_track.npz"))
    g4 = np.load(os.path.join(GOLD, "config4_track.npz"))
    n4 = int(g4["n"])
    return {
        "square4": (mesh.square4_mesh(10, 30), 40, 40),
        "disk": (mesh.disk_mesh(47.5, 40.0, 30.0, 9.0), 96, 80),
        "config1": (mesh.Mesh(g1["p"], g1["t"], 15.0), 128, 128),
        "config4": (mesh.Mesh(g4["p"], g4["t"], float(g4["h0"]) * n4), n4, n4),
    }


@pytest.mark.parametrize("name", ["square4", "disk", "config1", "config4"])
def test_restated_body_map_is_the_render_coverage(hm, name):
    """Validates the restatement (tests/body_ref.py) the GPU tests compare the library with: its body map is the
    coverage of oracle.ekf_ref.render at X = uv, every covered pixel once."""
    from oracle import ekf_ref
    dm, W, H = _meshes()[name]
    if name == "config4":
        c = (W - 1) / 2.0
        assert dm.size() == 201 and abs(dm.p[:, 0].mean() - c) < 5
    uv = np.asarray(dm.p, np.float32)
    N = uv.shape[0]
    X = np.concatenate((uv.astype(np.float64).reshape(-1), np.zeros(2 * N)))
    tex = np.zeros((H, W), np.uint8)
    _, _, _, m = ekf_ref.render(X, N, dm.t, uv, tex, W, H)
    tri_of, l1, l2, ids = body_ref.body_map(uv, dm.t, W, H)
    assert np.array_equal(tri_of >= 0, m == 255)
    assert (tri_of >= 0).sum() > 0
    # every covered pixel exactly once: the triangle counts add up to the covered pixels, and the barycentrics of a
    # pixel put it at its own centre (to rounding) at X = uv
    cnt = body_ref.counts(tri_of, dm.t.shape[0])
    assert int(cnt.sum()) == int((m == 255).sum())
    x, y = body_ref.positions(X, tri_of, l1, l2, ids)
    rr, cc = np.nonzero(tri_of >= 0)
    assert np.abs(x[rr, cc] - (cc + 0.5)).max() < 0.02 and np.abs(y[rr, cc] - (rr + 0.5)).max() < 0.02
    assert (l1[rr, cc] >= 0).all() and (l2[rr, cc] >= 0).all() and (l1 + l2)[rr, cc].max() <= 1.0


def test_points_at_pixel_centres_get_the_pixels_positions(hm):
    from hydra_mi import body
    dm, W, H = _meshes()["config1"]
    uv = np.asarray(dm.p, np.float32)
    tri_of, l1, l2, ids = body_ref.body_map(uv, dm.t, W, H)
    rr, cc = np.nonzero(tri_of >= 0)
    pick = np.random.default_rng(1).choice(rr.size, 200, replace=False)
    q = np.stack((cc[pick] + 0.5, rr[pick] + 0.5), 1)
    t, pids, pl1, pl2 = body.locate(uv, dm.t, q)
    assert np.array_equal(t, tri_of[rr[pick], cc[pick]])
    assert np.array_equal(pl1, l1[rr[pick], cc[pick]]) and np.array_equal(pl2, l2[rr[pick], cc[pick]])
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    X = g["X"][5]
    x, y = body_ref.positions(X, tri_of, l1, l2, ids)
    p = body.track(X[:2 * uv.shape[0]], pids, pl1, pl2, t >= 0)
    assert np.array_equal(p[:, 0], x[rr[pick], cc[pick]]) and np.array_equal(p[:, 1], y[rr[pick], cc[pick]])


def test_points_outside_the_mesh_are_nan(hm):
    from hydra_mi import body
    dm, W, H = _meshes()["square4"]
    q = np.array([[20.0, 20.0], [2.0, 2.0], [39.0, 5.0], [np.nan, 3.0], [1e30, 1.0]])
    t, ids, l1, l2 = body.locate(np.asarray(dm.p, np.float32), dm.t, q)
    assert t[0] >= 0 and (t[1:] < 0).all()
    N = dm.size()
    X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + 1.25, np.zeros(2 * N)))
    p = body.track(X[:2 * N], ids, l1, l2, t >= 0)
    assert np.isfinite(p[0]).all() and np.isnan(p[1:]).all()
    assert np.allclose(p[0], [21.25, 21.25])


def test_points_files_round_trip(tmp_path):
    from hydra_mi import body
    csv = tmp_path / "neurons.csv"
    csv.write_text("name,x,y\nn0,10.5,20.25\nn1,3,4\n\nn2,-1e-3,7.125\n")
    names, q = body.read_points_csv(str(csv))
    assert names == ["n0", "n1", "n2"]
    assert np.array_equal(q, [[10.5, 20.25], [3.0, 4.0], [-1e-3, 7.125]])
    pts = np.random.default_rng(2).normal(0, 50, (7, 3, 2))
    pts[2, 1] = np.nan
    txt = tmp_path / "out_points.txt"
    body.write_points_txt(str(txt), pts)
    lines = txt.read_text().splitlines()
    assert len(lines) == 7 and all(l.startswith("neurons,") and l.count(",") == 6 for l in lines)
    back = body.read_points_txt(str(txt))
    assert np.array_equal(back, pts, equal_nan=True)


def test_disc_labels_nearest_point_and_ties(hm):
    from hydra_mi import body
    tri = np.zeros((20, 30), np.int32)
    tri[:, 25:] = -1                                        # outside the map: never labelled
    q = np.array([[10.5, 10.5], [14.5, 10.5], [10.5, 10.5], [27.5, 5.5]])
    lab = body.disc_labels(tri, q, 3.0)
    # pixel (10, 12) centre (12.5, 10.5): 2 from point 0 and from point 1 -> the lower index; (10, 13): nearer point 1
    assert lab[10, 12] == 0 and lab[10, 13] == 1 and lab[10, 10] == 0
    assert not (lab == 2).any()                             # point 2 ties point 0 everywhere
    assert lab[10, 7] == 0 and lab[10, 6] == -1             # distance exactly 3 is within, 4 is not
    assert (lab[:, 25:] == -1).all()
    assert lab[5, 24] == 3                                  # a point beside the map labels the map pixels near it
    cx, cy = np.arange(30)[None, :] + 0.5, np.arange(20)[:, None] + 0.5
    near = np.zeros((20, 30), bool)
    for qx, qy in q:
        near |= (cx - qx) ** 2 + (cy - qy) ** 2 <= 9.0
    assert np.array_equal(lab >= 0, near & (tri >= 0))


def test_abi_argument_errors_need_no_gpu(hm):
    from hydra_mi import _lib
    L = _lib.lib()
    X = np.zeros(12)
    frame = np.zeros(16, np.uint8)
    assert L.hm_body_warp_dev(None, _lib.ptr(X), _lib.ptr(frame), None, 2, None, None, None) == -1
    assert b"out_channels 2" in L.hm_last_error()
    assert L.hm_body_warp_dev(None, _lib.ptr(X), None, None, 3, None, None, None) == -1
    assert b"NULL state or frame" in L.hm_last_error()
    assert L.hm_body_warp_dev(None, _lib.ptr(X), ctypes.c_void_p(4096 + 2), ctypes.c_void_p(4096 + 2), 1, None, None,
                              None) == -1
    assert b"aligned" in L.hm_last_error()
    assert L.hm_body_warp_dev(None, _lib.ptr(X), ctypes.c_void_p(4096), None, 1, ctypes.c_void_p(4096 + 4), None,
                              None) == -1
    assert b"sums are not 8-byte aligned" in L.hm_last_error()
    assert L.hm_body_warp_dev(None, _lib.ptr(X), ctypes.c_void_p(4096), None, 1, None, ctypes.c_void_p(4096 + 12),
                              None) == -1
    assert b"sums are not 8-byte aligned" in L.hm_last_error()
    assert L.hm_body_warp(None, _lib.ptr(X), None, None, None, None) == -1
    assert b"NULL state or frame" in L.hm_last_error()
    lab = np.zeros(16, np.int32)
    assert L.hm_body_set_labels(None, _lib.ptr(lab), 0, None) == -1
    assert b"0 labels" in L.hm_last_error()
    assert L.hm_body_map(None, None, None) == -1 and b"NULL handle" in L.hm_last_error()
    assert L.hm_body_fence(None, None) == -1


def _inner_points(tri_of, n, seed, margin=5):
    """n points of body coordinates whose disc of `margin` px lies in the map"""
    from scipy import ndimage
    inner = ndimage.binary_erosion(tri_of >= 0, np.ones((2 * margin + 1, 2 * margin + 1), bool))
    rr, cc = np.nonzero(inner)
    rng = np.random.default_rng(seed)
    pick = rng.choice(rr.size, min(n, rr.size), replace=False)
    return np.stack((cc[pick] + rng.random(pick.size), rr[pick] + rng.random(pick.size)), 1)


def _physics(uv, tri, frames0, frames, Xs, shifts, reg_bound, ratio):
    from hydra_mi import body
    H, W = frames0.shape
    tri_of, l1, l2, ids = body_ref.body_map(uv, tri, W, H)
    inside = tri_of >= 0
    for X, f in zip(Xs, frames):
        reg = body_ref.warp(X, f, tri_of, l1, l2, ids)
        d_reg = np.abs(reg.astype(np.float64) - frames0)[inside].mean()
        d_raw = np.abs(f.astype(np.float64) - frames0)[inside].mean()
        assert d_reg <= reg_bound, (d_reg, d_raw)
        if ratio is not None:
            assert d_reg <= ratio * d_raw, (d_reg, d_raw)
    q = _inner_points(tri_of, 60, 3)
    t, pids, pl1, pl2 = body.locate(uv, tri, q)
    assert (t >= 0).all()
    err = []
    for X, s in zip(Xs, shifts):
        p = body.track(np.asarray(X)[:2 * uv.shape[0]], pids, pl1, pl2, t >= 0)
        err.append(np.hypot(*(p - (q + s)).T))
    err = np.concatenate(err)
    assert np.sqrt((err ** 2).mean()) <= 1.0 and err.max() <= 4.0, (np.sqrt((err ** 2).mean()), err.max())


def test_registered_config1_golden_track_holds_still(hm):
    from hydra_mi import synth
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    video, _ = synth.test_data(128, 128)
    frames = [video[:, :, k] for k in range(g["X"].shape[0])]
    shifts = [np.array([-3.0 * k, -3.0 * k]) for k in range(len(frames))]
    _physics(np.asarray(g["p"], np.float32), g["t"], video[:, :, 0].astype(np.float64), frames, g["X"], shifts, 2.0, None)


def test_registered_config4_golden_track_holds_still(hm):
    from hydra_mi import synth
    g = np.load(os.path.join(GOLD, "config4_track.npz"))
    n = int(g["n"])
    video, _, _, _ = synth.disk_video(n, int(g["frames"]), "translate_leftup", 0)
    v = -1.5 * n / 600.0                                    # translate_leftup at n px (synth.scaled_field)
    frames = [video[k + 1] for k in range(g["X"].shape[0])]
    shifts = [np.array([v * (k + 1), v * (k + 1)]) for k in range(len(frames))]
    _physics(np.asarray(g["p"], np.float32), g["t"], video[0].astype(np.float64), frames, g["X"], shifts, 3.0, 0.25)
