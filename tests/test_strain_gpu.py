"""The deformation readout on the GPU (`pytest -m gpu`): hm_strain_tri and hm_strain_labels equal to the NumPy restatement
of tests/strain_ref.py in every bit, hm_view_strain / hm_view_strain_dev in every byte, at the smallest shapes where the
kernels can go wrong; the refusals; the view between frames changes nothing the filter computes; hydra_mi.strain and the
command line on a synthetic video."""
import os
import sys

import numpy as np
import pytest

import body_ref
import strain_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _renderer(p, t, W, H, seed=0):
    from hydra_mi import mesh, renderer
    dm = mesh.Mesh(np.asarray(p, np.float64), np.asarray(t, np.int64), 1.0)
    tex = np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    return renderer.Renderer(dm, np.zeros_like(dm.p), np.zeros((H, W, 2), np.float32), H, tex, True, 1.0, 1.0, 1.0)


def _states(p, F, rng, noise=0.6):
    """F states (F, 4N): another affine map of the body per frame plus noise per vertex; the velocities are random numbers
    (nothing reads them)"""
    out = np.empty((F, 4 * len(p)))
    for k in range(F):
        A = strain_ref.rot(rng.uniform(-0.5, 0.5))[()] @ np.diag(rng.uniform(0.6, 1.6, 2)) @ strain_ref.rot(rng.uniform(-3, 3))[()]
        x = p @ A.T + rng.uniform(-5, 5, 2) + rng.normal(0, noise, p.shape)
        out[k] = np.concatenate((x.reshape(-1), rng.normal(0, 1, 2 * len(p))))
    return out


# the meshes of the triangle test: (frames, mesh).  One thread per (frame, triangle), 64 to a wave, 256 to a workgroup:
# 2 x 130 has its frame boundary inside the third wave and past two whole ones, 65 x 7 has 455 pairs in two workgroups with
# a frame boundary every 7 lanes.
def _mesh(name):
    if name == "1x1":
        return 1, np.array([[5.25, 4.5], [20.0, 7.75], [9.5, 18.0]]), np.array([[0, 1, 2]])
    if name == "3x5":
        p, t = strain_ref.grid_mesh(4, 2, 4.0, 5.0, 9.0, 12.0, seed=1)
        return 3, p, t[:5]
    if name == "2x130":
        p, t = strain_ref.grid_mesh(12, 7, 3.0, 3.0, 5.0, 6.0, seed=2)
        return 2, p, t[:130]
    p, t = strain_ref.grid_mesh(5, 2, 4.0, 5.0, 9.0, 12.0, seed=3)
    return 65, p, t[:7]


@pytest.mark.parametrize("name", ["1x1", "3x5", "2x130", "65x7"])
def test_strain_tri_equals_the_restatement(hm, name):
    F, p, t = _mesh(name)
    W, H = 64, 48
    ids = body_ref.body_map(p, t, W, H)[3]
    if len(t) > 1:
        assert (ids != t).any(axis=1).any() and (ids == t).all(axis=1).any()    # the swap fires for some, not for others
    r = _renderer(p, t, W, H)
    states = _states(p, F, np.random.default_rng(len(t)))
    got = r.strain_tri(states)
    want = strain_ref.strain_tri(states, r.uv, ids)
    assert got.shape == (F, len(t), 7) and np.isfinite(got).all()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # (exchanging i1 and i2 negates d0 and every numerator exactly: the swap shows in no bit, only the choice of i0 would)
    assert np.array_equal(got, strain_ref.strain_tri(states, r.uv, t))
    if len(t) > 1:
        assert not np.array_equal(got, strain_ref.strain_tri(states, r.uv, np.roll(ids, 1, axis=1)))
    r.close()


def test_strain_tri_nan_rules(hm):
    """A triangle that is collapsed in the body frame and a vertex that is NaN or infinite in one frame, among good ones."""
    p = np.array([[4.0, 6.0], [20.0, 6.0], [12.0, 6.0], [12.0, 20.0], [26.0, 18.0], [30.0, 5.0]])     # 0, 1, 2 on a line
    t = np.array([[0, 2, 3], [2, 1, 3], [0, 1, 2], [1, 4, 3], [1, 5, 4]])
    W, H = 40, 32
    ids = body_ref.body_map(p, t, W, H)[3]
    r = _renderer(p, t, W, H)
    states = _states(p, 4, np.random.default_rng(7))
    states[1, 2 * 5 + 1] = np.nan                        # vertex 5 (triangle 4) in frame 1
    states[2, 2 * 4] = np.inf                            # vertex 4 (triangles 3, 4) in frame 2
    states[3, 2 * len(p):] = np.nan                      # the velocities are not read
    got = r.strain_tri(states)
    want = strain_ref.strain_tri(states, r.uv, ids)
    assert np.array_equal(got, want, equal_nan=True)
    bad = np.isnan(got).all(axis=2)
    assert np.array_equal(bad, np.isnan(got).any(axis=2))
    assert bad.tolist() == [[False, False, True, False, False], [False, False, True, False, True],
                            [False, False, True, True, True], [False, False, True, False, False]]
    from hydra_mi import strain
    d = strain.triangles(r, states)
    assert d["n_bad"].tolist() == [1, 2, 3, 1] and np.isfinite(d["body_area"]).all()
    r.close()


@pytest.fixture(scope="module")
def grid():
    """a 24-triangle mesh in a 56 x 40 frame, its body map restated once"""
    p, t = strain_ref.grid_mesh(5, 4, 6.3, 5.1, 9.0, 8.0, seed=4)
    W, H = 56, 40
    tri_of, _, _, ids = body_ref.body_map(p, t, W, H)
    return {"p": p, "t": t, "W": W, "H": H, "tri_of": tri_of, "ids": ids}


def _label_images(grid):
    rng = np.random.default_rng(12)
    W, H, tri_of = grid["W"], grid["H"], grid["tri_of"]
    one = np.full((H, W), -1, np.int32)
    one[8:30, 10:44] = 0                                  # one label over many triangles (and over pixels off the mesh)
    many = np.kron(rng.integers(-1, 66, (H // 4, W // 4)), np.ones((4, 4), np.int64)).astype(np.int32)
    many[many == 5] = -1
    many[0, 0] = 5                                        # label 5: a pixel, but none of the map; label 66: none at all
    assert tri_of[0, 0] < 0
    return {1: one, 67: many}


@pytest.mark.parametrize("L", [1, 67])
def test_strain_labels_equal_the_restatement(hm, grid, L):
    lab = _label_images(grid)[L]
    T = len(grid["t"])
    r = _renderer(grid["p"], grid["t"], grid["W"], grid["H"])
    tri_of = r.body_map()[0]
    assert np.array_equal(tri_of, grid["tri_of"])
    states = _states(grid["p"], 5, np.random.default_rng(L))
    cnt = strain_ref.label_counts(grid["tri_of"], lab, L, T)
    assert ((cnt > 0).sum(axis=1) >= 3).any()             # a label that spans three triangles and more
    big = int(np.argmax((cnt > 0).sum(axis=1)))
    t_nan = int(np.flatnonzero(cnt[big])[1])
    states[3, 2 * grid["ids"][t_nan, 0]] = np.nan         # a triangle under it is NaN in frame 3 only
    v = strain_ref.strain_tri(states, r.uv, grid["ids"])
    want = strain_ref.label_traces(v, cnt)
    got, n = r.strain_labels(states, lab, L)
    assert np.array_equal(n, cnt.sum(axis=1))
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]
    assert np.isnan(got[3, big]).all() and np.isfinite(got[[0, 1, 2, 4], big]).all()
    if L == 67:
        assert n[5] == 0 and n[66] == 0 and np.isnan(got[:, [5, 66]]).all() and np.isfinite(got[0, n > 0]).all()
    # labels = NULL: the image of the last hm_body_set_labels
    assert np.array_equal(r.body_set_labels(lab, L), cnt.sum(axis=1))
    got2, n2 = r.strain_labels(states, None, L)
    assert np.array_equal(got2, want, equal_nan=True) and np.array_equal(n2, n)
    from hydra_mi import strain
    c = strain.labels(r, states)
    assert np.array_equal(c["J"], want[:, :, 0], equal_nan=True) and np.array_equal(c["l2"], want[:, :, 2], equal_nan=True)
    r.close()


# ---- the view ------------------------------------------------------------------------------------------------------------
# A fan of five triangles round vertex 0, the winding alternating.  At the state X_B the centre sits on the pixel centre
# (cx, 8.5), the spoke 0-1 runs along the pixel centres of row 8 and the spoke 0-5 along those of a column: the pixels on them
# go to one triangle by the top-left rule, and the triangles either side differ in every value.
FAN_T = np.array([[0, 1, 2], [0, 3, 2], [0, 3, 4], [0, 5, 4], [0, 5, 1]])
FAN_UV = np.array([[8.0, 8.0], [13.0, 8.5], [9.0, 13.0], [1.5, 12.5], [1.0, 2.5], [9.5, 3.0]])
FAN_XB = np.array([[8.5, 8.5], [14.5, 8.5], [10.0, 14.2], [3.1, 12.4], [2.6, 4.3], [8.5, 2.5]])
SIZES = [(16, 16, 0.0), (33, 17, 12.0)]                  # W, H, shift of the fan along x


def _fan_state(x, dx):
    return np.concatenate(((x + (dx, 0.0)).reshape(-1), np.zeros(x.size)))


@pytest.mark.parametrize("W,H,dx", SIZES)
def test_view_strain_equals_the_restatement(hm, W, H, dx):
    from hydra_mi import strain
    rng = np.random.default_rng(W)
    frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    uv = FAN_UV + (dx, 0.0)
    ids = body_ref.body_map(uv, FAN_T, W, H)[3]
    r = _renderer(uv, FAN_T, W, H)
    X_B = _fan_state(FAN_XB, dx)
    X_A = _fan_state(8.5 + 1.5 * (FAN_UV - FAN_UV[0]), dx)           # exactly 1.5 times the body: l1 = l2 = 1.5, J = 2.25
    v_A = strain_ref.strain_tri(X_A, uv, ids)[0]
    assert np.array_equal(v_A[:, :3], np.tile([2.25, 1.5, 1.5], (5, 1)))
    # gain 1 and 5 on l1 - 1 = 0.5, gain 2 on J - 1 = 1.25: 0.5, 2.5, 2.5 -- exact halves, rounded to even
    for which, gain, level in ((1, 1.0, 128), (2, 5.0, 130), (0, 2.0, 130), (0, -2.0, 126)):
        assert set(strain_ref.levels(v_A[:, which], gain)[0]) == {level}
        got = r.view_strain(X_A, frame, which, gain, 255, lut)
        want = strain_ref.view_strain(X_A, FAN_T, uv, ids, frame, which, gain, 255, lut)
        assert np.array_equal(got, want), (which, gain, np.argwhere(got != want)[:5])
        assert (got == lut[level]).all(axis=2).sum() > 40
    # the state whose triangles differ: every value, gains that use the table's middle and both its ends, three alphas
    v_B = strain_ref.strain_tri(X_B, uv, ids)[0]
    seen = set()
    for which in (0, 1, 2):
        for gain in (40.0, 3000.0):
            lv = strain_ref.levels(v_B[:, which], gain)[0]
            seen |= set(lv.tolist())
            assert len(set(lv.tolist())) >= 2
            for alpha in (0, 100, 255):
                for wire in (False, True):
                    got = r.view_strain(X_B, frame, "J l1 l2".split()[which], gain, alpha, lut, wire)
                    want = strain_ref.view_strain(X_B, FAN_T, uv, ids, frame, which, gain, alpha, lut, wire)
                    assert got.shape == (H, W, 3) and got.dtype == np.uint8
                    assert np.array_equal(got, want), (which, gain, alpha, wire, np.argwhere(got != want)[:5])
                    if alpha == 0 and not wire:
                        assert np.array_equal(got, np.repeat(frame[:, :, None], 3, axis=2))
    assert 0 in seen and 255 in seen and len(seen) > 4
    # the pixels whose centre lies on the shared spokes and on the shared vertex are covered, by one triangle each
    import cellview_ref
    tri_of = cellview_ref.map_at(X_B, FAN_T, W, H, 6)[0]
    cx = int(8 + dx)
    assert tri_of[8, cx] >= 0 and (tri_of[8, cx + 1:cx + 6] >= 0).all() and (tri_of[3:8, cx] >= 0).all()
    assert len({int(tri_of[8, cx]), int(tri_of[8, cx + 2]), int(tri_of[5, cx]), int(tri_of[9, cx + 2])}) >= 2
    # the default table, and the device form: queued back to back, the host arrays overwritten right after each call
    from hydra_mi import _lib
    from hydra_mi.pipeline import DeviceBuffer
    d_frame = DeviceBuffer(W * H)
    d_frame.upload(frame)
    outs, wants = [], []
    for k, (X, which, gain, alpha, wire) in enumerate(((X_B, "J", 300.0, 128, True), (X_A, "l1", 1.0, 200, False), (X_B, "l2", 90.0, 77, False),
                                                       (X_B, "l1", 500.0, 255, True), (X_A, "J", 2.0, 13, True), (X_B, "J", 64.0, 100, False))):
        table = strain.default_lut() if k % 2 == 0 else lut.copy()
        wants.append(strain_ref.view_strain(X, FAN_T, uv, ids, frame, strain.WHICH.index(which), gain, alpha, table, wire))
        if k == 0:
            assert np.array_equal(r.view_strain(X, frame, which, gain, alpha, table, wire), wants[0])
        outs.append(DeviceBuffer(3 * W * H))
        Xc = X.copy()
        r.view_strain_dev(Xc, d_frame.ptr, outs[-1].ptr, which, gain, alpha, table, wire)
        Xc[:] = -1.0
        table[:] = 0
    _lib.check(_lib.lib().hm_ctx_sync(r._h), "hm_ctx_sync")
    for k, d in enumerate(outs):
        assert np.array_equal(d.download(np.empty((H, W, 3), np.uint8)), wants[k]), k
        d.close()
    d_frame.close()
    r.close()


def test_view_strain_keeps_the_base_under_a_nan_triangle(hm):
    """Triangle 4 (0, 5, 1) is collapsed in the body frame (u5, u0, u1 on a line) and covers pixels at X: its values are
    NaN, its pixels keep the frame; so do those of a triangle with a NaN vertex, which the coverage rule skips."""
    W, H = 16, 16
    uv = FAN_UV.copy()
    uv[1], uv[5] = (13.0, 8.0), (3.0, 8.0)
    ids = body_ref.body_map(uv, FAN_T, W, H)[3]
    r = _renderer(uv, FAN_T, W, H)
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    base = np.repeat(frame[:, :, None], 3, axis=2)
    import cellview_ref
    for X in (_fan_state(FAN_XB, 0.0), _fan_state(np.where(np.arange(6)[:, None] == 3, np.nan, FAN_XB), 0.0)):
        v = strain_ref.strain_tri(X, uv, ids)[0]
        tri_of = cellview_ref.map_at(X, FAN_T, W, H, 6)[0]
        assert np.isnan(v[4]).all() and (tri_of == 4).sum() > 8
        for which in (0, 1, 2):
            got = r.view_strain(X, frame, which, 100.0, 255, lut, False)
            assert np.array_equal(got, strain_ref.view_strain(X, FAN_T, uv, ids, frame, which, 100.0, 255, lut))
            assert np.array_equal(got[tri_of == 4], base[tri_of == 4]) and np.array_equal(got[tri_of < 0], base[tri_of < 0])
            assert (got[tri_of == 0] != base[tri_of == 0]).any()
    r.close()


def test_refusals_leave_the_handle_working(hm, grid):
    from hydra_mi import _lib
    W, H = grid["W"], grid["H"]
    r = _renderer(grid["p"], grid["t"], W, H)
    L = _lib.lib()
    states = _states(grid["p"], 2, np.random.default_rng(1))
    out = np.empty((2, len(grid["t"]), 7))
    lab = _label_images(grid)[67]
    tr = np.empty((2, 67, 3))
    frame = np.zeros((H, W), np.uint8)
    lut = np.zeros((256, 3), np.uint8)
    img = np.empty((H, W, 3), np.uint8)
    p = _lib.ptr
    for n in (0, -3):
        assert L.hm_strain_tri(r._h, n, p(states), p(out)) == -1 and b"%d frames" % n in L.hm_last_error()
        assert L.hm_strain_labels(r._h, n, p(states), p(lab), 67, p(tr), None) == -1 and b"%d frames" % n in L.hm_last_error()
    assert L.hm_strain_tri(None, 2, p(states), p(out)) == -1
    assert L.hm_strain_labels(r._h, 2, p(states), p(lab), 0, p(tr), None) == -1
    bad = lab.copy()
    bad[4, 7] = 67
    with pytest.raises(RuntimeError, match="code -1.*label 67 at pixel %d outside -1..66" % (4 * W + 7)):
        r.strain_labels(states, bad, 67)
    with pytest.raises(RuntimeError, match="code -3.*hm_body_set_labels has set none"):
        r.strain_labels(states, None, 67)
    for which in (-1, 3):
        with pytest.raises(RuntimeError, match="code -1.*which %d outside 0..2" % which):
            r.view_strain(states[0], frame, which, 10.0, 128, lut)
    for alpha in (-1, 256):
        with pytest.raises(RuntimeError, match="code -1.*alpha %d outside 0..255" % alpha):
            r.view_strain(states[0], frame, "J", 10.0, alpha, lut)
    with pytest.raises(RuntimeError, match="code -1.*NULL lut"):
        r.view_strain(states[0], frame, "J", 10.0, 128, None)
    assert L.hm_view_strain(r._h, p(states), p(frame), 0, 10.0, 128, p(lut), 1, p(img)) == -1 and b"flags 1" in L.hm_last_error()
    assert L.hm_view_strain_dev(r._h, p(states), None, 0, 10.0, 128, p(lut), 0, None, None) == -1
    # ... and the handle works
    assert np.array_equal(r.strain_tri(states), strain_ref.strain_tri(states, r.uv, grid["ids"]))
    got = r.view_strain(states[0], frame, "J", 10.0, 128, lut)
    assert np.array_equal(got, strain_ref.view_strain(states[0], grid["t"], r.uv, grid["ids"], frame, 0, 10.0, 128, lut))
    r.close()


def test_strain_views_between_frames_change_nothing(hm):
    """Config 1 (128^2, the golden track) with a strain view and the two strain read-outs between every two frames: states,
    covariance and error terms bit-identical to the run without, and the raw and overlay views either side of a strain view
    byte-identical."""
    from hydra_mi import kalman, mesh, strain, synth
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    video, flow = synth.test_data(128, 128)
    lut = strain.default_lut()
    runs = {}
    for views in (False, True):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), video[:, :, 0], flow[:, :, :, 0], True)
        r = kf.state.renderer
        out = []
        for k in range(5):
            frame = video[:, :, k]
            e = kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
            if views:
                before = [r.view(kf.state.X, w) for w in ("raw", "overlay")]
                img = r.view_strain(kf.state.X, frame, "J", 2000.0, 200, lut, wire=True)
                assert (img[:, :, 0] != img[:, :, 2]).any()
                strain.triangles(kf, [kf.state.X.reshape(-1)])
                strain.labels(kf, [kf.state.X.reshape(-1)], points=g["p"][:3], point_radius=4.0)
                after = [r.view(kf.state.X, w) for w in ("raw", "overlay")]
                assert all(np.array_equal(a, b) for a, b in zip(before, after))
            out.append((kf.state.X.copy(), kf.niter, e[:4], np.array(kf.state.W, np.float64).copy()))
        runs[views] = out
        kf.close()
    for (Xa, ia, ea, Wa), (Xb, ib, eb, Wb) in zip(runs[False], runs[True]):
        assert np.array_equal(Xa, Xb) and ia == ib and ea == eb and np.array_equal(Wa, Wb)


def test_product_and_cli_on_a_stretching_disk(hm, tmp_path):
    """64^2, six frames of a disk of radius 21 px under the affine velocity field translate_leftup_stretch, v = x / 300 + const:
    every frame stretches the last by 1 + 1 / 300 along both axes.  --strain --find-points 3 --rois --strain-video gives arrays
    equal to strain.triangles / strain.labels on the run's own states, video frames equal to the restated view, and leaves
    every other array as the run without --strain has it."""
    from hydra_mi import mesh, strain, synth
    from test_views_cpu import read_avi
    sys.path.insert(0, ROOT)
    import run_kalmanfilter
    n, F = 64, 6
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup_stretch", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    a, b, avi = str(tmp_path / "plain.npz"), str(tmp_path / "strain.npz"), str(tmp_path / "strain.avi")
    common = [vid, str(tmp_path / "noflow"), None, "-s", "10", "--find-points", "3", "--find-radius", "4", "--find-score", "std", "--rois"]
    common[2] = a
    assert run_kalmanfilter.main(list(common)) == 0
    common[2] = b
    assert run_kalmanfilter.main(common + ["--strain", "--strain-video", avi, "--strain-which", "l1", "--strain-gain", "900",
                                           "--strain-alpha", "160"]) == 0
    za, zb = np.load(a), np.load(b)
    new = {"strain_J", "strain_l1", "strain_l2", "strain_axis", "strain_rotation", "strain_body_area", "strain_cell_J",
           "strain_cell_l1", "strain_cell_l2", "strain_artifact_r"}
    assert set(zb.files) == set(za.files) | new
    for key in za.files:
        assert za[key].dtype == zb[key].dtype and za[key].tobytes() == zb[key].tobytes(), key
    X, p, t = zb["X"], zb["p"], zb["t"]
    K, T = X.shape[0], t.shape[0]
    assert K == F - 1
    r = _renderer(p, t, n, n)
    d = strain.triangles(r, X)
    for key in ("J", "l1", "l2", "axis", "rotation", "body_area"):
        assert zb["strain_" + key].shape == ((K, T) if key != "body_area" else (K,))
        assert np.array_equal(zb["strain_" + key], d[key], equal_nan=True), key
    cells = len(zb["roi_points"])
    assert cells >= 1
    cl = strain.labels(r, X, labels=zb["roi_labels"], L=cells)
    for key in ("J", "l1", "l2"):
        assert zb["strain_cell_" + key].shape == (K, cells) and np.array_equal(zb["strain_cell_" + key], cl[key], equal_nan=True)
    assert np.array_equal(zb["strain_artifact_r"], strain.artifact_score(cl["J"], zb["roi_dff"]), equal_nan=True)
    # the restatement agrees; and the area of the tracked mesh is the field's, (1 + 1 / 300)^(2 (k + 1)), as far as a mesh
    # whose edge is held to the object's within a pixel can tell: (1 + 1 / 21)^2 - 1 < 0.1 of the disk's area
    ids = body_ref.body_map(p, t, n, n)[3]
    assert np.array_equal(strain_ref.strain_tri(X, r.uv, ids)[:, :, 0], d["J"])
    truth = (1.0 + 1.0 / 300.0) ** (2.0 * np.arange(1, K + 1))
    print("body area, tracked:", d["body_area"], "true:", truth)
    assert d["n_bad"].sum() == 0 and np.abs(d["body_area"] - truth).max() < 0.1
    info = read_avi(avi)
    assert info["total"] == K and (info["width"], info["height"]) == (n, n)
    lut = strain.default_lut()
    for k in range(K):
        want = strain_ref.view_strain(X[k], t, r.uv, ids, video[k + 1], 1, 900.0, 160, lut)
        assert np.array_equal(info["frames"][k], want), k
    assert (info["frames"][K - 1][:, :, 0] != info["frames"][K - 1][:, :, 2]).any()
    r.close()
