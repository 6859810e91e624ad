"""The cell view on the GPU (`pytest -m gpu`): hm_view_cells / hm_view_cells_dev equal to the NumPy restatement of
tests/cellview_ref.py in every byte; the view between frames changes nothing the filter computes; the overlay video of
hydra_mi.cellview.write_video, frame by frame and against the true mesh states."""
import os

import numpy as np
import pytest

import cellview_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

# the kernel's constants (csrc/view_kernels.h): a CV_W x CV_H strip per workgroup, CV_CAP candidates per batch in LDS
CV_W, CV_H, CV_CAP = 64, 16, 32
# 40 x 24: W H a multiple of 4, every row of a strip starts on a dword; 37 x 29: rows start at every offset within a dword,
# single bytes at both ends of a strip's rows and at the end of the image; 65 x 17 = (CV_W + 1) x (CV_H + 1): a last strip
# of one column and a last strip of one row
SIZES = [(40, 24), (37, 29), (CV_W + 1, CV_H + 1)]


def _renderer(p, t, W, H, seed=0):
    from hydra_mi import mesh, renderer
    dm = mesh.Mesh(np.asarray(p, np.float64), np.asarray(t, np.int64), 1.0)
    tex = np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    return renderer.Renderer(dm, np.zeros_like(dm.p), np.zeros((H, W, 2), np.float32), H, tex, True, 1.0, 1.0, 1.0)


def _cells(W, H, L, n_layers, rng, weights=True):
    """blocky label planes (cells share edges, touch the frame border and each other), weights and levels from the
    values at which the blend can go wrong, random colours"""
    lab = np.empty((n_layers, H, W), np.int32)
    for j in range(n_layers):
        b = 3 + j
        blocks = rng.integers(-1, L, ((H + b - 1) // b, (W + b - 1) // b))
        lab[j] = np.kron(blocks, np.ones((b, b), np.int64))[:H, :W]
    lab[0, :2, :] = L - 1                               # a cell along the top border, one in the bottom right corner
    lab[0, -3:, -4:] = 0
    w = rng.choice(np.array([0, 1, 32768, 65535], np.uint16), (n_layers, H, W)) if weights else None
    lev = rng.choice(np.array([0, 1, 128, 255], np.uint8), L)
    col = rng.integers(0, 256, (L, 3), dtype=np.uint8)
    return lab, w, lev, col


def _disk(W, H):
    from hydra_mi import mesh
    rad = 0.38 * min(W, H)
    dm = mesh.disk_mesh(0.5 * W - 1.3, 0.5 * H + 0.4, rad, 0.62 * rad)
    assert 9 <= dm.size() <= 16, dm.size()             # about 12 vertices
    return dm.p, dm.t


def _area(p, t):
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def _disk_states(p, t):
    c = p.mean(axis=0)
    ang = np.deg2rad(30.0)
    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    q = (p - c) @ rot.T
    q[:, 0] *= 1.3
    # an interior vertex (the one nearest the centre) pushed across its opposite edges: a folded mesh -- triangles overlap
    # and some change orientation; the lowest index must win and the swap must hold
    v = int(np.argmin(np.hypot(*(p - c).T)))
    fold = p.copy()
    fold[v] += (0.9 * (p[:, 0].max() - c[0]), 0.35)
    assert (np.sign(_area(fold, t)) != np.sign(_area(p, t))).any()
    return {"rest": p, "rotated": q + c + (0.37, -0.21), "folded": fold}


def _square(W, H):
    x0, y0, x1, y1 = 0.2 * W, 0.15 * H, 0.8 * W, 0.85 * H
    p = np.array([[x0, y0], [x1, y0 + 0.3], [x1 - 0.6, y1], [x0 + 0.25, y1 - 0.4]])
    return p, np.array([[0, 1, 2], [0, 2, 3]])


def _square_states(p):
    s = {"rest": p}
    q = p.copy()
    q[1] = 0.5 * (p[0] + p[2])                           # vertex 1 on the edge 0-2: triangle 0 has area 0 and is skipped
    q = np.rint(q * 4) / 4                               # (exactly: quarters survive the snap)
    q[1] = 0.5 * (q[0] + q[2])
    s["degenerate"] = q
    q = p.copy()
    q[3] = np.nan                                        # triangle 1 is skipped, triangle 0 drawn
    s["nan"] = q
    q = p.copy()
    q[1, 0] += 50.0 + p[:, 0].max()                      # 50 px and more beyond the frame
    s["outside"] = q
    q = p.copy()
    q[2] = (2.0 ** 20 + 4096.0, 2.0 ** 20 + 512.0)       # beyond 2^20 px: still within the rasteriser's range, and drawn
    s["far"] = q
    q = p.copy()
    q[2, 1] = 2.0 ** 25                                  # beyond d_tri_sane: both triangles skipped
    s["insane"] = q
    return s


def _markers(W, H, P, rng):
    pts = np.column_stack((rng.uniform(-3, W + 3, P), rng.uniform(-3, H + 3, P)))
    fixed = [(-0.9, 5.5), (W - 0.2, 7.0), (9.3, -0.5), (11.0, H - 0.01), (W + 30.0, 3.0), (np.nan, 4.0), (3.0, np.inf),
             (12.2, 9.7), (13.9, 10.1), (-2.0 ** 21, 3.0)]            # the four borders, off the frame, not finite, overlapping, far
    for i, q in enumerate(fixed[:P]):
        pts[i] = q
    return pts, rng.integers(0, 256, (P, 3), dtype=np.uint8)


def _compare(r, X, frame, cells, tag, **kw):
    lab, w, lev, col = cells if cells is not None else (None, None, None, None)
    got = r.view_cells(X, frame, lev, **kw)
    want = cellview_ref.view_cells(X, r.tri, r.uv, frame, lab, w, col, lev, **kw)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:5])
    return got


@pytest.mark.parametrize("W,H", SIZES)
def test_cell_view_equals_the_restatement(hm, W, H):
    rng = np.random.default_rng(W)
    frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
    cells = _cells(W, H, 5, 2, rng)
    pts, pc = _markers(W, H, 10, rng)
    for mesh_name, (p, t), states in (("disk", _disk(W, H), None), ("square", _square(W, H), None)):
        states = _disk_states(p, t) if mesh_name == "disk" else _square_states(p)
        r = _renderer(p, t, W, H)
        r.view_set_cells(cells[0], cells[1], cells[3])
        painted = {}
        for name, q in states.items():
            X = np.concatenate((q.reshape(-1), np.zeros(q.size)))
            for outline, wire in ((True, True), (False, False)):
                img = _compare(r, X, frame, cells, (mesh_name, name, outline, wire), outline=outline, wire=wire, points=pts,
                               point_colours=pc, point_radius=2)
            painted[name] = int((img != np.repeat(frame[:, :, None], 3, axis=2)).any(axis=2).sum())
        if mesh_name == "square":
            assert painted["insane"] <= painted["nan"] < painted["rest"] and painted["degenerate"] < painted["rest"]
        r.close()


@pytest.mark.parametrize("n_layers,L,weights,levels", [(1, 1, True, True), (2, 300, True, True), (4, 7, True, True),
                                                       (2, 7, False, True), (2, 7, True, False), (1, 300, False, False)])
def test_cells_layers_labels_weights_levels(hm, n_layers, L, weights, levels):
    W, H = 40, 24
    rng = np.random.default_rng(n_layers * 1000 + L)
    frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
    p, t = _disk(W, H)
    X = _disk_states(p, t)["rotated"].reshape(-1)         # 2N values: the positions alone
    r = _renderer(p, t, W, H)
    lab, w, lev, col = _cells(W, H, L, n_layers, rng, weights)
    if L == 300:
        lab[0, 8:14, 10:30] = np.arange(280, 300)[None, :]         # labels past a byte under the mesh
    r.view_set_cells(lab, w, col)
    cells = (lab, w, lev if levels else None, col)
    for outline in (True, False):
        for wire in (True, False):
            _compare(r, X, frame, cells, (outline, wire), outline=outline, wire=wire)
    r.close()


@pytest.mark.parametrize("P,radius", [(0, 2), (1, 0), (1, 9), (10, 2), (70, 0), (70, 2), (70, 9)])
def test_markers(hm, P, radius):
    W, H = 37, 29
    rng = np.random.default_rng(P + radius)
    frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
    p, t = _disk(W, H)
    X = np.concatenate((p.reshape(-1) + 0.3, np.zeros(p.size)))
    r = _renderer(p, t, W, H)
    cells = _cells(W, H, 4, 1, rng)
    pts, pc = _markers(W, H, P, rng)                      # 70 points: more than one wave's worth of them, on top of each other
    r.view_set_cells(cells[0], cells[1], cells[3])
    _compare(r, X, frame, cells, "cells", points=pts, point_colours=pc, point_radius=radius)
    if P:
        r.view_set_cells(None)                            # cleared cells, then markers alone
        got = _compare(r, X, frame, None, "markers only", points=pts, point_colours=pc, point_radius=radius)
        untouched = np.ones((H, W), bool)
        for x, y in pts:
            if np.isfinite(x) and np.isfinite(y) and abs(x) < 1e6:
                yy, xx = np.mgrid[0:H, 0:W]
                untouched &= (xx - int(x)) ** 2 + (yy - int(y)) ** 2 > radius * radius
        assert np.array_equal(got[untouched], np.repeat(frame[:, :, None], 3, axis=2)[untouched])
    r.close()


def test_a_strip_with_more_candidates_than_one_batch(hm):
    """A disc of radius 40 meshed at 5 px in a 100 x 52 frame: the strips through its middle meet several times CV_CAP = 32
    triangles, so the kernel's LDS list is refilled within a strip."""
    from hydra_mi import mesh
    W, H = 100, 52
    dm = mesh.disk_mesh(48.7, 27.2, 40.0, 5.0)
    p, t = dm.p, dm.t
    ang = np.deg2rad(-12.0)
    q = (p - p.mean(0)) @ np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]).T * 1.05 + p.mean(0) + (1.4, -0.8)
    lo, hi = q[t].min(axis=1), q[t].max(axis=1)
    in_strip = (hi[:, 0] >= 0) & (lo[:, 0] < CV_W) & (hi[:, 1] >= CV_H) & (lo[:, 1] < 2 * CV_H)
    assert in_strip.sum() > 2 * CV_CAP, in_strip.sum()
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
    cells = _cells(W, H, 9, 2, rng)
    r = _renderer(p, t, W, H)
    r.view_set_cells(cells[0], cells[1], cells[3])
    _compare(r, np.concatenate((q.reshape(-1), np.zeros(q.size))), frame, cells, "fine", outline=True, wire=True)
    r.close()


def test_device_form_and_back_to_back_calls(hm):
    """hm_view_cells_dev followed by a copy equals hm_view_cells; two calls queued back to back with different levels,
    points and states, their host arrays overwritten right after each call, each equal their restatement."""
    from hydra_mi import _lib
    from hydra_mi.pipeline import DeviceBuffer
    W, H = 37, 29
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
    p, t = _disk(W, H)
    r = _renderer(p, t, W, H)
    lab, w, _, col = _cells(W, H, 6, 2, rng)
    r.view_set_cells(lab, w, col)
    d_frame = DeviceBuffer(W * H)
    d_frame.upload(frame)
    want, outs = [], []
    for k in range(6):                                     # more calls than the handle has staging slots
        X = np.concatenate((p.reshape(-1) + rng.normal(0, 1.0, p.size), np.zeros(p.size)))
        lev = rng.integers(0, 256, 6, dtype=np.uint8)
        pts, pc = _markers(W, H, 3 + 5 * k, rng)
        want.append(cellview_ref.view_cells(X, r.tri, r.uv, frame, lab, w, col, lev, points=pts, point_colours=pc))
        if k == 0:
            host = r.view_cells(X, frame, lev, points=pts, point_colours=pc)
            assert np.array_equal(host, want[0])
        outs.append(DeviceBuffer(3 * W * H))
        r.view_cells_dev(X, d_frame.ptr, outs[-1].ptr, lev, points=pts, point_colours=pc)
        X[:] = -1.0                                        # the call has taken its copies
        lev[:] = 0
        pts[:] = 5.0
        pc[:] = 0
    _lib.check(_lib.lib().hm_ctx_sync(r._h), "hm_ctx_sync")
    for k, d in enumerate(outs):
        got = d.download(np.empty((H, W, 3), np.uint8))
        assert np.array_equal(got, want[k]), k
        d.close()
    d_frame.close()
    r.close()


def test_refusals_leave_the_handle_working(hm):
    from hydra_mi import _lib
    W, H = 40, 24
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
    p, t = _disk(W, H)
    X = np.concatenate((p.reshape(-1), np.zeros(p.size)))
    r = _renderer(p, t, W, H)
    L = _lib.lib()
    with pytest.raises(RuntimeError, match="code -3.*nothing to draw"):
        r.view_cells(X, frame)                              # no cells, no points
    lab, w, lev, col = _cells(W, H, 3, 1, rng)
    bad = lab.copy()
    bad[0, 4, 7] = 3
    with pytest.raises(RuntimeError, match="code -1.*label 3 at pixel %d" % (4 * W + 7)):
        r.view_set_cells(bad, w, col)
    with pytest.raises(RuntimeError, match="nothing to draw"):
        r.view_cells(X, frame)                              # the refused cells were not set
    five = np.repeat(lab, 5, axis=0)
    with pytest.raises(RuntimeError, match="code -1.*n_layers 5 outside 1..4"):
        r.view_set_cells(five, None, col)
    pts, pc = _markers(W, H, 2, rng)
    with pytest.raises(RuntimeError, match="code -1.*radius -1"):
        r.view_cells(X, frame, points=pts, point_colours=pc, point_radius=-1)
    assert L.hm_view_cells(None, None, None, None, 0, 0, None, None, 2, None) == -1
    r.view_set_cells(lab, w, col)
    _compare(r, X, frame, (lab, w, lev, col), "after the refusals", points=pts, point_colours=pc)
    r.close()


def test_views_between_frames_change_nothing(hm):
    """Config 1 (128^2, the golden track) with a cell view between every two frames: states, covariance and error terms
    bit-identical to the run without -- what test_views_gpu states for hm_view, held for the new view."""
    from hydra_mi import kalman, mesh, synth
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    video, flow = synth.test_data(128, 128)
    rng = np.random.default_rng(2)
    cells = _cells(128, 128, 6, 2, rng)
    pts, pc = _markers(128, 128, 10, rng)
    runs = {}
    for views in (False, True):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), video[:, :, 0], flow[:, :, :, 0], True)
        if views:
            kf.state.renderer.view_set_cells(cells[0], cells[1], cells[3])
        out = []
        for k in range(10):
            frame = video[:, :, k]
            e = kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
            if views:
                img = kf.state.renderer.view_cells(kf.state.X, frame, cells[2], outline=True, wire=True, points=pts, point_colours=pc)
                assert (img[:, :, 0] != img[:, :, 2]).any()
            out.append((kf.state.X.copy(), kf.niter, e[:4], np.array(kf.state.W, np.float64).copy()))
        runs[views] = out
        kf.close()
    for (Xa, ia, ea, Wa), (Xb, ib, eb, Wb) in zip(runs[False], runs[True]):
        assert np.array_equal(Xa, Xb) and ia == ib and ea == eb and np.array_equal(Wa, Wb)


# The largest distance, over the frames and the two cells, between the centroid of a cell's pixels in the written video
# (drawn at the TRACKED states) and the centroid the restatement draws at the TRUE mesh states -- the tracker's error seen
# through the view.  Measured on one MI355X: 1.0000 px (the video is a pure translation, so the two drawings of a cell
# are the same shape a whole pixel apart); held at + 25 %, as TRUE_STATE_BOUND of test_configs_gpu.py.
E2E_MEASURED = 1.0
E2E_BOUND = 1.25 * E2E_MEASURED


def test_overlay_video_end_to_end(hm, tmp_path):
    from hydra_mi import cellview, kalman, mesh, synth
    from hydra_mi.pipeline import FlowEKFPipeline
    from test_views_cpu import read_avi
    name, n, frames = "translate_leftup", 256, 8
    video, masks, c, rad = synth.disk_video(n, frames, name, 5)
    dm = mesh.disk_mesh(c[0], c[1], rad - 2.0, 0.1 * n)
    N = dm.size()
    field = synth.scaled_field(name, n)
    true_p = [np.asarray(dm.p, np.float64).copy()]
    for _ in range(frames - 1):
        vx, vy = field(true_p[-1][:, 0], true_p[-1][:, 1])
        true_p.append(true_p[-1] + np.column_stack((vx * np.ones(N), vy * np.ones(N))))
    kf = kalman.IteratedMSKalmanFilter(dm, video[0], np.zeros((n, n, 2), np.float32), True)
    pipe = FlowEKFPipeline(kf, video, masks, flow_batch=4)
    states = []
    pipe.run(on_frame=lambda k, e: states.append(kf.state.X.reshape(-1).copy()))
    pipe.close()
    assert len(states) == frames - 1
    # two cells of radius 5 inside the object, in body coordinates (the frame-0 grid)
    yy, xx = np.mgrid[0:n, 0:n]
    lab = np.full((n, n), -1, np.int32)
    centres = [(c[0] - 0.4 * rad, c[1] + 0.2 * rad), (c[0] + 0.45 * rad, c[1] - 0.3 * rad)]
    for s, (x, y) in enumerate(centres):
        lab[(xx + 0.5 - x) ** 2 + (yy + 0.5 - y) ** 2 <= 25.0] = s
    pts = np.array(centres)
    path = str(tmp_path / "cells.avi")
    r = kf.state.renderer
    assert cellview.write_video(kf, states, video[1:], path, cells=lab, points=pts, point_radius=0) == frames - 1
    info = read_avi(path)
    assert info["total"] == frames - 1 and (info["width"], info["height"]) == (n, n)
    col = cellview.palette(2)
    layers, w = cellview.layers_from_labels(lab)
    r.view_set_cells(layers, w, col)
    from hydra_mi import body as bt
    t_of, ids, l1, l2 = bt.locate(r.uv, r.tri, pts)
    worst = 0.0
    for k in range(frames - 1):
        p_k = bt.track(states[k][:2 * N], ids, l1, l2, t_of >= 0)
        one = r.view_cells(states[k], video[k + 1], None, points=p_k, point_colours=col, point_radius=0)
        want = cellview_ref.view_cells(states[k], r.tri, r.uv, video[k + 1], layers, w, col, None, points=p_k, point_colours=col,
                                       point_radius=0)
        assert np.array_equal(info["frames"][k], one), k
        assert np.array_equal(one, want), k
        truth = cellview_ref.view_cells(true_p[k + 1].reshape(-1), r.tri, r.uv, video[k + 1], layers, w, col, None)
        for s in range(2):
            a = np.argwhere((info["frames"][k] == col[s]).all(axis=2))
            b = np.argwhere((truth == col[s]).all(axis=2))
            assert len(a) > 40 and len(b) > 40, (k, s, len(a), len(b))
            worst = max(worst, float(np.hypot(*(a.mean(axis=0) - b.mean(axis=0)))))
    kf.close()
    print("cell centroids, tracked against true states: worst %.4f px" % worst)
    assert worst <= E2E_BOUND, worst
