"""The body-frame readout on the GPU (`pytest -m gpu`): hm_body_map / hm_body_warp bit-equal to the NumPy restatement
(tests/body_ref.py) on small and full-size frames, golden tracks, large label sets and adversarial states; the device
call against the host call; the pipeline's readout against calls made afterwards, with the track unchanged; the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

import body_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _filter(dm, frame):
    from hydra_mi import kalman
    H, W = frame.shape
    return kalman.IteratedMSKalmanFilter(dm, frame, np.zeros((H, W, 2), np.float32), True)


def _check(r, dm, Xs, frames, labels=None):
    """hm_body_* of renderer r against the restatement for every (state, frame)"""
    H, W = r.ny, r.nx
    T = dm.t.shape[0]
    tri_of, l1, l2, ids = body_ref.body_map(np.asarray(dm.p, np.float32), dm.t, W, H)
    g_tri, g_cnt = r.body_map()
    assert np.array_equal(g_tri, tri_of)
    assert np.array_equal(g_cnt.astype(np.uint64), body_ref.counts(tri_of, T))
    L = 0
    if labels is not None:
        L = int(labels.max()) + 1
        keys = body_ref.label_keys(labels, tri_of)
        assert np.array_equal(r.body_set_labels(labels, L).astype(np.uint64), body_ref.counts(keys, L))
    for X, f in zip(Xs, frames):
        reg, ts, ls = r.body_warp(X, f)
        ref = body_ref.warp(X, f, tri_of, l1, l2, ids)
        assert np.array_equal(reg, ref)
        assert np.array_equal(ts, body_ref.sums(ref, tri_of, T))
        if L:
            assert ls.shape == (L,) and np.array_equal(ls, body_ref.sums(ref, keys, L))
    return tri_of


def _scene(name):
    from hydra_mi import mesh, synth
    rng = np.random.default_rng(len(name))
    if name == "16":
        dm = mesh.box_mesh(2.0, 3.0, 13.0, 12.5, 4.0)
        frames = [rng.integers(0, 256, (16, 16), dtype=np.uint8) for _ in range(3)]
    elif name == "33x17":                                   # an odd pixel count: the tail of k_body_warp
        dm = mesh.box_mesh(3.0, 2.0, 30.0, 14.5, 5.0)
        frames = [rng.integers(0, 256, (17, 33), dtype=np.uint8) for _ in range(3)]
    elif name == "96x160":
        dm = mesh.disk_mesh(80.0, 47.5, 40.0, 9.0)
        frames = [rng.integers(0, 256, (96, 160), dtype=np.uint8) for _ in range(3)]
    elif name == "config1":
        g = np.load(os.path.join(GOLD, "config1_track.npz"))
        video, _ = synth.test_data(128, 128)
        return mesh.Mesh(g["p"], g["t"], 15.0), list(g["X"]), [video[:, :, k] for k in range(10)], video[:, :, 0]
    else:
        g = np.load(os.path.join(GOLD, "config4_track.npz"))
        n = int(g["n"])
        video, _, _, _ = synth.disk_video(n, int(g["frames"]), "translate_leftup", 0)
        return mesh.Mesh(g["p"], g["t"], float(g["h0"]) * n), list(g["X"]), [video[k + 1] for k in range(3)], video[0]
    N = dm.size()
    Xs = []
    for s in (0.0, 0.7, 2.5):
        X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + rng.normal(0, s, 2 * N), rng.normal(0, 1, 2 * N)))
        Xs.append(X)
    return dm, Xs, frames, frames[0]


@pytest.mark.parametrize("name", ["16", "33x17", "96x160", "config1", "config4"])
def test_body_readout_equals_the_restatement(hm, name):
    dm, Xs, frames, f0 = _scene(name)
    kf = _filter(dm, f0)
    r = kf.state.renderer
    H, W = f0.shape
    rng = np.random.default_rng(7)
    labels = rng.integers(-1, 70000, (H, W)).astype(np.int32)
    labels[0, 0] = 69999
    _check(r, dm, Xs, frames, labels)
    white = [np.full((H, W), 255, np.uint8)] * 2
    _check(r, dm, Xs[:2], white, labels)
    reg, _, _ = r.body_warp(Xs[0], white[0])
    tri_of = r.body_map()[0]
    if name in ("16", "33x17", "96x160"):
        assert (reg[tri_of >= 0] == 255).all() and (reg[tri_of < 0] == 0).all()
    r.body_set_labels(None, 0)
    assert r.body_warp(Xs[0], frames[0])[2] is None
    from hydra_mi import _lib
    ls = np.empty(5, np.uint64)
    x = np.ascontiguousarray(Xs[0])
    f = np.ascontiguousarray(frames[0])
    assert _lib.lib().hm_body_warp(r._h, _lib.ptr(x), _lib.ptr(f), None, None, _lib.ptr(ls)) == -3
    assert b"no labels" in _lib.lib().hm_last_error()
    with pytest.raises(RuntimeError, match="outside -1"):
        r.body_set_labels(np.full((H, W), 3, np.int32), 3)
    assert r.body_labels[0] == 0 and r.body_warp(Xs[0], frames[0])[2] is None


def test_label_count_is_the_handles(hm):
    """The label sums are sized by the label image in place, whatever set it; a readout whose label image has been
    replaced on the tracker refuses to go on."""
    from hydra_mi import body, mesh
    H, W = 64, 80
    dm = mesh.disk_mesh(40.0, 30.0, 22.0, 7.0)
    rng = np.random.default_rng(11)
    f = rng.integers(0, 256, (H, W), dtype=np.uint8)
    kf = _filter(dm, f)
    r = kf.state.renderer
    X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + 0.4, np.zeros(2 * dm.size())))
    big = rng.integers(-1, 70000, (H, W)).astype(np.int32)
    b1 = body.BodyReadout(kf, points=np.array([[40.0, 30.0], [35.0, 25.0]]))
    _, _, m1 = b1.frame(X, f)
    assert m1.shape == (2,)
    r.body_set_labels(big, 70000)                           # the handle's label image replaced behind b1's back
    _, _, ls = r.body_warp(X, f)
    assert ls.shape == (70000,)
    with pytest.raises(RuntimeError, match="replaced"):
        b1.frame(X, f)
    small = np.where(big >= 0, big % 3, -1).astype(np.int32)
    b2 = body.BodyReadout(kf, labels=small)
    reg, _, m2 = b2.frame(X, f)
    tri_of, l1, l2, ids = body_ref.body_map(np.asarray(dm.p, np.float32), dm.t, W, H)
    keys = body_ref.label_keys(small, tri_of)
    assert m2.shape == (3,) and r.body_labels[0] == 3
    assert np.array_equal(b2.results()["label_sums"][0], body_ref.sums(reg, keys, 3))
    b3 = body.BodyReadout(kf)                               # no labels: clears the handle's
    assert r.body_labels[0] == 0 and b3.frame(X, f)[2].shape == (0,)
    with pytest.raises(RuntimeError, match="replaced"):
        b2.frame(X, f)


def test_adversarial_states(hm):
    from hydra_mi import mesh
    dm = mesh.disk_mesh(40.0, 30.0, 22.0, 7.0)
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (64, 80), dtype=np.uint8)
    kf = _filter(dm, f)
    N = dm.size()
    base = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + 0.3, np.zeros(2 * N)))
    t0 = dm.t[len(dm.t) // 2]
    Xs = []
    X = base.copy(); X[2 * t0[1]:2 * t0[1] + 2], X[2 * t0[2]:2 * t0[2] + 2] = base[2 * t0[2]:2 * t0[2] + 2], base[2 * t0[1]:2 * t0[1] + 2]
    Xs.append(X)                                            # a flipped triangle
    X = base.copy(); X[2 * t0[1]:2 * t0[1] + 2] = X[2 * t0[0]:2 * t0[0] + 2]; X[2 * t0[2]:2 * t0[2] + 2] = X[2 * t0[0]:2 * t0[0] + 2]
    Xs.append(X)                                            # a collapsed triangle
    X = base.copy(); X[2 * t0[0]] = np.nan
    Xs.append(X)                                            # a vertex at NaN
    X = base.copy(); X[2 * t0[0] + 1] = 1e30
    Xs.append(X)                                            # a vertex at 1e30
    X = base.copy(); X[:2 * N] = -3e6
    Xs.append(X)                                            # everything far off the frame
    _check(kf.state.renderer, dm, Xs, [f] * len(Xs), rng.integers(-1, 9, (64, 80)).astype(np.int32))


@pytest.mark.parametrize("H, W", [(72, 90), (17, 33)])
def test_device_call_with_three_channels_equals_the_host_call(hm, H, W):
    from hydra_mi import mesh
    from hydra_mi.pipeline import DeviceBuffer
    dm = mesh.box_mesh(20.0, 14.0, 70.0, 57.0, 9.0) if W == 90 else mesh.box_mesh(3.0, 2.0, 30.0, 14.5, 5.0)
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (H, W), dtype=np.uint8)
    kf = _filter(dm, f)
    r = kf.state.renderer
    labels = rng.integers(-1, 40, (H, W)).astype(np.int32)
    r.body_set_labels(labels, 40)
    N, T = dm.size(), dm.t.shape[0]
    X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + rng.normal(0, 1, 2 * N), np.zeros(2 * N)))
    reg, ts, ls = r.body_warp(X, f)
    d_f, d_o, d_s = DeviceBuffer(H * W), DeviceBuffer(3 * H * W), DeviceBuffer(8 * (T + 40))
    d_f.upload(f)
    r.body_warp_dev(X, d_f.ptr, d_o.ptr, 3, d_s.ptr, d_s.ptr + 8 * T)
    from hydra_mi import _lib
    _lib.check(_lib.lib().hm_ctx_sync(r._h), "hm_ctx_sync")
    out = np.empty((H, W, 3), np.uint8)
    sums = np.empty(T + 40, np.uint64)
    d_o.download(out)
    d_s.download(sums)
    assert np.array_equal(out, np.repeat(reg[:, :, None], 3, axis=2))
    assert np.array_equal(sums[:T], ts) and np.array_equal(sums[T:], ls)
    for b in (d_f, d_o, d_s):
        b.close()


def _pipeline_run(video, masks, c, rad, flow_batch, resident, body_args):
    from hydra_mi import body, kalman, mesh, videoio
    from hydra_mi.pipeline import FlowEKFPipeline
    n = video.shape[1]
    kf = kalman.IteratedMSKalmanFilter(mesh.disk_mesh(c[0], c[1], rad - 1.0, 12.0), video[0],
                                       np.zeros((n, n, 2), np.float32), True, nI=3)
    pipe = FlowEKFPipeline(kf, video, masks, flow_batch=flow_batch, resident=resident)
    got = []
    b = None
    if body_args is not None:
        b = body.BodyReadout(kf, **body_args)
    pipe.run(on_frame=lambda k, e: got.append((kf.state.X.copy(), tuple(e[:4]), kf.niter)), body=b)
    pipe.close()
    return kf, got, b


@pytest.mark.parametrize("resident", [True, False])
def test_pipeline_readout_changes_nothing_and_equals_later_calls(hm, tmp_path, resident):
    from hydra_mi import synth, videoio
    from test_views_cpu import read_avi
    n, F = 96, 24
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    _, plain, _ = _pipeline_run(video, masks, c, rad, 2, resident, None)
    pts = np.array([[c[0], c[1]], [c[0] + 10.0, c[1] - 7.5], [2.0, 2.0]])
    avi = videoio.AviWriter(str(tmp_path / "reg.avi"), n, n)
    kf, got, b = _pipeline_run(video, masks, c, rad, 2, resident, dict(points=pts, point_radius=4.0, video=avi))
    avi.close()
    assert len(got) == len(plain) == F - 1
    for (Xa, ea, ia), (Xb, eb, ib) in zip(plain, got):
        assert np.array_equal(Xa, Xb) and ea == eb and ia == ib
    res = b.results()
    assert res["tri_means"].shape == (F - 1, kf.state.tri.shape[0]) and res["points"].shape == (F - 1, 3, 2)
    assert np.isnan(res["points"][:, 2]).all() and np.isfinite(res["points"][:, :2]).all()
    avi_frames = read_avi(str(tmp_path / "reg.avi"))["frames"]
    assert len(avi_frames) == F - 1
    r = kf.state.renderer
    for k, (X, _, _) in enumerate(got):
        reg, ts, ls = r.body_warp(X, video[k + 1])
        assert np.array_equal(avi_frames[k], np.repeat(reg[:, :, None], 3, axis=2)), k
        assert np.array_equal(res["tri_sums"][k], ts), k
        assert np.array_equal(res["label_sums"][k], ls), k
        assert np.array_equal(res["points"][k], b.track(X), equal_nan=True), k


def test_cli_readout_on_both_paths(hm, tmp_path):
    from hydra_mi import synth
    from test_views_cpu import read_avi
    sys.path.insert(0, ROOT)
    import optical_flow_ext
    n, F = 96, 6
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    prefix = str(tmp_path / "flow")
    assert optical_flow_ext.main(["optical_flow_ext.py", vid, prefix]) == 0
    csv = tmp_path / "pts.csv"
    csv.write_text("a,%r,%r\nb,%r,%r\nout,1.0,1.0\n" % (c[0], c[1], c[0] - 8.0, c[1] + 5.0))
    for path, flow in (("files", prefix), ("inproc", str(tmp_path / "none"))):
        outs = {}
        for tag, extra in (("plain", []), ("body", ["--registered", str(tmp_path / (path + "_reg.avi")), "--points",
                                                     str(csv), "--point-radius", "2.5"])):
            out = str(tmp_path / ("%s_%s.npz" % (path, tag)))
            res = subprocess.run([sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, flow, out, "-s", "14"]
                                 + extra, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
            assert res.returncode == 0, res.stderr[-2000:]
            outs[tag] = (np.load(out), res.stdout)
        plain, body = outs["plain"][0], outs["body"][0]
        assert sorted(plain.files) == ["X", "err", "p", "t"]
        assert np.array_equal(plain["X"], body["X"]) and np.array_equal(plain["err"], body["err"])
        F1 = plain["X"].shape[0]
        assert body["tri_means"].shape == (F1, plain["t"].shape[0]) and body["points"].shape == (F1, 3, 2)
        assert body["point_means"].shape == (F1, 3) and body["point_counts"].shape == (3,)
        assert "outside the mesh" in outs["body"][1]
        assert read_avi(str(tmp_path / (path + "_reg.avi")))["total"] == F1
        lines = open(str(tmp_path / ("%s_body_points.txt" % path))).read().splitlines()
        assert len(lines) == F1 and all(l.startswith("neurons,") for l in lines)
        assert not os.path.exists(str(tmp_path / ("%s_plain_points.txt" % path)))


def test_tracked_config1_reads_out_still(hm):
    """config 1 tracked through compute with its exact flow, read out frame by frame: the body holds still"""
    from hydra_mi import body, kalman, mesh, synth
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    video, flow = synth.test_data(128, 128)
    kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), video[:, :, 0], flow[:, :, :, 0], True)
    b = body.BodyReadout(kf)
    inside = b.tri_of_pixel >= 0
    f0 = video[:, :, 0].astype(np.float64)
    for k in range(10):
        frame = video[:, :, k]
        kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
        reg, tri_means, _ = b.frame(kf.state.X, frame)
        assert np.abs(reg.astype(np.float64) - f0)[inside].mean() <= 2.0, k
    assert b.results()["tri_means"].shape == (10, g["t"].shape[0])
