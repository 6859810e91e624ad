"""The tracker's views on the GPU (`pytest -m gpu`): every view of hm_view / hm_view_forces bit-equal to the NumPy
restatement of tests/view_ref.py composed from Renderer.render(); views taken between frames change nothing the filter
computes; the pipeline's overlay video, the CLI's .avi output and the flow tools' preview videos."""
import os
import subprocess
import sys

import numpy as np
import pytest

import view_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
VIEWS = ("raw", "overlay", "texture", "mask", "flowx", "flowy")


def _scene(name):
    """-> (filter, frame, flow, mask, state X) of a scene: the config 1 mesh at 128^2, a box mesh at 90 x 72, the
    bench's 201-vertex mesh at 1024^2"""
    from hydra_mi import kalman, mesh, synth
    rng = np.random.default_rng(len(name))
    if name == "config1":
        g = np.load(os.path.join(GOLD, "config1_track.npz"))
        video, flow = synth.test_data(128, 128)
        dm = mesh.Mesh(g["p"], g["t"], 15.0)
        frame, fl = video[:, :, 1], flow[:, :, :, 1]
    elif name == "90x72":
        H, W = 72, 90
        frame = np.zeros((H, W), np.uint8)
        frame[14:58, 20:71] = rng.integers(60, 250, (44, 51), dtype=np.uint8)
        fl = rng.normal(0, 2, (H, W, 2)).astype(np.float32)
        dm = mesh.box_mesh(20.0, 14.0, 70.0, 57.0, 9.0)
        g = None
    else:
        g = np.load(os.path.join(GOLD, "config4_track.npz"))
        n = int(g["n"])
        video, masks, centre, radius = synth.disk_video(n, 2, "translate_leftup", 0)
        dm = mesh.disk_mesh(centre[0], centre[1], radius - 1.0, float(g["h0"]) * n)
        assert dm.size() == 201
        frame = video[1]
        fl = rng.normal(0, 3, (n, n, 2)).astype(np.float32)
    mask = (frame > 0).astype(np.uint8)
    kf = kalman.IteratedMSKalmanFilter(dm, frame, fl, True)
    r = kf.state.renderer
    r.set_observation(frame, fl, mask)
    N = dm.size()
    X = np.array(kf.state.X, np.float64).reshape(-1).copy()
    X[:2 * N] += rng.normal(0, 1.5, 2 * N)                   # off the texture's own positions, non-integer
    X[2 * N:] = rng.normal(0, 1.0, 2 * N)                    # velocities: a non-trivial rendered flow
    return kf, frame, fl, mask, X


@pytest.mark.parametrize("name", ["config1", "90x72", "1024"])
def test_views_equal_the_restatement(hm, name):
    kf, frame, fl, mask, X = _scene(name)
    r = kf.state.renderer
    N = r.n
    r.update_vertex_buffer(X[:2 * N], X[2 * N:])
    render = r.render()
    tri = r.tri
    for which in ("raw", "overlay", "texture", "flowx", "flowy"):
        got = r.view(X, which)
        want = view_ref.view(which, render, tri, X, obs=frame)
        assert got.shape == (r.ny, r.nx, 3) and got.dtype == np.uint8
        assert np.array_equal(got, want), (name, which, np.argwhere(got != want)[:5])
    assert view_ref.wire_count(tri, X, r.nx, r.ny).max() >= 2          # interior edges are drawn twice
    # the mask palette: every triangle the same label (0: G = B = 0; -1: 255, 255, saturated)
    T = tri.shape[0]
    keep = r.labels_hess
    try:
        for label in (0, -1):
            r.labels_hess = np.full((T, 2), label, np.int64)
            got = r.view(X, "mask")
            want = view_ref.view("mask", render, tri, X, ids=view_ref.uniform_ids(render[3], label))
            assert np.array_equal(got, want), (name, label)
    finally:
        r.labels_hess = keep
    # the filter's own palette (labels_hess[:, 1]): R is the mesh's coverage, G B decode to labels of the table where a
    # pixel is covered once and no edge runs through it
    got = r.view(X, "mask")
    assert np.array_equal(got[:, :, 2], np.where(render[3] > 0, 255, 0))
    # forces: the overlay halved, then the four layers of arrows
    rng = np.random.default_rng(7)
    orig = X + rng.normal(0, 2, X.shape)
    tv, fv, mv = (rng.normal(0, 0.8, X.shape) for _ in range(3))
    got = r.view_forces(X, orig, X, tv, fv, mv)
    want = view_ref.forces(r.view(X, "overlay"), orig, X, tv, fv, mv, N)
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
    kf.close()


def test_view_names_and_sizes(hm):
    from hydra_mi import kalman, mesh, synth
    video, flow = synth.test_data(64, 64)
    kf = kalman.IteratedMSKalmanFilter(mesh.box_mesh(21.0, 22.0, 42.0, 43.0, 10.0), video[:, :, 0], flow[:, :, :, 0], True)
    r = kf.state.renderer
    assert r.view(None, "raw").shape == (64, 64, 3)
    with pytest.raises(KeyError):
        r.view(None, "outline")
    with pytest.raises(ValueError):
        r.view(np.zeros(5), "raw")
    kf.close()


def test_views_between_frames_change_nothing(hm, tmp_path):
    """Config 1 tracked for 10 frames with every view, the forces and the screenshots of compute(imageoutput=) after
    every frame: states and iteration counts bit-equal to the same run without."""
    from hydra_mi import kalman, mesh, synth
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    video, flow = synth.test_data(128, 128)
    runs = {}
    for views in (False, True):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), video[:, :, 0], flow[:, :, :, 0], True)
        out = []
        for k in range(10):
            frame = video[:, :, k]
            shot = str(tmp_path / ("f%d" % k)) if views and k % 3 == 0 else None
            e = kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8), imageoutput=shot)
            if views:
                for w in VIEWS:
                    kf.state.renderer.view(kf.state.X, w)
            out.append((kf.state.X.copy(), kf.niter, e[:4]))
        runs[views] = out
        kf.close()
    for (Xa, ia, ea), (Xb, ib, eb) in zip(runs[False], runs[True]):
        assert np.array_equal(Xa, Xb) and ia == ib and ea == eb
    for v in VIEWS + ("forces",):
        assert os.path.exists(str(tmp_path / ("f0_%s.png" % v))), v
    from hydra_mi.videoio import read_png
    assert read_png(str(tmp_path / "f9_overlay.png")).shape == (128, 128, 3)


def test_pipeline_video_equals_the_overlay_views(hm, tmp_path):
    """FlowEKFPipeline.run(video=) over two phases: every AVI frame is Renderer.view(X_k, "overlay") taken in on_frame,
    and the states are those of the run without video."""
    from hydra_mi import kalman, mesh, synth
    from hydra_mi.pipeline import FlowEKFPipeline
    from hydra_mi.videoio import AviWriter
    from test_views_cpu import read_avi
    n, F = 96, 9
    video, masks, c, rad = synth.disk_video(n, F, "warp", 1)
    zero = np.zeros((n, n, 2), np.float32)
    results = {}
    for with_video in (False, True):
        kf = kalman.IteratedMSKalmanFilter(mesh.disk_mesh(c[0], c[1], rad - 1.0, 14.0), video[0], zero, True, nI=4)
        pipe = FlowEKFPipeline(kf, video, masks, flow_batch=3)
        seen = []

        def on_frame(k, e):
            seen.append((kf.state.X.copy(), kf.state.renderer.view(kf.state.X, "overlay") if with_video else None))
        path = str(tmp_path / "pipe.avi")
        w = AviWriter(path, n, n) if with_video else None
        pipe.run(0, 4, on_frame=on_frame, video=w)
        pipe.run(4, None, on_frame=on_frame, video=w)
        pipe.close()
        if w is not None:
            w.close()
        results[with_video] = seen
        kf.close()
    assert len(results[True]) == F - 1
    for (Xa, _), (Xb, _) in zip(results[False], results[True]):
        assert np.array_equal(Xa, Xb)
    info = read_avi(str(tmp_path / "pipe.avi"))
    assert info["total"] == F - 1
    for k, (fr, (_, ov)) in enumerate(zip(info["frames"], results[True])):
        assert np.array_equal(fr, ov), k


def test_cli_writes_the_overlay_video(hm, tmp_path):
    from hydra_mi import synth
    from test_views_cpu import read_avi
    n, F = 96, 5
    video, masks, c, r = synth.disk_video(n, F, "translate_leftup", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    env = dict(os.environ)
    outs = {}
    for out in ("out.npz", "out.avi"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none"),
                              str(tmp_path / out), "-s", "14"], capture_output=True, text=True, timeout=240, env=env,
                             cwd=str(tmp_path))
        assert res.returncode == 0, res.stderr[-2000:]
        outs[out] = np.load(str(tmp_path / (out if out.endswith(".npz") else out + ".npz")))
    assert np.array_equal(outs["out.npz"]["X"], outs["out.avi"]["X"])
    assert np.array_equal(outs["out.npz"]["err"], outs["out.avi"]["err"])
    info = read_avi(str(tmp_path / "out.avi"))
    assert info["total"] == F - 1 and (info["width"], info["height"]) == (n, n)
    assert not os.path.exists(str(tmp_path / "screenshots"))


def test_flow_preview_tools_agree_and_match_the_restatement(hm, tmp_path):
    from hydra_mi import matio, synth, videoio
    from test_views_cpu import read_avi
    sys.path.insert(0, ROOT)
    import optical_flow_ext
    exe = os.path.join(ROOT, "kalman-hydra_amd", "optical_flow_ext")
    n, F = 80, 5
    video, _, _, _ = synth.disk_video(n, F, "rotate", 3)
    rng = np.random.default_rng(0)
    colour = np.clip(video[..., None].astype(np.int32) + rng.integers(-20, 21, video.shape + (3,)), 0, 255).astype(np.uint8)
    for name, arr in (("gray", video), ("bgr", colour)):
        fn = str(tmp_path / (name + ".npy"))
        np.save(fn, arr)
        os.environ["HYDRA_MI_FLOW_PREVIEW"] = "1"
        try:
            assert optical_flow_ext.main(["optical_flow_ext.py", fn, str(tmp_path / (name + "_py"))]) == 0
        finally:
            del os.environ["HYDRA_MI_FLOW_PREVIEW"]
        env = dict(os.environ, HYDRA_MI_FLOW_BATCH="3", HYDRA_MI_FLOW_PREVIEW="1")
        res = subprocess.run([exe, fn, str(tmp_path / (name + "_cc"))], capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 0, res.stderr
        a = open(str(tmp_path / (name + "_py.avi")), "rb").read()
        b = open(str(tmp_path / (name + "_cc.avi")), "rb").read()
        assert a == b
        info = read_avi(str(tmp_path / (name + "_py.avi")))
        assert info["total"] == F - 1
        for k in range(F - 1):
            fx = matio.read_mat(str(tmp_path / ("%s_py_%03d_x.mat" % (name, k))))
            fy = matio.read_mat(str(tmp_path / ("%s_py_%03d_y.mat" % (name, k))))
            want = view_ref.flow_preview(arr[k + 1], fx, fy)
            got = info["frames"][k]
            d = np.abs(got.astype(int) - want.astype(int))
            assert d.max() <= 1, (name, k, d.max())
            # a difference only where the f32 arctangent may differ by an ulp: compare the wheel alone there
            if d.max():
                w = view_ref.wheel(fx, fy)
                assert np.count_nonzero(d) <= max(8, d.size // 1000), (name, k, np.count_nonzero(d))
                assert w.shape == got.shape
        # the device form on the whole video at once equals what the tools wrote
        fxs = np.stack([matio.read_mat(str(tmp_path / ("%s_py_%03d_x.mat" % (name, k)))) for k in range(F - 1)])
        fys = np.stack([matio.read_mat(str(tmp_path / ("%s_py_%03d_y.mat" % (name, k)))) for k in range(F - 1)])
        allp = videoio.flow_preview(arr[1:], fxs, fys)
        assert all(np.array_equal(allp[k], info["frames"][k]) for k in range(F - 1))
    # the wheel on a grid of vectors against the restatement: saturation past 15 px, non-finite flow black
    g = np.linspace(-40, 40, 161, dtype=np.float32)
    gx, gy = np.meshgrid(g, g)
    gx[0, 0] = np.nan
    gy[1, 1] = np.inf
    gray = np.zeros((1,) + gx.shape, np.uint8)
    got = videoio.flow_preview(gray, gx[None], gy[None])[0]
    want = view_ref.flow_preview(gray[0], gx, gy)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    assert np.count_nonzero(got != want) <= gx.size // 100
    assert not got[0, 0].any() and not got[1, 1].any()
