"""The statistics of the registered video on the GPU (`pytest -m gpu`): hm_body_stats_* equal to the NumPy restatement
(tests/bodystats_ref.py) -- the sums as integers, the images bit for bit, the peaks with their order --, at the limits of
values, maps and capacity, through the pipeline, and down to cells planted in a video and found again."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import bodystats_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_sums(r, regs, m):
    s1, s2, cross, vmax = r.body_stats_fetch()
    want = ref.accumulate(np.array(regs), m)
    assert r.body_stats_count() == len(regs)
    assert np.array_equal(s1, want[0]) and np.array_equal(s2, want[1])
    assert np.array_equal(cross, want[2]) and np.array_equal(vmax, want[3])
    return want


def _check_images(r, want, F, m):
    mean, std, corr, vmax = r.body_stats_images()
    rm, rs, rc, rx = ref.images(*want, F, m)
    assert np.array_equal(_bits(mean), _bits(rm))
    assert np.array_equal(_bits(std), _bits(rs))
    assert np.array_equal(_bits(corr), _bits(rc))
    assert np.array_equal(vmax, rx)
    assert np.isnan(mean[~m]).all() and np.isnan(std[~m]).all() and np.isnan(corr[~m]).all() and (vmax[~m] == 0).all()
    return rm, rs, rc, rx


def _check_peaks(r, imgs, m, radii=(1, 6, 16), brute=False):
    for which in ("corr", "std", "range"):
        score = ref.score_image(which, *imgs)
        thr = float(np.median(score[m]))
        for radius in radii:
            for min_score in (-np.inf, thr):
                find = ref.peaks if brute else ref.peaks_fast
                wi, ws = find(score, m, radius, min_score)
                gi, gs, n = r.body_stats_peaks(which, radius, min_score)
                assert n == len(wi), (which, radius, min_score)
                assert np.array_equal(gi, wi) and np.array_equal(_bits(gs), _bits(ws)), (which, radius, min_score)
                cap = max(len(wi) // 2, 1)
                gi, gs, n = r.body_stats_peaks(which, radius, min_score, cap=cap)
                assert n == len(wi) and np.array_equal(gi, wi[:cap]) and np.array_equal(_bits(gs), _bits(ws[:cap]))


@pytest.mark.parametrize("name", cases.NAMES)
def test_statistics_equal_the_restatement(hm, name):
    dm, Xs, frames, f0 = cases.scene(name)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    r.body_stats_begin()
    assert r.body_stats_count() == 0
    regs = []
    for k, (X, f) in enumerate(zip(Xs, frames)):
        regs.append(r.body_warp(X, f)[0])
        if k < 2 or k == len(frames) - 1:
            want = _check_sums(r, regs, m)
            imgs = _check_images(r, want, len(regs), m)
    _check_peaks(r, imgs, m, brute=name == "16")
    r.body_stats_end()
    kf.close()


def test_limits_of_values_and_maps(hm):
    from hydra_mi import _lib, mesh
    H, W = 24, 20
    dm = mesh.box_mesh(2.0, 3.0, 17.0, 20.5, 5.0)
    rng = np.random.default_rng(1)
    f0 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1), np.zeros(2 * dm.size())))
    const = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for video in ([np.full((H, W), 255, np.uint8)] * 3, [np.zeros((H, W), np.uint8)] * 2, [const] * 3, [f0]):
        r.body_stats_begin()
        regs = [r.body_warp(X, f)[0] for f in video]
        want = _check_sums(r, regs, m)
        imgs = _check_images(r, want, len(regs), m)
        mean, std, corr, vmax = r.body_stats_images()
        assert (std[m] == 0).all() and (corr[m] == 0).all()            # var = 0 everywhere (one frame included)
        _check_peaks(r, imgs, m, radii=(1, 6), brute=True)
    idx, sc, n = r.body_stats_peaks("corr", 2)                         # every map pixel ties: the tie rule alone
    assert n >= 1 and idx[0] == np.flatnonzero(m.reshape(-1))[0] and (sc == 0).all()
    L = _lib.lib()
    import ctypes
    cnt = ctypes.c_int(0)
    ii, ss = np.empty(4, np.int32), np.empty(4, np.float64)
    for bad in (0, 17, -1):
        assert L.hm_body_stats_peaks(r._h, 0, bad, 0.0, 4, _lib.ptr(ii), _lib.ptr(ss), ctypes.byref(cnt)) == -1
        assert b"outside 1..16" in L.hm_last_error()
    assert L.hm_body_stats_peaks(r._h, 3, 2, 0.0, 4, _lib.ptr(ii), _lib.ptr(ss), ctypes.byref(cnt)) == -1
    kf.close()


def test_a_map_one_pixel_wide(hm):
    from hydra_mi import mesh
    H, W = 20, 12
    p = np.array([[5.2, 2.0], [5.9, 2.0], [5.2, 17.0], [5.9, 17.0]])
    dm = mesh.Mesh(p, np.array([[0, 1, 2], [1, 3, 2]]), 15.0)
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(5)]
    kf = cases.make_filter(dm, frames[0])
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    assert m.any() and np.flatnonzero(m.any(0)).tolist() == [5]          # column 5 alone: neighbours above and below only
    X = np.concatenate((p.reshape(-1), np.zeros(8)))
    r.body_stats_begin()
    regs = [r.body_warp(X + 0.25 * k, f)[0] for k, f in enumerate(frames)]
    want = _check_sums(r, regs, m)
    assert (want[2][[0, 1, 3]] == 0).all() and want[2][2].any()
    imgs = _check_images(r, want, len(regs), m)
    _check_peaks(r, imgs, m, radii=(1, 16), brute=True)
    kf.close()


def test_adversarial_states_accumulate_what_the_warp_returns(hm):
    from hydra_mi import mesh
    dm = mesh.disk_mesh(40.0, 30.0, 22.0, 7.0)
    rng = np.random.default_rng(3)
    H, W = 64, 80
    f = rng.integers(1, 256, (H, W), dtype=np.uint8)
    kf = cases.make_filter(dm, f)
    r = kf.state.renderer
    N = dm.size()
    m = r.body_map()[0] >= 0
    base = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + 0.3, np.zeros(2 * N)))
    t0 = dm.t[len(dm.t) // 2]
    Xs = []
    X = base.copy(); X[2 * t0[1]:2 * t0[1] + 2], X[2 * t0[2]:2 * t0[2] + 2] = base[2 * t0[2]:2 * t0[2] + 2], base[2 * t0[1]:2 * t0[1] + 2]
    Xs.append(X)                                            # a flipped triangle
    X = base.copy(); X[2 * t0[0]] = np.nan
    Xs.append(X)                                            # a vertex at NaN
    X = base.copy(); X[2 * t0[0] + 1] = 1e30
    Xs.append(X)                                            # a vertex at 1e30
    X = base.copy(); X[:2 * N] = np.inf
    Xs.append(X)                                            # nothing finite: a registered frame of zeros
    r.body_stats_begin()
    regs = [r.body_warp(X, f)[0] for X in Xs]
    assert (regs[3] == 0).all() and (regs[1][m] == 0).any() and regs[1].any()
    want = _check_sums(r, regs, m)
    imgs = _check_images(r, want, len(regs), m)
    _check_peaks(r, imgs, m, radii=(6,))
    r.body_stats_begin()                                    # non-finite states alone accumulate zeros
    r.body_warp(Xs[3], f)
    r.body_warp(Xs[3], f)
    s1, s2, cross, vmax = r.body_stats_fetch()
    assert r.body_stats_count() == 2 and not s1.any() and not s2.any() and not cross.any() and not vmax.any()
    kf.close()


@pytest.mark.parametrize("H, W", [(72, 90), (17, 33)])
def test_warps_without_output_and_device_warps_accumulate_the_same(hm, H, W):
    from hydra_mi import _lib, mesh
    from hydra_mi.pipeline import DeviceBuffer
    dm = mesh.box_mesh(20.0, 14.0, 70.0, 57.0, 9.0) if W == 90 else mesh.box_mesh(3.0, 2.0, 30.0, 14.5, 5.0)
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(4)]
    kf = cases.make_filter(dm, frames[0])
    r = kf.state.renderer
    N, T = dm.size(), dm.t.shape[0]
    Xs = [np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + rng.normal(0, 1, 2 * N), np.zeros(2 * N))) for _ in frames]
    m = r.body_map()[0] >= 0
    r.body_stats_begin()
    regs = [r.body_warp(X, f)[0] for X, f in zip(Xs, frames)]
    want = _check_sums(r, regs, m)
    L = _lib.lib()
    r.body_stats_begin()                                    # host warps without an output (sums only, and nothing at all)
    ts = np.empty(T, np.uint64)
    for k, (X, f) in enumerate(zip(Xs, frames)):
        x, fr = np.ascontiguousarray(X), np.ascontiguousarray(f)
        _lib.check(L.hm_body_warp(r._h, _lib.ptr(x), _lib.ptr(fr), None, _lib.ptr(ts) if k % 2 else None, None), "hm_body_warp")
    got = r.body_stats_fetch()
    assert r.body_stats_count() == 4 and all(np.array_equal(a, b) for a, b in zip(got, want))
    r.body_stats_begin()                                    # device warps: 3 channels, 1 channel, no output
    d_f, d_o, d_s = DeviceBuffer(H * W), DeviceBuffer(3 * H * W), DeviceBuffer(8 * T)
    for k, (X, f) in enumerate(zip(Xs, frames)):
        d_f.upload(f)
        r.body_warp_dev(X, d_f.ptr, (d_o.ptr, d_o.ptr, None, None)[k], (3, 1, 1, 3)[k], d_s.ptr if k < 3 else None, None)
        _lib.check(L.hm_ctx_sync(r._h), "hm_ctx_sync")       # (the next upload overwrites the frame)
    got = r.body_stats_fetch()
    assert r.body_stats_count() == 4 and all(np.array_equal(a, b) for a, b in zip(got, want))
    for b in (d_f, d_o, d_s):
        b.close()
    kf.close()


def test_capacity_and_call_order(hm):
    import ctypes
    from hydra_mi import _lib, mesh
    H, W = 33, 40
    dm = mesh.box_mesh(4.0, 3.0, 35.0, 29.0, 8.0)
    rng = np.random.default_rng(6)
    frames = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(5)]
    kf = cases.make_filter(dm, frames[0])
    r = kf.state.renderer
    X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + 0.5, np.zeros(2 * dm.size())))
    m = r.body_map()[0] >= 0
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_stats_begin first"):
        r.body_stats_fetch()
    with pytest.raises(RuntimeError, match="code -3"):
        r.body_stats_images()
    with pytest.raises(RuntimeError, match="code -3"):
        r.body_stats_peaks()
    assert r.body_stats_count() == 0
    r.body_stats_end()                                      # harmless when not begun
    r.body_stats_begin()
    with pytest.raises(RuntimeError, match="code -3.*no frame"):
        r.body_stats_images()
    with pytest.raises(RuntimeError, match="code -3.*no frame"):
        r.body_stats_peaks()
    assert not r.body_stats_fetch()[0].any()                # fetch of zero frames: zeros
    with pytest.raises(RuntimeError, match="body_stats_cap"):
        r.tune("body_stats_cap", 65537)
    r.tune("body_stats_cap", 3)
    regs = [r.body_warp(X, f)[0] for f in frames[:3]]
    with pytest.raises(RuntimeError, match=r"code -3.*hold 3 frames.*capacity is 3"):
        r.body_warp(X, frames[3])
    want = _check_sums(r, regs, m)                          # the refused warp added nothing
    r.body_stats_begin()                                    # again: from zero
    assert r.body_stats_count() == 0 and not r.body_stats_fetch()[1].any()
    regs = [r.body_warp(X, frames[4])[0]]
    _check_sums(r, regs, m)
    r.body_stats_end()
    r.body_stats_end()
    with pytest.raises(RuntimeError, match="code -3"):
        r.body_stats_fetch()
    reg = r.body_warp(X, frames[3])[0]                      # statistics off: the warp as ever, beyond any capacity
    assert np.array_equal(reg, r.body_warp(X, frames[3])[0]) and np.array_equal(r.body_warp(X, frames[4])[0], regs[0])
    r.tune("body_stats_cap", 65536)
    r.body_stats_begin()
    r.body_warp(X, frames[0])
    r.body_stats_peaks("std", 3)
    kf.close()                                              # closed while accumulating, images and peak buffers in place
    kf2 = cases.make_filter(dm, frames[0])
    r2 = kf2.state.renderer
    r2.body_stats_begin()
    _check_sums(r2, [r2.body_warp(X, frames[1])[0]], m)
    kf2.close()


def _pipeline_run(video, masks, c, rad, resident, stats):
    from hydra_mi import body, kalman, mesh
    from hydra_mi.pipeline import FlowEKFPipeline
    n = video.shape[1]
    kf = kalman.IteratedMSKalmanFilter(mesh.disk_mesh(c[0], c[1], rad - 1.0, 12.0), video[0],
                                       np.zeros((n, n, 2), np.float32), True, nI=3)
    pipe = FlowEKFPipeline(kf, video, masks, flow_batch=2, resident=resident)
    got = []
    b = body.BodyReadout(kf, stats=True) if stats else None
    pipe.run(on_frame=lambda k, e: got.append((kf.state.X.copy(), tuple(e[:4]), kf.niter)), body=b)
    pipe.close()
    return kf, got, b


@pytest.mark.parametrize("resident", [True, False])
def test_pipeline_accumulates_and_changes_nothing(hm, resident):
    from hydra_mi import synth
    n, F = 96, 24
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    _, plain, _ = _pipeline_run(video, masks, c, rad, resident, False)
    kf, got, b = _pipeline_run(video, masks, c, rad, resident, True)
    assert len(got) == len(plain) == F - 1
    for (Xa, ea, ia), (Xb, eb, ib) in zip(plain, got):
        assert np.array_equal(Xa, Xb) and ea == eb and ia == ib
    r = kf.state.renderer
    sm = b.summary()
    assert sm["frames"] == F - 1
    got_sums = r.body_stats_fetch()
    r.body_stats_end()                                      # the calls below must not add to anything
    m = b.tri_of_pixel >= 0
    regs = [r.body_warp(X, video[k + 1])[0] for k, (X, _, _) in enumerate(got)]
    want = ref.accumulate(np.array(regs), m)
    assert all(np.array_equal(a, w) for a, w in zip(got_sums, want))
    rm, rs, rc, rx = ref.images(*want, F - 1, m)
    assert np.array_equal(_bits(sm["mean"]), _bits(rm)) and np.array_equal(_bits(sm["std"]), _bits(rs))
    assert np.array_equal(_bits(sm["corr"]), _bits(rc)) and np.array_equal(sm["max"], rx)
    kf.close()


@pytest.mark.parametrize("seed", range(6))
def test_planted_cells_are_found_and_read_out(hm, seed):
    """The condition of tests/test_bodystats_cpu.py through the product: 12 of 12 planted centres have a found point
    within 1 px, and the traces read at the found points (radius 3) correlate with the planted activity at >= 0.94
    (the restatement measures 0.9953..0.9972 at distance 0; 0.05 less for the pixel a centre may be off)."""
    from hydra_mi import body, mesh
    dm = mesh.box_mesh(*ref.PLANTED_BOX)
    frames, states, cs, act = ref.planted_scene(seed, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, stats=True)
    for X, f in zip(states, frames):
        b.registered(X, f)
    sm = b.summary()
    assert sm["frames"] == frames.shape[0] and sm["corr"].shape == frames.shape[1:]
    pts, scores = b.find_points(12, radius=6)
    assert pts.shape == (12, 2) and scores.shape == (12,) and (np.diff(scores) <= 0).all()
    centres = cs + 0.5                                       # pixel (col, row) -> its centre in body coordinates
    near = [int(np.abs(pts - c).max(1).argmin()) for c in centres]
    dist = [float(np.abs(pts[j] - c).max()) for j, c in zip(near, centres)]
    print("seed %d: distances %s, scores %.3f..%.3f" % (seed, dist, scores[-1], scores[0]))
    assert max(dist) <= 1.0 and sorted(near) == list(range(12)), dist
    for which in ("std", "range"):
        p2, _ = b.find_points(12, radius=6, score=which)
        assert max(np.abs(p2 - c).max(1).min() for c in centres) <= 1.0, which
    assert len(b.find_points(100, radius=6, min_score=0.5)[0]) == 12      # the gap: 12th >= 0.89, 13th <= 0.13
    kf.state.renderer.body_stats_end()
    res = body.read_out(kf, states, frames, pts, point_radius=3.0)
    assert res["point_means"].shape == (frames.shape[0], 12) and (res["point_counts"] > 0).all()
    tc = [np.corrcoef(res["point_means"][:, j], act[i])[0, 1] for i, j in enumerate(near)]
    print("seed %d: smallest trace correlation %.4f" % (seed, min(tc)))
    assert min(tc) >= 0.94, tc
    moved = res["points"][-1] - res["points"][0]
    assert np.abs(moved - np.array(ref.PLANTED_SHIFT, np.float64)).max() <= 1e-9
    kf.close()


def test_cli_finds_points_end_to_end(hm, tmp_path):
    from hydra_mi import body, synth
    n, F = 96, 6
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    out = str(tmp_path / "found.npz")
    csv = str(tmp_path / "found.csv")
    cmd = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none"), out, "-s", "14",
           "--find-points", "5", "--find-radius", "4", "--find-score", "std", "--points-out", csv,
           "--registered", str(tmp_path / "reg.avi")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z = np.load(out)
    F1 = z["X"].shape[0]
    assert F1 == F - 1
    for key in ("body_mean", "body_std", "body_corr"):
        assert z[key].shape == (n, n) and z[key].dtype == np.float64, key
    assert z["body_max"].shape == (n, n) and z["body_max"].dtype == np.uint8
    P = z["found_points"].shape[0]
    assert 1 <= P <= 5 and z["found_points"].shape == (P, 2) and z["found_scores"].shape == (P,)
    assert z["points"].shape == (F1, P, 2) and z["point_means"].shape == (F1, P) and z["point_counts"].shape == (P,)
    assert z["tri_means"].shape == (F1, z["t"].shape[0])
    inside = ~np.isnan(z["body_mean"])
    assert inside.any() and (z["body_max"][~inside] == 0).all()
    rr, cc = (z["found_points"][:, 1] - 0.5).astype(int), (z["found_points"][:, 0] - 0.5).astype(int)
    assert np.array_equal(z["found_scores"], z["body_std"][rr, cc])
    names, back = body.read_points_csv(csv)
    assert np.array_equal(back, z["found_points"]) and len(names) == P
    assert "Found %d points" % P in res.stdout
    bad = subprocess.run(cmd + ["--points", csv], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert bad.returncode == 2 and "not together with --points" in bad.stderr
