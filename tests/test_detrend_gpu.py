"""The running baseline per pixel of the kept registered video (`pytest -m gpu`): hm_body_rec_planes and
hm_body_rec_stats_add equal to the NumPy restatement (tests/detrend_ref.py) byte for byte, hydra_mi.detrend through the
product on the drifting planted video, the tracker unchanged by a bit, and the CLI end to end.  Every comparison is an
equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import bodystats_ref as bs
import detrend_ref as ref
import roi_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["16", "33x17", "96x160", "config1"]
F0 = 23


def windows(F):
    """(half, q): no window, the least one, a median, the maximum, windows clipped at both ends at every frame"""
    return ((0, 10), (1, 0), (2, 50), (5, 100), (F + 3, 10), (1024, 10))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _record(name, F=F0, levels=256, chunk=2, cycle=True):
    """A filter on the scene with F random frames of `levels` grey levels recorded, cycled over the scene's states (or all at
    its first, the mesh at rest), in chunks of two frames -> (kf, renderer, map, recorded frames).  Some pixels of every
    frame are 0 and 255."""
    dm, Xs, frames, f0 = cases.scene(name)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    rng = np.random.default_rng(len(name) + levels)
    H, W = f0.shape
    r.tune("body_rec_chunk", chunk)
    r.body_rec_begin()
    for k in range(F):
        f = (rng.integers(0, levels, (H, W)) * (255 // (levels - 1))).astype(np.uint8)
        f[rng.random((H, W)) < 0.05] = 0
        f[rng.random((H, W)) < 0.05] = 255
        r.body_warp(Xs[k % len(Xs) if cycle else 0], f)
    r.tune("body_rec_chunk", 0)
    regs = r.body_rec_fetch()
    assert regs.shape[0] == F and not regs[:, ~m].any()
    assert (regs[:, m] == 0).any() and (regs[:, m] == 255).any()
    return kf, r, m, regs


def _rest_record(F, chunk=64):
    """Scene "16" with the mesh at rest in every frame, so the record is the frames on the map; pixel (row 7, column 7) is
    held at 200, (7, 8) at 0 and (8, 7) at 255 -> (kf, renderer, map, recorded frames)"""
    dm, _, _, f0 = cases.scene("16")
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    p = np.asarray(dm.p, np.float32).astype(np.float64)
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * p.shape[0])))
    rng = np.random.default_rng(F)
    r.tune("body_rec_chunk", chunk)
    r.body_rec_begin()
    for k in range(F):
        f = rng.integers(0, 256, (16, 16), dtype=np.uint8)
        f[6:9, 6:9] = 200
        f[7, 8], f[8, 7] = 0, 255
        r.body_warp(rest, f)
    r.tune("body_rec_chunk", 0)
    regs = r.body_rec_fetch()
    assert m[7, 7] and (regs[:, 7, 7] == 200).all() and not regs[:, 7, 8].any() and (regs[:, 8, 7] == 255).all()
    return kf, r, m, regs


@pytest.mark.parametrize("name", SCENES)
def test_planes_equal_the_restatement(hm, name):
    kf, r, m, regs = _record(name)
    F = regs.shape[0]
    box = np.flatnonzero(m.any(0))
    bw = int(box[-1] - box[0]) + 1
    if name == "33x17":
        assert bw % 4 and bw % 64                                          # a box no multiple of 4 or 64 wide
    if name == "96x160":
        rows = np.flatnonzero(m.any(1))
        assert not m[rows[0]:rows[-1] + 1, box[0]:box[-1] + 1].all()       # a map that is no rectangle
    assert np.array_equal(r.body_rec_planes(0, 3, 10), regs) and np.array_equal(r.body_rec_planes("recorded", 0, 0, k0=2, n=3), regs[2:5])
    want = {}
    for half, q in windows(F):
        for what in (1, 2, 3):
            want[half, q, what] = ref.planes(regs, m, what, half, q, 16, 255)
    assert any((want[5, 100, 1] != want[1, 0, 1]).ravel()) and want[2, 50, 2].any() and want[2, 50, 3].any()
    first = None
    for run in (1, 3, 1 << 20):                                            # frames per run: 1, 3 (runs cross chunks), one run
        r.tune("rec_bl_frames", run)
        got = {key: r.body_rec_planes(key[2], key[0], key[1], 16, 255) for key in want}
        for key in want:
            assert got[key].dtype == np.uint8 and np.array_equal(got[key], want[key]), (run, key)
        first = first or got
        assert all(np.array_equal(got[key], first[key]) for key in want)
        k0, n = 1, F - 2                                                   # starts and ends inside a chunk
        for half, q in ((2, 50), (F + 3, 10)):
            for what, kind in ((1, "baseline"), (2, "excess"), (3, "dff")):
                assert np.array_equal(r.body_rec_planes(kind, half, q, 16, 255, k0, n), want[half, q, what][k0:k0 + n]), (run, what)
        assert r.body_rec_planes(1, 2, 50, k0=F, n=0).shape[0] == 0
    r.tune("rec_bl_frames", 256)
    for floor, gain in ((1, 1), (255, 1), (1, 65535), (255, 65535)):       # at their limits
        assert np.array_equal(r.body_rec_planes(3, 2, 50, floor, gain), ref.planes(regs, m, 3, 2, 50, floor, gain)), (floor, gain)
    assert np.array_equal(r.body_rec_fetch(), regs)                        # the record has not changed by a bit
    kf.close()


def test_ties_of_four_grey_levels(hm):
    kf, r, m, regs = _record("33x17", levels=4, cycle=False)
    F = regs.shape[0]
    assert len(np.unique(regs[:, m])) == 4
    for run in (3, 1 << 20):
        r.tune("rec_bl_frames", run)
        for half, q in windows(F) + ((3, 33), (4, 67)):
            for what in (1, 2, 3):
                assert np.array_equal(r.body_rec_planes(what, half, q, 16, 255), ref.planes(regs, m, what, half, q, 16, 255)), (half, q, what)
    kf.close()


def test_a_bin_passes_255_in_a_record_of_300_frames(hm):
    """A constant pixel fills one bin with the whole window (counts of 8 bits would wrap), beside pixels held at 0 and 255"""
    kf, r, m, regs = _rest_record(300)
    for run, (half, q) in ((256, (150, 10)), (7, (1024, 50)), (1 << 20, (200, 100))):
        r.tune("rec_bl_frames", run)
        for what in (1, 2, 3):
            got = r.body_rec_planes(what, half, q, 16, 255)
            assert np.array_equal(got, ref.planes(regs, m, what, half, q, 16, 255)), (run, what)
        assert (r.body_rec_planes(1, half, q)[:, 7, 7] == 200).all()
    assert np.array_equal(r.body_rec_fetch(), regs)
    kf.close()


@pytest.mark.parametrize("name", ["33x17", "96x160"])
def test_stats_add_equals_the_statistics_of_the_planes(hm, name):
    kf, r, m, regs = _record(name)
    F = regs.shape[0]
    r.tune("rec_bl_frames", 5)
    for what in (0, 1, 2, 3):
        planes = ref.planes(regs, m, what, 3, 30, 16, 255)
        want = bs.accumulate(planes, m)
        r.body_stats_begin()
        r.body_rec_stats_add(what, 3, 30, 16, 255)
        assert r.body_stats_count() == F
        got = r.body_stats_fetch()
        for g, w in zip(got, want):
            assert np.array_equal(g, w), what
        imgs, exp = r.body_stats_images(), bs.images(*want, F, m)
        for g, w in zip(imgs[:3], exp[:3]):
            assert np.array_equal(_bits(g), _bits(w)), what
        assert np.array_equal(imgs[3], exp[3])
        idx, sc, found = r.body_stats_peaks("std", 3)
        widx, wsc = bs.peaks_fast(exp[1], m, 3)
        assert found == len(widx) and np.array_equal(idx, widx) and np.array_equal(_bits(sc), _bits(wsc))
        r.body_rec_stats_add(what, 3, 30, 16, 255)                         # twice: the sums double
        assert r.body_stats_count() == 2 * F
        for g, w in zip(r.body_stats_fetch()[:3], want[:3]):
            assert np.array_equal(g, 2 * w), what
    # a warp after it goes on adding, and is recorded
    dm, Xs, frames, f0 = cases.scene(name)
    reg = r.body_warp(Xs[1], frames[1])[0]
    assert r.body_stats_count() == 2 * F + 1 and r.body_rec_count() == F + 1
    assert np.array_equal(r.body_stats_fetch()[0], 2 * want[0] + np.where(m, reg, 0))
    assert np.array_equal(r.body_rec_fetch(0, F), regs)
    kf.close()


def test_refusals_name_their_numbers(hm):
    kf, r, m, regs = _record("16", F=6)
    F = regs.shape[0]
    ok = dict(what=2, half=3, q=10, floor=16, gain=255)
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_stats_add: no statistics \(hm_body_stats_begin first\)"):
        r.body_rec_stats_add(**ok)
    r.body_stats_begin()
    limits = (("what", -1, 4, r"kind of plane %d outside 0\.\.3"), ("half", -1, 1025, r"half %d outside 0\.\.1024"),
              ("q", -1, 101, r"q %d outside 0\.\.100"), ("floor", 0, 256, r"floor %d outside 1\.\.255"),
              ("gain", 0, 65536, r"gain %d outside 1\.\.65535"))
    for key, lo, hi, text in limits:
        for v in (lo, hi):
            with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_planes: " + text % v):
                r.body_rec_planes(**dict(ok, **{key: v}))
            with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_stats_add: " + text % v):
                r.body_rec_stats_add(**dict(ok, **{key: v}))
    for k0, n in ((F - 1, 2), (-1, 2), (F + 1, 0)):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_planes: frames %d \.\. %d of a record of %d" % (k0, k0 + n - 1, F)):
            r.body_rec_planes(k0=k0, n=n, **ok)
    assert r.body_stats_count() == 0
    r.tune("body_stats_cap", 2 * F - 1)                                    # the second addition would pass the capacity
    r.body_rec_stats_add(**ok)
    before = r.body_stats_fetch()
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_stats_add: the statistics hold %d frames and the record %d, their "
                                           r"capacity is %d .*nothing added" % (F, F, 2 * F - 1)):
        r.body_rec_stats_add(**ok)
    assert r.body_stats_count() == F and all(np.array_equal(a, b) for a, b in zip(before, r.body_stats_fetch()))
    r.tune("body_stats_cap", 65536)
    for v in (0, (1 << 24) + 1):
        with pytest.raises(RuntimeError, match=r"rec_bl_frames must be in 1\.\.%d" % (1 << 24)):
            r.tune("rec_bl_frames", v)
    assert np.array_equal(r.body_rec_fetch(), regs)
    r.body_rec_begin()                                                      # an empty record
    for call in (lambda: r.body_rec_planes(k0=0, n=0, **ok), lambda: r.body_rec_stats_add(**ok)):
        with pytest.raises(RuntimeError, match="code -3.*no frame recorded"):
            call()
    r.body_rec_end()                                                        # before begin
    for call in (lambda: r.body_rec_planes(k0=0, n=0, **ok), lambda: r.body_rec_stats_add(**ok)):
        with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_begin first"):
            call()
    kf.close()


def test_detrending_between_frames_changes_nothing_of_the_filter(hm):
    """Config 1 (128^2, the golden track) with the record kept and its planes read and summed between every two frames:
    states, covariance and error terms bit-identical to the run without."""
    from hydra_mi import body, detrend, kalman, mesh, synth
    g = np.load(os.path.join(cases.GOLD, "config1_track.npz"))
    video, flow = synth.test_data(128, 128)
    runs = {}
    for det in (False, True):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), video[:, :, 0], flow[:, :, :, 0], True)
        b = body.BodyReadout(kf, keep=True) if det else None
        out = []
        for k in range(10):
            frame = video[:, :, k]
            e = kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
            if det:
                b.registered(kf.state.X, frame)
                assert detrend.summary(b, "excess", 2, 10)["frames"] == k + 1
                assert kf.state.renderer.body_rec_planes("dff", 2, 10, 16, 255).shape[0] == k + 1
                kf.state.renderer.body_stats_end()
            out.append((kf.state.X.copy(), kf.niter, e[:4], np.array(kf.state.W, np.float64).copy()))
        runs[det] = out
        kf.close()
    for (Xa, ia, ea, Wa), (Xb, ib, eb, Wb) in zip(runs[False], runs[True]):
        assert np.array_equal(Xa, Xb) and ia == ib and ea == eb and np.array_equal(Wa, Wb)


def test_seeds_of_the_drifting_scene_through_the_product(hm, tmp_path):
    """The drifting planted video as the tracker sees it, recorded with BodyReadout(keep=True): detrend.find_points gives
    the 12 planted centres back within 2 px where the raw statistics do not; detrend.summary equals the restatement bit
    for bit, what body.summary returned before stays untouched, and write_video's frames are the dF/F planes."""
    from hydra_mi import body, detrend, mesh
    from test_views_cpu import read_avi
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs, drift = ref.drifting_scene(0, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True, stats=True)
    regs = np.array([b.registered(X, f) for X, f in zip(states, frames)])
    m = b.tri_of_pixel >= 0
    F, H, W = regs.shape
    assert F == 300 and np.array_equal(m, roi_ref.planted_map()) and np.array_equal(regs, drift)
    raw = b.summary()
    keep = {k: np.array(v, copy=True) for k, v in raw.items()}
    raw_pts = b.find_points(12, radius=6)[0]
    near = lambda pts: ref.seeds_found((pts[:, 1] - 0.5).astype(np.int64) * W + (pts[:, 0] - 0.5).astype(np.int64), W, cs)
    assert near(raw_pts) <= 8
    pts, sc = detrend.find_points(b, 12, radius=6)
    assert pts.shape == (12, 2) and near(pts) == 12
    exc = ref.planes(regs, m, 2, detrend.DEFAULT_HALF, detrend.DEFAULT_Q)
    exp = bs.images(*bs.accumulate(exc, m), F, m)
    widx, wsc = bs.peaks_fast(exp[2], m, 6)
    assert np.array_equal(_bits(sc), _bits(wsc[:12]))
    assert np.array_equal((pts[:, 1] - 0.5) * W + (pts[:, 0] - 0.5), widx[:12].astype(np.float64))
    got = detrend.summary(b, "excess")
    assert got["frames"] == F and np.array_equal(got["max"], exp[3])
    for key, w in zip(("mean", "std", "corr"), exp[:3]):
        assert np.array_equal(_bits(got[key]), _bits(w)), key
    assert all(np.array_equal(raw[k], keep[k], equal_nan=True) for k in keep)
    with pytest.raises(RuntimeError, match="without keep=True"):
        detrend.summary(body.BodyReadout(kf))
    # the dF/F video, fetched in blocks of 37 frames
    kf2 = cases.make_filter(dm, frames[0])
    b2 = body.BodyReadout(kf2, keep=True)
    for X, f in zip(states[130:170], frames[130:170]):                     # 40 frames across the move of the mesh
        b2.registered(X, f)
    avi = str(tmp_path / "dff.avi")
    assert detrend.write_video(b2, avi, half=7, q=20, floor=20, gain=400, block=37) == 40
    vid = read_avi(avi)["frames"]
    want = ref.planes(regs[130:170], m, 3, 7, 20, 20, 400)
    assert len(vid) == 40 and want.any()
    for k in range(40):
        assert all(np.array_equal(vid[k][:, :, c], want[k]) for c in range(3)), k
    assert np.array_equal(kf2.state.renderer.body_rec_planes(3, 7, 20, 20, 400), want)
    kf2.close()
    kf.close()


def test_cli_detrend_end_to_end(hm, tmp_path):
    """run_kalmanfilter.py --find-points 12 --detrend --dff-video on the first frames of the drifting video, as an animal:
    a disc of it on black.  detrend_* are the summary images of the excess of the registered video (--registered writes
    it), the points found are their best peaks, the dF/F video its planes; body_* are what the run without the new flags
    writes, and that run's output has nothing new in it."""
    from test_views_cpu import read_avi
    Fv, half, q, floor, gain = 12, 3, 20, 12, 300
    d = ref.drifting_video(0)[0][:Fv]
    n = d.shape[1]
    yy, xx = np.mgrid[0:n, 0:n]
    video = d * ((xx - 63.5) ** 2 + (yy - 63.5) ** 2 <= 48.0 ** 2).astype(np.uint8)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "12", "--find-radius", "4"]
    out0, out1 = str(tmp_path / "plain.npz"), str(tmp_path / "det.npz")
    reg, dff = str(tmp_path / "reg.avi"), str(tmp_path / "dff.avi")
    res0 = subprocess.run(base + [out0] + find, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res0.returncode == 0, res0.stderr[-2000:]
    res = subprocess.run(base + [out1] + find + ["--registered", reg, "--detrend", "--detrend-half", str(half), "--detrend-q", str(q),
                                                 "--dff-video", dff, "--dff-floor", str(floor), "--dff-gain", str(gain)],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z0, z = np.load(out0), np.load(out1)
    F1 = z["X"].shape[0]
    assert F1 == Fv - 1 and np.array_equal(z["X"], z0["X"])
    for key in ("tri_means", "body_mean", "body_std", "body_max", "body_corr"):         # summed while tracking: as before
        assert np.array_equal(z[key], z0[key], equal_nan=True), key
    new = {"detrend_mean", "detrend_std", "detrend_max", "detrend_corr"}
    assert set(z.files) - set(z0.files) == new and set(z0.files) <= set(z.files)
    assert "Detrended" not in res0.stdout and "dF/F video" not in res0.stdout
    assert "Detrended: the excess over the running baseline (half %d, q %d) of %d frames summed up" % (half, q, F1) in res.stdout
    assert "dF/F video: %d frames in %s" % (F1, dff) in res.stdout
    regs = np.array([f[:, :, 0] for f in read_avi(reg)["frames"]])
    m = ~np.isnan(z["body_mean"])
    assert regs.shape == (F1, n, n) and m.any()
    exp = bs.images(*bs.accumulate(ref.planes(regs, m, 2, half, q), m), F1, m)
    for key, w in zip(("detrend_mean", "detrend_std", "detrend_corr"), exp[:3]):
        assert np.array_equal(_bits(z[key]), _bits(w)), key
    assert np.array_equal(z["detrend_max"], exp[3])
    widx, wsc = bs.peaks_fast(exp[2], m, 4)
    P = min(12, len(widx))
    rr, cc = np.divmod(widx[:P].astype(np.int64), n)
    assert np.array_equal(z["found_points"], np.stack((cc + 0.5, rr + 0.5), 1)) and np.array_equal(_bits(z["found_scores"]), _bits(wsc[:P]))
    raw = bs.images(*bs.accumulate(regs, m), F1, m)                        # the run without: the raw peaks, as ever
    ridx = bs.peaks_fast(raw[2], m, 4)[0][:12]
    rr, cc = np.divmod(ridx.astype(np.int64), n)
    assert np.array_equal(z0["found_points"], np.stack((cc + 0.5, rr + 0.5), 1))
    got = read_avi(dff)["frames"]
    want = ref.planes(regs, m, 3, half, q, floor, gain)
    assert len(got) == F1 and want.any()
    for k in range(F1):
        assert all(np.array_equal(got[k][:, :, c], want[k]) for c in range(3)), k
    bad = subprocess.run(base + [out1, "--detrend"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert bad.returncode == 2 and "--detrend finds the cells in the excess video: it needs --find-points" in bad.stderr


def _frame_bytes(m):
    """bytes of one frame of the record: the map's bounding box, rows padded to 4 bytes, the frame to 16"""
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    pitch = (int(cols[-1] - cols[0]) + 1 + 3) & ~3
    return (pitch * (int(rows[-1] - rows[0]) + 1) + 15) & ~15


def test_every_scratch_size_gives_the_same_planes_and_statistics(hm):
    """5 frames in chunks of 3, scratch for two frames (runs of 2, 2, 1), for less than one (the floor: one frame at a time)
    and for all of them"""
    kf, r, m, regs = _record("16", F=5, chunk=3)
    fs = _frame_bytes(m)
    want = {what: ref.planes(regs, m, what, 2, 50, 16, 255) for what in (1, 2, 3)}
    stats = bs.accumulate(want[2], m)
    assert want[2].any()
    for scratch in (2 * fs, fs - 1, 16 << 20):
        r.tune("rec_scratch_bytes", scratch)
        for what in (1, 2, 3):
            assert np.array_equal(r.body_rec_planes(what, 2, 50, 16, 255), want[what]), (scratch, what)
            assert np.array_equal(r.body_rec_planes(what, 2, 50, 16, 255, 1, 4), want[what][1:]), (scratch, what)
        r.body_stats_begin()
        r.body_rec_stats_add(2, 2, 50, 16, 255)
        assert r.body_stats_count() == 5
        for g, w in zip(r.body_stats_fetch(), stats):
            assert np.array_equal(g, w), scratch
    assert np.array_equal(r.body_rec_fetch(), regs)
    kf.close()


def test_the_scratch_knob_refuses_what_is_outside_its_range(hm):
    kf, r, m, regs = _record("16", F=1)
    for v in (0, (1 << 30) + 1):
        with pytest.raises(RuntimeError, match=r"code -1.*rec_scratch_bytes must be in 1\.\.%d" % (1 << 30)):
            r.tune("rec_scratch_bytes", v)
    r.tune("rec_scratch_bytes", 1)
    r.tune("rec_scratch_bytes", 1 << 30)
    r.tune("rec_scratch_bytes", 16 << 20)
    kf.close()
