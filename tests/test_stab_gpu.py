"""Stabilising the kept registered video (`pytest -m gpu`): hm_body_rec_match / _frame_sums / _shift equal to the NumPy
restatement (tests/stab_ref.py) as exact integers, hydra_mi.stabilize through the product equal to it bit for bit, the
tracker unchanged by a bit with stabilisation run between frames, and the CLI end to end.  Every comparison is an
equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import roi_ref
import stab_ref as ref
from test_roi_cpu import THR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ((4, 0), (7, 1), (16, 3), (64, 8))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _record(name, chunk=2, tp=3, F=None):
    """A filter on the scene with every frame recorded twice (the first F of those, if given), in chunks of two frames, runs
    of three frames per workgroup (so that runs cross chunks) -> (kf, renderer, map, recorded frames)"""
    dm, Xs, frames, f0 = cases.scene(name)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    r.tune("body_rec_chunk", chunk)
    r.tune("rec_tp_frames", tp)
    r.body_rec_begin()
    for X, f in (2 * list(zip(Xs, frames)))[:F]:
        r.body_warp(X, f)
    r.tune("body_rec_chunk", 0)
    regs = r.body_rec_fetch()
    assert not regs[:, ~m].any()
    return kf, r, m, regs


def _same_match(got, want, keys=("A", "V1", "V2")):
    assert got["n_core"].dtype == np.uint32 and np.array_equal(got["n_core"], want["n_core"])
    for key in keys:
        assert got[key].dtype == np.uint32 and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("name", cases.NAMES)
def test_match_frame_sums_and_shift_equal_the_restatement(hm, name):
    kf, r, m, regs = _record(name)
    F, H, W = regs.shape
    rng = np.random.default_rng(len(name) + 3)
    g = ref.patch_grid(m, 7)
    if name == "33x17":
        assert g["bw"] % 4 and g["bw"] % 7 and g["bw"] % 16                # a box no multiple of 4 or of B wide
    if name == "96x160":
        assert not m[g["r0"]:g["r0"] + g["bh"], g["c0"]:g["c0"] + g["bw"]].all()     # a map that is no rectangle
    empty = False
    for B, S in GRIDS:
        noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
        want = ref.match(regs, m, B, S, noise)
        empty |= bool((want["n_core"] == 0).any())
        assert r.body_rec_patches(B) == (ref.patch_grid(m, B)["npx"], ref.patch_grid(m, B)["npy"])
        _same_match(r.body_rec_match(noise, B, S), want)                   # a random template, all frames
        k0, n = 1, F - 2                                                    # starts and ends inside a chunk
        sub = r.body_rec_match(regs[2], B, S, k0, n)                        # a template equal to a record frame
        _same_match(sub, ref.match(regs, m, B, S, regs[2], k0, n))
        one = r.body_rec_match(noise, B, S, 3, 1, want=("V1",))             # NULL outputs
        assert set(one) == {"n_core", "V1"} and np.array_equal(one["V1"], want["V1"][3:4])
        only_n = r.body_rec_match(noise, B, S, 0, 0, want=())
        assert np.array_equal(only_n["n_core"], want["n_core"])
        # sums and the shift at random shifts within +-S (and once at the limit, +-16)
        npatch = len(want["n_core"])
        for lim in (S, 16):
            sh = rng.integers(-lim, lim + 1, (F, npatch, 2)).astype(np.int8)
            fs = r.body_rec_frame_sums(sh, B)
            assert fs.dtype == np.uint32 and np.array_equal(fs, ref.frame_sums(regs, m, B, sh))
            assert np.array_equal(r.body_rec_frame_sums(sh[k0:k0 + n], B, k0, n), ref.frame_sums(regs[k0:k0 + n], m, B, sh[k0:k0 + n]))
    assert empty                                                            # some patch of some grid has an empty core
    assert np.array_equal(r.body_rec_frame_sums(), regs.astype(np.uint32).sum(0))         # NULL shifts: the plain sum
    assert np.array_equal(r.body_rec_frame_sums(None, 0, 2, 3), regs[2:5].astype(np.uint32).sum(0))
    kf.close()


@pytest.mark.parametrize("name, B, S", [("33x17", 7, 1), ("96x160", 16, 3), ("config1", 64, 8), ("16", 4, 0)])
def test_shift_in_place_then_every_reduction_sees_the_shifted_frames(hm, name, B, S):
    from hydra_mi import body
    kf, r, m, regs = _record(name)
    F, H, W = regs.shape
    rng = np.random.default_rng(B)
    tri = r.body_map()[0]
    npatch = ref.patch_grid(m, B)["npx"] * ref.patch_grid(m, B)["npy"]
    r.body_rec_shift(np.zeros((F, npatch, 2), np.int8), B)                 # all-zero shifts: nothing changes
    assert np.array_equal(r.body_rec_fetch(), regs)
    lim = max(S, 1)
    sh = rng.integers(-lim, lim + 1, (F, npatch, 2)).astype(np.int8)
    r.body_rec_shift(sh, B)
    want = ref.shift(regs, m, B, sh)
    assert (want != regs).any() and np.array_equal(r.body_rec_fetch(), want)
    assert np.array_equal(r.body_rec_fetch(1, 3), want[1:4])
    rows, cols = np.nonzero(m)
    seeds = np.array([(cols[i], rows[i]) for i in rng.integers(0, len(rows), 5)], np.int32)
    labels = body.disc_labels(tri, seeds + 0.5, 2.5)
    assert np.array_equal(r.body_rec_label_sums(labels, 5), roi_ref.label_sums(want, m, labels, 5))
    got, exp = r.body_rec_seed_sums(seeds, 2.0, 3.0, 5.0, 4), roi_ref.seed_sums(want, m, seeds, 2.0, 3.0, 5.0, 4)
    for key in exp:
        assert np.array_equal(got[key], exp[key]), key
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    _same_match(r.body_rec_match(noise, B, S), ref.match(want, m, B, S, noise))
    sh2 = rng.integers(-16, 17, (F, npatch, 2)).astype(np.int8)            # a second time: shifts what is there
    r.body_rec_shift(sh2, B)
    assert np.array_equal(r.body_rec_fetch(), ref.shift(want, m, B, sh2))
    assert r.body_rec_count() == F
    r.body_warp(cases.scene(name)[1][0], cases.scene(name)[2][0])           # the record goes on
    assert r.body_rec_count() == F + 1
    kf.close()


def test_refusals_name_their_numbers(hm):
    kf, r, m, regs = _record("33x17")
    F, H, W = regs.shape
    t = regs[0]
    npatch = lambda B: ref.patch_grid(m, B)["npx"] * ref.patch_grid(m, B)["npy"]
    for B in (3, 65):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_match: patch size %d outside 4\.\.64" % B):
            r.body_rec_match(t, B, 1)
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_shift: patch size %d outside 4\.\.64" % B):
            r.body_rec_shift(np.zeros((F, 1, 2), np.int8), B)
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_frame_sums: patch size %d outside 4\.\.64" % B):
            r.body_rec_frame_sums(np.zeros((F, 1, 2), np.int8), B)
    with pytest.raises(RuntimeError, match=r"code -1.*search radius 9 outside 0\.\.8"):
        r.body_rec_match(t, 16, 9)
    sh = np.zeros((F, npatch(8), 2), np.int8)
    sh[2, 3, 1] = 17
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_shift: shift 17 \(dy of patch 3, frame 2"):
        r.body_rec_shift(sh, 8)
    sh[2, 3, 1], sh[1, 0, 0] = 0, -17
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_frame_sums: shift -17 \(dx of patch 0, frame 1"):
        r.body_rec_frame_sums(sh, 8)
    assert np.array_equal(r.body_rec_fetch(), regs)                         # a refused shift changes nothing
    with pytest.raises(RuntimeError, match=r"code -1.*frames 4 .. 7 of a record of 6"):
        r.body_rec_match(t, 8, 1, 4, 4)
    with pytest.raises(RuntimeError, match=r"code -1.*frames 5 .. 6 of a record of 6"):
        r.body_rec_frame_sums(None, 8, 5, 2)
    too_many = 2 ** 32 // 255 + 1                                           # n 255 >= 2^32
    with pytest.raises(RuntimeError, match=r"code -1.*%d frames x 255 could pass 2\^32" % too_many):
        r.body_rec_frame_sums(None, 8, 0, too_many)
    sh[1, 0, 0] = 0
    r.body_rec_begin()                                                      # an empty record
    for call in (lambda: r.body_rec_match(t, 8, 1, 0, 0), lambda: r.body_rec_frame_sums(None, 8, 0, 0),
                 lambda: r.body_rec_shift(sh[:0], 8)):
        with pytest.raises(RuntimeError, match="code -3.*no frame recorded"):
            call()
    r.body_rec_end()                                                        # before begin
    for call in (lambda: r.body_rec_match(t, 8, 1, 0, 0), lambda: r.body_rec_frame_sums(None, 8, 0, 0),
                 lambda: r.body_rec_shift(sh[:0], 8)):
        with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_begin first"):
            call()
    kf.close()


def test_stabilize_on_the_jittered_scene_equals_the_restatement(hm):
    """hydra_mi.stabilize through the product on the planted video with jitter as the tracker sees it: the estimate equals
    the restatement's, and roi.extract on the stabilised record equals roi_ref.extract on stab_ref.shift of the registered
    video bit for bit."""
    from hydra_mi import body, mesh, roi, stabilize
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs, act, planted, jit = ref.jittered_scene(0, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True)
    with pytest.raises(RuntimeError, match="no frame recorded"):
        stabilize.estimate(b)
    regs = np.array([b.registered(X, f) for X, f in zip(states, frames)])
    m = b.tri_of_pixel >= 0
    assert np.array_equal(m, roi_ref.planted_map()) and np.array_equal(regs, np.where(m[None], jit, 0))
    old = stabilize.MATCH_BYTES
    stabilize.MATCH_BYTES = 3 * 4 * 64 * 49 * 37                           # blocks of 37 frames
    try:
        est = stabilize.stabilize(b, passes=2)
    finally:
        stabilize.MATCH_BYTES = old
    want = ref.estimate(regs, m, passes=2, min_score=stabilize.DEFAULT_MIN_SCORE)
    assert np.array_equal(est["shifts"], want["shifts"]) and np.array_equal(est["fallback"], want["fallback"])
    assert np.array_equal(_bits(est["score"]), _bits(want["score"])) and np.array_equal(est["n_core"], want["n_core"])
    assert len(est["templates"]) == 2 and all(np.array_equal(a, c) for a, c in zip(est["templates"], want["templates"]))
    assert est["shifts"].any()
    stab = ref.shift(regs, m, 16, want["shifts"])
    assert np.array_equal(b.r.body_rec_fetch(), stab)
    got = roi.extract(b, cs + 0.5, thr=THR, alpha=1.0)
    exp = roi_ref.extract(stab, m, cs, thr=THR, alpha=1.0)
    for key in ("footprints", "F_roi", "F_np", "dff"):
        assert np.array_equal(_bits(got[key]), _bits(exp[key])), key
    for key in ("roi_labels", "roi_counts", "ring_counts", "seed_fallback"):
        assert np.array_equal(got[key], exp[key]), key
    with pytest.raises(RuntimeError, match="without keep=True"):
        stabilize.estimate(body.BodyReadout(kf))
    kf.close()


def test_stabilising_between_frames_changes_nothing_of_the_filter(hm):
    """Config 1 (128^2, the golden track) with the record kept and stabilised between every two frames: states, covariance
    and error terms bit-identical to the run without."""
    from hydra_mi import body, kalman, mesh, stabilize, synth
    g = np.load(os.path.join(cases.GOLD, "config1_track.npz"))
    video, flow = synth.test_data(128, 128)
    runs = {}
    for stab in (False, True):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), video[:, :, 0], flow[:, :, :, 0], True)
        b = body.BodyReadout(kf, keep=True) if stab else None
        out = []
        for k in range(10):
            frame = video[:, :, k]
            e = kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
            if stab:
                b.registered(kf.state.X, frame)
                est = stabilize.stabilize(b, B=8, S=2, min_score=0.0)
                assert est["shifts"].shape[0] == k + 1
            out.append((kf.state.X.copy(), kf.niter, e[:4], np.array(kf.state.W, np.float64).copy()))
        runs[stab] = out
        kf.close()
    for (Xa, ia, ea, Wa), (Xb, ib, eb, Wb) in zip(runs[False], runs[True]):
        assert np.array_equal(Xa, Xb) and ia == ib and ea == eb and np.array_equal(Wa, Wb)


def test_cli_stabilize_end_to_end(hm, tmp_path):
    """run_kalmanfilter.py --find-points 12 --rois --stabilize on the first frames of the jittered video, as an animal: a
    disc of it on black.  The tracker follows what it can of the planted motion; what is left in the registered video
    (--registered writes it) is what --stabilize sees.  The written shifts equal the restatement's estimate on those frames,
    some are not zero, and everything the run reads from the kept record afterwards -- the disc read-out and the ROI
    traces -- equals the restatement on stab_ref.shift of them at the written shifts, and differs from the run without."""
    from hydra_mi import body, roi, stabilize
    from test_views_cpu import read_avi
    F, B, S = 10, 16, 3
    j = ref.jittered_video(0)[0][:F]
    n = j.shape[1]
    yy, xx = np.mgrid[0:n, 0:n]
    video = j * ((xx - 63.5) ** 2 + (yy - 63.5) ** 2 <= 48.0 ** 2).astype(np.uint8)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "12", "--find-radius", "4", "--find-score", "std", "--rois"]
    out0, out1, avi = str(tmp_path / "rois.npz"), str(tmp_path / "stab.npz"), str(tmp_path / "reg.avi")
    res0 = subprocess.run(base + [out0] + find, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res0.returncode == 0, res0.stderr[-2000:]
    res = subprocess.run(base + [out1] + find + ["--registered", avi, "--stabilize", "--stab-patch", str(B), "--stab-search",
                                                 str(S), "--stab-passes", "2"],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z0, z = np.load(out0), np.load(out1)
    F1 = z["X"].shape[0]
    assert F1 == F - 1 and np.array_equal(z["X"], z0["X"]) and np.array_equal(z["found_points"], z0["found_points"])
    for key in ("tri_means", "body_mean", "body_std", "body_max", "body_corr"):         # summed while tracking
        assert np.array_equal(z[key], z0[key], equal_nan=True), key
    npatch = z["stab_shifts"].shape[1]
    assert z["stab_shifts"].shape == (F1, npatch, 2) and z["stab_shifts"].dtype == np.int8
    assert z["stab_score"].shape == (F1, npatch) and z["stab_score"].dtype == np.float64
    assert z["stab_fallback"].shape == (F1, npatch) and z["stab_fallback"].dtype == np.bool_
    mean_abs = np.abs(z["stab_shifts"].astype(np.float64)).sum(2).mean()
    print("fallbacks %.3f, mean |shift| %.3f, frames with a shift %d of %d" % (
        z["stab_fallback"].mean(), mean_abs, z["stab_shifts"].any((1, 2)).sum(), F1))
    assert "Stabilised: %d patches of %d px, search %d, 2 passes: %.1f %% fallbacks, mean |shift| %.3f px" % (
        npatch, B, S, 100.0 * z["stab_fallback"].mean(), mean_abs) in res.stdout
    assert "stab_shifts" not in z0.files and "Stabilised" not in res0.stdout
    # the registered frames as the tracker left them, and the restatement on them
    regs = np.array([f[:, :, 0] for f in read_avi(avi)["frames"]])
    m = ~np.isnan(z["body_mean"])
    assert regs.shape == (F1, n, n) and m.any()
    want = ref.estimate(regs, m, B, S, passes=2, min_score=stabilize.DEFAULT_MIN_SCORE)
    assert np.array_equal(z["stab_shifts"], want["shifts"]) and np.array_equal(z["stab_fallback"], want["fallback"])
    assert np.array_equal(_bits(z["stab_score"]), _bits(want["score"]))
    assert z["stab_shifts"].any() and not z["stab_shifts"][z["stab_fallback"]].any()     # stabilisation had work to do
    stab = ref.shift(regs, m, B, z["stab_shifts"])
    assert (stab != regs).any()
    pts = z["found_points"]
    P = len(pts)
    assert np.array_equal(z["roi_points"], np.arange(P)) and np.array_equal(z0["roi_points"], np.arange(P))
    labels = body.disc_labels(np.where(m, 0, -1), pts, 3.0)
    counts = np.bincount(labels[labels >= 0], minlength=P)
    for zz, video_read in ((z0, regs), (z, stab)):                   # without: the frames as they were; with: the shifted
        exp = roi_ref.extract(video_read, m, roi.seeds_of(pts), r_disc=3.0, thr=roi.DEFAULT_THR, alpha=0.7)
        for key, name in (("roi_footprints", "footprints"), ("roi_F", "F_roi"), ("roi_Fnp", "F_np"), ("roi_dff", "dff")):
            assert np.array_equal(_bits(zz[key]), _bits(exp[name])), key
        assert np.array_equal(zz["roi_labels"], exp["roi_labels"]) and np.array_equal(zz["roi_counts"], exp["roi_counts"])
        means = roi_ref.label_sums(video_read, m, labels, P).astype(np.float64) / counts[None, :]
        assert np.array_equal(_bits(zz["point_means"]), _bits(means))
    for key in ("roi_F", "roi_dff", "point_means"):
        assert not np.array_equal(z[key], z0[key]), key
    small = subprocess.run(base + [str(tmp_path / "small.npz")] + find + ["--stabilize", "--rois-max-gb", "1e-6"],
                           capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert small.returncode == 0, small.stderr[-2000:]
    assert "no ROIs, no stabilisation, the disc read-out instead" in small.stdout
    assert "stab_shifts" not in np.load(str(tmp_path / "small.npz")).files
    bad = subprocess.run(base + [out1, "--find-points", "3", "--stabilize"], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert bad.returncode == 2 and "--stabilize works on the kept record: it needs --rois or --demix" in bad.stderr


def _frame_bytes(m):
    """bytes of one frame of the record: the map's bounding box, rows padded to 4 bytes, the frame to 16"""
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    pitch = (int(cols[-1] - cols[0]) + 1 + 3) & ~3
    return (pitch * (int(rows[-1] - rows[0]) + 1) + 15) & ~15


def test_every_scratch_size_gives_the_same_shifted_record(hm):
    """5 frames in chunks of 3, scratch for two frames (runs of 2, 1, 2: they stop at the chunk), for less than one (the
    floor: one frame at a time) and for all of them"""
    kf, r, m, regs = _record("16", chunk=3, F=5)
    fs = _frame_bytes(m)
    npatch = ref.patch_grid(m, 4)["npx"] * ref.patch_grid(m, 4)["npy"]
    sh = np.random.default_rng(5).integers(-3, 4, (5, npatch, 2)).astype(np.int8)
    want = ref.shift(regs, m, 4, sh)
    assert regs.shape[0] == 5 and all((want[k] != regs[k]).any() for k in range(5))
    dm, Xs, frames, f0 = cases.scene("16")
    for scratch in (2 * fs, fs - 1, 16 << 20):
        r.tune("rec_scratch_bytes", scratch)
        r.body_rec_shift(sh, 4)
        assert np.array_equal(r.body_rec_fetch(), want), scratch
        r.tune("body_rec_chunk", 3)                                         # the record as it was
        r.body_rec_begin()
        for X, f in (2 * list(zip(Xs, frames)))[:5]:
            r.body_warp(X, f)
        r.tune("body_rec_chunk", 0)
        assert np.array_equal(r.body_rec_fetch(), regs)
    r.tune("rec_scratch_bytes", 16 << 20)
    kf.close()
