"""The smooth sub-pixel shift field of the stabiliser (`pytest -m gpu`): hm_body_rec_warp / _field_sums equal to the NumPy
restatement (tests/stabfield_ref.py) as exact integers, hydra_mi.stabilize(mode="field") through the product equal to it
bit for bit, the tracker unchanged by a bit with field stabilisation run between frames, and the CLI end to end.  Every
comparison is an equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import roi_ref
import stab_ref
import stabfield_ref as ref
from test_roi_cpu import THR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("33x17", "96x160", "config1", "16")
GRIDS = ((4, 1), (7, 2), (16, 3), (64, 8))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _fill(r, name, chunk=2, F=None):
    """(re)start the record and record every frame of the scene twice (the first F of those, if given), in chunks of two
    frames"""
    dm, Xs, frames, f0 = cases.scene(name)
    r.tune("body_rec_chunk", chunk)
    r.body_rec_begin()
    for X, f in (2 * list(zip(Xs, frames)))[:F]:
        r.body_warp(X, f)
    r.tune("body_rec_chunk", 0)


def _record(name, chunk=2, tp=3, F=None):
    """A filter on the scene with every frame recorded twice, in chunks of two frames, runs of three frames per workgroup
    (so that runs cross chunks) -> (kf, renderer, map, recorded frames)"""
    dm, Xs, frames, f0 = cases.scene(name)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    r.tune("rec_tp_frames", tp)
    _fill(r, name, chunk, F)
    regs = r.body_rec_fetch()
    assert not regs[:, ~m].any()
    return kf, r, m, regs


def _npatch(m, B):
    g = stab_ref.patch_grid(m, B)
    return g["npx"] * g["npy"]


def _field(rng, F, npatch, lim):
    """random q within +-lim, about 70 % of the patches valid; frame 1 all invalid, frame 2 with a single valid patch"""
    q = rng.integers(-lim, lim + 1, (F, npatch, 2)).astype(np.int16)
    valid = (rng.random((F, npatch)) < 0.7).astype(np.uint8)
    valid[1] = 0
    valid[2] = 0
    valid[2, rng.integers(0, npatch)] = 1
    return q, valid


@pytest.mark.parametrize("name", SCENES)
def test_warp_and_field_sums_equal_the_restatement(hm, name):
    kf, r, m, regs = _record(name)
    F, H, W = regs.shape
    rng = np.random.default_rng(len(name) + 11)
    g = stab_ref.patch_grid(m, 7)
    if name == "33x17":
        assert g["bw"] % 4 and g["bw"] % 7 and g["bw"] % 16                # a box no multiple of 4 or of B wide
    if name == "96x160":
        assert not m[g["r0"]:g["r0"] + g["bh"], g["c0"]:g["c0"] + g["bw"]].all()     # a map that is no rectangle
    if name == "16":
        assert _npatch(m, 64) == 1                                          # a single patch per axis
    k0, n = 1, F - 2                                                        # starts and ends inside a chunk
    first = True
    for B, S in GRIDS:
        npatch = _npatch(m, B)
        for lim in (16 * S, 256):
            q, valid = _field(rng, F, npatch, lim)
            if lim == 256:
                q[0, 0], q[F - 1, npatch - 1] = (256, -256), (-256, 256)
                valid[0, 0] = valid[F - 1, npatch - 1] = 1
            if not first:
                _fill(r, name)                                              # the record as it was
            first = False
            fs = r.body_rec_field_sums(q, valid, B)
            assert fs.dtype == np.uint32 and np.array_equal(fs, ref.field_sums(regs, m, B, q, valid))
            assert np.array_equal(r.body_rec_field_sums(q[k0:k0 + n], valid[k0:k0 + n].astype(bool), B, k0, n),
                                  ref.field_sums(regs[k0:k0 + n], m, B, q[k0:k0 + n], valid[k0:k0 + n]))
            r.body_rec_warp(q, valid, B)
            want = ref.warp(regs, m, B, q, valid)
            assert np.array_equal(want[1], regs[1])                         # the frame without a valid patch stays
            assert (want != regs).any() and want.any() and np.array_equal(r.body_rec_fetch(), want)
    assert r.body_rec_count() == F
    kf.close()


@pytest.mark.parametrize("name, B, S", [("33x17", 7, 1), ("96x160", 16, 3), ("config1", 64, 8), ("16", 4, 1)])
def test_warp_in_place_then_every_reduction_sees_the_warped_frames(hm, name, B, S):
    from hydra_mi import body
    kf, r, m, regs = _record(name)
    F, H, W = regs.shape
    rng = np.random.default_rng(B + 100)
    tri = r.body_map()[0]
    npatch = _npatch(m, B)
    r.body_rec_warp(np.zeros((F, npatch, 2), np.int16), np.ones((F, npatch), np.uint8), B)     # nothing changes
    assert np.array_equal(r.body_rec_fetch(), regs)
    q, valid = _field(rng, F, npatch, 16 * S)
    sh = np.repeat(rng.integers(-S, S + 1, (F, 1, 2)), npatch, 1).astype(np.int8)      # one whole-pixel shift per frame, all
    sums = r.body_rec_field_sums(16 * sh.astype(np.int16), np.ones((F, npatch), bool), B)   # valid: the whole-pixel gather
    assert np.array_equal(sums, stab_ref.frame_sums(regs, m, B, sh))
    r.body_rec_warp(q, valid, B)
    want = ref.warp(regs, m, B, q, valid)
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
    ms, exp = r.body_rec_match(noise, B, S), stab_ref.match(want, m, B, S, noise)
    for key in ("n_core", "A", "V1", "V2"):
        assert np.array_equal(ms[key], exp[key]), key
    q2, valid2 = _field(rng, F, npatch, 256)                               # a second time: warps what is there
    r.body_rec_warp(q2, valid2, B)
    assert np.array_equal(r.body_rec_fetch(), ref.warp(want, m, B, q2, valid2))
    assert r.body_rec_count() == F
    r.body_warp(cases.scene(name)[1][0], cases.scene(name)[2][0])           # the record goes on
    assert r.body_rec_count() == F + 1
    kf.close()


def test_refusals_name_their_numbers(hm):
    kf, r, m, regs = _record("33x17")
    F, H, W = regs.shape
    one = np.ones((F, 1), np.uint8)
    for B in (3, 65):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_warp: patch size %d outside 4\.\.64" % B):
            r.body_rec_warp(np.zeros((F, 1, 2), np.int16), one, B)
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_field_sums: patch size %d outside 4\.\.64" % B):
            r.body_rec_field_sums(np.zeros((F, 1, 2), np.int16), one, B)
    npatch = _npatch(m, 8)
    q, valid = np.zeros((F, npatch, 2), np.int16), np.ones((F, npatch), np.uint8)
    q[2, 3, 1] = 257
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_warp: q 257 \(dy of patch 3, frame 2"):
        r.body_rec_warp(q, valid, 8)
    q[2, 3, 1], q[1, 0, 0] = 0, -257
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_warp: q -257 \(dx of patch 0, frame 1"):
        r.body_rec_warp(q, valid, 8)
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_field_sums: q -257 \(dx of patch 0, frame 1"):
        r.body_rec_field_sums(q, valid, 8)
    assert np.array_equal(r.body_rec_fetch(), regs)                         # a refused warp changes nothing
    q[1, 0, 0] = 0
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_field_sums: frames 5 .. 6 of a record of 6"):
        r.body_rec_field_sums(q[:2], valid[:2], 8, 5, 2)
    too_many = 2 ** 32 // 255 + 1                                           # n 255 >= 2^32 (refused before q is looked at)
    with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_field_sums: %d frames x 255 could pass 2\^32" % too_many):
        _field_sums_raw(r, too_many, q, valid)
    with pytest.raises(ValueError, match="q for 1 patches"):
        r.body_rec_warp(np.zeros((F, 1, 2), np.int16), one, 8)
    with pytest.raises(ValueError, match="need int16"):
        r.body_rec_warp(np.zeros((F, npatch, 2), np.int8), valid, 8)
    r.body_rec_begin()                                                      # an empty record
    for call in (lambda: r.body_rec_field_sums(q[:0], valid[:0], 8, 0, 0), lambda: r.body_rec_warp(q[:0], valid[:0], 8)):
        with pytest.raises(RuntimeError, match="code -3.*no frame recorded"):
            call()
    r.body_rec_end()                                                        # before begin
    for call in (lambda: r.body_rec_field_sums(q[:0], valid[:0], 8, 0, 0), lambda: r.body_rec_warp(q[:0], valid[:0], 8)):
        with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_begin first"):
            call()
    kf.close()


def _field_sums_raw(r, n, q, valid):
    """the C call with a frame count the wrapper would not size arrays for"""
    from hydra_mi import _lib
    out = np.empty((r.ny, r.nx), np.uint32)
    _lib.check(_lib.lib().hm_body_rec_field_sums(r._h, 0, n, 8, _lib.ptr(q), _lib.ptr(valid), _lib.ptr(out)),
               "hm_body_rec_field_sums")


def test_stabilize_field_on_the_smooth_scene_equals_the_restatement(hm):
    """hydra_mi.stabilize(mode="field") through the product on the planted video with the smooth sub-pixel jitter as the
    tracker sees it: the estimate equals the restatement's, and roi.extract on the warped record equals roi_ref.extract on
    the restatement's warp of the registered video bit for bit."""
    from hydra_mi import body, mesh, roi, stabilize
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs, act, jit = ref.smooth_jittered_scene(0, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True)
    regs = np.array([b.registered(X, f) for X, f in zip(states, frames)])
    m = b.tri_of_pixel >= 0
    assert np.array_equal(m, roi_ref.planted_map()) and np.array_equal(regs, np.where(m[None], jit, 0))
    old = stabilize.MATCH_BYTES
    stabilize.MATCH_BYTES = 3 * 4 * 64 * 49 * 37                           # blocks of 37 frames
    try:
        est = stabilize.stabilize(b, passes=2, mode="field")
    finally:
        stabilize.MATCH_BYTES = old
    want = ref.estimate(regs, m, passes=2, min_score=stabilize.DEFAULT_MIN_SCORE, mode="field")
    assert est["mode"] == "field" and est["q"].dtype == np.int16 and est["valid"].dtype == np.uint8
    assert np.array_equal(est["q"], want["q"]) and np.array_equal(est["valid"], want["valid"])
    assert np.array_equal(est["shifts"], want["shifts"]) and np.array_equal(est["fallback"], want["fallback"])
    assert np.array_equal(_bits(est["score"]), _bits(want["score"])) and np.array_equal(est["n_core"], want["n_core"])
    assert len(est["templates"]) == 2 and all(np.array_equal(a, c) for a, c in zip(est["templates"], want["templates"]))
    assert (est["q"] % 16).any() and not est["q"][est["valid"] == 0].any()
    stab = ref.warp(regs, m, 16, want["q"], want["valid"])
    assert (stab != regs).any() and np.array_equal(b.r.body_rec_fetch(), stab)
    got = roi.extract(b, cs + 0.5, thr=THR, alpha=1.0)
    exp = roi_ref.extract(stab, m, cs, thr=THR, alpha=1.0)
    for key in ("footprints", "F_roi", "F_np", "dff"):
        assert np.array_equal(_bits(got[key]), _bits(exp[key])), key
    for key in ("roi_labels", "roi_counts", "ring_counts", "seed_fallback"):
        assert np.array_equal(got[key], exp[key]), key
    with pytest.raises(ValueError, match="mode 'fields'"):
        stabilize.estimate(b, mode="fields")
    kf.close()


def test_field_stabilising_between_frames_changes_nothing_of_the_filter(hm):
    """Config 1 (128^2, the golden track) with the record kept and field-stabilised between every two frames: states,
    covariance and error terms bit-identical to the run without."""
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
                est = stabilize.stabilize(b, B=8, S=2, min_score=0.0, passes=2, mode="field")
                assert est["q"].shape[0] == k + 1
            out.append((kf.state.X.copy(), kf.niter, e[:4], np.array(kf.state.W, np.float64).copy()))
        runs[stab] = out
        kf.close()
    for (Xa, ia, ea, Wa), (Xb, ib, eb, Wb) in zip(runs[False], runs[True]):
        assert np.array_equal(Xa, Xb) and ia == ib and ea == eb and np.array_equal(Wa, Wb)


def test_cli_stab_mode_field_end_to_end(hm, tmp_path):
    """run_kalmanfilter.py --find-points 12 --rois --stabilize --stab-mode field on ten frames of the smoothly jittered video,
    as an animal: a disc of it on black.  stab_q equals the restatement's estimate on the --registered frames and has
    sub-pixel parts; the ROI traces equal the restatement on its warp of them and differ from --stab-mode patch; without
    --stab-mode the output is today's."""
    from hydra_mi import roi, stabilize
    from test_views_cpu import read_avi
    F, B, S = 10, 16, 3
    j = ref.smooth_jittered_video(0)[0][:F]
    n = j.shape[1]
    yy, xx = np.mgrid[0:n, 0:n]
    video = j * ((xx - 63.5) ** 2 + (yy - 63.5) ** 2 <= 48.0 ** 2).astype(np.uint8)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "12", "--find-radius", "4", "--find-score", "std", "--rois", "--stabilize",
            "--stab-patch", str(B), "--stab-search", str(S)]
    outs = {}
    for key, more in (("default", []), ("patch", ["--stab-mode", "patch"]),
                      ("field", ["--stab-mode", "field", "--registered", str(tmp_path / "reg.avi")])):
        out = str(tmp_path / (key + ".npz"))
        res = subprocess.run(base + [out] + find + more, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert res.returncode == 0, res.stderr[-2000:]
        outs[key] = (np.load(out), res.stdout)
    (z0, s0), (zp, sp), (z, sf) = outs["default"], outs["patch"], outs["field"]
    assert "stab_q" not in z0.files and sorted(z0.files) == sorted(zp.files)           # without the flag: today's keys
    for key in z0.files:
        assert z0[key].tobytes() == zp[key].tobytes(), key
    assert "Stabilised: " in s0 and "Stabilised: " in sp and "Stabilised (field): " in sf
    assert sorted(z.files) == sorted(z0.files + ["stab_q"])
    F1 = z["X"].shape[0]
    npatch = z["stab_shifts"].shape[1]
    assert F1 == F - 1 and z["stab_q"].shape == (F1, npatch, 2) and z["stab_q"].dtype == np.int16
    regs = np.array([f[:, :, 0] for f in read_avi(str(tmp_path / "reg.avi"))["frames"]])
    m = ~np.isnan(z["body_mean"])
    want = ref.estimate(regs, m, B, S, min_score=stabilize.DEFAULT_MIN_SCORE, mode="field")
    assert np.array_equal(z["stab_q"], want["q"]) and np.array_equal(z["stab_shifts"], want["shifts"])
    assert np.array_equal(z["stab_fallback"], want["fallback"]) and np.array_equal(_bits(z["stab_score"]), _bits(want["score"]))
    assert (z["stab_q"] % 16).any()                                         # some q is not a whole pixel
    assert "%.1f %% fallbacks, mean |shift| %.3f px" % (100.0 * z["stab_fallback"].mean(),
                                                        np.abs(z["stab_q"] / 16.0).sum(2).mean()) in sf
    stab = ref.warp(regs, m, B, want["q"], want["valid"])
    assert (stab != regs).any()
    pts = z["found_points"]
    assert np.array_equal(pts, zp["found_points"])
    exp = roi_ref.extract(stab, m, roi.seeds_of(pts), r_disc=3.0, thr=roi.DEFAULT_THR, alpha=0.7)
    for key, name in (("roi_footprints", "footprints"), ("roi_F", "F_roi"), ("roi_Fnp", "F_np"), ("roi_dff", "dff")):
        assert np.array_equal(_bits(z[key]), _bits(exp[name])), key
    assert np.array_equal(z["roi_labels"], exp["roi_labels"]) and np.array_equal(z["roi_counts"], exp["roi_counts"])
    for key in ("roi_F", "roi_dff", "point_means"):
        assert not np.array_equal(z[key], zp[key]), key


def _frame_bytes(m):
    """bytes of one frame of the record: the map's bounding box, rows padded to 4 bytes, the frame to 16"""
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    pitch = (int(cols[-1] - cols[0]) + 1 + 3) & ~3
    return (pitch * (int(rows[-1] - rows[0]) + 1) + 15) & ~15


def test_every_scratch_size_gives_the_same_warped_record(hm):
    """5 frames in chunks of 3, scratch for two frames (runs of 2, 1, 2: they stop at the chunk), for less than one (the
    floor: one frame at a time) and for all of them"""
    kf, r, m, regs = _record("16", chunk=3, F=5)
    fs = _frame_bytes(m)
    q, valid = _field(np.random.default_rng(6), 5, _npatch(m, 4), 48)
    want = ref.warp(regs, m, 4, q, valid)
    assert regs.shape[0] == 5 and (want != regs).any()
    for scratch in (2 * fs, fs - 1, 16 << 20):
        r.tune("rec_scratch_bytes", scratch)
        r.body_rec_warp(q, valid, 4)
        assert np.array_equal(r.body_rec_fetch(), want), scratch
        _fill(r, "16", 3, 5)                                                # the record as it was
    r.tune("rec_scratch_bytes", 16 << 20)
    kf.close()
