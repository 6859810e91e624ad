"""The registered video kept on the device and what is built on it (`pytest -m gpu`): hm_body_rec_* equal to what the
warps returned and to the NumPy restatement (tests/roi_ref.py) as exact integers, hydra_mi.roi.extract equal to it bit for
bit, the tracker unchanged by a bit with the record on, and the CLI end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import bodystats_ref
import roi_ref as ref
from test_roi_cpu import BOUND, THR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _seeds(m, rng, extra=4):
    """Seeds at the corners and edges of the map (first and last map pixel in raster order, the ends of a middle row and
    of a middle column), two neighbours (overlapping discs and rings) and a few anywhere."""
    rows, cols = np.nonzero(m)
    out = [(cols[0], rows[0]), (cols[-1], rows[-1])]
    rm = rows[len(rows) // 2]
    cm = cols[rows == rm]
    out += [(cm.min(), rm), (cm.max(), rm)]
    cmid = cm[len(cm) // 2]
    rr = rows[cols == cmid]
    out += [(cmid, rr.min()), (cmid, rr.max()), (cmid, rm)]
    if m[rm, min(cmid + 1, m.shape[1] - 1)]:
        out.append((cmid + 1, rm))
    for i in rng.integers(0, len(rows), extra):
        out.append((cols[i], rows[i]))
    return np.array(out, np.int32)


def _same_sums(got, want):
    for key in ("n_T", "n_G", "T", "G", "U", "w1", "w2", "c", "u1", "u2"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("name", cases.NAMES)
def test_record_and_reductions_equal_the_warp_and_the_restatement(hm, name):
    from hydra_mi import body
    dm, Xs, frames, f0 = cases.scene(name)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    tri = r.body_map()[0]
    m = tri >= 0
    H, W = m.shape
    rng = np.random.default_rng(11)
    seeds = _seeds(m, rng)
    P = len(seeds)
    labels = body.disc_labels(tri, seeds + 0.5, 2.5)
    r.body_set_labels(labels, P)
    r.tune("body_rec_chunk", 2)                                 # more than one chunk
    r.body_rec_begin()
    assert r.body_rec_count() == 0
    regs, lsums = [], []
    for rep in range(2):                                        # every frame twice: 6 (config 1: 20) frames
        for X, f in zip(Xs, frames):
            reg, _, ls = r.body_warp(X, f)
            regs.append(reg)
            lsums.append(ls)
    r.tune("body_rec_chunk", 0)
    regs = np.array(regs)
    F = len(regs)
    assert r.body_rec_count() == F
    got = r.body_rec_fetch()
    assert got.shape == regs.shape and np.array_equal(got, regs)
    assert np.array_equal(r.body_rec_fetch(1, 3), regs[1:4]) and r.body_rec_fetch(F, 0).shape[0] == 0
    assert not regs[:, ~m].any()
    # label sums: a label image given now against the sums the warps gave with the same labels set beforehand
    ls = r.body_rec_label_sums(labels, P)
    assert ls.dtype == np.uint64 and np.array_equal(ls, np.array(lsums)) and np.array_equal(ls, ref.label_sums(regs, m, labels, P))
    other = rng.integers(-1, 3, (H, W)).astype(np.int32)       # labels on and off the map, none set on the handle
    assert np.array_equal(r.body_rec_label_sums(other, 3), ref.label_sums(regs, m, other, 3))
    # seed sums: windows cut by the frame and by the map, discs that overlap
    for (rd, ri, ro, R) in ((3.0, 6.0, 8.5, 8), (1.0, 0.0, 2.0, 16), (5.5, 2.0, 4.0, 0)):
        _same_sums(r.body_rec_seed_sums(seeds, rd, ri, ro, R), ref.seed_sums(regs, m, seeds, rd, ri, ro, R))
    for R in (0, 3, 8, 20):
        S = 2 * R + 1
        w = rng.integers(0, 65536, (P, S, S)).astype(np.uint16)
        w[0] = 65535
        ws = r.body_rec_weighted_sums(seeds, w, R)
        assert ws.dtype == np.uint64 and np.array_equal(ws, ref.weighted_sums(regs, m, seeds, w, R))
    r.body_rec_end()
    assert r.body_rec_count() == 0
    kf.close()


def test_empty_ring_overflow_and_argument_errors(hm):
    dm, Xs, frames, f0 = cases.scene("96x160")
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    r.body_rec_begin()
    regs = np.array([r.body_warp(X, f)[0] for X, f in zip(Xs, frames)])
    centre = np.array([[80, 47]], np.int32)
    edge = np.array([[np.flatnonzero(m[47])[0], 47]], np.int32)
    far = np.array([[np.nonzero(m)[1][0], np.nonzero(m)[0][0]]], np.int32)     # the first map pixel: the top of the disk
    got = r.body_rec_seed_sums(centre, 2.0, 3.0, 4.0, 2)
    _same_sums(got, ref.seed_sums(regs, m, centre, 2.0, 3.0, 4.0, 2))
    # a ring without a map pixel: n_G = 0 is reported, ring sums and U are 0
    dm1, X1, fr1, f01 = cases.scene("16")
    kf1 = cases.make_filter(dm1, f01)
    r1 = kf1.state.renderer
    m1 = r1.body_map()[0] >= 0
    r1.body_rec_begin()
    regs1 = np.array([r1.body_warp(X, f)[0] for X, f in zip(X1, fr1)])
    s1 = np.array([[np.nonzero(m1)[1][0], np.nonzero(m1)[0][0]]], np.int32)
    got1 = r1.body_rec_seed_sums(s1, 2.0, 30.0, 32.0, 4)
    assert got1["n_G"][0] == 0 and got1["n_T"][0] > 0 and not got1["G"].any() and not got1["U"].any() and got1["T"].any()
    _same_sums(got1, ref.seed_sums(regs1, m1, s1, 2.0, 30.0, 32.0, 4))
    kf1.close()
    # the overflow refusal: 3 frames x (255 n_T n_G)^2 with discs and rings of about 3200 pixels
    nT = int(ref.disc_and_ring(m, centre[0], 32.0, 0.0, 32.0)[0].sum())
    assert ref.overflow_bound(3, nT, nT) >= 2 ** 63
    with pytest.raises(RuntimeError, match=r"code -1.*could pass 2\^63"):
        r.body_rec_seed_sums(centre, 32.0, 0.0, 32.0, 2)
    with pytest.raises(OverflowError):
        ref.seed_sums(regs, m, centre, 32.0, 0.0, 32.0, 2)
    _same_sums(r.body_rec_seed_sums(edge, 32.0, 31.0, 32.0, 16), ref.seed_sums(regs, m, edge, 32.0, 31.0, 32.0, 16))
    _same_sums(r.body_rec_seed_sums(far, 3.0, 6.0, 8.5, 8), ref.seed_sums(regs, m, far, 3.0, 6.0, 8.5, 8))
    for bad in (dict(R=17), dict(r_out=33.0), dict(r_in=9.0), dict(r_disc=-1.0)):
        a = dict(r_disc=3.0, r_in=6.0, r_out=8.5, R=8)
        a.update(bad)
        with pytest.raises(RuntimeError, match="code -1"):
            r.body_rec_seed_sums(centre, a["r_disc"], a["r_in"], a["r_out"], a["R"])
    off = np.array([[0, 0]], np.int32)                          # a pixel outside the map
    assert not m[0, 0]
    with pytest.raises(RuntimeError, match="code -1.*not a pixel of the body map"):
        r.body_rec_seed_sums(off, 3.0, 6.0, 8.5, 8)
    with pytest.raises(RuntimeError, match="code -1.*not a pixel of the body map"):
        r.body_rec_weighted_sums(np.array([[500, 3]], np.int32), np.ones((1, 3, 3), np.uint16), 1)
    with pytest.raises(RuntimeError, match="code -1"):
        r.body_rec_weighted_sums(centre, np.ones((1, 67, 67), np.uint16), 33)
    with pytest.raises(RuntimeError, match="code -1.*outside -1..1"):
        r.body_rec_label_sums(np.full(m.shape, 2, np.int32), 2)
    with pytest.raises(RuntimeError, match="code -1"):
        r.body_rec_fetch(2, 2)
    kf.close()


@pytest.mark.parametrize("H, W", [(72, 90), (17, 33)])
def test_warps_without_output_device_warps_budget_and_call_order(hm, H, W):
    from hydra_mi import _lib, body, mesh
    from hydra_mi.pipeline import DeviceBuffer
    dm = mesh.box_mesh(20.0, 14.0, 70.0, 57.0, 9.0) if W == 90 else mesh.box_mesh(3.0, 2.0, 30.0, 14.5, 5.0)
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(4)]
    kf = cases.make_filter(dm, frames[0])
    r = kf.state.renderer
    N, T = dm.size(), dm.t.shape[0]
    Xs = [np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + rng.normal(0, 1, 2 * N), np.zeros(2 * N))) for _ in frames]
    tri = r.body_map()[0]
    L = _lib.lib()
    r.body_rec_end()                                            # harmless before begin
    assert r.body_rec_count() == 0
    for call in (lambda: r.body_rec_fetch(0, 0), lambda: r.body_rec_label_sums(np.zeros((H, W), np.int32), 1),
                 lambda: r.body_rec_seed_sums(np.zeros((1, 2), np.int32), 1.0, 2.0, 3.0, 1),
                 lambda: r.body_rec_weighted_sums(np.zeros((1, 2), np.int32), np.ones((1, 1, 1), np.uint16), 0)):
        with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_begin first"):
            call()
    want = np.array([r.body_warp(X, f)[0] for X, f in zip(Xs, frames)])      # no record: the warp as ever
    r.body_rec_begin()
    with pytest.raises(RuntimeError, match="code -3.*no frame recorded"):
        r.body_rec_label_sums(np.zeros((H, W), np.int32), 1)
    ts = np.empty(T, np.uint64)
    for k, (X, f) in enumerate(zip(Xs, frames)):                # host warps without an output (sums only, nothing at all)
        x, fr = np.ascontiguousarray(X), np.ascontiguousarray(f)
        _lib.check(L.hm_body_warp(r._h, _lib.ptr(x), _lib.ptr(fr), None, _lib.ptr(ts) if k % 2 else None, None), "hm_body_warp")
    assert r.body_rec_count() == 4 and np.array_equal(r.body_rec_fetch(), want)
    r.body_rec_begin()                                          # again: starts over; device warps of every kind
    assert r.body_rec_count() == 0
    d_f, d_o, d_s = DeviceBuffer(H * W), DeviceBuffer(3 * H * W), DeviceBuffer(8 * T)
    for k, (X, f) in enumerate(zip(Xs, frames)):
        d_f.upload(f)
        r.body_warp_dev(X, d_f.ptr, (d_o.ptr, d_o.ptr, None, None)[k], (3, 1, 1, 3)[k], d_s.ptr if k < 3 else None, None)
        _lib.check(L.hm_ctx_sync(r._h), "hm_ctx_sync")           # (the next upload overwrites the frame)
    assert r.body_rec_count() == 4 and np.array_equal(r.body_rec_fetch(), want)
    for b in (d_f, d_o, d_s):
        b.close()
    # the budget: room for three frames, with the statistics on as well; the refused warp changes neither
    per_frame = body.record_bytes(tri, 1)
    assert body.record_bytes(tri, 7) == 7 * per_frame and per_frame % 16 == 0
    r.tune("body_rec_chunk", 2)
    r.body_rec_begin(3 * per_frame + per_frame - 1)
    r.body_stats_begin()
    for X, f in zip(Xs[:3], frames[:3]):
        r.body_warp(X, f)
    with pytest.raises(RuntimeError, match=r"code -3.*holds 3 frames of %d bytes.*budget of %d bytes holds 3" %
                       (per_frame, 4 * per_frame - 1)):
        r.body_warp(Xs[3], frames[3])
    assert r.body_rec_count() == 3 and r.body_stats_count() == 3
    assert np.array_equal(r.body_rec_fetch(), want[:3])
    s1 = r.body_stats_fetch()[0]
    assert np.array_equal(s1, bodystats_ref.accumulate(want[:3], tri >= 0)[0])
    r.body_stats_end()                                          # the record goes on without the statistics
    assert np.array_equal(r.body_rec_label_sums(np.zeros((H, W), np.int32), 1)[:, 0],
                          want[:3][:, tri >= 0].astype(np.uint64).sum(1))
    r.body_rec_begin(per_frame - 1)                             # room for no frame at all
    with pytest.raises(RuntimeError, match="code -3.*holds 0 frames"):
        r.body_warp(Xs[0], frames[0])
    r.body_rec_end()
    r.body_rec_end()
    r.tune("body_rec_chunk", 0)
    assert np.array_equal(r.body_warp(Xs[1], frames[1])[0], want[1])
    r.body_rec_begin()
    r.body_warp(Xs[0], frames[0])
    kf.close()                                                  # closed while recording


def _config1_run(keep):
    from hydra_mi import body, kalman, mesh, synth
    video, flow = synth.test_data(128, 128)
    g = np.load(os.path.join(cases.GOLD, "config1_track.npz"))
    kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), video[:, :, 0], flow[:, :, :, 0], True)
    b = body.BodyReadout(kf, stats=True, keep=keep)
    out = []
    for k in range(1, 6):
        frame = video[:, :, k]
        e = kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
        reg = b.frame(kf.state.X, frame)[0]
        out.append((kf.state.X.copy(), tuple(float(x) for x in e[:4]), reg))
    return kf, b, out


def test_config1_track_and_statistics_unchanged_by_the_record(hm):
    kf0, b0, plain = _config1_run(False)
    s0 = kf0.state.renderer.body_stats_fetch()
    kf0.close()
    kf, b, got = _config1_run(True)
    r = kf.state.renderer
    for (Xa, ea, ra), (Xb, eb, rb) in zip(plain, got):
        assert np.array_equal(Xa, Xb) and ea == eb and np.array_equal(ra, rb)
    assert all(np.array_equal(a, c) for a, c in zip(s0, r.body_stats_fetch()))
    assert r.body_rec_count() == 5 and np.array_equal(r.body_rec_fetch(), np.array([g[2] for g in got]))
    kf.close()


def _pipeline_run(video, masks, c, rad, resident, keep):
    from hydra_mi import body, kalman, mesh
    from hydra_mi.pipeline import FlowEKFPipeline
    n = video.shape[1]
    kf = kalman.IteratedMSKalmanFilter(mesh.disk_mesh(c[0], c[1], rad - 1.0, 12.0), video[0],
                                       np.zeros((n, n, 2), np.float32), True, nI=3)
    pipe = FlowEKFPipeline(kf, video, masks, flow_batch=2, resident=resident)
    got = []
    b = body.BodyReadout(kf, stats=True, keep=keep)
    pipe.run(on_frame=lambda k, e: got.append((kf.state.X.copy(), tuple(e[:4]), kf.niter)), body=b)
    pipe.close()
    return kf, got, b


@pytest.mark.parametrize("resident", [True, False])
def test_pipeline_records_and_changes_nothing(hm, resident):
    from hydra_mi import synth
    n, F = 96, 24
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    kf0, plain, b0 = _pipeline_run(video, masks, c, rad, resident, False)
    s0 = kf0.state.renderer.body_stats_fetch()
    res0 = b0.results()
    kf0.close()
    kf, got, b = _pipeline_run(video, masks, c, rad, resident, True)
    assert len(got) == len(plain) == F - 1
    for (Xa, ea, ia), (Xb, eb, ib) in zip(plain, got):
        assert np.array_equal(Xa, Xb) and ea == eb and ia == ib
    r = kf.state.renderer
    assert all(np.array_equal(a, c) for a, c in zip(s0, r.body_stats_fetch()))
    assert np.array_equal(res0["tri_sums"], b.results()["tri_sums"])
    assert r.body_rec_count() == F - 1
    rec = r.body_rec_fetch()
    r.body_rec_end()                                            # the warps below must not append
    r.body_stats_end()
    regs = np.array([r.body_warp(X, video[k + 1])[0] for k, (X, _, _) in enumerate(got)])
    assert np.array_equal(rec, regs)
    kf.close()


@pytest.mark.parametrize("seed", [0, 3])
def test_extract_on_the_planted_scene_equals_the_restatement(hm, seed):
    """hydra_mi.roi.extract through the product on the planted video with neuropil as the tracker sees it (half the
    frames at rest, half shifted): footprints, labels, traces and dF/F equal the restatement on the registered video
    bit for bit, and the corrected ROI traces meet the bound of tests/test_roi_cpu.py (seed 3 is the worst of the six)."""
    from hydra_mi import body, mesh, roi
    dm = mesh.box_mesh(*ref.PLANTED_BOX)
    frames, states, cs, act = ref.planted_scene(seed, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True)
    with pytest.raises(RuntimeError, match="no frame recorded"):
        roi.extract(b, cs + 0.5)
    regs = np.array([b.registered(X, f) for X, f in zip(states, frames)])
    m = b.tri_of_pixel >= 0
    assert np.array_equal(m, ref.planted_map())
    assert np.array_equal(np.where(m[None], regs, 0), np.where(m[None], ref.planted_video(seed)[0], 0))
    got = roi.extract(b, cs + 0.5, thr=THR, alpha=1.0)
    want = ref.extract(regs, m, cs, thr=THR, alpha=1.0)
    for key in ("footprints", "F_roi", "F_np", "dff"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key
    for key in ("roi_labels", "roi_counts", "ring_counts", "seed_fallback"):
        assert np.array_equal(got[key], want[key]), key
    assert got["roi_labels"].dtype == np.int32 and got["roi_labels"].shape == m.shape
    assert np.array_equal(_bits(roi.extract(b, cs + 0.5, alpha=1.0)["dff"]), _bits(got["dff"]))      # thr None: the default
    F_c = got["F_roi"] - got["F_np"]
    worst = min(np.corrcoef(F_c[:, s], act[s])[0, 1] for s in range(12))
    print("seed %d: worst corrected ROI trace %.4f" % (seed, worst))
    assert worst > BOUND and not got["seed_fallback"].any()
    # the disc traces from the record: what the second pass over the video reads
    kf.state.renderer.body_rec_end()
    b2 = body.BodyReadout(kf, keep=True)
    for X, f in zip(states[:20], frames[:20]):
        b2.registered(X, f)
    rec = body.read_out_recorded(b2, states[:20], cs + 0.5, 3.0)
    kf.state.renderer.body_rec_end()
    two = body.read_out(kf, states[:20], frames[:20], cs + 0.5, 3.0)
    for key in ("points", "point_means", "point_counts"):
        assert rec[key].dtype == two[key].dtype and np.array_equal(rec[key], two[key], equal_nan=True), key
    with pytest.raises(RuntimeError, match="without keep=True"):
        roi.extract(body.BodyReadout(kf), cs + 0.5)
    kf.close()


def test_cli_rois_end_to_end(hm, tmp_path):
    from hydra_mi import synth
    n, F = 96, 6
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "5", "--find-radius", "4", "--find-score", "std"]
    out0, out1 = str(tmp_path / "plain.npz"), str(tmp_path / "rois.npz")
    res0 = subprocess.run(base + [out0] + find, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res0.returncode == 0, res0.stderr[-2000:]
    res = subprocess.run(base + [out1] + find + ["--rois"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z0, z = np.load(out0), np.load(out1)
    F1 = z["X"].shape[0]
    assert F1 == F - 1 and np.array_equal(z["X"], z0["X"])
    P = z["found_points"].shape[0]
    assert 1 <= P <= 5 and np.array_equal(z["found_points"], z0["found_points"])
    for key in ("points", "point_means", "point_counts", "tri_means"):
        assert z[key].dtype == z0[key].dtype and np.array_equal(z[key], z0[key], equal_nan=True), key
    Q = z["roi_points"].shape[0]
    assert Q == P                                               # found points are map pixels
    assert z["roi_footprints"].shape == (Q, 17, 17) and z["roi_footprints"].dtype == np.float64
    assert z["roi_labels"].shape == (n, n) and z["roi_labels"].dtype == np.int32
    assert z["roi_counts"].shape == (Q,) and z["roi_ring_counts"].shape == (Q,) and z["roi_seed_fallback"].shape == (Q,)
    assert z["roi_seed_fallback"].dtype == np.bool_
    for key in ("roi_F", "roi_Fnp", "roi_dff"):
        assert z[key].shape == (F1, Q) and z[key].dtype == np.float64, key
    assert (z["roi_counts"] >= 1).all() and np.array_equal(np.bincount(z["roi_labels"][z["roi_labels"] >= 0], minlength=Q),
                                                           z["roi_counts"])
    assert (z["roi_labels"][np.isnan(z["body_mean"])] == -1).all()
    assert "ROIs: %d cells" % Q in res.stdout and "roi_F" not in z0.files
    small = subprocess.run(base + [str(tmp_path / "small.npz")] + find + ["--rois", "--rois-max-gb", "1e-6"],
                           capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert small.returncode == 0, small.stderr[-2000:]
    zs = np.load(str(tmp_path / "small.npz"))
    assert "no ROIs, the disc read-out instead" in small.stdout and "roi_F" not in zs.files
    assert np.array_equal(zs["point_means"], z0["point_means"], equal_nan=True)
    bad = subprocess.run(base + [out1, "--rois"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert bad.returncode == 2 and "needs --find-points or --points" in bad.stderr
