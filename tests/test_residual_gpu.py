"""The residual video of the demixed model on the device (`pytest -m gpu`): hm_body_rec_residual_planes and
hm_body_rec_residual_stats_add equal to the NumPy restatement (tests/residual_ref.py) byte for byte, their refusals,
hydra_mi.residual.find_more through the product on the paired planted video, and the CLI end to end.  Every comparison
is an equality."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import bodystats_ref as bs
import demix_ref
import residual_ref as ref
import roi_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, F = 48, 64, 7


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _record(F=F, chunk=2):
    """A 64 x 48 frame with a disc of a mesh (a box 41 px wide: the last dword of a row and the last segment of a frame are
    partial; pixels of the box off the map), F random frames recorded at perturbed states in chunks of `chunk` frames
    -> (kf, renderer, map, recorded frames)"""
    from hydra_mi import mesh
    dm = mesh.disk_mesh(31.5, 23.5, 20.3, 7.0)
    rng = np.random.default_rng(7)
    f0 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    N = dm.size()
    r.tune("body_rec_chunk", chunk)
    r.body_rec_begin()
    for k in range(F):
        f = rng.integers(0, 256, (H, W), dtype=np.uint8)
        f[rng.random((H, W)) < 0.05] = 0
        f[rng.random((H, W)) < 0.05] = 255
        X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + rng.normal(0, 0.7 * (k % 3), 2 * N), np.zeros(2 * N)))
        r.body_warp(X, f)
    r.tune("body_rec_chunk", 0)
    regs = r.body_rec_fetch()
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    assert bw % 4 and ((bw + 3) // 4 * bh) % 64                          # partial last dword of a row, partial last segment
    assert not m[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].all()       # a map that is no rectangle
    assert regs.shape == (F, H, W) and not regs[:, ~m].any()
    return kf, r, m, regs


def _cells(m):
    """Five cells as discs: on the box's first and last column and first and last row (partly off the map), and in the
    middle; the four middle pixels also belong to cells 0, 1 and 2 -> (L, H, W) bool"""
    yy, xx = np.mgrid[0:H, 0:W]
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    at = [(cols[0], np.flatnonzero(m[:, cols[0]])[0]), (cols[-1], np.flatnonzero(m[:, cols[-1]])[-1]),
          (np.flatnonzero(m[rows[0]])[0], rows[0]), (np.flatnonzero(m[rows[-1]])[-1], rows[-1]), (31, 23)]
    cells = np.array([(xx - c) ** 2 + (yy - r) ** 2 <= 9 for c, r in at])
    cells[:3, 23:25, 31:33] = True
    assert all((cells[s] & m).any() and (cells[s] & ~m).any() for s in range(4))          # partly off the map
    assert m[23:25, 31:33].all() and (cells[:, 23, 31].sum() == 4)
    return cells


def _layers(cells, n_layers, L, rng):
    """-> (labels (n_layers, H, W) int32, weights uint16): per pixel its cells (all of them cell 0 when L is 1) in
    ascending index, the first n_layers kept; weights random with 0 and 65535 among them"""
    lab = np.full((n_layers, H, W), -1, np.int32)
    depth = np.zeros((H, W), np.int64)
    for s in range(cells.shape[0] if L > 1 else 1):
        on = (cells[s] if L > 1 else cells.any(0)) & (depth < n_layers)
        lab[depth[on], np.nonzero(on)[0], np.nonzero(on)[1]] = s
        depth += on
    wt = rng.integers(0, 65536, lab.shape).astype(np.uint16)
    wt[rng.random(lab.shape) < 0.1] = 65535
    wt[rng.random(lab.shape) < 0.05] = 0
    return lab, wt


#: (n_layers, L, weights given)
CASES = ((1, 1, False), (1, 5, True), (2, 5, True), (4, 5, True), (4, 5, False))


def test_planes_equal_the_restatement(hm):
    kf, r, m, regs = _record()
    cells = _cells(m)
    rng = np.random.default_rng(11)
    blank = ((rng.random((H, W)) < 0.1) * rng.integers(1, 256, (H, W))).astype(np.uint8)
    blank[23, 31] = 0
    assert (blank[m] != 0).any() and (blank[cells.any(0) & m] != 0).any()
    for n_layers, L, given in CASES:
        lab, wt = _layers(cells, n_layers, L, rng)
        wt = wt if given else None
        if n_layers == 4:
            assert (lab[:, 23, 31] >= 0).all()                               # a pixel carrying four cells
        # traces of both signs, up to +-450 grey levels at full weight: both clamps are reached
        tr = rng.integers(-450 * 256, 450 * 256, (F, L)).astype(np.int32)
        want = {}
        for bl in (None, blank):
            for offset in (0, 64, 255):
                want[bl is not None, offset] = ref.planes(regs, m, lab, wt, tr, bl, offset)
        w64 = want[False, 64]
        on = cells.any(0) & m
        assert (w64[0][:, on] == 0).any() and (w64[0][:, on] == 255).any() and w64[1] > 0
        assert not want[True, 64][0][:, blank != 0].any() and want[True, 64][1] < w64[1]
        first = None
        for run in (1, 3, 1 << 20):                                          # frames per run: 1, 3 (runs cross chunks), one run
            r.tune("rec_res_frames", run)
            got = {key: r.body_rec_residual_planes(lab, wt, tr, blank if key[0] else None, key[1]) for key in want}
            for key in want:
                assert got[key][0].dtype == np.uint8 and np.array_equal(got[key][0], want[key][0]), (n_layers, L, run, key)
                assert got[key][1] == want[key][1], (n_layers, L, run, key)
            first = first or got
            assert all(np.array_equal(got[key][0], first[key][0]) for key in want)
            for k0, n in ((1, F - 2), (2, 1), (0, 3), (F, 0), (3, 0)):          # sub-ranges: inside chunks, across them, empty
                p, c = r.body_rec_residual_planes(lab, wt, tr, blank, 64, k0, n)
                w = ref.planes(regs[k0:k0 + n], m, lab, wt, tr[k0:k0 + n], blank, 64)
                assert p.shape == (n, H, W) and np.array_equal(p, w[0]) and c == w[1], (n_layers, L, run, k0, n)
        r.tune("rec_res_frames", 8)
    # no cell anywhere: offset + v, clamped, in the map
    none = np.full((2, H, W), -1, np.int32)
    for offset in (0, 64, 255):
        p, c = r.body_rec_residual_planes(none, None, np.zeros((F, 3), np.int32), None, offset)
        assert np.array_equal(p, np.where(m, np.minimum(255, regs.astype(np.int64) + offset), 0))
        assert c == int((regs[:, m].astype(np.int64) + offset > 255).sum())
    # the largest magnitudes: four layers of weight 65535, traces at the ends of int32
    full = np.zeros((4, H, W), np.int32)
    ends = np.array([[-2 ** 31], [2 ** 31 - 1], [0], [1], [-1], [2 ** 31 - 1], [-2 ** 31]], np.int32)
    p, c = r.body_rec_residual_planes(full, None, ends, None, 64)
    w = ref.planes(regs, m, full, None, ends, None, 64)
    assert np.array_equal(p, w[0]) and c == w[1] and (p[0][m] == 255).all() and not p[1].any()
    assert np.array_equal(r.body_rec_fetch(), regs)                        # the record has not changed by a bit
    kf.close()


def test_stats_add_equals_the_statistics_of_the_planes(hm):
    kf, r, m, regs = _record()
    cells = _cells(m)
    rng = np.random.default_rng(13)
    lab, wt = _layers(cells, 4, 5, rng)
    tr = rng.integers(-100 * 256, 100 * 256, (F, 5)).astype(np.int32)
    blank = np.zeros((H, W), np.uint8)
    blank[22:26, 30:34] = 1
    planes, clipped = ref.planes(regs, m, lab, wt, tr, blank, 64)
    want = bs.accumulate(planes, m)
    r.tune("rec_res_frames", 3)
    r.body_stats_begin()
    assert r.body_rec_residual_stats_add(lab, wt, tr, blank, 64) == clipped
    assert r.body_stats_count() == F
    for g, w in zip(r.body_stats_fetch(), want):
        assert np.array_equal(g, w)
    imgs, exp = r.body_stats_images(), bs.images(*want, F, m)
    for g, w in zip(imgs[:3], exp[:3]):
        assert np.array_equal(_bits(g), _bits(w))
    assert np.array_equal(imgs[3], exp[3])
    assert (imgs[2][23:25, 31:33] == 0.0).all()                            # a blanked pixel is constant: corr 0
    idx, sc, found = r.body_stats_peaks("corr", 3)
    widx, wsc = bs.peaks_fast(exp[2], m, 3)
    assert found == len(widx) and np.array_equal(idx, widx) and np.array_equal(_bits(sc), _bits(wsc))
    assert r.body_rec_residual_stats_add(lab, wt, tr, blank, 64) == clipped     # twice: the sums double
    assert r.body_stats_count() == 2 * F
    for g, w in zip(r.body_stats_fetch()[:3], want[:3]):
        assert np.array_equal(g, 2 * w)
    r.tune("body_stats_cap", 3 * F - 1)                                     # the third addition would pass the capacity
    before = r.body_stats_fetch()
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_residual_stats_add: the statistics hold %d frames and the "
                                           r"record %d, their capacity is %d .*nothing added" % (2 * F, F, 3 * F - 1)):
        r.body_rec_residual_stats_add(lab, wt, tr, blank, 64)
    assert r.body_stats_count() == 2 * F and all(np.array_equal(a, b) for a, b in zip(before, r.body_stats_fetch()))
    r.tune("body_stats_cap", 65536)
    assert np.array_equal(r.body_rec_fetch(), regs)
    kf.close()


def test_refusals_name_their_numbers(hm):
    from hydra_mi import _lib
    kf, r, m, regs = _record()
    lab = np.full((2, H, W), -1, np.int32)
    lab[0, 23, 31], lab[1, 23, 31] = 0, 2
    tr = np.full((F, 3), 256 * 10, np.int32)
    want = ref.planes(regs, m, lab, None, tr, None, 64)
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_residual_stats_add: no statistics \(hm_body_stats_begin first\)"):
        r.body_rec_residual_stats_add(lab, None, tr)
    r.body_stats_begin()
    both = (("hm_body_rec_residual_planes", lambda *a, **k: r.body_rec_residual_planes(*a, **k)),
            ("hm_body_rec_residual_stats_add", lambda *a, **k: r.body_rec_residual_stats_add(*a, **k)))
    for who, call in both:
        bad = lab.copy()
        bad[1, 30, 20] = 3                                                  # a label >= L, off the box even
        with pytest.raises(RuntimeError, match=r"code -1.*%s: label 3 at pixel %d of layer 1 outside -1\.\.2" % (who, 30 * W + 20)):
            call(bad, None, tr)
        bad[1, 30, 20] = -2
        with pytest.raises(RuntimeError, match=r"code -1.*%s: label -2 at pixel" % who):
            call(bad, None, tr)
        for nl in (0, 5):
            with pytest.raises(RuntimeError, match=r"code -1.*%s: %d layers outside 1\.\.4" % (who, nl)):
                call(np.full((nl, H, W), -1, np.int32), None, tr)
        for L in (0, 65537):
            with pytest.raises(RuntimeError, match=r"code -1.*%s: %d labels outside 1\.\.65536" % (who, L)):
                call(lab, None, np.zeros((F, L), np.int32))
        for offset in (-1, 256):
            with pytest.raises(RuntimeError, match=r"code -1.*%s: offset %d outside 0\.\.255" % (who, offset)):
                call(lab, None, tr, None, offset)
        with pytest.raises(ValueError, match="traces of shape"):
            call(lab, None, tr[:-1])
    for k0, n in ((F - 1, 2), (-1, 2), (F + 1, 0)):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_residual_planes: frames %d \.\. %d of a record of %d"
                                               % (k0, k0 + n - 1, F)):
            r.body_rec_residual_planes(lab, None, tr, None, 64, k0, n)
    # the argument errors come before the handle is looked at: no handle, no GPU context
    lib = _lib.lib()
    out, cl = np.zeros((1, H, W), np.uint8), ctypes.c_uint64(0)
    P = _lib.ptr
    for args, text in (((0, P(lab), None, 3, P(tr), None, 64), "0 layers outside 1..4"),
                       ((2, P(lab), None, 0, P(tr), None, 64), "0 labels outside 1..65536"),
                       ((2, P(lab), None, 3, P(tr), None, 256), "offset 256 outside 0..255"),
                       ((2, None, None, 3, P(tr), None, 64), "NULL labels or traces"),
                       ((2, P(lab), None, 3, None, None, 64), "NULL labels or traces"),
                       ((2, P(lab), None, 3, P(tr), None, 64), "NULL handle")):
        assert lib.hm_body_rec_residual_planes(None, 0, 1, *args, P(out), ctypes.byref(cl)) == -1
        assert ("hm_body_rec_residual_planes: " + text) in lib.hm_last_error().decode()
        assert lib.hm_body_rec_residual_stats_add(None, *args, ctypes.byref(cl)) == -1
        assert ("hm_body_rec_residual_stats_add: " + text) in lib.hm_last_error().decode()
    # nothing was added, and the handle works as before
    assert r.body_stats_count() == 0
    for v in (0, (1 << 24) + 1):
        with pytest.raises(RuntimeError, match=r"rec_res_frames must be in 1\.\.%d" % (1 << 24)):
            r.tune("rec_res_frames", v)
    got = r.body_rec_residual_planes(lab, None, tr)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    assert r.body_rec_residual_stats_add(lab, None, tr) == want[1] and r.body_stats_count() == F
    assert np.array_equal(r.body_stats_fetch()[0], bs.accumulate(want[0], m)[0])
    assert np.array_equal(r.body_rec_fetch(), regs)
    r.body_rec_begin()                                                      # an empty record
    for who, call in both:
        with pytest.raises(RuntimeError, match="code -3.*%s: no frame recorded" % who):
            call(lab, None, np.zeros((1, 3), np.int32))
    r.body_rec_end()                                                        # before begin
    for who, call in both:
        with pytest.raises(RuntimeError, match=r"code -3.*%s: no record \(hm_body_rec_begin first\)" % who):
            call(lab, None, np.zeros((1, 3), np.int32))
    kf.close()


def test_hidden_partners_through_the_product(hm, tmp_path):
    """demix_ref.paired_scene(0, 6) as the tracker sees it, recorded with BodyReadout(keep=True): body.find_points(12)
    does not contain the twelve cells (a pair's partner lies inside the leader's window); find_points at min_score 0.8
    gives the six leaders and residual.find_more the same twelve points, in the same order, as the restatement, with its
    scores and its demixed traces bit for bit.  write_video's frames are the residual planes."""
    from hydra_mi import body, mesh, residual
    from test_views_cpu import read_avi
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs, act = demix_ref.paired_scene(0, 6, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True, stats=True)
    regs = np.array([b.registered(X, f) for X, f in zip(states, frames)])
    m = b.tri_of_pixel >= 0
    v, cs_v, act_v, s0, sc0, o = ref.paired_more(0, 6)
    assert np.array_equal(regs, np.where(m, v, 0)) and np.array_equal(m, roi_ref.planted_map()) and np.array_equal(cs, cs_v)
    plain = b.find_points(12, radius=6)[0]
    assert plain.shape == (12, 2) and ref.found(np.floor(plain), cs) < 12
    pts, sc = b.find_points(12, radius=6, min_score=0.8)
    assert np.array_equal(np.floor(pts).astype(np.int64), s0) and np.array_equal(_bits(sc), _bits(sc0[:6]))
    more = residual.find_more(b, pts, 0.8, alpha=1.0)
    assert np.array_equal(more["points"], o["seeds"] + 0.5) and ref.matched(np.floor(more["points"]), cs)
    assert np.array_equal(more["points"][:6], pts) and np.array_equal(more["round"], o["round"])
    assert more["ended"] == o["ended"] == "none accepted" and more["accepted"] == o["accepted"] == [6, 0]
    assert more["clipped"] == o["clipped"] and more["dropped"] == o["dropped"] and not more["refused"]
    assert len(more["scores"]) == 2 and all(np.array_equal(_bits(a), _bits(c)) for a, c in zip(more["scores"], o["scores"]))
    assert np.array_equal(_bits(more["new_scores"]), _bits(o["scores"][0]))
    assert np.array_equal(_bits(more["e"]["C"]), _bits(o["e"]["C"])) and np.array_equal(more["e"]["shapes_q"], o["e"]["shapes_q"])
    assert np.array_equal(more["e"]["points"], more["points"])
    # the summary of the last model, and its video
    lab, wt, tr, dropped = ref.model(o["e"], o["seeds"], m.shape)
    got = residual.model(more["e"], m.shape)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], (lab, wt, tr))) and got[3] == dropped
    s = residual.summary(b, more["e"])
    planes, clipped = ref.planes(regs, m, lab, wt, tr, ref.blank_discs(o["seeds"], 2, m.shape), 64)
    exp = bs.images(*bs.accumulate(planes, m), regs.shape[0], m)
    assert s["frames"] == regs.shape[0] and s["clipped"] == clipped and s["dropped"] == dropped
    for key, w in zip(("mean", "std", "corr"), exp[:3]):
        assert np.array_equal(_bits(s[key]), _bits(w)), key
    assert np.array_equal(s["max"], exp[3])
    kf.state.renderer.body_stats_end()
    kf2 = cases.make_filter(dm, frames[0])
    b2 = body.BodyReadout(kf2, keep=True)
    for X, f in zip(states[130:170], frames[130:170]):                     # 40 frames across the move of the mesh
        b2.registered(X, f)
    e40 = {"shapes_q": o["e"]["shapes_q"], "C": o["e"]["C"][130:170]}
    avi = str(tmp_path / "res.avi")
    want = ref.planes(regs[130:170], m, *ref.model(e40, o["seeds"], m.shape)[:3], None, 64)
    assert residual.write_video(b2, avi, e40, points=more["points"], block=17) == (40, want[1])
    vid = read_avi(avi)["frames"]
    assert len(vid) == 40 and all(np.array_equal(vid[k][:, :, c], want[0][k]) for k in range(40) for c in range(3))
    kf2.close()
    kf.close()


def test_cli_find_more_end_to_end(hm, tmp_path):
    """run_kalmanfilter.py --find-points 12 --find-min-score 0.8 --find-more 3 --residual-video on the first frames of
    the paired video, as an animal: a disc of it on black.  The points are those of the restatement on the registered
    video (--registered writes it), first pass and residual rounds; the residual video is the planes of the model the
    run's demix_* arrays describe.  Without the new flags nothing of them is in the output."""
    from test_views_cpu import read_avi
    Fv = 25
    d = demix_ref.paired_video(0, 6)[0][:Fv]
    n = d.shape[1]
    yy, xx = np.mgrid[0:n, 0:n]
    video = d * ((xx - 63.5) ** 2 + (yy - 63.5) ** 2 <= 48.0 ** 2).astype(np.uint8)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "12", "--find-radius", "4"]
    out0, out1 = str(tmp_path / "plain.npz"), str(tmp_path / "more.npz")
    reg, res_avi, csv = str(tmp_path / "reg.avi"), str(tmp_path / "res.avi"), str(tmp_path / "pts.csv")
    res0 = subprocess.run(base + [out0] + find + ["--demix", "--demix-iters", "2"], capture_output=True, text=True, timeout=300,
                          cwd=str(tmp_path))
    assert res0.returncode == 0, res0.stderr[-2000:]
    res = subprocess.run(base + [out1] + find + ["--registered", reg, "--find-min-score", "0.8", "--find-more", "3",
                                                 "--demix-iters", "2", "--residual-video", res_avi, "--points-out", csv],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z0, z = np.load(out0), np.load(out1)
    F1 = z["X"].shape[0]
    assert F1 == Fv - 1 and np.array_equal(z["X"], z0["X"])
    new = {"residual_round", "residual_scores", "residual_scores_round", "residual_clipped"}
    assert set(z.files) - set(z0.files) == new and set(z0.files) <= set(z.files)
    assert "residual" not in res0.stdout.lower()
    regs = np.array([f[:, :, 0] for f in read_avi(reg)["frames"]])
    m = ~np.isnan(z["body_mean"])
    assert regs.shape == (F1, n, n) and m.any()
    s0, sc0 = ref.first_pass(regs, m, 4, 0.8)
    s0, sc0 = s0[:12], sc0[:len(s0)][:12]
    assert 1 <= len(s0)
    o = ref.find_more(regs, m, s0, 0.8, rounds=3, radius=4, iters=2, r_disc=3.0)
    P = len(o["seeds"])
    assert np.array_equal(z["found_points"], o["seeds"] + 0.5) and np.array_equal(z["residual_round"], o["round"])
    assert np.array_equal(_bits(z["found_scores"][:len(s0)]), _bits(sc0)) and z["found_scores"].shape == (P,)
    assert np.array_equal(_bits(z["residual_scores"]), _bits(np.concatenate(o["scores"])))
    assert np.array_equal(z["residual_scores_round"], np.concatenate([np.full(len(s), k + 1) for k, s in enumerate(o["scores"])]))
    assert np.array_equal(z["residual_clipped"], np.array(o["clipped"], np.uint64))
    assert z["points"].shape == (F1, P, 2) and z["demix_C"].shape == (F1, P) and z["demix_shapes"].shape == (P, 17, 17)
    assert "Found %d more points in %d rounds of the residual video" % (P - len(s0), len(o["scores"])) in res.stdout
    with open(csv) as fh:
        assert len([ln for ln in fh if ln.strip()]) == P
    # the video is the planes of the model that the run's own demix_* arrays describe (all the points, demixed once)
    e = {"shapes_q": np.rint(z["demix_shapes"] * 65535.0).astype(np.uint16), "C": z["demix_C"]}
    want = ref.planes(regs, m, *ref.model(e, o["seeds"], m.shape)[:3], None, 64)
    got = read_avi(res_avi)["frames"]
    assert len(got) == F1 and all(np.array_equal(got[k][:, :, c], want[0][k]) for k in range(F1) for c in range(3))
    assert "Residual video: %d frames in %s (%d values clipped)" % (F1, res_avi, want[1]) in res.stdout
    for flags, text in ((["--find-more", "3"], "--find-more looks beside the points found: it needs --find-points and --find-min-score"),
                        (["--find-points", "3", "--find-more", "3"], "it needs --find-points and --find-min-score"),
                        (["--find-min-score", "0.8"], "--find-min-score is the least score of --find-points"),
                        (["--find-points", "3", "--residual-video", "x.avi"], "it needs --demix or --find-more")):
        bad = subprocess.run(base + [out1] + flags, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert bad.returncode == 2 and text in bad.stderr, flags


def _frame_bytes(m):
    """bytes of one frame of the record: the map's bounding box, rows padded to 4 bytes, the frame to 16"""
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    pitch = (int(cols[-1] - cols[0]) + 1 + 3) & ~3
    return (pitch * (int(rows[-1] - rows[0]) + 1) + 15) & ~15


def test_every_scratch_size_gives_the_same_planes_and_statistics(hm):
    """5 frames in chunks of 3, scratch for two frames (runs of 2, 2, 1), for less than one (the floor: one frame at a time)
    and for all of them"""
    kf, r, m, regs = _record(F=5, chunk=3)
    fs = _frame_bytes(m)
    rng = np.random.default_rng(17)
    lab, wt = _layers(_cells(m), 4, 5, rng)
    tr = rng.integers(-450 * 256, 450 * 256, (5, 5)).astype(np.int32)
    blank = np.zeros((H, W), np.uint8)
    blank[22:26, 30:34] = 1
    planes, clipped = ref.planes(regs, m, lab, wt, tr, blank, 64)
    part = ref.planes(regs[1:], m, lab, wt, tr[1:], blank, 64)
    stats = bs.accumulate(planes, m)
    assert clipped > 0
    for scratch in (2 * fs, fs - 1, 16 << 20):
        r.tune("rec_scratch_bytes", scratch)
        p, c = r.body_rec_residual_planes(lab, wt, tr, blank, 64)
        assert np.array_equal(p, planes) and c == clipped, scratch
        p, c = r.body_rec_residual_planes(lab, wt, tr, blank, 64, 1, 4)
        assert np.array_equal(p, part[0]) and c == part[1], scratch
        r.body_stats_begin()
        assert r.body_rec_residual_stats_add(lab, wt, tr, blank, 64) == clipped, scratch
        assert r.body_stats_count() == 5
        for g, w in zip(r.body_stats_fetch(), stats):
            assert np.array_equal(g, w), scratch
    assert np.array_equal(r.body_rec_fetch(), regs)
    kf.close()
