"""Events per pixel of the kept registered video (`pytest -m gpu`): hm_body_rec_event_planes, _event_sums and the
statistics after _event_stats_add equal to the restatement in Python floats (tests/events_ref.py) bit for bit, on a
48 x 40 video whose box frame ends inside a 64-byte segment; every pass size and scratch size gives the same bytes; the
refusals name their numbers; hydra_mi.events.deconvolve on a pixel's bytes equals the device; and the CLI end to end.
Every comparison is an equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import bodystats_ref as bs
import detrend_ref
import events_ref as ref
import roi_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 40, 48
MESH = (5.0, 4.0, 42.0, 35.0, 8.0)          # mesh.box_mesh: a box of 37 x 31 pixels, rows of 40 bytes, 1240 bytes a frame
DET = dict(half=3, q=20, floor=16, gain=255)
G, LAM, SMIN = 0.9, 2.5, 4.0


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def rig(hm):
    """One filter for the module -> (renderer, map, state of the mesh at rest, box, segments of a box frame)"""
    from hydra_mi import mesh
    dm = mesh.box_mesh(*MESH)
    kf = cases.make_filter(dm, np.random.default_rng(0).integers(0, 256, (H, W), dtype=np.uint8))
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    p = np.asarray(dm.p, np.float32).astype(np.float64)
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * p.shape[0])))
    box = ref.box_of(m)
    pitch = (box[3] - box[2] + 3) & ~3
    nbytes = pitch * (box[1] - box[0])
    assert nbytes % 256 and nbytes % 64                                    # the last segment is partial
    yield r, m, rest, box, -(-nbytes // 64)
    kf.close()


def _load(rig, frames):
    """A record of these frames with the mesh at rest -> the recorded frames: the frames on the map"""
    r, m, rest = rig[:3]
    r.body_rec_begin()
    for f in frames:
        r.body_warp(rest, np.ascontiguousarray(f, np.uint8))
    regs = r.body_rec_fetch()
    assert np.array_equal(regs, np.where(m[None], np.asarray(frames, np.uint8), 0))
    return regs


def _records():
    rng = np.random.default_rng(19)
    pix = np.arange(H * W).reshape(H, W)
    k37 = np.arange(37)[:, None, None]
    impulse = np.zeros((37, H, W), np.uint8)
    impulse[0] = 255
    v = roi_ref.planted_video(0)[0][:48, 30:30 + H, 40:40 + W]             # the planted video: a cut with cells in it
    return {
        "F1": rng.integers(0, 256, (1, H, W)), "F2": rng.integers(0, 256, (2, H, W)), "F37": rng.integers(0, 256, (37, H, W)),
        "zero": np.zeros((9, H, W), np.uint8),
        "constant": np.full((37, H, W), 100, np.uint8),                    # (no fall: s = 100 (1 - g) > 0, F pools, no merge)
        "impulse": impulse,                                                 # one pool of length F: the longest merge chain
        "ramp": 6 * k37 + (pix % 30)[None],                                # strictly increasing: F pools, no merge
        "sawtooth": np.array([10, 120, 240])[np.arange(37) % 3][:, None, None] + (pix % 7)[None],
        "planted": v,
    }


RECORDS = _records()


def _check_all(rig, regs, what, g, lam, s_min, tag, stats=True):
    """planes, sums and (if asked) the statistics of the device against the restatement on the planes of kind `what`"""
    r, m, _, box, _ = rig
    y = detrend_ref.planes(regs, m, what, **DET)
    E, n, S = ref.video(y, box, g, lam, s_min)
    got = r.body_rec_event_planes(what, g=g, lam=lam, **DET)
    assert got.dtype == np.uint8 and np.array_equal(got, E), tag
    cnt, tot = r.body_rec_event_sums(what, g=g, lam=lam, s_min=s_min, **DET)
    assert cnt.dtype == np.uint32 and np.array_equal(cnt, n), tag
    assert np.array_equal(_bits(tot), _bits(S)), tag
    if stats:
        F = regs.shape[0]
        r.body_stats_begin()
        r.body_rec_event_stats_add(what, g=g, lam=lam, **DET)
        assert r.body_stats_count() == F
        want = bs.accumulate(E, m)
        for a, b in zip(r.body_stats_fetch(), want):
            assert np.array_equal(a, b), tag
        imgs, exp = r.body_stats_images(), bs.images(*want, F, m)
        for a, b in zip(imgs[:3], exp[:3]):
            assert np.array_equal(_bits(a), _bits(b)), tag
        r.body_stats_end()
    return E, n, S


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_planes_sums_and_statistics_equal_the_restatement(rig, name):
    """Every record, raw (kind 0), with a penalty and without.  The constant record is in the list as a case of its own;
    under the rule it never merges (c constant is feasible: s = y (1 - g)), so the impulse record is the one whose pixels
    end as one pool of length F."""
    regs = _load(rig, RECORDS[name])
    F = regs.shape[0]
    for lam in (LAM, 0.0):
        E, n, S = _check_all(rig, regs, 0, G, lam, SMIN, (name, lam))
        if name == "zero":
            assert not E.any() and not n.any() and not S.any()
        if name in ("constant", "ramp") and lam == 0.0 and F > 1:          # F pools: an event in every frame but the first
            assert (n[rig[1]] == F - 1).all()
        if name == "impulse":                                               # one pool: no event anywhere
            assert not E.any() and not S.any()
    if name in ("F37", "planted"):
        assert E.any()
    assert np.array_equal(rig[0].body_rec_fetch(), regs)                    # the record has not changed by a bit


def test_kinds_of_plane_and_a_large_penalty(rig):
    regs = _load(rig, RECORDS["planted"])
    some = False
    for what in (0, 2, 3):
        E, n, S = _check_all(rig, regs, what, G, LAM, SMIN, what)
        some = some or bool(E.any())
        E, n, S = _check_all(rig, regs, what, 0.5, 1e4, SMIN, (what, "large"), stats=False)
        assert not E.any() and not n.any() and not S.any()                  # a large penalty: everything zero
    assert some
    E0 = _check_all(rig, regs, 3, G, 0.0, 1.0, "lam 0", stats=False)[0]
    assert E0.any()


def test_every_pass_size_and_scratch_size_gives_the_same_bytes(rig):
    """rec_ev_bytes for one pass, three passes (7, 7, 6 of the 20 segments) and a pass per segment (also below one
    segment's worth: the floor); rec_scratch_bytes for batches of two frames of the detrended source; a window in the
    middle of the record."""
    r, m, _, box, segs = rig
    regs = _load(rig, RECORDS["planted"])
    F = regs.shape[0]
    assert segs == 20
    seg_bytes = 20 * 64 * F
    fs = (((box[3] - box[2] + 3) & ~3) * (box[1] - box[0]) + 15) & ~15    # bytes of a box frame in the record
    want = {what: ref.video(detrend_ref.planes(regs, m, what, **DET), box, G, LAM, SMIN) for what in (0, 3)}
    assert want[3][0].any()
    try:
        for ev_bytes in (1 << 34, 7 * seg_bytes, seg_bytes, 1):
            for scratch in (16 << 20, 2 * fs):
                r.tune("rec_ev_bytes", ev_bytes)
                r.tune("rec_scratch_bytes", scratch)
                for what in (0, 3):
                    E, n, S = want[what]
                    tag = (ev_bytes, scratch, what)
                    assert np.array_equal(r.body_rec_event_planes(what, g=G, lam=LAM, **DET), E), tag
                    assert np.array_equal(r.body_rec_event_planes(what, g=G, lam=LAM, k0=5, n=9, **DET), E[5:14]), tag
                    cnt, tot = r.body_rec_event_sums(what, g=G, lam=LAM, s_min=SMIN, **DET)
                    assert np.array_equal(cnt, n) and np.array_equal(_bits(tot), _bits(S)), tag
                r.body_stats_begin()
                r.body_rec_event_stats_add(3, g=G, lam=LAM, **DET)
                for a, b in zip(r.body_stats_fetch(), bs.accumulate(want[3][0], m)):
                    assert np.array_equal(a, b), (ev_bytes, scratch)
                r.body_stats_end()
        assert r.body_rec_event_planes(3, g=G, lam=LAM, k0=F, n=0, **DET).shape[0] == 0
    finally:
        r.tune("rec_ev_bytes", 1 << 34)
        r.tune("rec_scratch_bytes", 16 << 20)
    for v in (0, (1 << 34) + 1, -1):
        with pytest.raises(RuntimeError, match=r"code -1.*rec_ev_bytes must be in 1\.\.%d" % (1 << 34)):
            r.tune("rec_ev_bytes", v)


def test_the_host_rule_equals_the_device_on_a_pixels_bytes(rig):
    """events.deconvolve on a trace of integers 0..255 is the device's per-pixel result: the sum of its s, added in
    ascending order, and the bytes of its s, bit for bit"""
    from hydra_mi import events
    r, m, _, box, _ = rig
    regs = _load(rig, RECORDS["F37"])
    E = r.body_rec_event_planes(0, g=G, lam=LAM, **DET)
    cnt, tot = r.body_rec_event_sums(0, g=G, lam=LAM, s_min=SMIN, **DET)
    rows, cols = np.nonzero(m)
    for i in range(0, len(rows), 37):
        rr, cc = rows[i], cols[i]
        s = events.deconvolve(regs[:, rr, cc], G, LAM)[1]
        S = np.float64(0.0)
        for x in s:
            S = S + x
        assert _bits(S) == _bits(tot[rr, cc]) and int(events.binarise(s, SMIN).sum()) == cnt[rr, cc]
        assert np.array_equal(np.minimum(255, np.floor(s + 0.5)).astype(np.uint8), E[:, rr, cc])


def test_refusals_name_their_numbers_and_the_handle_goes_on(rig):
    r, m, _, box, _ = rig
    regs = _load(rig, RECORDS["F37"][:6])
    F = regs.shape[0]
    ok = dict(what=3, g=G, lam=LAM, **DET)
    calls = (("hm_body_rec_event_planes", lambda **a: r.body_rec_event_planes(**a)),
             ("hm_body_rec_event_stats_add", lambda **a: r.body_rec_event_stats_add(**a)),
             ("hm_body_rec_event_sums", lambda **a: r.body_rec_event_sums(s_min=SMIN, **a)))
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_event_stats_add: no statistics \(hm_body_stats_begin first\)"):
        r.body_rec_event_stats_add(**ok)
    r.body_stats_begin()
    limits = (("what", (-1, 4), r"kind of plane %d outside 0\.\.3"), ("half", (-1, 1025), r"half %d outside 0\.\.1024"),
              ("q", (-1, 101), r"q %d outside 0\.\.100"), ("floor", (0, 256), r"floor %d outside 1\.\.255"),
              ("gain", (0, 65536), r"gain %d outside 1\.\.65535"),
              ("g", (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")), r"g %g outside 0 < g < 1"),
              ("lam", (-0.5, float("nan"), float("inf")), r"lam %g negative or not finite"))
    for key, values, text in limits:
        for v in values:
            for who, call in calls:
                with pytest.raises(RuntimeError, match=r"code -1.*" + who + ": " + (text % v).replace("+", r"\+")):
                    call(**dict(ok, **{key: v}))
    for v in (-1.0, float("nan"), float("-inf")):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_event_sums: s_min %g negative or not finite" % v):
            r.body_rec_event_sums(s_min=v, **ok)
    for k0, n in ((F - 1, 2), (-1, 2), (F + 1, 0)):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_event_planes: frames %d \.\. %d of a record of %d" % (k0, k0 + n - 1, F)):
            r.body_rec_event_planes(k0=k0, n=n, **ok)
    assert r.body_stats_count() == 0
    r.tune("body_stats_cap", 2 * F - 1)                                    # the second addition would pass the capacity
    r.body_rec_event_stats_add(**ok)
    before = r.body_stats_fetch()
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_event_stats_add: the statistics hold %d frames and the record %d, their "
                                           r"capacity is %d .*nothing added" % (F, F, 2 * F - 1)):
        r.body_rec_event_stats_add(**ok)
    assert r.body_stats_count() == F and all(np.array_equal(a, b) for a, b in zip(before, r.body_stats_fetch()))
    r.tune("body_stats_cap", 65536)
    r.body_stats_end()
    # after every error the handle still works, and the record has not changed
    y = detrend_ref.planes(regs, m, 3, **DET)
    assert np.array_equal(r.body_rec_event_planes(**ok), ref.video(y, box, G, LAM, SMIN)[0])
    assert np.array_equal(r.body_rec_fetch(), regs)
    r.body_rec_begin()                                                      # an empty record
    for who, call in calls:
        with pytest.raises(RuntimeError, match="code -3.*" + who + ": no frame recorded"):
            call(**ok)
    r.body_rec_end()                                                        # before begin
    for who, call in calls:
        with pytest.raises(RuntimeError, match=r"code -3.*" + who + r".*hm_body_rec_begin first"):
            call(**ok)


def test_a_record_of_more_than_65535_frames_is_refused(hm):
    """The stack keeps frame numbers in 16 bits: frame 65536 of a 16 x 16 record turns the calls away, with the numbers"""
    dm, _, _, f0 = cases.scene("16")
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    p = np.asarray(dm.p, np.float32).astype(np.float64)
    rest = np.concatenate((p.reshape(-1), np.zeros(2 * p.shape[0])))
    r.body_rec_begin()
    for _ in range(65536):
        r.body_warp(rest, f0)
    text = r"code -1.*%s: a record of 65536 frames \(the pool stack holds frame numbers in 16 bits: 65535 frames at most\)"
    with pytest.raises(RuntimeError, match=text % "hm_body_rec_event_planes"):
        r.body_rec_event_planes(0, 0, 0, g=G, lam=LAM, k0=0, n=1)
    with pytest.raises(RuntimeError, match=text % "hm_body_rec_event_sums"):
        r.body_rec_event_sums(0, 0, 0, g=G, lam=LAM, s_min=SMIN)
    assert r.body_rec_count() == 65536
    kf.close()


def test_cli_events_end_to_end(hm, tmp_path):
    """run_kalmanfilter.py --rois --network --events --events-video on the first frames of the planted video, as an
    animal: a disc of it on black.  The ev_* arrays are hydra_mi.events on the run's own traces, the images and the AVI
    the restatement on the dF/F bytes of the registered video (--registered writes it); and the run without the new flags
    writes what it wrote before: no array of it changes by a bit, and nothing new is in it."""
    from hydra_mi import events, network
    from test_views_cpu import read_avi
    Fv = 14
    d = roi_ref.planted_video(0)[0][:Fv]
    n = d.shape[1]
    yy, xx = np.mgrid[0:n, 0:n]
    video = d * ((xx - 63.5) ** 2 + (yy - 63.5) ** 2 <= 48.0 ** 2).astype(np.uint8)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    out0, out1 = str(tmp_path / "plain.npz"), str(tmp_path / "ev.npz")
    reg, avi = str(tmp_path / "reg.avi"), str(tmp_path / "ev.avi")
    opts = ["-s", "14", "--find-points", "12", "--find-radius", "4", "--rois", "--network", "--network-lag", "2",
            "--detrend-half", "3", "--detrend-q", "20", "--dff-floor", "12", "--dff-gain", "300"]
    res0 = subprocess.run(base + [out0] + opts, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res0.returncode == 0, res0.stderr[-2000:]
    res = subprocess.run(base + [out1] + opts + ["--registered", reg, "--events", "--events-video", avi],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z0, z = np.load(out0), np.load(out1)
    new = {"ev_g", "ev_lambda", "ev_c", "ev_s", "ev_binary", "ev_count_image", "ev_sum_image", "ev_params", "net_r_events"}
    assert set(z.files) - set(z0.files) == new and set(z0.files) <= set(z.files)
    for key in z0.files:                                                    # no existing array changes by a bit
        a, b = z0[key], z[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    assert "Events" not in res0.stdout and "Events: " in res.stdout
    F1 = z["X"].shape[0]
    tr = np.ascontiguousarray(z["roi_dff"].T)
    K = tr.shape[0]
    assert F1 == Fv - 1 and K >= 1 and z["ev_c"].shape == (K, F1) and z["ev_binary"].dtype == np.bool_
    g = np.array([events.estimate_g(x) for x in tr])
    sig = np.array([events.noise(x) for x in tr])
    lam = np.array([events.default_lam(a, b) for a, b in zip(g, sig)])
    c, s = events.deconvolve(tr, g, lam)
    for key, w in (("ev_g", g), ("ev_lambda", lam), ("ev_c", c), ("ev_s", s)):
        assert np.array_equal(_bits(z[key]), _bits(w)), key
    assert np.array_equal(z["ev_binary"], events.binarise(s, [events.default_smin(b) for b in sig]))
    assert np.array_equal(_bits(z["net_r_events"]), _bits(network.coactivity(s, 2)))
    g_px, lam_px, smin_px = z["ev_params"][:3]
    assert list(z["ev_params"][3:]) == [3, 20, 12, 300]
    assert g_px == np.median(g) and lam_px == np.median(lam) * 300 and smin_px == max(1.0, np.median([events.default_smin(b) for b in sig]) * 300)
    regs = np.array([f[:, :, 0] for f in read_avi(reg)["frames"]])
    m = ~np.isnan(z["body_mean"])
    E, cnt, S = ref.video(detrend_ref.planes(regs, m, 3, 3, 20, 12, 300), ref.box_of(m), float(g_px), float(lam_px), float(smin_px))
    assert z["ev_count_image"].dtype == np.uint32 and np.array_equal(z["ev_count_image"], cnt)
    assert z["ev_sum_image"].dtype == np.float32 and np.array_equal(z["ev_sum_image"], S.astype(np.float32))
    got = read_avi(avi)["frames"]
    assert len(got) == F1 and "Event video: %d frames in %s" % (F1, avi) in res.stdout
    for k in range(F1):
        assert all(np.array_equal(got[k][:, :, ch], E[k]) for ch in range(3)), k
    bad = subprocess.run(base + [out1, "--find-points", "3", "--events"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert bad.returncode == 2 and "--events reads the cells' traces: it needs --rois or --demix" in bad.stderr


def test_events_through_the_product(hm, tmp_path):
    """The first 30 frames of the planted scene recorded with BodyReadout(keep=True): hydra_mi.events' stats_add,
    find_points, count_image and event_video are the restatement's planes summed, searched, counted and written."""
    from hydra_mi import body, events, mesh
    from test_views_cpu import read_avi
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states = roi_ref.planted_scene(0, dm.p)[:2]
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True)
    regs = np.array([b.registered(X, f) for X, f in zip(states[:30], frames[:30])])
    m = b.tri_of_pixel >= 0
    F, Hh, Ww = regs.shape
    px = dict(what="dff", half=3, q=20, floor=16, gain=255)
    E, n, S = ref.video(detrend_ref.planes(regs, m, 3, 3, 20, 16, 255), ref.box_of(m), 0.8, 6.0, 5.0)
    assert E.any()
    assert events.stats_add(b, 0.8, 6.0, **px) == F
    want = bs.accumulate(E, m)
    for a, w in zip(b.r.body_stats_fetch(), want):
        assert np.array_equal(a, w)
    pts, sc = events.find_points(b, 12, 0.8, 6.0, radius=6, score="std", **px)
    exp = bs.images(*want, F, m)
    widx, wsc = bs.peaks_fast(exp[1], m, 6)
    P = min(12, len(widx))
    assert P >= 1 and np.array_equal(_bits(sc), _bits(wsc[:P]))
    assert np.array_equal((pts[:, 1] - 0.5) * Ww + (pts[:, 0] - 0.5), widx[:P].astype(np.float64))
    b.r.body_stats_end()
    cnt, tot = events.count_image(b, 0.8, 6.0, 5.0, **px)
    assert np.array_equal(cnt, n) and np.array_equal(_bits(tot), _bits(S))
    avi = str(tmp_path / "ev.avi")
    assert events.event_video(b, avi, 0.8, 6.0, block=7, **px) == F        # blocks of 7, 7, 7, 7, 2 frames
    got = read_avi(avi)["frames"]
    for k in range(F):
        assert all(np.array_equal(got[k][:, :, ch], E[k]) for ch in range(3)), k
    with pytest.raises(ValueError, match="g 1.0 outside 0 < g < 1"):
        events.count_image(b, 1.0, 6.0, 5.0, **px)
    kf.close()
