"""Activity waves on the kept registered video (`pytest -m gpu`): every output of hm_body_rec_waves equal to the restatement
in NumPy and Python integers (tests/waves_ref.py) on records with planted pulses (tests/waves_cases.py), whatever the size
of a launch; the refusals; the tracker unchanged by a bit; hydra_mi.waves through the product on a planted plane wave, and
the command end to end.  Every comparison is an equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import border_cases
import detrend_ref
import waves_cases as wc
import waves_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["16", "33x17", "96x160"]
OUTPUTS = ("n_bin", "lat", "rise", "why", "cnt", "sum_lat", "sum_lat2", "fit")
DFF = dict(half=2, q=50, floor=16, gain=16)          # kind 3: the median of five frames; a grey level of excess is a byte


def _rest(dm):
    p = np.asarray(dm.p, np.float32).astype(np.float64)
    return np.concatenate((p.reshape(-1), np.zeros(2 * p.shape[0])))


def _record(name, win, chunk=2):
    """A filter on the scene with the F frames of waves_cases.video recorded as tests/test_detrend_gpu.py::_record records
    its own, the mesh at rest, in chunks of two frames (every window spans chunks) -> (kf, renderer, map, recorded frames)"""
    dm, _, _, f0 = cases.scene(name)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    video = wc.video(m, *win, seed=len(name))
    r.tune("body_rec_chunk", chunk)
    r.body_rec_begin()
    for f in video:
        r.body_warp(_rest(dm), f)
    r.tune("body_rec_chunk", 0)
    regs = r.body_rec_fetch()
    assert regs.shape[0] == wc.F and not regs[:, ~m].any()
    return kf, r, m, regs


def _planes(regs, m, kind):
    return regs if kind == 0 else detrend_ref.planes(regs, m, 3, DFF["half"], DFF["q"], DFF["floor"], DFF["gain"])


def _call(r, trig, kind, b, win, step=5, Rf=1, want=OUTPUTS, min_rise=wc.MIN_RISE):
    kw = DFF if kind else dict(half=0, q=0)
    return r.body_rec_waves(trig, kind, b=b, pre=win[0], lead=win[1], post=win[2], min_rise=min_rise, step=step, Rf=Rf, want=want, **kw)


def _same(got, want, keys=OUTPUTS, note=None):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (key, note)
        assert np.array_equal(got[key], want[key]), (key, note)


@pytest.mark.parametrize("win", wc.WINDOWS, ids=lambda w: "%d-%d-%d" % w)
@pytest.mark.parametrize("name", SCENES)
def test_every_output_equals_the_restatement(hm, name, win):
    kf, r, m, regs = _record(name, win)
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    if name == "33x17":
        assert (int(cols[-1] - cols[0]) + 1) % 4                           # a box no multiple of 4 wide
    if name == "96x160":
        assert not m[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].all()     # a map that is no rectangle
    if name == "16":
        assert 8 > max(cols[-1] - cols[0], rows[-1] - rows[0]) // 2        # b = 8 reaches past the box from its middle
    trig = wc.triggers(*win)
    assert trig[0] - win[1] - win[0] == 0 and trig[1] + win[2] == wc.F - 1 and trig[2] == trig[4] and trig[3] == trig[2] + 1
    assert r.body_rec_wave_nodes(5) == ref.nodes(m, 5)
    for kind in (0, 3):
        planes = _planes(regs, m, kind)
        for b in wc.BINS:
            want = ref.waves(planes, m, trig, b, *win, wc.MIN_RISE, 5, 1)
            codes = set(np.unique(want["why"]).tolist())
            share = float((want["why"] <= 1).sum()) / (len(trig) * m.sum())
            print("%s %r kind %d b %d: codes %s, %.3f of (event, map pixel) valid" % (name, win, kind, b, sorted(codes), share))
            # Code 0 needs a search frame after the first and before the last: (1, 0, 1) has none.  In scene "16" a bin of
            # 17 x 17 holds the planted half from every pixel: none is left without a rise.
            need = {0, 1, 2, 3, 255} - ({0} if win[2] == 1 else set()) - ({2} if name == "16" and b == 8 else set())
            assert need <= codes <= {0, 1, 2, 3, 255} and share >= 0.25
            _same(_call(r, trig, kind, b, win), want, note=(kind, b))
    assert np.array_equal(r.body_rec_fetch(), regs)                        # the record has not changed by a bit
    kf.close()


@pytest.mark.parametrize("name", SCENES)
def test_fit_sums_at_every_step_and_radius(hm, name):
    win = wc.WINDOWS[1]
    kf, r, m, regs = _record(name, win)
    trig = wc.triggers(*win)
    binned = ref.binned(regs, m, 1)
    for step in (1, 5, 64):
        assert r.body_rec_wave_nodes(step) == ref.nodes(m, step)
        for Rf in (1, 16):
            want = ref.waves(regs, m, trig, 1, *win, wc.MIN_RISE, step, Rf, binned_planes=binned)
            if step < 64:                                                   # (at 64 the few nodes may see no valid pixel: a disc's corner)
                assert want["fit"][:, :, 0].max() >= 4 and want["fit"][:, :, 6:].any()
            _same(_call(r, trig, 0, 1, win, step, Rf, want=("fit", "why")), want, ("fit", "why"), (step, Rf))
    kf.close()


def _frame_bytes(m):
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    pitch = (int(cols[-1] - cols[0]) + 1 + 3) & ~3
    return (pitch * (int(rows[-1] - rows[0]) + 1) + 15) & ~15


def test_single_outputs_and_every_launch_size_give_the_same_bytes(hm):
    win = wc.WINDOWS[1]
    kf, r, m, regs = _record("33x17", win)
    trig = wc.triggers(*win)
    for kind in (0, 3):
        want = ref.waves(_planes(regs, m, kind), m, trig, 3, *win, wc.MIN_RISE, 5, 16)
        _same(_call(r, trig, kind, 3, win, 5, 16), want, note=kind)
        for key in OUTPUTS:                                                # each alone, all others NULL
            got = _call(r, trig, kind, 3, win, 5, 16, want=(key,))
            assert list(got) == [key]
            _same(got, want, (key,), kind)
        assert _call(r, trig, kind, 3, win, 5, 16, want=()) == {}
        # (the call stages its planes in a buffer of its own, so the scratch's size reaches no path of it: a guard that it stays so)
        for key, value, back in (("rec_wv_frames", 1, 16), ("rec_wv_frames", 65535, 16), ("rec_wv_frames", 2, 16),
                                 ("rec_scratch_bytes", _frame_bytes(m), 16 << 20)):
            r.tune(key, value)
            _same(_call(r, trig, kind, 3, win, 5, 16), want, note=(kind, key, value))
            r.tune(key, back)
    for v in (0, 65536):
        with pytest.raises(RuntimeError, match=r"rec_wv_frames must be in 1\.\.65535"):
            r.tune("rec_wv_frames", v)
    assert np.array_equal(r.body_rec_fetch(), regs)
    kf.close()


def test_refusals_name_their_numbers(hm):
    win = wc.WINDOWS[1]
    pre, lead, post = win
    kf, r, m, regs = _record("16", win)
    F = wc.F
    trig = wc.triggers(*win)
    want = ref.waves(regs, m, trig, 1, *win, wc.MIN_RISE, 5, 1)
    ok = dict(what=0, half=0, q=0, b=1, pre=pre, lead=lead, post=post, min_rise=wc.MIN_RISE, step=5, Rf=1)
    early, late = int(trig[0]) - 1, int(trig[1]) + 1
    refusals = (
        (dict(triggers=np.zeros(0, np.int32)), r"0 events outside 1\.\.65536"),
        (dict(triggers=[trig[2], early]), r"event 1: trigger %d needs the frames -1 \.\. %d \(pre %d, lead %d, post %d\) of a record of F = %d"
         % (early, early + post, pre, lead, post, F)),
        (dict(triggers=[late]), r"event 0: trigger %d needs the frames %d \.\. %d \(pre %d, lead %d, post %d\) of a record of F = %d"
         % (late, late - lead - pre, F, pre, lead, post, F)),
        (dict(b=9), r"bin radius 9 outside 0\.\.8"), (dict(b=-1), r"bin radius -1 outside 0\.\.8"),
        (dict(pre=0), r"pre 0 outside 1\.\.64"), (dict(pre=65), r"pre 65 outside 1\.\.64"),
        (dict(lead=-1), r"lead -1 outside 0\.\.64"), (dict(lead=65), r"lead 65 outside 0\.\.64"),
        (dict(post=0), r"post 0 outside 1\.\.256"), (dict(post=257), r"post 257 outside 1\.\.256"),
        (dict(min_rise=0), r"min_rise 0 outside 1\.\.255"), (dict(min_rise=256), r"min_rise 256 outside 1\.\.255"),
        (dict(step=0), r"node step 0 outside 1\.\.64"), (dict(step=65), r"node step 65 outside 1\.\.64"),
        (dict(Rf=0), r"fit radius 0 outside 1\.\.16"), (dict(Rf=17), r"fit radius 17 outside 1\.\.16"),
        (dict(what=4), r"kind of plane 4 outside 0\.\.3"), (dict(what=3, half=1025), r"half 1025 outside 0\.\.1024"),
    )
    for change, text in refusals:
        kw = dict(ok, triggers=trig)
        kw.update(change)
        if "step" in change:
            kw["want"] = ("lat", "why")                                    # (with `fit` the wrapper asks hm_body_rec_wave_nodes first)
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_waves: " + text):
            r.body_rec_waves(**kw)
        assert np.array_equal(r.body_rec_fetch(), regs)                    # a refusal leaves the record usable
        _same(r.body_rec_waves(trig, **ok), want, note=text)
    for step in (0, 65):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_wave_nodes: node step %d outside 1\.\.64" % step):
            r.body_rec_wave_nodes(step)
    r.body_rec_begin()                                                      # an empty record
    with pytest.raises(RuntimeError, match="code -3.*hm_body_rec_waves: no frame recorded"):
        r.body_rec_waves(trig, **ok)
    assert r.body_rec_wave_nodes(5) == ref.nodes(m, 5)                      # (the box is known from the begin)
    r.body_rec_end()                                                        # before begin
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_waves: no record \(hm_body_rec_begin first\)"):
        r.body_rec_waves(trig, want=("lat", "why"), **ok)                   # (with `fit` the wrapper asks hm_body_rec_wave_nodes first)
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_wave_nodes: no record \(hm_body_rec_begin first\)"):
        r.body_rec_wave_nodes(5)
    kf.close()


def test_a_map_without_a_pixel(hm):
    """tests/border_cases.py `empty`: the mesh covers no pixel centre; the record's box is one pixel off the map"""
    dm, Xs, frames, f0 = border_cases.scene("empty")
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    assert not m.any()
    r.body_rec_begin()
    for X, f in border_cases.record_pairs("empty", 7):
        r.body_warp(X, f)
    regs = r.body_rec_fetch()
    trig = np.array([2, 4], np.int32)
    for kind in (0, 3):
        got = _call(r, trig, kind, 2, (2, 0, 2), 3, 2)
        _same(got, ref.waves(_planes(regs, m, kind), m, trig, 2, 2, 0, 2, wc.MIN_RISE, 3, 2), note=kind)
        assert (got["why"] == 255).all() and (got["lat"] == ref.NONE).all()
        assert not any(got[k].any() for k in ("n_bin", "rise", "cnt", "sum_lat", "sum_lat2", "fit"))
    kf.close()


def test_waves_between_frames_change_nothing_of_the_filter(hm):
    """Config 1 (128^2, the golden track) with the record kept and its waves read between every two frames: states,
    covariance and error terms bit-identical to the run without."""
    from hydra_mi import body, kalman, mesh, synth, waves
    g = np.load(os.path.join(cases.GOLD, "config1_track.npz"))
    video, flow = synth.test_data(128, 128)
    runs = {}
    for on in (False, True):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), video[:, :, 0], flow[:, :, :, 0], True)
        b = body.BodyReadout(kf, keep=True) if on else None
        out = []
        for k in range(8):
            frame = video[:, :, k]
            e = kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
            if on:
                b.registered(kf.state.X, frame)
                if k >= 3:
                    for what in ("recorded", "dff"):
                        w = waves.latency(b, [1, k - 1], what=what, half=2, q=50, b=1, pre=1, lead=0, post=1, min_rise=1, keep=True)
                        assert w["lat"].shape[0] == 2 and w["fit"].shape[0] == 2
            out.append((kf.state.X.copy(), kf.niter, e[:4], np.array(kf.state.W, np.float64).copy()))
        runs[on] = out
        kf.close()
    for (Xa, ia, ea, Wa), (Xb, ib, eb, Wb) in zip(runs[False], runs[True]):
        assert np.array_equal(Xa, Xb) and ia == ib and ea == eb and np.array_equal(Wa, Wb)


def test_a_planted_plane_wave_through_the_product(hm):
    """Scene "96x160" at rest with a ramp 0, 48, .., 192 that comes a quarter of a frame later per column, recorded with
    BodyReadout(keep=True): waves.latency and waves.velocity equal the restatement exactly, the latency is the planted
    one, and where a node's whole window is valid the gradient is (1/4, 0) frames per pixel and the velocity (4, 0)."""
    from hydra_mi import body, waves
    dm, _, _, f0 = cases.scene("96x160")
    kf = cases.make_filter(dm, f0)
    b = body.BodyReadout(kf, keep=True)
    m = b.tri_of_pixel >= 0
    c0 = int(np.flatnonzero(m.any(0))[0])
    t, F = 8, 40
    k, x = np.arange(F)[:, None, None], np.arange(160)[None, None, :]
    video = np.broadcast_to(np.clip(48 * (k - t) - 12 * (x - c0), 0, 192), (F, 96, 160)).astype(np.uint8)
    regs = np.array([b.registered(_rest(dm), f) for f in video])
    assert np.array_equal(regs, video * m[None])
    par = dict(b=0, pre=4, lead=2, post=28, min_rise=8, step=8, Rf=6)
    trig = np.array([t, t], np.int32)
    got = waves.latency(b, trig, what="recorded", keep=True, **par)
    want = ref.waves(regs, m, trig, 0, 4, 2, 28, 8, 8, 6)
    for key in ("n_bin", "lat", "rise", "why", "cnt", "fit"):
        assert np.array_equal(got[key], want[key]), key
    mean, sd = waves.mean_sd(want["cnt"], want["sum_lat"], want["sum_lat2"])
    assert np.array_equal(got["lat_mean"], mean, equal_nan=True) and np.array_equal(got["lat_sd"], sd, equal_nan=True)
    assert (got["why"][0][m] == 0).all() and (got["cnt"][m] == 2).all() and not got["lat_sd"][m].any()
    assert np.array_equal(got["lat"][0][m], np.broadcast_to(512 + 64 * (x[0] - c0), (96, 160))[m])
    assert np.array_equal(got["lat_mean"][m], np.broadcast_to(2 + (x[0] - c0) / 4, (96, 160))[m].astype(np.float32))
    nx, ny, nc0, nr0 = ref.nodes(m, 8)
    assert got["nodes_shape"] == (ny, nx) and got["nodes"][0].tolist() == [nc0, nr0] and got["nodes"][nx + 1].tolist() == [nc0 + 8, nr0 + 8]
    g, v = waves.velocity(got["fit"], 20)
    gr, vr = ref.velocity(want["fit"], 20)
    assert np.array_equal(g, gr, equal_nan=True) and np.array_equal(v, vr, equal_nan=True)
    whole = got["fit"][0, :, 0] == 13 * 13
    assert whole.sum() >= 20 and (g[0][whole] == (0.25, 0.0)).all() and (v[0][whole] == (4.0, 0.0)).all()
    part = np.isfinite(v[0][:, 0])
    assert (v[0][part][:, 0] > 0).all() and (np.abs(v[0][part][:, 1]) < v[0][part][:, 0]).all()      # rightwards everywhere
    o = waves.origin(got["lat_mean"], got["cnt"], 2)
    assert o[0] == c0 and m[o[1], o[0]] and o[1] == int(np.flatnonzero(m[:, c0])[0])
    gm, vm = waves.mean_velocity(got["lat_mean"], got["cnt"], got["nodes"], 6, 2, n_min=169)
    assert (gm[whole] == (0.25, 0.0)).all() and (vm[whole] == (4.0, 0.0)).all()
    e = waves.extract(b, trig=[trig, np.zeros(0, np.int32)], what="recorded", n_min=20, **par)
    assert e["lat_mean"].shape == (2, 96, 160) and np.array_equal(e["lat_mean"][0], got["lat_mean"], equal_nan=True)
    assert np.isnan(e["lat_mean"][1]).all() and e["origin"].tolist() == [[o[0], o[1]], [-1, -1]]
    assert e["speed"][0] == 4.0 and np.isnan(e["speed"][1]) and e["valid"][0] == 1.0 and e["trigger_ens"].tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="without keep=True"):
        waves.latency(body.BodyReadout(kf), trig)
    kf.close()


def test_cli_waves_end_to_end(hm, tmp_path):
    """run_kalmanfilter.py --find-points .. --rois --network --waves --waves-map on the moving disk with two flashes of the
    whole animal: the wave_* arrays are there in their shapes and the PNG is written; the same command without --waves
    writes no wave_ key."""
    from hydra_mi import synth, videoio
    n, F = 96, 16
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    video = np.array(video)
    for k in (6, 11):                                                      # a flash a frame long: an event of every cell
        video[k] = np.minimum(video[k].astype(np.int64) * 3 // 2, 255).astype(video.dtype)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    opts = ["-s", "14", "--find-points", "12", "--find-radius", "4", "--find-score", "std", "--rois", "--network", "--network-thr", "-1"]
    wv = ["--waves", "--waves-map", str(tmp_path / "w.png"), "--waves-pre", "2", "--waves-lead", "1", "--waves-post", "3", "--waves-step", "4",
          "--waves-fit", "3", "--waves-keep", "--detrend-half", "3", "--dff-gain", "2000"]
    out0, out1 = str(tmp_path / "plain.npz"), str(tmp_path / "waves.npz")
    res0 = subprocess.run(base + [out0] + opts, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res0.returncode == 0, res0.stderr[-2000:]
    res = subprocess.run(base + [out1] + opts + wv, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z0, z = np.load(out0), np.load(out1)
    assert not [k for k in z0.files if k.startswith("wave_")] and "Waves" not in res0.stdout and "Wave map" not in res0.stdout
    new = set(z.files) - set(z0.files)
    assert new == {"wave_triggers", "wave_trigger_ens", "wave_lat_mean", "wave_lat_sd", "wave_count", "wave_nodes", "wave_velocity",
                   "wave_speed", "wave_origin", "wave_params", "wave_lat", "wave_rise", "wave_why", "wave_fit"}
    assert set(z0.files) <= set(z.files)
    for key in ("X", "roi_dff", "net_r", "net_labels", "net_ens_traces", "net_map"):         # what there was: as before
        assert np.array_equal(z[key], z0[key], equal_nan=True), key
    K, E = z["net_ens_traces"].shape[0], z["wave_triggers"].shape[0]
    N = z["wave_nodes"].shape[0]
    print("CLI: %d ensembles, %d triggers %s" % (K, E, z["wave_triggers"].tolist()))
    assert z["wave_triggers"].dtype == np.int32 and z["wave_trigger_ens"].shape == (E,)
    assert z["wave_lat_mean"].shape == (K, n, n) and z["wave_lat_mean"].dtype == np.float32 and z["wave_lat_sd"].shape == (K, n, n)
    assert z["wave_count"].shape == (K, n, n) and z["wave_count"].dtype == np.uint32
    assert z["wave_nodes"].shape == (N, 2) and z["wave_velocity"].shape == (K, N, 2) and z["wave_speed"].shape == (K,)
    assert z["wave_origin"].shape == (K, 2) and z["wave_params"].tolist() == [2, 1, 3, 2, 8, 4, 3, 3, 10, 16, 2000]
    assert z["wave_lat"].shape == (E, n, n) and z["wave_rise"].shape == (E, n, n) and z["wave_why"].shape == (E, n, n)
    assert z["wave_fit"].shape == (E, N, 9) and z["wave_fit"].dtype == np.int64
    off = np.isnan(z["body_mean"])
    assert (z["wave_why"][:, off] == 255).all() and not z["wave_count"][:, off].any() and np.isnan(z["wave_lat_mean"][:, off]).all()
    assert np.array_equal(z["wave_count"], np.array([(z["wave_why"][z["wave_trigger_ens"] == k] <= 1).sum(0) for k in range(K)],
                                                    np.uint32).reshape(K, n, n))
    img = videoio.read_png(str(tmp_path / "w.png"))
    assert img.shape == (n, n, 3) and img.dtype == np.uint8
    assert res.stdout.count("Waves: ensemble ") == K and "Wave map: " in res.stdout
    bad = subprocess.run(base + [out1, "--waves", "--waves-frames", "t.txt"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert bad.returncode == 2 and "--waves works on the kept record" in bad.stderr
