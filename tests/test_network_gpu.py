"""The trace maps on the device (`pytest -m gpu`): hm_body_rec_trace_maps equal to the NumPy restatement
(tests/network_ref.py) as exact integers for every number of traces and every run length, to hm_body_rec_trace_products
and hm_body_rec_fetch where they overlap, its refusals, hydra_mi.network through the product on the planted video with
ensembles, and the CLI end to end.  Every comparison is an equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import demix_ref
import network_ref as ref
import roi_ref
from test_network_cpu import BETWEEN, ROI_THR, THR, WITHIN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, F = 48, 64, 7


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _record(F=F, chunk=2):
    """A 64 x 48 frame with a disc of a mesh (a box 41 px wide: the last dword of a row and the last segment of a frame are
    partial; pixels of the box off the map), F random frames with 0 and 255 among their values recorded at perturbed
    states in chunks of `chunk` frames -> (kf, renderer, map, recorded frames)"""
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
    assert (regs[:, m] == 0).any() and (regs[:, m] == 255).any()
    return kf, r, m, regs


def _traces(rng, L, F=F):
    """(F, L) int32 with +-32767, zeros and negative values among them; of several traces, trace 0 is 32767 and the last
    -32767 throughout"""
    if L == 1:
        return np.array([32767, -32767, 0, -5, 12345, -32767, 1][:F], np.int32).reshape(-1, 1)
    q = rng.integers(-32767, 32768, (F, L)).astype(np.int32)
    q[rng.random((F, L)) < 0.15] = 0
    q[rng.random((F, L)) < 0.15] = 32767
    q[rng.random((F, L)) < 0.15] = -32767
    q[:, 0] = 32767
    q[:, -1] = -32767
    q[:4, 1] = (0, -5, 32767, -32767)
    assert (q == 0).any() and (q == 32767).any() and (q == -32767).any() and ((q < 0) & (q > -32767)).any()
    return np.ascontiguousarray(q)


def _same(got, want):
    c, w1, w2 = want
    assert got["c"].dtype == np.int64 and got["w1"].dtype == np.uint64 and got["w2"].dtype == np.uint64
    return np.array_equal(got["c"], c) and np.array_equal(got["w1"], w1) and np.array_equal(got["w2"], w2)


def test_trace_maps_equal_the_restatement(hm):
    kf, r, m, regs = _record()
    rng = np.random.default_rng(3)
    first = None
    for L in (1, 8, 9, 17):                                             # one trace, a full group, a partial one, several
        q = _traces(rng, L)
        want = ref.trace_maps(regs, m, q)
        assert want[0][:, m].any()
        for run in (1, 3, 64, 256):                                     # 7 runs, 3 with a partial one, one run
            r.tune("rec_map_frames", run)
            got = r.body_rec_trace_maps(q)
            assert got["c"].shape == (L, H, W) and got["w1"].shape == (H, W)
            assert _same(got, want), (L, run)
            if first is None:
                first = got
            assert got["w1"].tobytes() == first["w1"].tobytes() and got["w2"].tobytes() == first["w2"].tobytes()
        r.tune("rec_map_frames", 64)
        # NULL outputs, one at a time
        for drop in ("c", "w1", "w2"):
            keep = tuple(k for k in ("c", "w1", "w2") if k != drop)
            got = r.body_rec_trace_maps(q, want=keep)
            assert sorted(got) == sorted(keep)
            assert all(np.array_equal(got[k], want[("c", "w1", "w2").index(k)]) for k in keep), (L, drop)
        assert r.body_rec_trace_maps(q, want=()) == {}
    assert not first["w1"][~m].any() and not first["w2"][~m].any()
    assert np.array_equal(r.body_rec_fetch(), regs)                      # the record as it was
    for bad in (0, 257):
        with pytest.raises(RuntimeError, match=r"code -1.*rec_map_frames must be in 1\.\.256"):
            r.tune("rec_map_frames", bad)
    kf.close()


def test_trace_maps_against_trace_products_and_fetch(hm):
    """Inside a seed's window c is what hm_body_rec_trace_products gives for the same q, and w1 the sum of the fetched
    frames: two kernels of different work splits and the plain copy agree."""
    kf, r, m, regs = _record()
    rng = np.random.default_rng(4)
    rows, cols = np.nonzero(m)
    seeds = np.array([(cols[0], rows[0]), (cols[-1], rows[-1]), (31, 23), (cols[len(cols) // 3], rows[len(rows) // 3])], np.int32)
    P, R = len(seeds), 6
    q = _traces(rng, P)
    got = r.body_rec_trace_maps(q)
    tp = r.body_rec_trace_products(seeds, q, R)
    assert np.array_equal(tp, demix_ref.trace_products(regs, m, seeds, q, R))
    for s in range(P):
        rr, cc, on = roi_ref.window(H, W, seeds[s], R)
        assert np.array_equal(np.where(on, got["c"][s][rr, cc], 0), tp[s]), s
    assert np.array_equal(got["w1"], regs.astype(np.uint64).sum(0))
    assert np.array_equal(got["w2"], (regs.astype(np.uint64) ** 2).sum(0))
    kf.close()


def test_trace_maps_refusals_leave_the_record_usable(hm):
    kf, r, m, regs = _record()
    rng = np.random.default_rng(5)
    q = _traces(rng, 3)
    want = ref.trace_maps(regs, m, q)
    assert _same(r.body_rec_trace_maps(q), want)
    for L in (0, 1025):
        with pytest.raises(RuntimeError, match=r"code -1.*%d traces outside 1\.\.1024" % L):
            r.body_rec_trace_maps(np.zeros((F, L), np.int32))
        assert _same(r.body_rec_trace_maps(q), want)
    for v in (32768, -32768):
        bad = q.copy()
        bad[4, 1] = v
        bad[5, 0] = v                                                   # (the first offender in the call's order is named)
        with pytest.raises(RuntimeError, match=r"code -1.*q %d \(frame 4, trace 1\) outside -32767\.\.32767" % v):
            r.body_rec_trace_maps(bad)
        assert _same(r.body_rec_trace_maps(q), want)
    for wrong in (q.astype(np.int64), q[:5], q.reshape(-1)):
        with pytest.raises(ValueError, match="need int32, frames x traces"):
            r.body_rec_trace_maps(wrong)
    top = r.body_rec_trace_maps(np.full((F, 1024), 32767, np.int32), want=("c",))["c"]      # the most traces of a call
    assert top.shape == (1024, H, W) and np.array_equal(top[0], 32767 * want[1].astype(np.int64)) and (top == top[0]).all()
    assert np.array_equal(r.body_rec_fetch(), regs)
    # no frame recorded, and before begin: the record takes frames and gives their sums afterwards
    X, one = np.ascontiguousarray(kf.state.X, np.float64).reshape(-1), np.array([[-5]], np.int32)
    for state in ("no frame", "no record"):
        if state == "no frame":
            r.body_rec_begin()
            with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_trace_maps.*no frame recorded"):
                r.body_rec_trace_maps(one)
        else:
            r.body_rec_end()
            with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_trace_maps.*hm_body_rec_begin first"):
                r.body_rec_trace_maps(one)
            r.body_rec_begin()
        reg = r.body_warp(X, regs[2])[0]
        assert r.body_rec_count() == 1 and _same(r.body_rec_trace_maps(one), ref.trace_maps(reg[None], m, one))
    kf.close()


@pytest.mark.parametrize("seed", [1, 4])
def test_network_on_the_planted_scene_equals_the_restatement(hm, seed):
    """hydra_mi.network through the product on the planted video with ensembles as the tracker sees it (half the frames
    at rest, half shifted; seeds 1 and 4 carry the two figures of tests/test_network_cpu.py: the lowest correlation within
    an ensemble, 0.6822, and the highest between two, 0.4235): the maps and every host step equal the restatement on the
    registered video bit for bit, and the three planted ensembles and the lag of 8 frames are found."""
    from hydra_mi import body, mesh, network, roi
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs = ref.planted_scene(seed, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True)
    with pytest.raises(RuntimeError, match="no frame recorded"):
        network.maps(b, np.zeros((1, 1)))
    regs = np.array([b.registered(X, f) for X, f in zip(states, frames)])
    m = b.tri_of_pixel >= 0
    assert np.array_equal(m, roi_ref.planted_map())
    assert np.array_equal(np.where(m[None], regs, 0), np.where(m[None], ref.planted_video(seed)[0], 0))
    e = roi.extract(b, cs + 0.5, thr=ROI_THR)
    want_e = roi_ref.extract(regs, m, cs, thr=ROI_THR)
    assert np.array_equal(_bits(e["dff"]), _bits(want_e["dff"]))
    x = e["dff"].T
    got = network.extract(b, x)
    lo, hi, (lag, peak, at0) = ref.figures(e["dff"])
    print("seed %d: within %.4f between %.4f, 0 -> 2 at lag %d r %.4f (lag 0: %.4f)" % (seed, lo, hi, lag, peak, at0))
    assert lo >= WITHIN and hi <= BETWEEN and network.DEFAULT_THR == THR
    r = ref.coactivity(x, 10)
    labels = ref.ensembles(r[:, :, 10], THR)
    ens = ref.ensemble_traces(x, labels)
    ll, pk = ref.lead_lag(ens, 10)
    assert np.array_equal(_bits(got["r"]), _bits(r)) and np.array_equal(got["labels"], labels)
    assert np.array_equal(labels, ref.planted_labels())
    assert np.array_equal(_bits(got["ens_traces"]), _bits(ens))
    assert np.array_equal(got["lead_lag"], ll) and np.array_equal(_bits(got["lead_r"]), _bits(pk))
    assert got["lead_lag"][0, 2] == 8 and got["lead_lag"][2, 0] == -8 and got["lead_r"][0, 2] == peak
    rho = ref.maps(regs, m, ens)
    assert got["rho"].shape == (3,) + m.shape and np.array_equal(_bits(got["rho"]), _bits(rho))
    assert np.array_equal(got["map"], ref.ensemble_map(rho, network.DEFAULT_MAP_THR)) and got["map"].dtype == np.int16
    assert [int(got["map"][rw, c]) for c, rw in cs] == [ref.planted_ensemble(i) for i in range(12)]
    assert np.array_equal(got["gray"], np.rint(regs.astype(np.uint64).sum(0).astype(np.float64) / np.float64(len(regs))).astype(np.uint8))
    # the cells' own maps, more than one group of traces, a trace that is constant
    xs = np.concatenate((x, np.zeros((1, x.shape[1]))))
    assert np.array_equal(_bits(network.maps(b, xs)), _bits(ref.maps(regs, m, xs)))
    kf.close()


def test_cli_network_end_to_end(hm, tmp_path):
    from hydra_mi import synth, videoio
    n, F = 96, 14
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "12", "--find-radius", "4", "--find-score", "std"]
    out, png = str(tmp_path / "net.npz"), str(tmp_path / "m.png")
    # thresholds of -1: every pair of cells with a correlation at all is joined, every map pixel belongs to an ensemble
    res = subprocess.run(base + [out] + find + ["--rois", "--network", "--network-map", png, "--strain", "--network-lag", "3",
                                                "--network-thr", "-1", "--network-map-thr", "-1"],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z = np.load(out)
    F1, T = z["X"].shape[0], z["t"].shape[0]
    K = z["roi_points"].shape[0]
    assert F1 == F - 1 and 1 <= K <= 12
    assert z["net_r"].shape == (K, K, 7) and z["net_r"].dtype == np.float64
    assert z["net_labels"].shape == (K,) and z["net_labels"].dtype == np.int32
    E = int(z["net_labels"].max()) + 1
    print("CLI: %d cells, %d ensembles" % (K, E))
    assert z["net_ens_traces"].shape == (E, F1) and z["net_lead_lag"].shape == (E, E) and z["net_lead_r"].shape == (E, E)
    assert z["net_lead_lag"].dtype == np.int32 and (np.abs(z["net_lead_lag"]) <= 3).all()
    assert z["net_rho"].shape == (E, n, n) and z["net_rho"].dtype == np.float32
    assert z["net_map"].shape == (n, n) and z["net_map"].dtype == np.int16
    assert z["net_map"].min() >= -1 and z["net_map"].max() < max(E, 1) and (z["net_map"][np.isnan(z["body_mean"])] == -1).all()
    assert z["net_strain_r"].shape == (E, T) and z["strain_J"].shape == (F1, T)
    if E:
        assert (z["net_map"][~np.isnan(z["body_mean"])] >= 0).all() and np.isnan(z["net_rho"][:, np.isnan(z["body_mean"])]).all()
    img = videoio.read_png(png)
    assert img.shape == (n, n, 3) and img.dtype == np.uint8
    off = z["net_map"] < 0
    assert (img[off][:, 0] == img[off][:, 1]).all() and (img[off][:, 1] == img[off][:, 2]).all()       # gray where there is none
    assert "Network: %d ensembles" % E in res.stdout and "Ensemble map: " in res.stdout
    bad = subprocess.run(base + [out] + find + ["--network"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert bad.returncode == 2 and "needs --rois or --demix" in bad.stderr
