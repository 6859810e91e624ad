"""The surrogate reduction on the device (`pytest -m gpu`): hm_body_rec_trace_null equal to the restatement
(tests/network_null_ref.py) as bytes for every number of columns and every run length, to hydra_mi.network.maps and to
hm_body_rec_trace_maps where they overlap, its accumulators at their limit, its refusals, hydra_mi.network.map_null and
extract(null=...) through the product on the planted video with ensembles, and the CLI end to end.  Every comparison is
an equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import network_null_ref as nref
import network_ref as ref
import roi_ref
from test_network_null_cpu import NULL_TOP, OWN, ROI_THR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, F = 48, 64, 7
HELD = ((23, 31, 77), (12, 25, 0), (35, 40, 255))       # (row, column, value): map pixels that keep their value in every frame
KEYS = ("tmax", "tmin", "ge", "le")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _record(F=F, chunk=2, full=None):
    """A 64 x 48 frame with a disc of a mesh (a box 41 px wide: the last dword of a row and the last segment of a frame are
    partial; pixels of the box off the map), F random frames with 0 and 255 among their values, recorded with the mesh at
    rest in chunks of `chunk` frames; the pixels of HELD (and their neighbours, so that no interpolation changes them) keep
    one value throughout, and the rows of `full` (a slice) are 255 in every frame -> (kf, renderer, map, recorded frames)"""
    from hydra_mi import mesh
    dm = mesh.disk_mesh(31.5, 23.5, 20.3, 7.0)
    rng = np.random.default_rng(7)
    f0 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    N = dm.size()
    rest = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1), np.zeros(2 * N)))
    r.tune("body_rec_chunk", chunk)
    r.body_rec_begin()
    for k in range(F):
        f = rng.integers(0, 256, (H, W), dtype=np.uint8)
        f[rng.random((H, W)) < 0.05] = 0
        f[rng.random((H, W)) < 0.05] = 255
        if full is not None:
            f[full] = 255
        for y, x, v in HELD:
            f[y - 1:y + 2, x - 1:x + 2] = v
        r.body_warp(rest, f)
    r.tune("body_rec_chunk", 0)
    regs = r.body_rec_fetch()
    cols, rows = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    assert bw % 4 and ((bw + 3) // 4 * bh) % 64                          # partial last dword of a row, partial last segment
    assert not m[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].all()       # a map that is no rectangle
    assert regs.shape == (F, H, W) and not regs[:, ~m].any()
    assert (regs[:, m] == 0).any() and (regs[:, m] == 255).any()
    assert all(m[y, x] and (regs[:, y, x] == v).all() for y, x, v in HELD)
    return kf, r, m, regs


def _columns(rng, L, F=F):
    """(F, L) int32 with +-32767, zeros and negative values among them; column 0 reaches both ends (it is its own
    quantisation).  Of nine and more: column 3 equals column 0 (a tie in every pixel), column 4 is zero (vb = 0), columns 5
    and 6 are 32767 and -32767 throughout -> (q, vb)"""
    q = rng.integers(-32767, 32768, (F, L)).astype(np.int32)
    q[rng.random((F, L)) < 0.15] = 0
    q[rng.random((F, L)) < 0.15] = 32767
    q[rng.random((F, L)) < 0.15] = -32767
    q[:4, 0] = (32767, -32767, 0, -5)
    if L >= 9:
        q[:, 3] = q[:, 0]
        q[:, 4] = 0
        q[:, 5], q[:, 6] = 32767, -32767
    q = np.ascontiguousarray(q)
    return q, np.array([nref.vb_of(q[:, s]) for s in range(L)])


def _same(got, want, keys=KEYS):
    assert sorted(got) == sorted(keys)
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    return all(got[k].tobytes() == want[k].tobytes() for k in keys)


def _shim(r):
    """what hydra_mi.network.maps needs of a BodyReadout(keep=True)"""
    return type("B", (), dict(keep=True, r=r, tri_of_pixel=r.body_map()[0]))()


def test_trace_null_equals_the_restatement(hm):
    from hydra_mi import network
    kf, r, m, regs = _record()
    rng = np.random.default_rng(3)
    for L in (2, 9, 10, 25):                                            # one surrogate, a full group plus one, partial groups
        q, vb = _columns(rng, L)
        want = nref.trace_null(regs, m, q, vb)
        assert want["ge"][m].any() and want["le"][m].any() and want["tmax"][0] > 0.0 > want["tmin"][0]
        first = None
        for run in (1, 3, 256):                                         # 7 runs, 3 with a partial one, one run
            r.tune("rec_null_frames", run)
            got = r.body_rec_trace_null(q, vb)
            assert got["tmax"].shape == (L,) and got["ge"].shape == (H, W) and got["ge"].dtype == np.uint32
            assert _same(got, want), (L, run)
            first = got if first is None else first
            assert _same(got, first)                                    # the same bytes for every run length
        r.tune("rec_null_frames", 256)
        assert not got["ge"][~m].any() and not got["le"][~m].any()
        for y, x, _ in HELD:                                            # a constant pixel: every numerator is 0
            assert got["ge"][y, x] == L - 1 and got["le"][y, x] == L - 1
        if L >= 9:
            assert ((got["ge"].astype(np.int64) + got["le"])[m] >= L).all()     # (column 3 ties with column 0 everywhere)
            assert got["tmax"][4] == 0.0 and got["tmin"][4] == 0.0 and got["tmax"][5] == 0.0 and got["tmin"][6] == 0.0
            assert got["tmax"][3] == got["tmax"][0] and got["tmin"][3] == got["tmin"][0]
        # the observed column against hydra_mi.network.maps: the same rho, bit for bit
        rho = network.maps(_shim(r), q[:, 0][None].astype(np.float64))[0]
        assert np.array_equal(network.quantise(q[:, 0][None].astype(np.float64))[0], q[:, 0])
        assert _bits(got["tmax"][0]) == _bits(np.nanmax(rho)) and _bits(got["tmin"][0]) == _bits(np.nanmin(rho))
        # the counts against hm_body_rec_trace_maps' products of the same q: two kernels of different work splits
        s = r.body_rec_trace_maps(q)
        num = F * s["c"] - s["w1"].astype(np.int64)[None] * q.astype(np.int64).sum(0)[:, None, None]
        assert np.array_equal(got["ge"], np.where(m, (num[1:] >= num[0]).sum(0), 0))
        assert np.array_equal(got["le"], np.where(m, (num[1:] <= num[0]).sum(0), 0))
        # NULL outputs, one at a time
        for drop in KEYS:
            keep = tuple(k for k in KEYS if k != drop)
            assert _same(r.body_rec_trace_null(q, vb, want=keep), want, keep), (L, drop)
        assert r.body_rec_trace_null(q, vb, want=()) == {}
    assert np.array_equal(r.body_rec_fetch(), regs)                      # the record as it was
    for bad in (0, 257):
        with pytest.raises(RuntimeError, match=r"code -1.*rec_null_frames must be in 1\.\.256"):
            r.tune("rec_null_frames", bad)
    kf.close()


def test_trace_null_accumulators_at_their_limit(hm):
    """257 frames, rows 20..27 of them 255 throughout, columns of +-32767: with runs of 256 frames a 32-bit accumulator
    takes exactly 256 products of 255 x 32767 (2^31 - 8453888) before it is widened, then a run of one frame; with runs of 3
    it is widened 86 times.  Equal to the restatement in vectorised int64."""
    n = 257
    kf, r, m, regs = _record(F=n, chunk=100, full=slice(20, 28))
    assert ((regs == 255).all(0) & m).sum() >= 200
    rng = np.random.default_rng(6)
    q = rng.integers(-32767, 32768, (n, 11)).astype(np.int32)
    q[:, 1], q[:, 2] = 32767, -32767
    q[:, 3] = 32767
    q[256:, 3] = -32767                                                 # full scale through the first run, then the sign turns
    q[:, 4] = np.where(np.arange(n) % 2, 32767, -32767)
    q[:, 5] = np.where(np.arange(n) < 128, -32767, 32767)
    q[:, 9] = -q[:, 3]
    vb = np.array([nref.vb_of(q[:, s]) for s in range(q.shape[1])])
    want = nref.trace_null_np(regs, m, q, vb)
    assert 255 * 32767 * 256 == 2 ** 31 - 8453888
    for run in (256, 3):
        r.tune("rec_null_frames", run)
        assert _same(r.body_rec_trace_null(q, vb), want), run
    assert np.array_equal(r.body_rec_fetch(0, 3), regs[:3])
    kf.close()


def test_trace_null_refusals_leave_the_record_usable(hm):
    kf, r, m, regs = _record()
    rng = np.random.default_rng(5)
    q, vb = _columns(rng, 9)
    want = nref.trace_null(regs, m, q, vb)
    assert _same(r.body_rec_trace_null(q, vb), want)
    for L in (1, 4097):
        with pytest.raises(RuntimeError, match=r"code -1.*hm_body_rec_trace_null: %d traces outside 2\.\.4096" % L):
            r.body_rec_trace_null(np.zeros((F, L), np.int32), np.zeros(L))
        assert _same(r.body_rec_trace_null(q, vb), want)
    for v in (32768, -32768):
        bad = q.copy()
        bad[4, 1] = v
        bad[5, 0] = v                                                   # (the first offender in the call's order is named)
        with pytest.raises(RuntimeError, match=r"code -1.*q %d \(frame 4, trace 1\) outside -32767\.\.32767" % v):
            r.body_rec_trace_null(bad, vb)
        assert _same(r.body_rec_trace_null(q, vb), want)
    for v, text in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        bad = vb.copy()
        bad[2], bad[7] = v, v
        with pytest.raises(RuntimeError, match=r"code -1.*vb %s \(trace 2\) is negative or not finite" % text):
            r.body_rec_trace_null(q, bad)
        assert _same(r.body_rec_trace_null(q, vb), want)
    for wrong in (q.astype(np.int64), q[:5], q.reshape(-1)):
        with pytest.raises(ValueError, match="need int32, frames x traces"):
            r.body_rec_trace_null(wrong, vb)
    with pytest.raises(ValueError, match="vb of shape"):
        r.body_rec_trace_null(q, vb[:5])
    assert np.array_equal(r.body_rec_fetch(), regs)
    # no frame recorded, and before begin: the record takes frames and gives their results afterwards
    X, two = np.ascontiguousarray(kf.state.X, np.float64).reshape(-1), np.array([[-5, 3]], np.int32)
    for state in ("no frame", "no record"):
        if state == "no frame":
            r.body_rec_begin()
            with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_trace_null.*no frame recorded"):
                r.body_rec_trace_null(two, np.zeros(2))
        else:
            r.body_rec_end()
            with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_trace_null.*hm_body_rec_begin first"):
                r.body_rec_trace_null(two, np.zeros(2))
            r.body_rec_begin()
        reg = r.body_warp(X, regs[2])[0]
        assert r.body_rec_count() == 1 and _same(r.body_rec_trace_null(two, np.zeros(2)), nref.trace_null(reg[None], m, two, np.zeros(2)))
    kf.close()


@pytest.mark.parametrize("seed", [1, 4])
def test_map_null_on_the_planted_scene_equals_the_restatement(hm, seed):
    """hydra_mi.network.map_null and extract(null=...) through the product on the planted video with ensembles as the
    tracker sees it, against all 279 shifts beyond a guard of 10 frames (seeds 1 and 4 carry the two figures of
    tests/test_network_null_cpu.py: the lowest own-map value at a centre, 0.8120, and the largest null maximum, 0.5163):
    every array equals the restatement on the registered video, and every planted centre is significant in its own
    ensemble's map."""
    from hydra_mi import body, mesh, network, roi
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs = ref.planted_scene(seed, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True)
    regs = np.array([b.registered(X, f) for X, f in zip(states, frames)])
    m = b.tri_of_pixel >= 0
    e = roi.extract(b, cs + 0.5, thr=ROI_THR)
    x = e["dff"].T
    plain = network.extract(b, x)
    got = network.extract(b, x, null=1000)
    assert sorted(set(got) - set(plain)) == ["map_sig", "p_map", "p_r", "rho_max", "shifts", "sig"]
    for k in plain:                                                     # what there was is as it was
        assert plain[k].dtype == got[k].dtype and plain[k].tobytes() == got[k].tobytes(), k
    ens = ref.ensemble_traces(x, ref.planted_labels())
    assert np.array_equal(_bits(got["ens_traces"]), _bits(ens))
    want = nref.map_null(regs, m, ens, n=1000, guard=10)
    assert np.array_equal(got["shifts"], np.arange(11, 290)) and np.array_equal(want["shifts"], got["shifts"])
    full = network.map_null(b, ens)
    for k in ("rho", "rho_max", "rho_min", "p_map", "p_pix"):
        assert full[k].shape == want[k].shape and np.array_equal(_bits(full[k]), _bits(want[k])), k
    assert full["sig"].dtype == bool and np.array_equal(full["sig"], want["sig"])
    for k in ("rho_max", "p_map"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert np.array_equal(got["sig"], want["sig"])
    assert np.array_equal(_bits(got["p_r"]), _bits(nref.coactivity_null(x, got["shifts"])))
    assert got["map_sig"].dtype == np.int16 and np.array_equal(got["map_sig"], nref.map_sig(got["map"], want["sig"]))
    top = want["rho_max"].max()
    own = [want["rho"][ref.planted_ensemble(i), rw, c] for i, (c, rw) in enumerate(cs)]
    print("seed %d: the largest null maximum %.4f, the lowest own-map value at a centre %.4f, %s significant pixels" % (
        seed, top, min(own), want["sig"].sum((1, 2)).tolist()))
    assert top <= NULL_TOP and min(own) >= OWN
    assert all(got["sig"][ref.planted_ensemble(i), rw, c] for i, (c, rw) in enumerate(cs))
    assert [int(got["map_sig"][rw, c]) for c, rw in cs] == [ref.planted_ensemble(i) for i in range(12)]
    kf.close()


def test_cli_network_null_end_to_end(hm, tmp_path):
    """The 96 x 96 disc video of tests/test_network_gpu.py's CLI test with 21 frames instead of 14: 20 tracked frames have
    exactly the 19 circular shifts a null needs at the least."""
    from hydra_mi import synth, videoio
    n, F = 96, 21
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "12", "--find-radius", "4", "--find-score", "std"]
    net = ["--rois", "--network", "--strain", "--network-lag", "3", "--network-thr", "-1", "--network-map-thr", "-1"]
    out, png, old = str(tmp_path / "net.npz"), str(tmp_path / "m.png"), str(tmp_path / "old.npz")
    res = subprocess.run(base + [out] + find + net + ["--network-map", png, "--network-null", "19", "--network-guard", "0"],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z = np.load(out)
    F1, K = z["X"].shape[0], z["roi_points"].shape[0]
    E = int(z["net_labels"].max()) + 1
    S = 19
    assert F1 == F - 1 and 2 <= K <= 12 and E >= 1
    assert z["net_p_r"].shape == (K, K) and z["net_p_r"].dtype == np.float64 and np.isnan(np.diag(z["net_p_r"])).all()
    assert z["net_rho_max"].shape == (E, S) and z["net_rho_max"].dtype == np.float64
    assert z["net_p_map"].shape == (E, n, n) and z["net_p_map"].dtype == np.float32
    assert z["net_sig"].shape == (E, n, n) and z["net_sig"].dtype == np.bool_
    assert z["net_map_sig"].shape == (n, n) and z["net_map_sig"].dtype == np.int16
    off = np.isnan(z["body_mean"])
    assert np.isnan(z["net_p_map"][:, off]).all() and not z["net_sig"][:, off].any()
    on = z["net_p_map"][:, ~off]
    assert (on >= np.float32(1.0 / (S + 1))).all() and (on <= 1.0).all()
    assert np.array_equal(z["net_sig"], np.where(np.isnan(z["net_p_map"]), False, z["net_p_map"] <= np.float32(0.05)))
    won = np.take_along_axis(z["net_sig"], np.maximum(z["net_map"], 0).astype(np.int64)[None], 0)[0] & (z["net_map"] >= 0)
    assert np.array_equal(z["net_map_sig"], np.where(won, z["net_map"], -1))
    assert (z["net_map_sig"][~won] == -1).all()
    for k in range(E):
        line = "Null: ensemble %d: the largest rho of %d shifted traces %.4f, %d significant pixels" % (
            k, S, z["net_rho_max"][k].max(), z["net_sig"][k].sum())
        assert line in res.stdout, res.stdout
    img = videoio.read_png(png)
    gray = z["net_map_sig"] < 0
    assert img.shape == (n, n, 3) and (img[gray][:, 0] == img[gray][:, 1]).all() and (img[gray][:, 1] == img[gray][:, 2]).all()
    # without the flag: none of the new arrays
    res0 = subprocess.run(base + [old] + find + net, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res0.returncode == 0, res0.stderr[-2000:]
    z0 = np.load(old)
    new = {"net_p_r", "net_p_map", "net_rho_max", "net_sig", "net_map_sig"}
    assert set(z.files) - set(z0.files) == new and set(z0.files) <= set(z.files) and "Null:" not in res0.stdout
    bad = subprocess.run(base + [out] + find + ["--rois", "--network-null", "19"], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert bad.returncode == 2 and "needs --network" in bad.stderr
