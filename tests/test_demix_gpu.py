"""Demixing on the device (`pytest -m gpu`): hm_body_rec_trace_products equal to the restatement (tests/demix_ref.py) as
exact integers with run and chunk boundaries in awkward places, hydra_mi.demix.extract through the product equal to the
restatement bit for bit, and the CLI end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bodystats_cases as cases
import demix_ref as ref
import roi_ref
from test_roi_gpu import _seeds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", cases.NAMES)
def test_trace_products_equal_the_restatement(hm, name):
    """Every frame recorded twice over in chunks of 2 frames (6 frames, config 1: 20), runs of 1 frame (a run boundary at
    every chunk boundary), of 3 (the two interleave) and of more than there are frames (one partial run)."""
    dm, Xs, frames, f0 = cases.scene(name)
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    rng = np.random.default_rng(13)
    seeds = _seeds(m, rng)
    P = len(seeds)
    r.tune("body_rec_chunk", 2)
    r.body_rec_begin()
    regs = []
    for rep in range(2):
        for X, f in zip(Xs, frames):
            regs.append(r.body_warp(X, f)[0])
    r.tune("body_rec_chunk", 0)
    regs = np.array(regs)
    F = len(regs)
    before = r.body_rec_fetch()
    lo, hi = -2 ** 31, 2 ** 31 - 1
    qs = [rng.integers(lo, hi + 1, (F, P)).astype(np.int32), np.full((F, P), hi, np.int32), np.full((F, P), lo, np.int32),
          np.zeros((F, P), np.int32)]
    for tpf in (1, 3, F + 5):
        r.tune("rec_tp_frames", tpf)
        for R in (0, 3, 8, 16):
            for i, q in enumerate(qs if tpf == 3 else qs[:1]):
                got = r.body_rec_trace_products(seeds, q, R)
                assert got.dtype == np.int64 and got.shape == (P, 2 * R + 1, 2 * R + 1)
                assert np.array_equal(got, ref.trace_products(regs, m, seeds, q, R)), (tpf, R, i)
        one = r.body_rec_trace_products(seeds[3:4], np.ascontiguousarray(qs[0][:, 3:4]), 8)      # P = 1
        assert np.array_equal(one, ref.trace_products(regs, m, seeds[3:4], qs[0][:, 3:4], 8)), tpf
    r.tune("rec_tp_frames", 32)
    assert np.array_equal(r.body_rec_trace_products(seeds, qs[0], 8), ref.trace_products(regs, m, seeds, qs[0], 8))
    assert np.array_equal(r.body_rec_fetch(), before)
    kf.close()


def test_trace_products_call_order_and_argument_errors(hm):
    dm, Xs, frames, f0 = cases.scene("96x160")
    kf = cases.make_filter(dm, f0)
    r = kf.state.renderer
    m = r.body_map()[0] >= 0
    centre = np.array([[80, 47]], np.int32)
    with pytest.raises(RuntimeError, match=r"code -3.*hm_body_rec_begin first"):
        r.body_rec_trace_products(centre, np.zeros((1, 1), np.int32), 1)
    r.body_rec_begin()
    with pytest.raises(RuntimeError, match="code -3.*no frame recorded"):
        r.body_rec_trace_products(centre, np.zeros((1, 1), np.int32), 1)
    regs = np.array([r.body_warp(X, f)[0] for X, f in zip(Xs, frames)])
    q = np.arange(-1, len(regs) - 1, dtype=np.int32).reshape(-1, 1)
    assert np.array_equal(r.body_rec_trace_products(centre, q, 2), ref.trace_products(regs, m, centre, q, 2))
    with pytest.raises(RuntimeError, match="code -1.*window radius 17 outside 0..16"):
        r.body_rec_trace_products(centre, q, 17)
    assert not m[0, 0]
    with pytest.raises(RuntimeError, match="code -1.*not a pixel of the body map"):
        r.body_rec_trace_products(np.array([[0, 0]], np.int32), q, 2)
    with pytest.raises(RuntimeError, match="code -1.*not a pixel of the body map"):
        r.body_rec_trace_products(np.array([[500, 3]], np.int32), q, 2)
    with pytest.raises(ValueError, match="need int32"):
        r.body_rec_trace_products(centre, q.astype(np.int64), 2)
    for bad in (0, 1025):
        with pytest.raises(RuntimeError, match="code -1.*rec_tp_frames must be in 1..1024"):
            r.tune("rec_tp_frames", bad)
    kf.close()


def test_extract_on_the_paired_scene_equals_the_restatement(hm):
    """hydra_mi.demix.extract(iters=3) through the product on paired_scene(4, 4) as the tracker sees it (half the frames
    at rest, half shifted): the whole numbers D, M, G and shapes_q equal the restatement on the registered video, shapes,
    C and dF/F bit for bit; the worst cell beats the ROI trace (seed 4 is the one where the ROI trace is worst, 0.8702;
    three rounds give 0.9429 on the CPU); the record and the track are unchanged by the calls."""
    from hydra_mi import body, demix, mesh
    dm = mesh.box_mesh(*roi_ref.PLANTED_BOX)
    frames, states, cs, act = ref.paired_scene(4, 4, dm.p)
    kf = cases.make_filter(dm, frames[0])
    b = body.BodyReadout(kf, keep=True)
    regs = np.array([b.registered(X, f) for X, f in zip(states, frames)])
    m = b.tri_of_pixel >= 0
    assert np.array_equal(m, roi_ref.planted_map())
    r = kf.state.renderer
    r.tune("rec_tp_frames", 7)                                  # 300 frames: 42 runs and a partial one
    X0 = kf.state.X.copy()
    before = r.body_rec_fetch()
    got = demix.extract(b, cs + 0.5, iters=3, alpha=1.0)
    assert np.array_equal(r.body_rec_fetch(), before) and np.array_equal(before, regs) and np.array_equal(kf.state.X, X0)
    want = ref.demix(regs, m, cs, iters=3, alpha=1.0)
    for key in ("demix_D", "demix_M", "demix_G", "shapes_q", "demix_kept", "roi_labels"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    for key in ("shapes", "C", "dff_demixed", "demix_change", "F_roi", "F_np"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key
    roi_worst = ref.worst_cell(got["F_roi"] - got["F_np"], act)
    worst = ref.worst_cell(got["C"], act)
    print("paired scene: ROI trace %.4f, demixed after 3 rounds %.4f" % (roi_worst, worst))
    assert worst > roi_worst
    kf.close()


def test_cli_demix_end_to_end(hm, tmp_path):
    from hydra_mi import synth
    n, F = 96, 6
    video, masks, c, rad = synth.disk_video(n, F, "translate_leftup", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    base = [sys.executable, os.path.join(ROOT, "run_kalmanfilter.py"), vid, str(tmp_path / "none")]
    find = ["-s", "14", "--find-points", "5", "--find-radius", "4", "--find-score", "std"]
    out0, out1 = str(tmp_path / "rois.npz"), str(tmp_path / "demix.npz")
    res0 = subprocess.run(base + [out0] + find + ["--rois"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res0.returncode == 0, res0.stderr[-2000:]
    res = subprocess.run(base + [out1] + find + ["--demix", "--demix-iters", "2"], capture_output=True, text=True,
                         timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    z0, z = np.load(out0), np.load(out1)
    F1 = z["X"].shape[0]
    assert F1 == F - 1 and np.array_equal(z["X"], z0["X"])
    Q = z["roi_points"].shape[0]
    assert 1 <= Q <= 5
    for key in ("roi_footprints", "roi_labels", "roi_F", "roi_Fnp", "roi_dff"):               # --demix implies --rois
        assert np.array_equal(z[key], z0[key], equal_nan=True), key
    assert z["demix_shapes"].shape == (Q, 17, 17) and z["demix_shapes"].dtype == np.float64
    assert z["demix_shapes"].min() >= 0.0 and z["demix_shapes"].max() == 1.0
    for key in ("demix_C", "demix_dff"):
        assert z[key].shape == (F1, Q) and z[key].dtype == np.float64, key
    assert z["demix_change"].shape == (2,) and z["demix_change"].dtype == np.float64
    assert "Demixed: %d cells, 2 rounds, last change %.3g" % (Q, z["demix_change"][-1]) in res.stdout
    assert not [k for k in z0.files if k.startswith("demix_")] and "Demixed" not in res0.stdout
