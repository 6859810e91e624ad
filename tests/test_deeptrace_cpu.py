"""The host side of the full-depth traces: tests/deeptrace_ref.py against values computed by hand, deeptrace.columns, the
host path of deeptrace.run against the restatement, the trace formulas on sums given by hand, and the CLI's refusals."""
import os
import sys

import numpy as np
import pytest

import body_ref
import border_cases as bc
import deeptrace_ref as ref


# ---- the restatement by hand -------------------------------------------------------------------------------------------
F22 = np.array([[10, 13], [20, 60001]], np.uint16)


def test_sample_by_hand():
    # at a pixel centre: the texel itself
    assert ref.sample16(0.5, 0.5, F22) == 10 and ref.sample16(1.5, 1.5, F22) == 60001
    # halfway between (0, 0) and (0, 1): (10 + 13) / 2 = 11.5, a tie -> 12 (even); between 10 and 20 = 15 exactly
    assert ref.sample16(1.0, 0.5, F22) == 12
    assert ref.sample16(0.5, 1.0, F22) == 15
    # a tie that rounds down to even: 0.5 * 20 + 0.5 * 60001 = 30010.5 -> 30010
    assert ref.sample16(1.0, 1.5, F22) == 30010
    # the centre of the four: (10 + 13 + 20 + 60001) / 4 = 15011.0
    assert ref.sample16(1.0, 1.0, F22) == 15011
    # clamped texels: left of column 0 both columns are column 0; beyond the last row both rows are row 1
    assert ref.sample16(0.25, 0.5, F22) == 10
    assert ref.sample16(-3.0, 1.5, F22) == 20
    assert ref.sample16(1.5, 7.0, F22) == 60001
    # a quarter of the way: 0.75 * 10 + 0.25 * 13 = 10.75 -> 11
    assert ref.sample16(0.75, 0.5, F22) == 11
    # not finite, beyond +-2^20: 0; at 2^20 itself: the clamped texel
    assert ref.sample16(np.nan, 0.5, F22) == 0 and ref.sample16(0.5, np.inf, F22) == 0
    assert ref.sample16(1048577.0, 0.5, F22) == 0 and ref.sample16(0.5, -1048576.5, F22) == 0
    assert ref.sample16(1048576.0, 0.5, F22) == 13
    # full scale survives
    assert ref.sample16(0.5, 0.5, np.full((2, 2), 65535, np.uint16)) == 65535


def test_swap_and_column_sums_by_hand():
    assert ref.swap_bytes(np.array([0x1234, 0x00FF, 0xFF00, 0], np.uint16)).tolist() == [0x3412, 0xFF00, 0x00FF, 0]
    plane = np.array([[1, 2], [3, 65535]], np.uint16)
    ptr, pix, wt = [0, 2, 2, 5], [3, 3, 0, 1, 3], [65535, 65535, 1, 10, 2]
    assert ref.column_sums(plane, ptr, pix, wt) == [2 * 4294836225, 0, 1 + 20 + 131070]
    # swapped frames warp as their values
    name = "full33x17"
    W, H = bc.size(name)
    dm, Xs, _, _ = bc.scene(name)
    m = body_ref.body_map(dm.p, dm.t, W, H)
    fr = np.random.default_rng(1).integers(0, 65536, (H, W)).astype(np.uint16)
    assert np.array_equal(ref.warp16(Xs[1], fr.byteswap(), *m, swap=1), ref.warp16(Xs[1], fr, *m))
    # values that fit 8 bits: the old warp's bytes
    f8 = np.random.default_rng(2).integers(0, 256, (H, W)).astype(np.uint8)
    assert np.array_equal(ref.warp16(Xs[2], f8.astype(np.uint16), *m), body_ref.warp(Xs[2], f8, *m))


# ---- deeptrace.columns -------------------------------------------------------------------------------------------------
def test_columns(hm):
    from hydra_mi import deeptrace
    H, W = 5, 7
    labels = np.full((H, W), -1, np.int32)
    labels[1, 2] = 2
    labels[0, 6] = 0
    labels[4, 0] = 2                                                 # label 1 has no pixel: an empty column
    seeds = np.array([[0, 0], [6, 4], [3, 2]], np.int32)             # (column, row): two corners, one inside
    w = np.zeros((3, 3, 3), np.uint16)
    w[0] = 7                                                         # 5 of 9 off the frame
    w[1, 1, 1] = 65535                                               # the seed pixel alone; the rest has weight 0
    w[2] = np.arange(9).reshape(3, 3)                                # one zero weight, at (row 1, column 2)
    w2 = np.ones((3, 1, 1), np.uint16)                               # a second set over the same seeds: overlapping windows
    cols = deeptrace.columns(labels, 3, [(seeds, w, 1), (seeds, w2, 0)])
    assert cols.directory == {"labels": (0, 3), "windows": [(3, 6), (6, 9)]}
    assert cols.col_ptr.dtype == np.int64 and cols.pix.dtype == np.int32 and cols.wt.dtype == np.uint16
    assert cols.col_ptr.tolist() == [0, 1, 1, 3, 7, 8, 16, 17, 18, 19]
    assert cols.pix[:3].tolist() == [6, 1 * W + 2, 4 * W + 0] and cols.wt[:3].tolist() == [1, 1, 1]
    assert cols.pix[3:7].tolist() == [0, 1, W, W + 1] and cols.wt[3:7].tolist() == [7] * 4
    assert cols.pix[7:8].tolist() == [4 * W + 6] and cols.wt[7] == 65535
    assert cols.pix[8:16].tolist() == [1 * W + 3, 1 * W + 4, 2 * W + 2, 2 * W + 3, 2 * W + 4, 3 * W + 2, 3 * W + 3, 3 * W + 4]
    assert cols.wt[8:16].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert cols.pix[16:].tolist() == [0, 4 * W + 6, 2 * W + 3]
    # the pixel (2, 3) sits in two columns; without labels the shape is needed
    assert (cols.pix == 2 * W + 3).sum() == 2
    only = deeptrace.columns(windows=[(seeds, w2, 0)], shape=(H, W))
    assert only.directory == {"labels": None, "windows": [(0, 3)]} and only.col_ptr.tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        deeptrace.columns(windows=[(seeds, w2, 0)])
    with pytest.raises(ValueError):
        deeptrace.columns(labels, 2)                                 # the image holds label 2
    with pytest.raises(ValueError):
        deeptrace.columns(labels, 3, [(seeds, w, 2)])                # weights of the wrong shape


# ---- the host path -----------------------------------------------------------------------------------------------------
def _columns_for(tri_of, rng, C=5):
    from hydra_mi import deeptrace
    H, W = tri_of.shape
    labels = rng.integers(-1, C, (H, W)).astype(np.int32)
    seeds = np.stack((rng.integers(0, W, 4), rng.integers(0, H, 4)), 1).astype(np.int32)
    w = rng.integers(0, 65536, (4, 7, 7)).astype(np.uint16)
    w[rng.random(w.shape) < 0.3] = 0
    return deeptrace.columns(labels, C, [(seeds, w, 3)])


@pytest.mark.parametrize("name", bc.NAMES)
def test_host_path_equals_the_restatement(hm, name):
    from hydra_mi import deeptrace
    W, H = bc.size(name)
    dm, Xs, _, _ = bc.scene(name)
    rng = np.random.default_rng(bc.seed_of(name) + 5)
    video = rng.integers(0, 65536, (4, H, W)).astype(np.uint16)
    m = body_ref.body_map(dm.p, dm.t, W, H)
    hmap = deeptrace.HostMap(dm.p, dm.t, W, H)
    assert np.array_equal(hmap.tri_of, m[0]) and np.array_equal(hmap.l1, m[1]) and np.array_equal(hmap.l2, m[2])
    assert np.array_equal(hmap.ids, m[3])
    cols = _columns_for(m[0], rng)
    X = list(Xs)
    X[1] = X[1].copy()
    X[1][0] = np.nan                                                 # a vertex that is not finite, one beyond 2^20
    X[2] = X[2].copy()
    X[2][3] = 3.0e6
    # three states for four frames: the body readout's pairing, state i with frame i + 1
    want_s, want_p = ref.run(X, video[1:], *m, cols.col_ptr, cols.pix, cols.wt)
    sums, planes = deeptrace.run(hmap, video, X, cols, planes=True, device=None)
    assert sums.dtype == np.uint64 and planes.dtype == np.uint16
    assert np.array_equal(planes, want_p) and np.array_equal(sums, want_s)
    # big-endian frames give the same numbers; states alone give the sums alone
    assert np.array_equal(deeptrace.run(hmap, video.astype(">u2"), X, cols, device=None), want_s)
    # a run that ended early: fewer states than frames - 1 still read frames 1, 2, ... -- never the file's last frames
    assert np.array_equal(deeptrace.run(hmap, video, X[:2], cols, device=None), want_s[:2])
    assert np.array_equal(deeptrace.run(hmap, video, X[:1], cols, device=None), want_s[:1])
    late = ref.run(X[:2], video[2:], *m, cols.col_ptr, cols.pix, cols.wt)[0]
    assert np.array_equal(deeptrace.run(hmap, video, X[:2], cols, device=None, first=2), late)
    with pytest.raises(ValueError, match="first = 2"):
        deeptrace.run(hmap, video, X, cols, device=None, first=2)    # 3 states from frame 2 on, 4 frames
    with pytest.raises(ValueError):
        deeptrace.run(hmap, video, X, None, device=None)
    with pytest.raises(ValueError):
        deeptrace.run(hmap, video, X + X, cols, device=None)         # more states than frames


def test_wide_sums_on_the_host(hm):
    """two entries of 65535 x 65535, and a column whose sum passes 2^32 with small terms"""
    from hydra_mi import deeptrace, mesh
    W = H = 16
    dm = mesh.box_mesh(-1.0, -1.0, 17.0, 17.0, 4.0)
    hmap = deeptrace.HostMap(dm.p, dm.t, W, H)
    assert (hmap.tri_of >= 0).all()
    X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1), np.zeros(2 * dm.size())))
    video = np.full((1, H, W), 65535, np.uint16)
    cols = deeptrace.Columns(np.array([0, 2, 258], np.int64), np.concatenate(([5, 9], np.arange(256))).astype(np.int32),
                             np.full(258, 65535, np.uint16), {})
    sums = deeptrace.run(hmap, video, [X], cols, device=None, first=0)
    assert sums.tolist() == [[2 * 4294836225, 256 * 4294836225]]


# ---- the traces --------------------------------------------------------------------------------------------------------
def test_traces_by_hand(hm):
    from hydra_mi import deeptrace, roi
    # three cells over four frames: 4 ROI pixels and a ring of 2; 2 ROI pixels and an empty ring; an ROI of count 0
    roi_sums = np.array([[4400, 2200, 0], [4800, 2200, 0], [8400, 2600, 0], [4400, 2200, 0]], np.uint64)
    ring_sums = np.array([[2200, 0, 10], [2200, 0, 10], [2400, 0, 10], [2200, 0, 10]], np.uint64)
    F_roi, F_np, dff = deeptrace.traces(roi_sums, [4, 2, 0], ring_sums, [2, 0, 1], alpha=0.5, q=0.0, half=100, offset=100.0)
    assert F_roi[:, 0].tolist() == [1000.0, 1100.0, 2000.0, 1000.0] and F_roi[:, 1].tolist() == [1000.0, 1000.0, 1200.0, 1000.0]
    assert np.isnan(F_roi[:, 2]).all()
    assert F_np[:, 0].tolist() == [1000.0, 1000.0, 1100.0, 1000.0]
    assert F_np[:, 1].tolist() == [0.0] * 4                         # an empty ring: nothing to correct with, offset or not
    # F_c = F_roi - 0.5 F_np = 500, 600, 1450, 500; q = 0: the baselines are the minima, 500 and 1000
    assert dff[:, 0].tolist() == [0.0, 0.1, 0.95, 0.0]
    assert dff[:, 1].tolist() == [0.0, 0.0, 0.2, 0.0]
    assert np.isnan(dff[:, 2]).all()
    # offset 0: roi.extract's own expressions, bit for bit
    F_roi0, F_np0, dff0 = deeptrace.traces(roi_sums, [4, 2, 0], ring_sums, [2, 0, 1], alpha=0.7, q=10.0, half=1)
    a, b = roi._means(roi_sums, [4, 2, 0], np.nan), roi._means(ring_sums, [2, 0, 1], 0.0)
    c = a - np.float64(0.7) * b
    with np.errstate(invalid="ignore"):
        want = np.stack([(c[:, s] - roi.baseline(c[:, s], 10.0, 1)) / roi.baseline(a[:, s], 10.0, 1) for s in range(3)], 1)
    assert np.array_equal(F_roi0, a, equal_nan=True) and np.array_equal(F_np0, b) and np.array_equal(dff0, want, equal_nan=True)
    assert deeptrace.point_means(roi_sums[:1], [4, 2, 0], 100.0)[0, :2].tolist() == [1000.0, 1000.0]


def test_demix_solve_is_the_step_of_extract(hm):
    """demix.solve_traces on whole numbers by hand: two cells that do not overlap decouple into c = d / G_ss"""
    from hydra_mi import demix, roi
    A = np.zeros((2, 3, 3), np.int64)
    A[0, 1, 1], A[0, 1, 2] = 65535, 32768
    A[1, 1, 1] = 65535
    G = np.array([[65535 ** 2 + 32768 ** 2, 0], [0, 65535 ** 2]], np.int64)
    ws = roi._ints(np.array([[98303 * 1000, 65535 * 500], [98303 * 3000, 65535 * 700]], np.uint64))
    gsum = roi._ints(np.array([[0, 200], [0, 200]], np.uint64))
    C, sa, bad = demix.solve_traces(G, A, ws, gsum, [1, 2])
    assert sa == [98303, 65535] and bad == -1
    # cell 1: d = 65535 (v - 100), c = d / 65535^2, C = c 65535^2 / 65535 = v - 100
    assert np.allclose(C[:, 1], [400.0, 600.0], rtol=1e-15)
    assert np.allclose(C[:, 0], [1000.0, 3000.0], rtol=1e-15)
    assert demix.solve_traces(np.array([[1, 2], [2, 1]], np.int64), A, ws, gsum, [1, 2])[0] is None


# ---- the command line --------------------------------------------------------------------------------------------------
def test_cli_refusals(hm, tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_kalmanfilter as cli
    monkeypatch.chdir(tmp_path)
    np.save("v8.npy", np.zeros((3, 16, 16), np.uint8))
    with open("pts.csv", "w") as f:
        f.write("a,8,8\n")
    cases = [
        (["v8.npy", "none", "o.npz", "--deep-traces", "--points", "pts.csv"], "reads 16-bit frames"),
        (["v8.npy", "none", "o.npz", "--deep-traces"], "needs --rois, --demix or --points"),
        (["v8.npy", "none", "o.npz", "--deep-traces", "--points", "pts.csv", "--rois", "--stabilize"], "--stabilize rewrites"),
        (["v8.npy", "none", "o.npz", "--deep-traces", "--points", "pts.csv", "--rois", "--deform-correct"], "--deform-correct rewrites"),
        (["v8.npy", "none", "o.npz", "--deep-offset", "100"], "goes with --deep-traces"),
    ]
    for argv, words in cases:
        with pytest.raises(SystemExit):
            cli.main(argv)
        err = capsys.readouterr().err
        assert words in err, (argv, err)
        assert not os.path.exists("o.npz")
