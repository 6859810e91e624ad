"""CPU checks of the statistics of the registered video: the restatement (tests/bodystats_ref.py) against the textbook
definitions it stands for, recovery of planted cells with the restatement alone, the ABI, the points CSV and the CLI's
argument check."""
import os
import re
import sys

import numpy as np
import pytest

import body_ref
import bodystats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ragged_map(rng, H, W):
    m = rng.random((H, W)) < 0.8
    m[0, :3] = True                       # map pixels on the frame's border and corner
    m[-1, -2:] = True
    m[H // 2, W // 2] = True              # an island: a map pixel without map neighbours
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                m[H // 2 + dr, W // 2 + dc] = False
    return m


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_corr_is_the_mean_pearson_correlation_with_the_neighbours(seed):
    """1e-12 absolute: the rounding of two formulas for a number in [-1, 1] (a few ulp of 1.1e-16 each over eight
    terms), not a property of the code under test."""
    rng = np.random.default_rng(seed)
    F, H, W = 40, 13, 17
    v = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    v[:, 3, 4] = 77                       # constant pixels: no neighbour to anybody, corr 0 themselves
    v[:, 3, 5] = 0
    v[:, 9, 9] = v[:, 9, 10]              # a perfectly correlated pair
    m = _ragged_map(rng, H, W)
    m[3, 4] = m[3, 5] = m[9, 9] = m[9, 10] = True
    regs = np.where(m, v, 0).astype(np.uint8)
    s1, s2, cross, vmax = ref.accumulate(regs, m)
    assert (s1[~m] == 0).all() and (s2[~m] == 0).all() and (cross[:, ~m] == 0).all() and (vmax[~m] == 0).all()
    mean, std, corr, mx = ref.images(s1, s2, cross, vmax, F, m)
    x = regs.astype(np.float64)
    want = np.full((H, W), np.nan)
    for r in range(H):
        for c in range(W):
            if not m[r, c]:
                continue
            rho = []
            for dc, dr in ref.EIGHT:
                rq, cq = r + dr, c + dc
                if not (0 <= rq < H and 0 <= cq < W and m[rq, cq]):
                    continue
                if x[:, r, c].std() == 0 or x[:, rq, cq].std() == 0:
                    continue
                rho.append(np.corrcoef(x[:, r, c], x[:, rq, cq])[0, 1])
            want[r, c] = np.mean(rho) if rho else 0.0
    assert np.isnan(corr[~m]).all() and np.isnan(mean[~m]).all() and np.isnan(std[~m]).all() and (mx[~m] == 0).all()
    assert np.abs(corr[m] - want[m]).max() <= 1e-12
    assert corr[3, 4] == 0.0 and corr[3, 5] == 0.0 and corr[H // 2, W // 2] == 0.0
    assert np.abs(mean[m] - x.mean(0)[m]).max() <= 1e-12 * 255
    assert np.abs(std[m] - x.std(0)[m]).max() <= 1e-12 * 255
    assert np.array_equal(mx[m], regs.max(0)[m])


def _peaks_by_dilation(score, m, radius, min_score):
    """grey dilation over the window with -inf outside the map: a peak equals the window's maximum, and no pixel before
    it in raster order within the window has the same score"""
    from scipy import ndimage
    H, W = m.shape
    s = np.where(m, score, -np.inf)
    top = ndimage.maximum_filter(s, size=2 * radius + 1, mode="constant", cval=-np.inf)
    out = []
    for p in np.flatnonzero((m & (s == top) & (s >= min_score)).reshape(-1)):
        r, c = divmod(int(p), W)
        win = s[max(0, r - radius):r + radius + 1, max(0, c - radius):c + radius + 1]
        first = np.argwhere(win == s[r, c])[0] + [max(0, r - radius), max(0, c - radius)]
        if tuple(first) == (r, c):
            out.append((s[r, c], p))
    out.sort(key=lambda e: (-e[0], e[1]))
    return np.array([e[1] for e in out], np.int32), np.array([e[0] for e in out], np.float64)


@pytest.mark.parametrize("radius", [1, 2, 6])
def test_peak_rule_against_dilation(radius):
    rng = np.random.default_rng(radius)
    H, W = 40, 48
    m = _ragged_map(rng, H, W)
    cases = []
    cases.append(rng.integers(0, 5, (H, W)).astype(np.float64))          # few levels: plateaus and ties everywhere
    cases.append(np.zeros((H, W)))                                       # one plateau: the tie rule alone
    a = rng.random((H, W))
    a[12, 14] = a[12, 14 + radius] = 2.0                                 # a tie at the window's edge: the first wins
    a[30, 10] = a[30, 10 + radius + 1] = 3.0                             # ... and just beyond it: both stand
    a[0, 0] = a[H - 1, W - 1] = 4.0                                      # on the frame's corners
    m[12, 14] = m[12, 14 + radius] = m[30, 10] = m[30, 10 + radius + 1] = True
    cases.append(a)
    b = rng.random((H, W))
    b[~m] = 9.0                                                          # scores outside the map never count
    cases.append(b)
    for score in cases:
        for thr in (-np.inf, 0.5):
            i0, s0 = ref.peaks(score, m, radius, thr)
            i1, s1 = _peaks_by_dilation(score, m, radius, thr)
            i2, s2 = ref.peaks_fast(score, m, radius, thr)
            assert np.array_equal(i0, i1) and np.array_equal(s0, s1)
            assert np.array_equal(i0, i2) and np.array_equal(s0, s2)
            rr, cc = np.divmod(i0.astype(np.int64), W)
            for k in range(len(i0)):                                     # two peaks are more than `radius` apart
                d = np.maximum(np.abs(rr - rr[k]), np.abs(cc - cc[k]))
                assert (np.delete(d, k) > radius).all()
    i, _ = ref.peaks(a, m, radius)
    assert 12 * W + 14 in i and 12 * W + 14 + radius not in i and 30 * W + 10 in i and 30 * W + 10 + radius + 1 in i
    assert 0 in i and H * W - 1 in i
    i, _ = ref.peaks(np.zeros((H, W)), m, radius)
    assert i[0] == 0                                                     # every pixel ties: raster order decides


def _planted_map():
    from hydra_mi import mesh
    dm = mesh.box_mesh(*ref.PLANTED_BOX)
    H, W = ref.PLANTED["H"], ref.PLANTED["W"]
    return dm, body_ref.body_map(np.asarray(dm.p, np.float32), dm.t, W, H)


@pytest.mark.parametrize("seed", range(6))
def test_planted_cells_are_recovered_by_the_restatement(hm, seed):
    """12 of 12 within 1 px for every seed and score, with the box-mesh map and the restated warp.  Measured here (box
    map, seeds 0..5): all 18 runs (six seeds, three scores) put the 12 best peaks ON the planted centres (distance 0) of
    56..73 peaks in all; the 12th corr score is 0.895..0.936 and the 13th 0.093..0.121; the disc traces (radius 3)
    correlate with the planted activity at 0.9953..0.9972 (smallest over cells); the bound is that minimum less 0.05 for
    the pixel a centre may be off: 0.94."""
    dm, (tri_of, l1, l2, ids) = _planted_map()
    m = tri_of >= 0
    frames, states, cs, act = ref.planted_scene(seed, dm.p)
    video = ref.planted_video(seed)[0]
    F = frames.shape[0]
    assert all(m[cy - 8:cy + 9, cx - 8:cx + 9].all() for cx, cy in cs)           # the cells lie well inside the map
    regs = np.array([body_ref.warp(states[k], frames[k], tri_of, l1, l2, ids) for k in (0, F // 2, F - 1)])
    for k, reg in zip((0, F // 2, F - 1), regs):
        assert np.array_equal(reg[m], video[k][m]), k                            # the warp undoes the whole-pixel shift
    regs = np.where(m, video, 0).astype(np.uint8)
    mean, std, corr, mx = ref.images(*ref.accumulate(regs, m), F, m)
    for which in ("corr", "std", "range"):
        idx, sc = ref.peaks_fast(ref.score_image(which, mean, std, corr, mx), m, 6)
        assert len(idx) > 12
        rr, cc = np.divmod(idx[:12].astype(np.int64), m.shape[1])
        pts = np.stack((cc, rr), 1)
        near = [int(np.abs(pts - c).max(1).argmin()) for c in cs]
        dist = [int(np.abs(pts[j] - c).max()) for j, c in zip(near, cs)]
        print("seed %d %s: %d peaks, largest distance %d, 12th score %.3f, 13th %.3f" % (seed, which, len(idx), max(dist),
                                                                                         sc[11], sc[12]))
        assert max(dist) <= 1, (which, dist)
        if which == "corr":
            tc = [np.corrcoef(ref.disc_trace(regs, pts[j] + 0.5, 3.0), act[i])[0, 1] for i, j in enumerate(near)]
            print("seed %d: smallest trace correlation %.4f" % (seed, min(tc)))
            assert min(tc) >= 0.94, tc


def test_the_abi_declares_and_exports_the_statistics(hm):
    import ctypes
    from hydra_mi import _lib
    names = ["hm_body_stats_begin", "hm_body_stats_end", "hm_body_stats_count", "hm_body_stats_fetch",
             "hm_body_stats_images", "hm_body_stats_peaks"]
    header = open(os.path.join(ROOT, "include", "hydra_mi.h")).read()
    declared = set(re.findall(r"\b(hm_[a-z_0-9]+)\s*\(", header))
    so = ctypes.CDLL(_lib.SO_PATH)
    for n in names:
        assert n in declared, n
        assert n in _lib.SIGNATURES, n
        assert hasattr(so, n), n
    L = _lib.lib()
    cnt = ctypes.c_int(0)
    assert L.hm_body_stats_begin(None) == -1 and b"NULL" in L.hm_last_error()
    assert L.hm_body_stats_peaks(None, 0, 0, 0.0, 0, None, None, ctypes.byref(cnt)) == -1
    assert b"radius 0 outside 1..16" in L.hm_last_error()
    assert L.hm_body_stats_peaks(None, 0, 17, 0.0, 0, None, None, ctypes.byref(cnt)) == -1
    assert b"radius 17" in L.hm_last_error()
    assert L.hm_body_stats_peaks(None, 3, 6, 0.0, 0, None, None, ctypes.byref(cnt)) == -1


def test_points_csv_round_trip(hm, tmp_path):
    from hydra_mi import body
    rng = np.random.default_rng(0)
    pts = np.concatenate((rng.uniform(0, 1000, (7, 2)), [[12.5, 0.5], [1 / 3, 2e-7]]))
    p1 = str(tmp_path / "a.csv")
    body.write_points_csv(p1, pts)
    names, back = body.read_points_csv(p1)
    assert np.array_equal(back, pts) and names == ["p%d" % i for i in range(9)]
    body.write_points_csv(p1, pts[:2], names=["left", "right"])
    names, back = body.read_points_csv(p1)
    assert names == ["left", "right"] and np.array_equal(back, pts[:2])
    body.write_points_csv(p1, np.zeros((0, 2)))
    assert body.read_points_csv(p1)[1].shape == (0, 2)
    with pytest.raises(ValueError):
        body.write_points_csv(p1, pts, names=["one"])
    with pytest.raises(ValueError):
        body.write_points_csv(p1, pts[:1], names=["a,b"])


def test_cli_refuses_find_points_with_points(hm, capsys):
    sys.path.insert(0, ROOT)
    import run_kalmanfilter
    with pytest.raises(SystemExit) as e:
        run_kalmanfilter.main(["v.npy", "flow", "out.npz", "--find-points", "5", "--points", "p.csv"])
    assert e.value.code == 2
    assert "not together with --points" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run_kalmanfilter.main(["v.npy", "flow", "out.npz", "--find-points", "5", "--find-radius", "17"])
    with pytest.raises(SystemExit):
        run_kalmanfilter.main(["v.npy", "flow", "out.npz", "--points-out", "found.csv"])
