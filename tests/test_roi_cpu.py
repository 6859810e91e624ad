"""Footprints, ROIs and traces on the CPU: the restatement (tests/roi_ref.py) against np.corrcoef and hand-made cases, the
host arithmetic of hydra_mi.roi against the restatement bit for bit, and the planted video with neuropil, which has to
show both the need for the ring correction and its cure."""
import numpy as np
import pytest

import roi_ref as ref

THR = 0.47            # hydra_mi.roi.DEFAULT_THR: halfway between 0.542 and 0.401 (test_planted_video_*'s docstring)
BOUND = 0.9688        # the worst corrected ROI trace of the restatement over six seeds, 0.9888, minus 0.02


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _small_video(seed, F=40, H=24, W=30):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    m = np.zeros((H, W), bool)
    m[2:21, 3:27] = True
    m[10:13, 12:15] = False                                   # a hole in the map
    seeds = np.array([[8, 7], [20, 12], [4, 3], [25, 19], [13, 13]])
    # something to correlate with: every seed's disc brightens together
    for s, (c, r) in enumerate(seeds):
        a = rng.integers(0, 60, F)
        v[:, max(r - 2, 0):r + 3, max(c - 2, 0):c + 3] = np.clip(
            v[:, max(r - 2, 0):r + 3, max(c - 2, 0):c + 3] // 2 + a[:, None, None], 0, 255)
    return v, m, seeds


def test_footprints_equal_corrcoef(hm):
    from hydra_mi import roi
    v, m, seeds = _small_video(0)
    F, H, W = v.shape
    R = 5
    ss = ref.seed_sums(v, m, seeds, 2.0, 3.0, 5.5, R)
    rho = ref.footprints(ss, F, m, seeds, R)
    assert np.array_equal(_bits(roi.footprints(ss, F, m, seeds, R)), _bits(rho))
    worst = 0.0
    for s, seed in enumerate(seeds):
        disc, ring = ref.disc_and_ring(m, seed, 2.0, 3.0, 5.5)
        vm = np.where(m[None], v, 0).astype(np.float64)
        u = vm[:, disc].sum(1) * ring.sum() - vm[:, ring].sum(1) * disc.sum()
        assert np.array_equal(u, ss["U"][:, s].astype(np.float64))
        rr, cc, on = ref.window(H, W, seed, R)
        for i in range(2 * R + 1):
            for j in range(2 * R + 1):
                if not (on[i, j] and m[rr[i, j], cc[i, j]]):
                    assert np.isnan(rho[s, i, j])
                    continue
                want = np.corrcoef(vm[:, rr[i, j], cc[i, j]], u)[0, 1]
                worst = max(worst, abs(want - rho[s, i, j]))
    print("footprints against np.corrcoef: %.2e" % worst)
    assert worst <= 1e-12
    assert np.isnan(rho).any() and (~np.isnan(rho)).any()


def test_flat_pixels_and_flat_seeds_give_zero(hm):
    from hydra_mi import roi
    v, m, seeds = _small_video(1)
    v[:, 7, 9] = 17                                             # a pixel that never changes, in seed 0's window
    v[:, 10:15, 18:23] = 200                                    # seed 1's disc and ring flat: U is constant
    ss = ref.seed_sums(v, m, seeds[:2], 1.0, 1.5, 2.0, 4)
    for f in (ref.footprints, roi.footprints):
        rho = f(ss, v.shape[0], m, seeds[:2], 4)
        assert rho[0, 4, 5] == 0.0 and (rho[1][~np.isnan(rho[1])] == 0.0).all()


@pytest.mark.parametrize("which", ["ref", "product"])
def test_roi_growth_on_hand_made_windows(hm, which):
    from hydra_mi import roi
    grow = ref.grow if which == "ref" else roi.grow
    rois = ref.rois if which == "ref" else roi.assign
    rho = np.zeros((7, 7))
    rho[3, 3] = rho[3, 4] = rho[2, 4] = 0.9                     # connected through (3, 4)
    rho[1, 5] = 0.9                                             # touches (2, 4) by a corner only
    rho[5, 5] = np.nan
    g = grow(rho, 0.5)
    assert g.sum() == 3 and g[3, 3] and g[3, 4] and g[2, 4] and not g[1, 5]
    rho[3, 3] = 0.4                                             # the seed's own pixel below thr: nothing grows
    assert not grow(rho, 0.5).any()
    rho[3, 3] = np.nan
    assert not grow(rho, 0.5).any()
    # two seeds 4 px apart whose windows both cover the pixels between them; seed 2 is below thr and keeps its disc
    H, W, R = 20, 24, 3
    m = np.ones((H, W), bool)
    m[0, :] = False
    seeds = np.array([[8, 9], [12, 9], [19, 1]])
    win = np.zeros((3, 7, 7))
    win[0, 3, 3:7] = 0.8                                        # seed 0 reaches columns 8..11 of row 9
    win[1, 3, 0:4] = 0.8                                        # seed 1 reaches columns 9..12
    win[2] = 0.1
    labels, counts, fallback = rois(win, 0.5, m, seeds, R, 1.0)
    assert labels[9, 8:13].tolist() == [0, 0, 0, 1, 1]          # column 10 is 2 px from both: the lower index
    assert counts.tolist() == [3, 2, 4] and fallback.tolist() == [False, False, True]
    assert labels[1, 18:21].tolist() == [2, 2, 2] and labels[2, 19] == 2 and labels[0, 19] == -1     # the disc, map pixels only
    assert (labels >= 0).sum() == 9
    w, ring_counts, Rg = (ref.ring_weights if which == "ref" else roi.ring_weights)(labels, m, seeds, 2.0, 3.0)
    assert Rg == 3 and w.shape == (3, 7, 7) and w.dtype == np.uint16
    assert w[0, 3, 5] == 0 and w[0, 3, 6] == 0                  # (9, 10) and (9, 11) are ROI pixels: out of every ring
    assert w[0, 3, 0] == 1 and w[0, 3, 1] == 1 and w[0, 3, 2] == 0
    assert ring_counts[0] == w[0].sum() and w[2, 0].sum() == 0  # rows above the frame


def test_percentile_baseline_on_a_hand_made_trace(hm):
    from hydra_mi import roi
    x = np.array([5.0, 1.0, 4.0, 2.0, 3.0, 9.0, 0.0])
    for f in (ref.baseline, roi.baseline):
        b = f(x, 50.0, 1)
        assert b.tolist() == [3.0, 4.0, 2.0, 3.0, 3.0, 3.0, 4.5]      # medians of 2 values at the ends, of 3 inside
        b = f(x, 10.0, 2)
        want = [np.percentile(x[max(0, k - 2):k + 3], 10.0) for k in range(7)]
        assert np.array_equal(b, np.array(want))
        assert b[0] == 1.0 + 0.2 * (4.0 - 1.0)                        # sorted 1, 4, 5: position 0.2
        assert f(x, 10.0, 100).tolist() == [np.percentile(x, 10.0)] * 7


def test_overflow_bound_and_empty_ring():
    assert ref.overflow_bound(300, 29, 116) < 2 ** 63
    assert ref.overflow_bound(1 << 20, 3000, 3000) >= 2 ** 63
    v, m, seeds = _small_video(2)
    m2 = np.zeros_like(m)
    m2[7, 8] = True                                              # the seed's pixel alone in the map
    ss = ref.seed_sums(v, m2, seeds[:1], 2.0, 3.0, 5.0, 3)
    assert ss["n_T"][0] == 1 and ss["n_G"][0] == 0 and not ss["G"].any() and not ss["U"].any()
    assert (ref.footprints(ss, v.shape[0], m2, seeds[:1], 3)[0, 3, 3]) == 0.0


@pytest.mark.parametrize("seed", range(6))
def test_planted_video_needs_the_ring_and_is_cured_by_it(hm, seed):
    """The planted video with neuropil (roi_ref.planted_video: 12 elliptical cells of sigma 1.5..2.5 px, amplitude 50, a
    frame-wide AR(1) signal of 0..30 grey levels, 300 frames), seeds at the planted centres, alpha = 1.

    Measured on the restatement over the six seeds: the lowest footprint value within 2 px of a planted centre is
    0.542..0.664, the highest on ring pixels (6 <= d <= 8.5) 0.250..0.401; thr = 0.47 lies halfway between 0.542 and
    0.401.  (With sigmas up to 3 px the two were 0.558 and 0.517, a gap below 0.05: the largest sigma is 2.5.)
    The need: the uncorrected radius-3 disc trace correlates with the planted activity at 0.687..0.805 in the worst cell
    (< 0.85).  The cure: the corrected ROI trace at 0.9888..0.9923 in the worst cell; the bound is 0.9888 - 0.02.  Every
    cell gets an ROI of its own (20..64 pixels), none falls back to its disc."""
    from hydra_mi import roi
    v, cs, act, _ = ref.planted_video(seed)
    m = ref.planted_map()
    F = v.shape[0]
    e = ref.extract(v, m, cs, thr=THR, alpha=1.0)
    rho = e["footprints"]
    d = np.arange(-8, 9)
    d2 = d[None, :] ** 2 + d[:, None] ** 2
    lo = min(rho[s][d2 <= 4].min() for s in range(12))
    hi = max(rho[s][(d2 >= 36) & (d2 <= 72.25)].max() for s in range(12))
    ss = ref.seed_sums(v, m, cs, 3.0, 6.0, 8.5, 8)
    disc = ss["T"].astype(np.float64) / ss["n_T"]
    need = min(np.corrcoef(disc[:, s], act[s])[0, 1] for s in range(12))
    F_c = e["F_roi"] - e["F_np"]
    cure = min(np.corrcoef(F_c[:, s], act[s])[0, 1] for s in range(12))
    dff = min(np.corrcoef(e["dff"][:, s], act[s])[0, 1] for s in range(12))
    print("seed %d: lowest rho within 2 px %.3f, highest on the ring %.3f; disc trace %.4f, corrected ROI trace %.4f, "
          "dF/F %.4f; ROIs of %d..%d pixels" % (seed, lo, hi, need, cure, dff, e["roi_counts"].min(), e["roi_counts"].max()))
    assert hi + 0.025 <= THR <= lo - 0.025                      # the gap is at least 0.05 and thr is inside it
    assert need < 0.85
    assert cure > BOUND
    assert not e["seed_fallback"].any() and (e["roi_counts"] >= 5).all()
    assert sorted(np.unique(e["roi_labels"][e["roi_labels"] >= 0]).tolist()) == list(range(12))
    assert all(e["roi_labels"][r, c] == s for s, (c, r) in enumerate(cs))
    assert np.isfinite(e["dff"]).all() and roi.DEFAULT_THR == THR
    # the host arithmetic of the product on the same sums: bit for bit
    got = roi.footprints(ss, F, m, cs, 8)
    assert np.array_equal(_bits(got), _bits(rho))
    labels, counts, fb = roi.assign(got, THR, m, cs, 8, 3.0)
    assert np.array_equal(labels, e["roi_labels"]) and np.array_equal(counts, e["roi_counts"]) and not fb.any()
    w, rc, Rg = roi.ring_weights(labels, m, cs, 6.0, 8.5)
    assert np.array_equal(rc, e["ring_counts"]) and Rg == 8
