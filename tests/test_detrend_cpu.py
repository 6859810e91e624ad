"""The running baseline per pixel, without a GPU: the restatement (tests/detrend_ref.py) against brute force, its rank
rule against np.percentile(method="lower"), what detrending is for -- the planted cells found again under drift, measured
on six seeds --, and the host logic of hydra_mi.detrend."""
import numpy as np
import pytest

import bodystats_ref as bs
import detrend_ref as ref
import roi_ref

CASES = ((0, 10), (1, 0), (2, 50), (5, 100), (14, 10), (1024, 10), (3, 37), (4, 99))


def _tiny():
    rng = np.random.default_rng(5)
    F, H, W = 11, 3, 4
    v = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    v[:, 0, 1] = rng.integers(0, 4, F) * 85                  # four grey levels: ranks fall into ties
    v[:, 1, 1] = 200                                         # a constant pixel
    v[:, 1, 2] = 0
    v[:, 2, 0] = 255
    m = np.ones((H, W), bool)
    m[2, 3] = False
    return v, m


@pytest.mark.parametrize("half, q", CASES)
def test_restatement_equals_brute_force(half, q):
    v, m = _tiny()
    F, H, W = v.shape
    floor, gain = 7, 300
    got = [ref.planes(v, m, what, half, q, floor, gain) for what in range(4)]
    assert all(g.dtype == np.uint8 and g.shape == v.shape for g in got)
    for k in range(F):
        a, b = max(0, k - half), min(F - 1, k + half)
        n = b - a + 1
        for r in range(H):
            for c in range(W):
                if not m[r, c]:
                    assert [int(g[k, r, c]) for g in got] == [0, 0, 0, 0]
                    continue
                win = sorted(int(x) for x in v[a:b + 1, r, c])
                B = win[(q * (n - 1)) // 100]
                E = max(int(v[k, r, c]) - B, 0)
                D = min(255, (gain * E) // max(B, floor))
                assert [int(g[k, r, c]) for g in got] == [int(v[k, r, c]), B, E, D], (k, r, c)


@pytest.mark.parametrize("half, q", CASES)
def test_rank_rule_is_numpys_lower_percentile(half, q):
    v, m = _tiny()
    F = v.shape[0]
    base = ref.planes(v, np.ones_like(m), 1, half, q)
    for k in range(F):
        win = v[max(0, k - half):min(F, k + half + 1)]
        assert np.array_equal(base[k], np.percentile(win, q, axis=0, method="lower").astype(np.uint8)), k
    # the rank in integers is the floor of the exact product, also where q / 100 (n - 1) rounds in binary64
    for n in range(1, 2050):
        for qq in (0, 1, 7, 10, 29, 50, 57, 99, 100):
            assert 100 * ref.rank(qq, n) <= qq * (n - 1) < 100 * (ref.rank(qq, n) + 1)


def test_floor_and_gain_at_their_limits():
    v, m = _tiny()
    for floor, gain in ((1, 1), (255, 1), (1, 65535), (255, 65535)):
        B = ref.planes(v, m, 1, 2, 10).astype(np.int64)
        E = ref.planes(v, m, 2, 2, 10).astype(np.int64)
        D = ref.planes(v, m, 3, 2, 10, floor, gain)
        assert np.array_equal(D, np.minimum(255, gain * E // np.maximum(B, floor)))
    assert D.max() == 255 and (D == 0).any()


def _scores(video, m):
    im = bs.images(*bs.accumulate(video, m), video.shape[0], m)
    return bs.peaks_fast(im[2], m, 6)


@pytest.mark.parametrize("seed", range(6))
def test_seeds_survive_the_drift_only_after_detrending(seed):
    """The table of DESIGN.md section 14, measured: the 12 best corr peaks at radius 6, a planted centre found when a
    peak lies within 2 px.  The excess video (half 20, q 10) gives all 12 back on every seed with a gap between the 12th
    and the 13th score; the raw drifting video at most 8 (measured 4..6)."""
    m = roi_ref.planted_map()
    drift, cs, clean = ref.drifting_video(seed)
    W = m.shape[1]
    row = {}
    for name, video in (("clean", clean), ("raw", drift), ("excess", ref.planes(drift, m, 2, 20, 10))):
        idx, sc = _scores(video, m)
        row[name] = (ref.seeds_found(idx[:12], W, cs), sc[11], sc[12])
    print("seed %d: " % seed + ", ".join("%s %d of 12 (12th %.3f, 13th %.3f)" % ((k,) + row[k]) for k in row))
    assert row["clean"][0] == 12
    assert row["excess"][0] == 12
    assert row["raw"][0] <= 8
    assert row["excess"][1] > row["excess"][2]


def test_block_walking(hm):
    from hydra_mi import detrend
    assert detrend.blocks(0, 5) == []
    assert detrend.blocks(5, 5) == [(0, 5)]
    assert detrend.blocks(11, 4) == [(0, 4), (4, 4), (8, 3)]
    assert detrend.blocks(3, 100) == [(0, 3)]
    for F in (1, 7, 64):
        for b in (1, 3, 64, 65):
            w = detrend.blocks(F, b)
            assert sum(n for _, n in w) == F and all(0 < n <= b for _, n in w)
            assert [k for k, _ in w] == list(np.cumsum([0] + [n for _, n in w])[:-1])
    with pytest.raises(ValueError, match="blocks of 0 frames"):
        detrend.blocks(4, 0)


def test_argument_checks_need_no_device(hm):
    from hydra_mi import detrend

    class NoKeep:
        keep = False
    for bad in (dict(half=-1), dict(half=1025), dict(q=-1), dict(q=101), dict(q=10.5)):
        with pytest.raises(ValueError, match="outside"):
            detrend.summary(NoKeep(), **bad)
        with pytest.raises(ValueError, match="outside"):
            detrend.find_points(NoKeep(), 3, **bad)
    for bad in (dict(floor=0), dict(floor=256), dict(gain=0), dict(gain=65536), dict(half=1025), dict(q=101)):
        with pytest.raises(ValueError, match="outside"):
            detrend.write_video(NoKeep(), "unused.avi", **bad)
    with pytest.raises(ValueError, match="what 'median'"):
        detrend.summary(NoKeep(), what="median")
    for call in (lambda: detrend.summary(NoKeep()), lambda: detrend.find_points(NoKeep(), 3),
                 lambda: detrend.write_video(NoKeep(), "unused.avi")):
        with pytest.raises(RuntimeError, match="without keep=True"):
            call()
