"""Inputs for the tests of hm_body_rec_waves: the trigger frames of a window and a video with a pulse planted for each on
the left half of a map, shaped so that every code of the rule occurs (tests/test_waves_gpu.py records it on the scenes of
bodystats_cases; tests/test_waves_cpu.py checks the plan on a map of its own)."""
import numpy as np

F = 40
WINDOWS = ((1, 0, 1), (5, 3, 10), (16, 0, 8))          # (pre, lead, post)
BINS = (0, 1, 3, 8)
MIN_RISE = 30
HEIGHT = 120


def triggers(pre, lead, post, frames=F):
    """The earliest admissible trigger, the latest, two with overlapping windows, the first of those again -> int32 (5,)"""
    first, last = lead + pre, frames - 1 - post
    mid = (first + last) // 2
    return np.array([first, last, mid, mid + 1, mid], np.int32)


def pulse(o, d, frames=F):
    """0 before frame o, then HEIGHT reached in d equal steps (at frame o + d - 1), then 0 again: short enough that the
    running median of five frames (kind 3 with half 2, q 50) stays below it"""
    k = np.arange(frames)
    return np.where((k >= o) & (k < o + d), HEIGHT * (k - o + 1) // d, 0)


def video(m, pre, lead, post, seed, frames=F):
    """m (H, W) bool: where pulses may be planted (the map, or a guess of it) -> (frames, H, W) uint8: random levels 0..3
    times 8 everywhere, and on the left half of m's columns a pulse for each of the first three triggers:
      the earliest   a jump to HEIGHT at the first search frame: at half height when the search starts (code 3)
      the latest     a jump to HEIGHT at the last search frame: still rising at the window's end (code 1)
      the middle one a wave: the pulse starts a frame later every eighth column and row, and ends inside the window
                     where the window has room for that (code 0); else as the latest
    The fourth trigger, a frame after the middle one, sees the same wave a frame earlier (where it starts with the search:
    code 3), the fifth repeats the third.  Where pulses overlap the larger value stands."""
    m = np.asarray(m, bool)
    H, W = m.shape
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 4, (frames, H, W)) * 8
    cols = np.flatnonzero(m.any(0))
    half = np.zeros((H, W), bool)
    if len(cols):
        half[:, :(int(cols[0]) + int(cols[-1]) + 2) // 2] = True          # (an odd number of columns: the middle one too)
    half &= m
    t = triggers(pre, lead, post, frames)
    d = min(post, 2)
    plant = np.zeros((frames, H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for j, tj in enumerate(t[:3]):
        kb, kc = int(tj) - lead, int(tj) + post
        if j == 0:
            o, dd = np.full((H, W), kb), 1
        elif j == 1 or kb + 1 > kc - d:
            o, dd = np.full((H, W), kc), 1
        else:
            o, dd = kb + 1 + (xx // 8 + yy // 8) % (kc - d - kb), d
        for oo in np.unique(o):
            plant = np.maximum(plant, pulse(int(oo), dd, frames)[:, None, None] * (half & (o == oo))[None])
    return (v + plant).astype(np.uint8)
