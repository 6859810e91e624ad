"""The rules of the 16-bit input (include/hydra_mi.h, "16-bit input") restated in loops and Python integers: the histogram,
the window, the table and the mapping of a frame.  Slow and plain on purpose; hydra_mi.deepio and the device are held to it."""
import math

VALUES = 65536
MILLION = 10 ** 6


def swapped(v):
    """the two bytes of a 16-bit value exchanged"""
    return ((v & 0xff) << 8) | (v >> 8)


def histogram(frames, swap=0):
    """frames: any nesting of lists (or arrays) of 16-bit values -> h[v] as a list of Python integers"""
    h = [0] * VALUES

    def walk(x):
        if hasattr(x, "__len__"):
            for y in x:
                walk(y)
        else:
            v = int(x)
            h[swapped(v) if swap else v] += 1
    walk(frames)
    return h


def window(hist, lo_ppm=1000, hi_ppm=999990):
    N = 0
    for c in hist:
        N += int(c)
    assert N >= 1
    below = N * lo_ppm // MILLION
    need = max(1, (N * hi_ppm + MILLION - 1) // MILLION)
    lo = hi = None
    cum = 0
    for v in range(VALUES):
        cum += int(hist[v])
        if lo is None and cum > below:
            lo = v
        if hi is None and cum >= need:
            hi = v
    if lo is None:                      # lo_ppm = 10^6: no value has more than all pixels at or below it
        lo = VALUES - 1
    if hi <= lo:
        hi = lo + 1
        if hi > VALUES - 1:
            lo, hi = VALUES - 2, VALUES - 1
    return lo, hi


def make_lut(lo, hi, gamma=1.0):
    assert 0 <= lo < hi <= VALUES - 1
    D = hi - lo
    lut = []
    for v in range(VALUES):
        t = min(max(v, lo), hi) - lo
        if gamma == 1.0:
            lut.append((510 * t + D) // (2 * D))
        else:
            lut.append(int(math.floor(255.0 * (t / D) ** gamma + 0.5)))
    return lut


def map_frame(frame, lut, lo, hi, threshold, swap=0):
    """frame: a flat sequence of 16-bit values -> (raw, mask, shown, [below lo, above hi]), lists"""
    raw, mask, shown = [], [], []
    below = above = 0
    for x in frame:
        v = swapped(int(x)) if swap else int(x)
        below += v < lo
        above += v > hi
        r = lut[min(max(v, lo), hi)]
        m = 1 if r > threshold else 0
        raw.append(r)
        mask.append(m)
        shown.append(r if m else 0)
    return raw, mask, shown, [below, above]
