"""Masks shared by the CPU and GPU tests of the reference's contour pruning (imgproc.py:198-228)."""
import numpy as np


def blobs(rng, H, W, k, specks=0.01):
    """a random mask of k soft blobs with pinholes and specks (the fraction `specks` of pixels flipped)"""
    yy, xx = np.mgrid[:H, :W]
    f = np.zeros((H, W))
    for _ in range(k):
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(4, 0.3 * min(H, W))
        f += np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r)) * rng.uniform(0.5, 1.5)
    m = f > rng.uniform(0.5, 0.9)
    m ^= rng.random((H, W)) < specks                                 # pinholes in the objects, specks outside
    for _ in range(3):                                              # a few larger holes, some with something inside
        cx, cy, a, b = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(3, 10)), int(rng.integers(3, 10))
        m[max(0, cy - b):cy + b, max(0, cx - a):cx + a] = False
        if rng.random() < 0.5:
            m[cy:cy + 2, cx:cx + 2] = True
    return m


# ---- structures placed against the 64 x 16 tiles of the device labelling (k_ccl_local / k_ccl_border) ----------------
# Every generator takes the frame size and an anchor (Y, X) -- a tile corner (Y % 16 == 0, X % 64 == 0) or a point
# shifted from one -- and returns the mask, or None when the structure does not fit the frame around that anchor.
TW, TH = 64, 16


def _canvas(H, W, y0, y1, x0, x1, margin=1):
    """an empty H x W mask if rows [y0, y1) and columns [x0, x1) lie inside the frame with `margin` pixels to spare"""
    if y0 < margin or x0 < margin or y1 > H - margin or x1 > W - margin:
        return None
    return np.zeros((H, W), bool)


def diag_corner(H, W, Y, X, flip=False):
    """two unequal blocks meeting only in the diagonal pair (Y-1, X-1) / (Y, X) -- (Y-1, X) / (Y, X-1) with flip -- at a
    tile corner: NW / NE unions across both seams at once; one object"""
    m = _canvas(H, W, Y - 6, Y + 5, X - 12, X + 12)
    if m is None:
        return None
    if not flip:
        m[Y - 6:Y, X - 10:X] = True
        m[Y:Y + 5, X:X + 12] = True
    else:
        m[Y - 6:Y, X:X + 10] = True
        m[Y:Y + 5, X - 12:X] = True
    return m


def diag_vseam(H, W, Y, X, flip=False):
    """the same diagonal join down a vertical seam, 8 rows below a tile's top row (the left / right column's NW / NE
    unions of k_ccl_border, not the top row's)"""
    y = Y + 8
    m = _canvas(H, W, y - 6, y + 5, X - 12, X + 12)
    if m is None:
        return None
    if not flip:
        m[y - 6:y, X - 10:X] = True
        m[y:y + 5, X:X + 12] = True
    else:
        m[y - 6:y, X:X + 10] = True
        m[y:y + 5, X - 12:X] = True
    return m


def bg_diag_corner(H, W, Y, X, big=False, flip=False):
    """background meeting only diagonally at a tile corner: a hole ending in (Y-1, X-1) and a 1-px channel from (Y, X)
    down to the outside (mirrored with flip).  Background is 4-connected: the hole stays a hole -- filled (3 x 4, area
    18) or kept (6 x 10, area 75 with big)"""
    m = _canvas(H, W, Y - 8, Y + 7, X - 14, X + 14)
    if m is None:
        return None
    m[Y - 8:Y + 7, X - 14:X + 14] = True
    h, w = (6, 10) if big else (3, 4)
    if not flip:
        m[Y - h:Y, X - w:X] = False
        m[Y:Y + 7, X] = False
    else:
        m[Y - h:Y, X:X + w] = False
        m[Y:Y + 7, X - 1] = False
    return m


def bridge_vseam(H, W, Y, X):
    """two blocks joined by a 1-px horizontal bridge across a vertical seam, 6 rows below a tile's top row"""
    m = _canvas(H, W, Y + 2, Y + 12, X - 15, X + 14)
    if m is None:
        return None
    m[Y + 2:Y + 12, X - 15:X - 3] = True
    m[Y + 4:Y + 10, X + 3:X + 14] = True
    m[Y + 6, X - 3:X + 3] = True
    return m


def bridge_hseam(H, W, Y, X):
    """two blocks joined by a 1-px vertical bridge across a row seam (away from the vertical seams)"""
    m = _canvas(H, W, Y - 7, Y + 7, X + 14, X + 30)
    if m is None:
        return None
    m[Y - 7:Y - 3, X + 14:X + 30] = True
    m[Y + 3:Y + 7, X + 16:X + 26] = True
    m[Y - 3:Y + 3, X + 20] = True
    return m


def corridor(H, W, Y, X, vertical=True):
    """a pocket (3 x 5, area 22) whose only way out is a 1-px background corridor across a seam: a row seam (vertical
    corridor up to the object's top) or a vertical seam (horizontal corridor out to its right side).  The pocket is
    outside, not a hole that would be filled"""
    if vertical:
        m = _canvas(H, W, Y - 7, Y + 7, X - 14, X + 14)
        if m is None:
            return None
        m[Y - 7:Y + 7, X - 14:X + 14] = True
        m[Y + 1:Y + 4, X - 5:X] = False
        m[Y - 7:Y + 1, X - 3] = False
    else:
        m = _canvas(H, W, Y + 1, Y + 15, X - 20, X + 8)
        if m is None:
            return None
        m[Y + 1:Y + 15, X - 20:X + 8] = True
        m[Y + 5:Y + 10, X - 12:X - 9] = False
        m[Y + 7, X - 9:X + 8] = False
    return m


def serpentine(H, W, Y, X, w=1, g=1, n=None):
    """stripes 15 px high and w px wide, g apart, across the row seam Y (rows Y-8 .. Y+6), joined alternately at their
    top (the tile above) and bottom (the tile below): one object, but within a tile only pairs of stripes are joined --
    the rest is a chain of unions across the seam, also across the vertical seam X"""
    n = n or 2 * (30 // (w + g))
    x0 = X - (n // 2) * (w + g)
    x1 = x0 + n * (w + g) - g
    m = _canvas(H, W, Y - 8, Y + 7, x0, x1)
    if m is None:
        return None
    for i in range(n):
        a = x0 + i * (w + g)
        m[Y - 8:Y + 7, a:a + w] = True
        if i + 1 < n:
            m[Y - 8 if i % 2 == 0 else Y + 6, a + w:a + w + g] = True
    return m


def comb(H, W, Y, X, tw=1, tg=1, kind="down", transpose=False):
    """teeth tw wide and tg apart across the row seam Y: kind "down" hangs them from a spine in the tile above (free
    below), "up" stands them on a spine in the tile below, "closed" has both spines (the gaps are small holes, filled).
    Along the tile's top row object and background alternate, the label pairs repeating with interruptions (the `dup`
    shortcuts of k_ccl_border).  transpose: the same across the vertical seam X (teeth along rows, the W unions down a
    tile's left side)"""
    L = 40                                                       # the spines' length, centred on the seam crossing
    if transpose:
        m = _canvas(H, W, Y + 16 - L // 2 - 8, Y + 16 + L // 2 - 8, X - 4, X + 7)
    else:
        m = _canvas(H, W, Y - 4, Y + 7, X - L // 2, X + L // 2)
    if m is None:
        return None
    t = np.zeros((11, L), bool)                                  # rows: seam - 4 .. seam + 6, the seam at t-row 4
    if kind in ("down", "closed"):
        t[0:2] = True
    if kind in ("up", "closed"):
        t[9:11] = True
    for a in range(1, L - 1, tw + tg):
        t[2:9, a:a + tw] = True
    if transpose:
        y0 = Y + 16 - L // 2 - 8
        m[y0:y0 + L, X - 4:X + 7] = t.T
    else:
        m[Y - 4:Y + 7, X - L // 2:X + L // 2] = t
    return m


def checker(H, W, Y, X, parity=0):
    """a 10 x 12 checkerboard patch around a tile corner: the object is connected only through diagonals, every
    background cell inside is a 1-px hole (filled)"""
    m = _canvas(H, W, Y - 5, Y + 5, X - 6, X + 6)
    if m is None:
        return None
    yy, xx = np.mgrid[Y - 5:Y + 5, X - 6:X + 6]
    m[Y - 5:Y + 5, X - 6:X + 6] = (yy + xx) % 2 == parity
    return m


def hole_threshold(H, W, Y, X, a2=80):
    """an object with one hole straddling a tile corner, of doubled area (Pick: 2 I + R - 2) exactly a2:
    80 = 5 x 6 (I 30, R 22: kept), 79 = 5 x 6 with one pixel added above and the opposite corner removed (I 30, R 21:
    filled), 78 = 5 x 6 without the middle pixel of its top side (I 29, R 22: filled)"""
    m = _canvas(H, W, Y - 7, Y + 7, X - 9, X + 9)
    if m is None:
        return None
    m[Y - 7:Y + 7, X - 9:X + 9] = True
    m[Y - 2:Y + 3, X - 3:X + 3] = False
    if a2 == 79:
        m[Y - 3, X - 1] = False
        m[Y + 2, X + 2] = True
    elif a2 == 78:
        m[Y - 2, X - 1] = True
    else:
        assert a2 == 80
    return m


def object_threshold(H, W, Y, X, a2=80):
    """the only object, straddling a tile corner: 6 x 9 (doubled area 2 x 5 x 8 = 80: kept) or 6 x 9 without a corner
    (79: nothing is kept)"""
    m = _canvas(H, W, Y - 3, Y + 3, X - 4, X + 5)
    if m is None:
        return None
    m[Y - 3:Y + 3, X - 4:X + 5] = True
    if a2 == 79:
        m[Y + 2, X + 4] = False
    else:
        assert a2 == 80
    return m


def tie(H, W, Y, X):
    """two 6 x 9 objects of area 40: P (rows Y-6 .., columns X+2 ..) comes first in raster order, Q (rows Y-4 ..,
    columns X-12 .., across the row seam) first in x.  P is kept"""
    m = _canvas(H, W, Y - 6, Y + 2, X - 12, X + 11)
    if m is None:
        return None
    m[Y - 6:Y, X + 2:X + 11] = True
    m[Y - 4:Y + 2, X - 12:X - 3] = True
    return m


def frame_edge(H, W, kind="pockets"):
    """contact with the frame's last column and row (partial last tiles when W % 64, H % 16 are not 0).
    "pockets": a block in the bottom-right corner with a background pocket open to x = W-1 and one open to y = H-1
    (outside, not holes that would be filled); "tie_before": a 6 x 9 object in the corner (area 40: its pixels on the
    frame edge are border pixels) against an equal one further left in the same rows, which is first in raster order and
    kept; "tie_after": against a 5 x 11 one (area 40 too) a row lower: the corner one is kept"""
    if kind == "pockets":
        if H < 14 or W < 16:
            return None
        m = np.zeros((H, W), bool)
        m[H - 12:H, W - 14:W] = True
        m[H - 8:H - 5, W - 3:W] = False
        m[H - 3:H, W - 10:W - 7] = False
        return m
    if H < 8 or W < 32:
        return None
    m = np.zeros((H, W), bool)
    m[H - 6:H, W - 9:W] = True
    if kind == "tie_before":
        m[H - 6:H, W - 30:W - 21] = True
    else:
        assert kind == "tie_after"
        m[H - 5:H, W - 30:W - 19] = True
    return m


def _rings(m, y0, x0, k=40, S=160):
    """k concentric square outlines, 1 px wide and 2 px apart, the outermost S px across: 2 k levels of nesting"""
    for i in range(k):
        a, b, e = x0 + 2 * i, y0 + 2 * i, S - 1 - 4 * i
        m[b, a:a + e + 1] = m[b + e, a:a + e + 1] = True
        m[b:b + e + 1, a] = m[b:b + e + 1, a + e] = True


def deep_rings(H, W, Y=0, X=0):
    """object A: 40 concentric outlines 160 px across (the innermost pixels 80 components deep; doubled area 2 x 159^2 =
    50562), object B: a solid 159 x 159 square (2 x 158^2 = 49928).  A is kept: its outermost outline (what lies inside
    it is a kept hole)"""
    m = _canvas(H, W, Y + 20, Y + 184, X + 10, X + 349)
    if m is None:
        return None
    _rings(m, Y + 20, X + 10)
    m[Y + 25:Y + 184, X + 190:X + 349] = True
    return m


def deep_in_hole(H, W, Y=0, X=0):
    """object A: a 176 x 176 square with a 168 x 168 hole around the same 40 outlines (doubled area 2 x 175^2 = 61250,
    to which the pixels 64 and more levels below it -- on and inside the 32nd outline -- add 2 x 36^2 = 2592), object B: a solid
    173 x 173 square (2 x 172^2 = 59168).  A is kept with its hole (everything in it goes)"""
    m = _canvas(H, W, Y + 4, Y + 180, X + 4, X + 362)
    if m is None:
        return None
    m[Y + 4:Y + 180, X + 4:X + 180] = True
    m[Y + 8:Y + 176, X + 8:X + 176] = False
    _rings(m, Y + 12, X + 12)
    m[Y + 6:Y + 179, X + 188:X + 361] = True
    return m


def seam_cases(H, W, Y, X):
    """{name: mask} of every structure above that fits around the anchor (Y, X)"""
    gens = {
        "diag_corner": lambda: diag_corner(H, W, Y, X),
        "diag_corner_flip": lambda: diag_corner(H, W, Y, X, flip=True),
        "diag_vseam": lambda: diag_vseam(H, W, Y, X),
        "diag_vseam_flip": lambda: diag_vseam(H, W, Y, X, flip=True),
        "bg_diag": lambda: bg_diag_corner(H, W, Y, X),
        "bg_diag_flip": lambda: bg_diag_corner(H, W, Y, X, flip=True),
        "bg_diag_big": lambda: bg_diag_corner(H, W, Y, X, big=True),
        "bg_diag_big_flip": lambda: bg_diag_corner(H, W, Y, X, big=True, flip=True),
        "bridge_vseam": lambda: bridge_vseam(H, W, Y, X),
        "bridge_hseam": lambda: bridge_hseam(H, W, Y, X),
        "corridor_v": lambda: corridor(H, W, Y, X),
        "corridor_h": lambda: corridor(H, W, Y, X, vertical=False),
        "serpentine_1_1": lambda: serpentine(H, W, Y, X, 1, 1),
        "serpentine_2_1": lambda: serpentine(H, W, Y, X, 2, 1),
        "serpentine_1_2": lambda: serpentine(H, W, Y, X, 1, 2),
        "serpentine_2_2": lambda: serpentine(H, W, Y, X, 2, 2),
        "checker_0": lambda: checker(H, W, Y, X, 0),
        "checker_1": lambda: checker(H, W, Y, X, 1),
        "hole_80": lambda: hole_threshold(H, W, Y, X, 80),
        "hole_79": lambda: hole_threshold(H, W, Y, X, 79),
        "hole_78": lambda: hole_threshold(H, W, Y, X, 78),
        "object_80": lambda: object_threshold(H, W, Y, X, 80),
        "object_79": lambda: object_threshold(H, W, Y, X, 79),
        "tie": lambda: tie(H, W, Y, X),
    }
    for kind in ("down", "up", "closed"):
        for tw, tg in ((1, 1), (2, 1), (1, 2), (3, 2)):
            for tr in (False, True):
                gens["comb_%s_%d_%d%s" % (kind, tw, tg, "_T" if tr else "")] = (
                    lambda kind=kind, tw=tw, tg=tg, tr=tr: comb(H, W, Y, X, tw, tg, kind, tr))
    out = {}
    for name, g in gens.items():
        m = g()
        if m is not None:
            out[name] = m
    return out


def anchors(H, W, shifts=((0, 0), (1, 1), (-1, -1), (5, 33))):
    """tile corners inside the frame (the first, one in the middle, the last) and the frame's centre, each also shifted
    off the grid"""
    ys = list(range(TH, H, TH)) or [H // 2]
    xs = list(range(TW, W, TW)) or [W // 2]
    points = {(ys[0], xs[0]), (ys[len(ys) // 2], xs[len(xs) // 2]), (ys[-1], xs[-1]), (H // 2, W // 2)}
    return [(y + dy, x + dx) for y, x in sorted(points) for dy, dx in shifts]
