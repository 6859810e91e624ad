"""NumPy restatement of the body-frame readout (include/hydra_mi.h: hm_body_map, hm_body_warp; hydra_mi.body).

Coverage comes from oracle.ekf_ref (snap, the top-left rule, the orientation swap); this file restates what the readout
adds: the lowest covering triangle per pixel, binary64 barycentrics, the position formula, the bilinear sample and the
region sums.  NumPy evaluates a * b + c as two rounded operations, as the library (-ffp-contract=off) does.
"""
import numpy as np

from oracle import ekf_ref

SUB = ekf_ref.SUB
COORD_MAX = 1048576.0


def body_map(uv, tri, W, H):
    """-> (triangle per pixel (H, W) int64, -1: none; l1, l2 (H, W) float64; vertex ids (T, 3) after the swap)."""
    P = ekf_ref.snap(np.asarray(uv, np.float32).astype(np.float64))
    tri = np.asarray(tri, np.int64)
    out = np.full((H, W), -1, np.int64)
    l1 = np.zeros((H, W))
    l2 = np.zeros((H, W))
    ids = tri.copy()
    for t, (i0, i1, i2) in enumerate(tri):
        i0, i1, i2 = int(i0), int(i1), int(i2)
        (x0, y0), (x1, y1), (x2, y2) = P[i0], P[i1], P[i2]
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        if area < 0:
            i1, i2 = i2, i1
            (x1, y1), (x2, y2) = (x2, y2), (x1, y1)
            area = -area
        ids[t] = (i0, i1, i2)
        c_lo = max(0, int((min(x0, x1, x2) - 128) // SUB))
        c_hi = min(W - 1, int((max(x0, x1, x2) - 128) // SUB) + 1)
        r_lo = max(0, int((min(y0, y1, y2) - 128) // SUB))
        r_hi = min(H - 1, int((max(y0, y1, y2) - 128) // SUB) + 1)
        if c_lo > c_hi or r_lo > r_hi:
            continue
        px = (np.arange(c_lo, c_hi + 1, dtype=np.int64) * SUB + 128)[None, :]
        py = (np.arange(r_lo, r_hi + 1, dtype=np.int64) * SUB + 128)[:, None]
        e0 = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)
        e1 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)
        e2 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
        tl = ekf_ref._topleft
        ins = ((e0 > 0) | ((e0 == 0) & tl(x2 - x1, y2 - y1))) & \
              ((e1 > 0) | ((e1 == 0) & tl(x0 - x2, y0 - y2))) & \
              ((e2 > 0) | ((e2 == 0) & tl(x1 - x0, y1 - y0)))
        sl = (slice(r_lo, r_hi + 1), slice(c_lo, c_hi + 1))
        take = ins & (out[sl] < 0)                           # the lowest index wins
        out[sl] = np.where(take, t, out[sl])
        l1[sl] = np.where(take, e1.astype(np.float64) / np.float64(area), l1[sl])
        l2[sl] = np.where(take, e2.astype(np.float64) / np.float64(area), l2[sl])
    return out, l1, l2, ids


def positions(X, tri_of, l1, l2, ids):
    """(x, y) per pixel of the map in the frame of state X (NaN outside the map)."""
    pos = np.asarray(X, np.float64).reshape(-1)
    n = pos.shape[0] // 4                                   # X: 4N values, positions first
    P = pos[:2 * n].reshape(n, 2)
    inside = tri_of >= 0
    t = np.where(inside, tri_of, 0)
    v = ids[t]
    a, b, c = P[v[..., 0]], P[v[..., 1]], P[v[..., 2]]
    xy = (a + l1[..., None] * (b - a)) + l2[..., None] * (c - a)
    xy[~inside] = np.nan
    return xy[..., 0], xy[..., 1]


def warp(X, frame, tri_of, l1, l2, ids):
    """The registered frame (H, W) uint8."""
    frame = np.asarray(frame, np.uint8)
    H, W = frame.shape
    x, y = positions(X, tri_of, l1, l2, ids)
    with np.errstate(invalid="ignore"):
        ok = (tri_of >= 0) & (x >= -COORD_MAX) & (x <= COORD_MAX) & (y >= -COORD_MAX) & (y <= COORD_MAX)
    u = np.where(ok, x, 0.5) - 0.5
    v = np.where(ok, y, 0.5) - 0.5
    fc, fr = np.floor(u), np.floor(v)
    a, b = u - fc, v - fr
    c0, r0 = fc.astype(np.int64), fr.astype(np.int64)
    ca, cb = np.clip(c0, 0, W - 1), np.clip(c0 + 1, 0, W - 1)
    ra, rb = np.clip(r0, 0, H - 1), np.clip(r0 + 1, 0, H - 1)
    f = frame.astype(np.float64)
    f00, f01, f10, f11 = f[ra, ca], f[ra, cb], f[rb, ca], f[rb, cb]
    val = (1.0 - b) * ((1.0 - a) * f00 + a * f01) + b * ((1.0 - a) * f10 + a * f11)
    return np.where(ok, np.rint(val), 0).astype(np.uint8)


def sums(reg, keys, n):
    """uint64 sums of reg per key 0..n-1 (keys < 0: nowhere)."""
    k = np.asarray(keys).reshape(-1)
    m = k >= 0
    # (float64 weights: every partial sum is a whole number below 2^53, so exact)
    return np.bincount(k[m], weights=reg.reshape(-1)[m].astype(np.float64), minlength=n).astype(np.uint64)


def counts(keys, n):
    k = np.asarray(keys).reshape(-1)
    return np.bincount(k[k >= 0], minlength=n).astype(np.uint64)


def label_keys(labels, tri_of):
    """labels count only on pixels of the map"""
    return np.where(np.asarray(tri_of) >= 0, np.asarray(labels), -1)
