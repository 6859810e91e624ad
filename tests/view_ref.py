"""NumPy restatement of the tracker's views (include/hydra_mi.h: hm_view, hm_view_forces, hm_flow_preview).

The renders themselves come from Renderer.render(), which the other tests pin to the oracle; this file restates only
what the views add: the wireframe and arrow segments, the mask palette, the flow normalisation and the colour wheel.
All views are (H, W, 3) uint8, B G R.
"""
import numpy as np

COORD_MAX = 1048576.0
HEAD_K = 0.070710678118654752          # 0.1 sqrt(1/2), the same binary64 number as VIEW_HEAD_K


def segment(x0, y0, x1, y1, W, H):
    """pixel indices (row-major) of the segment, i = 0..n: x0 + floor((2 i dx + n) / (2 n)); outside pixels dropped"""
    dx, dy = int(x1) - int(x0), int(y1) - int(y0)
    n = max(abs(dx), abs(dy))
    i = np.arange(n + 1, dtype=np.int64)
    if n == 0:
        x = np.array([int(x0)], np.int64)
        y = np.array([int(y0)], np.int64)
    else:
        x = int(x0) + (2 * i * dx + n) // (2 * n)
        y = int(y0) + (2 * i * dy + n) // (2 * n)
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    return y[ok] * W + x[ok]


def _ok(*v):
    return all(-COORD_MAX <= a <= COORD_MAX for a in v)


def wire_count(tri, X, W, H):
    """per-pixel count of the wireframe: the three edges of every triangle, end points rint(vertex)"""
    P = np.rint(np.asarray(X, np.float64).reshape(-1)).reshape(-1, 2)
    count = np.zeros(W * H, np.int64)
    for t in np.asarray(tri):
        for k in range(3):
            a, b = P[t[k]], P[t[(k + 1) % 3]]
            if not _ok(a[0], a[1], b[0], b[1]):
                continue
            np.add.at(count, segment(a[0], a[1], b[0], b[1], W, H), 1)
    return count.reshape(H, W)


def _stack(b, g, r):
    return np.dstack((b, g, r)).astype(np.uint8)


def _blue(base, wire):
    return np.minimum(255, base.astype(np.int64) + 128 * wire)


def norm_plane(p):
    """floor(255 (p - min) / (max - min)) in f64, min and max over the finite pixels.  A pixel that is not finite (NaN,
    +-inf) takes no part in them and shows 0; with no finite pixel, or max == min (-0 == +0), every pixel shows 0.  No
    non-finite value is ever converted to an integer."""
    p = np.asarray(p, np.float32)
    fin = np.isfinite(p)
    out = np.zeros(p.shape, np.uint8)
    if not fin.any():
        return out
    q = p[fin].astype(np.float64)
    lo, hi = q.min(), q.max()
    if hi == lo:
        return out
    out[fin] = np.floor(255.0 * (q - lo) / (hi - lo)).astype(np.int64).astype(np.uint8)
    return out


def view(which, render, tri, X, obs=None, ids=None, wire=None):
    """render: Renderer.render() at X -> (im, fx, fy, m); obs: the observed frame (overlay);
    ids: 256 G + B of the mask palette per pixel (mask view); wire: wire_count(tri, X, W, H) where the caller has it"""
    im, fx, fy, m = render
    H, W = im.shape
    if which == "raw":
        return _stack(im, im, im)
    if which in ("flowx", "flowy"):
        v = norm_plane(fx if which == "flowx" else fy)
        return _stack(v, v, v)
    if wire is None:
        wire = wire_count(tri, X, W, H)
    if which == "texture":
        return _stack(_blue(im, wire), im, im)
    if which == "overlay":
        return _stack(_blue(np.zeros_like(im), wire), im, np.asarray(obs, np.uint8))
    if which == "mask":
        return ids_view(ids, wire, m)
    raise ValueError(which)


def ids_view(ids, wire, m):
    """The mask view of a per-pixel id image (256 G + B of the mask render, oracle/ekf_ref.render(..., labels=palette)[4]),
    the wireframe counts and the mask render m: B = min(255, id % 256 + 128 wire), G = id // 256, R = 255 where m > 0"""
    ids = np.asarray(ids, np.int64)
    assert ids.min() >= 0 and ids.max() <= 65535
    return _stack(_blue(ids % 256, np.asarray(wire, np.int64)), ids // 256, np.where(np.asarray(m) > 0, 255, 0))


def uniform_ids(m, label):
    """the mask palette's 256 G + B where every triangle carries `label` and the render covers a pixel (m > 0) once
    or more: label -1 draws (255, 255) and saturates, label 0 draws (0, 0)"""
    if label == -1:
        return np.where(m > 0, 256 * 255 + 255, 0)
    assert label == 0
    return np.zeros(m.shape, np.int64)


def arrows(img, start, end, colour):
    """one layer of plotforces: start / end (N, 2) f64, truncated as C int(); head at +-45 degrees, 0.1 of the shaft"""
    H, W = img.shape[:2]
    flat = img.reshape(-1, 3)
    for (sx, sy), (ex, ey) in zip(start, end):
        if not _ok(sx, sy, ex, ey):
            continue
        x0, y0, x1, y1 = int(sx), int(sy), int(ex), int(ey)
        dx, dy = float(x0 - x1), float(y0 - y1)
        segs = [(x0, y0, x1, y1),
                (x1, y1, x1 + int(np.rint(HEAD_K * (dx - dy))), y1 + int(np.rint(HEAD_K * (dy + dx)))),
                (x1, y1, x1 + int(np.rint(HEAD_K * (dx + dy))), y1 + int(np.rint(HEAD_K * (dy - dx))))]
        for s in segs:
            flat[segment(*s, W, H)] = colour
    return img


def forces(overlay, orig, pred, tv, fv, mv, N):
    img = (np.asarray(overlay, np.uint8) >> 1).copy()
    o, p = [np.asarray(a, np.float64).reshape(-1)[: 2 * N].reshape(-1, 2) for a in (orig, pred)]
    arrows(img, o, p, (255, 255, 255))
    for vec, colour in ((tv, (255, 0, 0)), (fv, (0, 255, 0)), (mv, (0, 0, 255))):
        v = np.asarray(vec, np.float64).reshape(-1)[: 2 * N].reshape(-1, 2)
        arrows(img, p, p + 10.0 * v, colour)
    return img


# ---- the colour wheel (Middlebury colour code: RY 15, YG 6, GC 4, CB 11, BM 13, MR 6) -----------------------------
def wheel_table():
    rows = []
    for s, n in enumerate((15, 6, 4, 11, 13, 6)):
        for k in range(n):
            up, down = 255 * k // n, 255 - 255 * k // n
            rows.append([(255, up, 0), (down, 255, 0), (0, 255, up), (0, down, 255), (up, 0, 255), (255, 0, down)][s])
    return np.array(rows, np.int64)


def wheel(fx, fy):
    """-> (.., 3) B G R uint8 of the flow at 15 px saturation"""
    fx = np.asarray(fx, np.float32)
    fy = np.asarray(fy, np.float32)
    good = np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < np.float32(1e9)) & (np.abs(fy) < np.float32(1e9))
    fx = np.where(good, fx, np.float32(0))
    fy = np.where(good, fy, np.float32(0))
    ux, uy = fx / np.float32(15), fy / np.float32(15)
    rad = np.sqrt(ux * ux + uy * uy)
    a = np.arctan2(-uy, -ux) / np.float32(np.pi)
    fk = (a + np.float32(1)) / np.float32(2) * np.float32(54)
    k0 = fk.astype(np.int64)
    k1 = (k0 + 1) % 55
    f = fk - k0.astype(np.float32)
    tab = wheel_table()
    out = np.zeros(fx.shape + (3,), np.uint8)
    for b in range(3):
        c0 = tab[k0, b].astype(np.float32) / np.float32(255)
        c1 = tab[k1, b].astype(np.float32) / np.float32(255)
        col = (np.float32(1) - f) * c0 + f * c1
        col = np.where(rad <= np.float32(1), rad * col, col * np.float32(0.75)).astype(np.float32)
        out[..., 2 - b] = (255.0 * col.astype(np.float64)).astype(np.int64).astype(np.uint8)
    out[~good] = 0
    return out


def wheel64(fx, fy):
    """The wheel once more, in binary64 throughout and with Python's own atan2, written independently of `wheel` (a
    direct table lookup per vector, no masks): what the colour code means, free of binary32 rounding.  Where `wheel`
    and the kernel differ by an ulp of atan2f, both stay within one level of this."""
    import math
    fx = np.asarray(fx, np.float32)
    fy = np.asarray(fy, np.float32)
    tab = wheel_table()
    out = np.zeros(fx.shape + (3,), np.uint8)
    for idx in np.ndindex(fx.shape):
        x, y = float(fx[idx]), float(fy[idx])
        if not (math.isfinite(x) and math.isfinite(y) and abs(x) < 1e9 and abs(y) < 1e9):
            continue
        ux, uy = x / 15.0, y / 15.0
        rad = math.sqrt(ux * ux + uy * uy)
        fk = (math.atan2(-uy, -ux) / math.pi + 1.0) / 2.0 * 54.0
        k0 = int(fk)
        f = fk - k0
        for b in range(3):
            col = (1.0 - f) * tab[k0, b] / 255.0 + f * tab[(k0 + 1) % 55, b] / 255.0
            col = rad * col if rad <= 1.0 else 0.75 * col
            out[idx + (2 - b,)] = int(255.0 * col)
    return out


def flow_preview(frames, fx, fy, wheel_fn=wheel):
    f = np.asarray(frames, np.int64)
    if f.ndim == fx.ndim:
        f = np.repeat(f[..., None], 3, axis=-1)
    w = wheel_fn(fx, fy).astype(np.int64)
    return ((2 * (2 * f + 3 * w) + 5) // 10).astype(np.uint8)
