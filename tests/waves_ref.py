"""The rule of hm_body_rec_waves (include/hydra_mi.h) restated in NumPy and Python integers, from the header's text alone:
the binned planes, the latency, rise and code per event and pixel, the count and sums over the events, the nine sums of
the local fit per event and node, and hydra_mi.waves.velocity's closed form in Python floats.  Slow and plain on purpose."""
import numpy as np

NONE = -(1 << 31)


def box(m):
    """(c0, r0, bw, bh) of the map's bounding box; an empty map: the pixel (0, 0)"""
    m = np.asarray(m, bool)
    if not m.any():
        return 0, 0, 1, 1
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    return int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)


def nodes(m, step):
    """(nx, ny, c0, r0) of the fit's grid"""
    c0, r0, bw, bh = box(m)
    return -(-bw // step), -(-bh // step), c0, r0


def binned(planes, m, b):
    """planes (F, H, W) uint8, the map m (H, W) bool -> (Y (F, H, W) int64, n (H, W) int64): the sums of the planes and the
    count over the pixels of the (2b+1)^2 window that are on the frame and in the map (in the map is in the box)"""
    y = np.asarray(planes).astype(np.int64) * m[None]
    F, H, W = y.shape
    yp = np.zeros((F, H + 2 * b, W + 2 * b), np.int64)
    mp = np.zeros((H + 2 * b, W + 2 * b), np.int64)
    yp[:, b:b + H, b:b + W] = y
    mp[b:b + H, b:b + W] = m
    Y, n = np.zeros((F, H, W), np.int64), np.zeros((H, W), np.int64)
    for dy in range(2 * b + 1):
        for dx in range(2 * b + 1):
            Y += yp[:, dy:dy + H, dx:dx + W]
            n += mp[dy:dy + H, dx:dx + W]
    return Y, n


def event(Y, n, m, t, pre, lead, post, min_rise):
    """One event at trigger t -> (lat, rise int32, why uint8), each (H, W)"""
    F, H, W = Y.shape
    t = int(t)
    kb, kc = t - lead, t + post
    assert kb - pre >= 0 and kc <= F - 1
    S = Y[kb - pre:kb].sum(0)
    search = Y[kb:kc + 1]
    M = search.max(0)
    kM = kb + search.argmax(0)                       # (argmax: the first)
    R = pre * M - S
    theta = S + pre * M
    crossed = 2 * pre * search >= theta[None]
    has = crossed.any(0)
    kx = kb + crossed.argmax(0)                      # (the first True; kb where there is none: those end as code 2)
    lat = np.full((H, W), NONE, np.int64)
    why = np.full((H, W), 255, np.int64)
    rise = np.where(m, R, 0)
    for r, c in zip(*np.nonzero(m)):
        if R[r, c] < pre * n[r, c] * min_rise:
            why[r, c] = 2
        elif kx[r, c] == kb:
            assert has[r, c]
            why[r, c] = 3
        else:
            assert has[r, c]
            k = int(kx[r, c])
            y0, y1 = int(Y[k - 1, r, c]), int(Y[k, r, c])
            d0 = int(theta[r, c]) - 2 * pre * y0
            d1 = 2 * pre * (y1 - y0)
            assert d1 >= d0 > 0
            frac = (256 * d0) // d1
            assert 0 <= frac <= 256
            lat[r, c] = 256 * (k - 1 - t) + frac
            why[r, c] = 1 if kM[r, c] == kc else 0
    return lat.astype(np.int32), rise.astype(np.int32), why.astype(np.uint8)


def fit_sums(lat, m, step, Rf):
    """lat (H, W) of one event -> (nodes, 9) int64: n, sum dx, dy, dx^2, dx dy, dy^2, Lat, dx Lat, dy Lat over the valid
    pixels within Rf of every node, nodes row-major"""
    H, W = lat.shape
    nx, ny, c0, r0 = nodes(m, step)
    jj, ii = np.divmod(np.arange(nx * ny), nx)
    cx, cy = c0 + ii * step, r0 + jj * step
    L = lat.astype(np.int64)
    out = np.zeros((nx * ny, 9), np.int64)
    for dy in range(-Rf, Rf + 1):
        for dx in range(-Rf, Rf + 1):
            x, y = cx + dx, cy + dy
            on = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            v = np.where(on, L[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], NONE)
            ok = (v != NONE).astype(np.int64)
            v = v * ok
            out += np.stack((ok, ok * dx, ok * dy, ok * dx * dx, ok * dx * dy, ok * dy * dy, v, v * dx, v * dy), 1)
    return out


def waves(planes, m, trig, b, pre, lead, post, min_rise, step, Rf, binned_planes=None):
    """Every output of hm_body_rec_waves for the planes (F, H, W) of the kind asked for -> dict"""
    m = np.asarray(m, bool)
    Y, n = binned(planes, m, b) if binned_planes is None else binned_planes
    H, W = m.shape
    E = len(trig)
    lat, rise, why = np.empty((E, H, W), np.int32), np.empty((E, H, W), np.int32), np.empty((E, H, W), np.uint8)
    for e, t in enumerate(trig):
        lat[e], rise[e], why[e] = event(Y, n, m, t, pre, lead, post, min_rise)
    ok = why <= 1
    assert np.array_equal(ok, lat != NONE)
    L = np.where(ok, lat.astype(np.int64), 0)
    return dict(n_bin=np.where(m, n, 0).astype(np.uint16), lat=lat, rise=rise, why=why, cnt=ok.sum(0).astype(np.uint32),
                sum_lat=L.sum(0), sum_lat2=(L * L).sum(0), fit=np.stack([fit_sums(lat[e], m, step, Rf) for e in range(E)]))


def velocity(fit, n_min):
    """hydra_mi.waves.velocity in Python integers and floats, a node at a time -> (g, v), each (..., 2)"""
    f = np.asarray(fit).reshape(-1, 9)
    g, v = np.full((len(f), 2), np.nan), np.full((len(f), 2), np.nan)
    for i, row in enumerate(f):
        n, sx, sy, sxx, sxy, syy, sl, sxl, syl = (int(x) for x in row)
        a11, a12, a22 = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
        b1, b2 = n * sxl - sx * sl, n * syl - sy * sl
        a11, a12, a22, b1, b2 = float(a11), float(a12), float(a22), float(b1), float(b2)
        det = a11 * a22 - a12 * a12
        if n < n_min or not det > 0.0:
            continue
        gx = ((a22 * b1 - a12 * b2) / det) / 256.0
        gy = ((a11 * b2 - a12 * b1) / det) / 256.0
        s = gx * gx + gy * gy
        if not s > 0.0:
            continue
        g[i] = gx, gy
        v[i] = gx / s, gy / s
    shape = np.asarray(fit).shape[:-1] + (2,)
    return g.reshape(shape), v.reshape(shape)
