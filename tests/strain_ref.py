"""NumPy restatement of the deformation readout (include/hydra_mi.h: hm_strain_tri, hm_strain_labels, hm_view_strain;
hydra_mi.strain).

The body map, its vertex order and the triangle under an image pixel come from tests/body_ref.body_map and
tests/cellview_ref.map_at; this file restates what the readout adds: the deformation of a triangle in the order of
operations the header gives, the count-weighted traces per label, and the level, colour and blend of the view.  NumPy
evaluates a * b + c as two rounded operations, as the library (-ffp-contract=off) does, so binary64 input gives the
library's bits; the same code runs in np.longdouble when it is given that (the CPU tests measure the one against the
other).
"""
import numpy as np

import cellview_ref
import view_ref

NAMES = ("J", "l1", "l2", "c2", "s2", "rc", "rs")


def deform(U, x):
    """U (..., 3, 2) body coordinates, x (..., 3, 2) positions of the three vertices, in the order i0, i1, i2 ->
    (..., 7): J, l1, l2, c2, s2, rc, rs in the dtype of the input.  NaN where d0 == 0 or a position is not finite."""
    U, x = np.broadcast_arrays(np.asarray(U), np.asarray(x))
    ft = U.dtype
    one, zero, two = ft.type(1), ft.type(0), ft.type(2)
    px, py = U[..., 1, 0] - U[..., 0, 0], U[..., 1, 1] - U[..., 0, 1]
    qx, qy = U[..., 2, 0] - U[..., 0, 0], U[..., 2, 1] - U[..., 0, 1]
    with np.errstate(all="ignore"):
        ax, ay = x[..., 1, 0] - x[..., 0, 0], x[..., 1, 1] - x[..., 0, 1]
        bx, by = x[..., 2, 0] - x[..., 0, 0], x[..., 2, 1] - x[..., 0, 1]
        d0 = px * qy - py * qx
        bad = (d0 == 0) | ~np.isfinite(x).all(axis=(-1, -2))
        F11, F12 = (ax * qy - bx * py) / d0, (bx * px - ax * qx) / d0
        F21, F22 = (ay * qy - by * py) / d0, (by * px - ay * qx) / d0
        J = (ax * by - ay * bx) / d0
        c11, c12, c22 = F11 * F11 + F21 * F21, F11 * F12 + F21 * F22, F12 * F12 + F22 * F22
        m, d = (c11 + c22) / two, (c11 - c22) / two
        r = np.sqrt(d * d + c12 * c12)
        l1 = np.sqrt(m + r)
        l2 = np.where(l1 == 0, zero, np.abs(J) / l1)
        c2, s2 = np.where(r == 0, one, d / r), np.where(r == 0, zero, c12 / r)
        tr, sk = F11 + F22, F21 - F12
        s = np.sqrt(tr * tr + sk * sk)
        rc, rs = np.where(s == 0, one, tr / s), np.where(s == 0, zero, sk / s)
    out = np.stack((J, l1, l2, c2, s2, rc, rs), axis=-1).astype(ft)
    out[bad] = np.nan
    return out


def strain_tri(states, uv, ids, dtype=np.float64):
    """states (F, 4N) or (F, 2N), uv (N, 2) (taken as binary32), ids (T, 3) the body map's vertex order
    (body_ref.body_map(...)[3]) -> (F, T, 7)"""
    uv = np.asarray(uv, np.float32)
    N = uv.shape[0]
    S = np.asarray(states, np.float64)
    S = S.reshape(1, -1) if S.ndim == 1 else S
    P = S[:, :2 * N].reshape(S.shape[0], N, 2).astype(dtype)
    U = uv.astype(dtype)
    ids = np.asarray(ids, np.int64)
    return deform(U[ids][None], P[:, ids])


def label_counts(tri_of, labels, L, T):
    """cnt (L, T): the body-map pixels of label s in triangle t"""
    t = np.asarray(tri_of).reshape(-1)
    s = np.asarray(labels).reshape(-1)
    on = (t >= 0) & (s >= 0)
    cnt = np.zeros((L, T), np.int64)
    np.add.at(cnt, (s[on], t[on]), 1)
    return cnt


def label_traces(v, cnt):
    """v (F, T, 7), cnt (L, T) -> (F, L, 3): per label the triangles with a pixel of it in ascending order, count * value
    added one by one to 0.0, divided by the label's pixels; NaN for a label without one."""
    v = np.asarray(v, np.float64)
    F, L = v.shape[0], cnt.shape[0]
    out = np.full((F, L, 3), np.nan)
    for s in range(L):
        n = int(cnt[s].sum())
        if n == 0:
            continue
        acc = np.zeros((F, 3))
        for t in np.flatnonzero(cnt[s]):
            with np.errstate(invalid="ignore"):
                acc = acc + np.float64(cnt[s, t]) * v[:, t, :3]
        out[:, s] = acc / np.float64(n)
    return out


def levels(value, gain):
    """-> (level int64, keep): level = clamp(128 + rint(gain (value - 1)), 0, 255) in binary64; keep where it is NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        lv = 128.0 + np.rint(np.float64(gain) * (np.asarray(value, np.float64) - 1.0))
    keep = np.isnan(lv)
    return np.clip(np.where(keep, 0.0, lv), 0.0, 255.0).astype(np.int64), keep


def view_strain(X, tri, uv, ids, frame, which, gain, alpha, lut, wire=False):
    """-> (H, W, 3) uint8, B G R.  ids: the body map's vertex order; which: 0 J, 1 l1, 2 l2."""
    frame = np.asarray(frame, np.uint8)
    H, W = frame.shape
    N = len(uv)
    ch = np.repeat(frame[:, :, None], 3, axis=2).astype(np.int64)
    tri_of = cellview_ref.map_at(X, tri, W, H, N)[0]
    pos = np.asarray(X, np.float64).reshape(-1)[:2 * N]
    lv, keep = levels(strain_tri(pos, uv, ids)[0, :, which], gain)
    t = np.where(tri_of >= 0, tri_of, 0)
    on = (tri_of >= 0) & ~keep[t]
    col = np.asarray(lut, np.uint8).reshape(256, 3).astype(np.int64)[lv[t]]
    a = int(alpha)
    ch = np.where(on[:, :, None], (ch * (255 - a) + col * a + 127) // 255, ch)
    img = ch.astype(np.uint8)
    if wire:
        with np.errstate(invalid="ignore"):
            img[:, :, 0] = view_ref._blue(img[:, :, 0], view_ref.wire_count(tri, pos, W, H))
    return img


# ---- cases shared by test_strain_cpu.py and test_strain_gpu.py ---------------------------------------------------------
def rot(t):
    t = np.asarray(t, np.float64)
    return np.stack((np.stack((np.cos(t), -np.sin(t)), -1), np.stack((np.sin(t), np.cos(t)), -1)), -2)


def random_triangles(seed, n):
    """The draw the tolerance is measured on: n triangles with sides of 4 .. 64 px and every angle >= 20 degrees somewhere
    in a 1024^2 frame, uv rounded to binary32, each under its own x = F u + c, F = R(t1) diag(l1, l2) R(t2)^T with stretches
    log-uniform in [0.25, 4]; every other one listed clockwise.  -> U (n, 3, 2), x (n, 3, 2) float64."""
    rng = np.random.default_rng(seed)
    m = 4 * n
    a, b = rng.uniform(4, 64, m), rng.uniform(4, 64, m)
    al = rng.uniform(np.deg2rad(20), np.deg2rad(140), m)
    th = rng.uniform(0, 2 * np.pi, m)
    v0 = rng.uniform(64, 960, (m, 2))
    v1 = v0 + a[:, None] * np.stack((np.cos(th), np.sin(th)), 1)
    v2 = v0 + b[:, None] * np.stack((np.cos(th + al), np.sin(th + al)), 1)
    c = np.hypot(*(v2 - v1).T)
    be = np.arccos(np.clip((a * a + c * c - b * b) / (2 * a * c), -1, 1))
    ok = (c >= 4) & (c <= 64) & (be >= np.deg2rad(20)) & (np.pi - al - be >= np.deg2rad(20))
    U = np.stack((v0, v1, v2), 1)[ok][:n].astype(np.float32).astype(np.float64)
    assert len(U) == n
    l = np.exp(rng.uniform(np.log(0.25), np.log(4), (n, 2)))
    D = np.zeros((n, 2, 2))
    D[:, 0, 0], D[:, 1, 1] = l[:, 0], l[:, 1]
    F = rot(rng.uniform(0, 2 * np.pi, n)) @ D @ rot(rng.uniform(0, 2 * np.pi, n)).transpose(0, 2, 1)
    x = np.einsum("nij,nkj->nki", F, U) + rng.uniform(-20, 20, (n, 1, 2))
    flip = rng.random(n) < 0.5
    U[flip], x[flip] = U[flip][:, [0, 2, 1]], x[flip][:, [0, 2, 1]]
    return U, x


def grid_mesh(nx, ny, x0, y0, dx, dy, seed=0, jitter=0.2):
    """(nx x ny) vertices on a jittered grid from (x0, y0), spacing (dx, dy); two triangles per cell, the diagonal and the
    winding alternating from cell to cell: the body map's orientation swap fires for about half of them.
    -> p (N, 2) float64 (binary32 values), t (T, 3) int64"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny))
    p = np.stack((x0 + dx * gx.reshape(-1), y0 + dy * gy.reshape(-1)), 1) + rng.uniform(-jitter, jitter, (nx * ny, 2)) * (dx, dy)
    t = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            if (i + j) % 2:
                t += [(a, b, c), (a, d, c)]                # counter-clockwise in image axes, then clockwise
            else:
                t += [(b, d, a), (b, c, d)]
    return p.astype(np.float32).astype(np.float64), np.array(t, np.int64)
