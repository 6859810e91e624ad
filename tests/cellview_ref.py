"""NumPy restatement of the cell view (include/hydra_mi.h: hm_view_set_cells, hm_view_cells; hydra_mi.cellview).

The triangle under an image pixel, its barycentrics and the swapped vertex ids come from tests/body_ref.body_map, called
with the positions of the state X in place of uv; this file restates what the view adds: which triangles are skipped, the
body pixel, the layers in unsigned 64-bit integers, the outline plane, the markers, and the wireframe through
tests/view_ref.wire_count.

body_map takes its positions as binary32 (they are uv there).  Only the snapped position rint(256 x) enters the coverage
rule, so it is given rint(256 x) / 256, which it snaps back to the same whole number -- as long as that is a binary32
value: 24 bits, every position within +-65536 px whatever its fraction.  `map_at` asserts it rather than go wrong.
"""
import numpy as np

import body_ref
import view_ref

SUB = body_ref.SUB
D = np.uint64(65535 * 255)
SANE = 2 ** 32          # d_tri_sane: snapped positions strictly inside +-2^32 (2^24 px)
POINT_MAX = 1048576.0


def map_at(X, tri, W, H, N):
    """body_map at the positions of X -> (triangle per pixel, l1, l2, ids).  Triangles with a vertex that is not finite or
    not sane are skipped (they go in as a triangle of area 0, which body_map skips, so the indices stay)."""
    pos = np.asarray(X, np.float64).reshape(-1)
    tri = np.asarray(tri, np.int64)
    P = pos[:2 * N].reshape(N, 2)                      # X: 2N positions, or the state of 4N
    with np.errstate(invalid="ignore", over="ignore"):
        good = np.isfinite(P).all(axis=1) & (np.abs(P) <= 2.0 ** 24).all(axis=1)
        S = np.rint(np.where(good[:, None], P, 0.0) * SUB)
    good &= (np.abs(S) < SANE).all(axis=1)
    Q = np.where(good[:, None], S, 0.0) / SUB
    used = np.unique(tri[good[tri].all(axis=1)])
    assert (Q[used].astype(np.float32).astype(np.float64) == Q[used]).all(), \
        "a snapped position is no binary32 value: beyond what this restatement can hand to body_ref.body_map"
    t2 = np.where(good[tri].all(axis=1)[:, None], tri, tri[:, :1])       # (i0, i0, i0): area 0
    return body_ref.body_map(Q, t2, W, H)


def body_pixel(uv, tri_of, l1, l2, ids):
    """-> (row, column) int64 of the body pixel under every image pixel, and whether there is one"""
    U = np.asarray(uv, np.float32).astype(np.float64)
    H, W = tri_of.shape
    inside = tri_of >= 0
    v = ids[np.where(inside, tri_of, 0)]
    a, b, c = U[v[..., 0]], U[v[..., 1]], U[v[..., 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        xy = (a + l1[..., None] * (b - a)) + l2[..., None] * (c - a)
        bx, by = xy[..., 0], xy[..., 1]
        ok = inside & (bx >= 0) & (bx < W) & (by >= 0) & (by < H)
    col = np.floor(np.where(ok, bx, 0)).astype(np.int64)
    row = np.floor(np.where(ok, by, 0)).astype(np.int64)
    return row, col, ok


def outline_plane(lab0):
    """layer 0 (H, W): label >= 0 and a 4-neighbour with another label; off the frame counts as another"""
    lab0 = np.asarray(lab0, np.int64)
    pad = np.pad(lab0, 1, constant_values=-2)
    c = pad[1:-1, 1:-1]
    diff = (pad[1:-1, :-2] != c) | (pad[1:-1, 2:] != c) | (pad[:-2, 1:-1] != c) | (pad[2:, 1:-1] != c)
    return (lab0 >= 0) & diff


def markers(img, points, colours, radius):
    """filled discs in place, in order: a later point over an earlier one"""
    H, W = img.shape[:2]
    if points is None:
        return img
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    col = np.asarray(colours, np.uint8).reshape(-1, 3)
    R = int(radius)
    for i, (x, y) in enumerate(pts):
        if not (-POINT_MAX <= x <= POINT_MAX and -POINT_MAX <= y <= POINT_MAX):      # (NaN fails both)
            continue
        cx, cy = int(x), int(y)                      # truncation toward zero, as C does
        for py in range(max(cy - R, 0), min(cy + R, H - 1) + 1):
            for px in range(max(cx - R, 0), min(cx + R, W - 1) + 1):
                if (px - cx) ** 2 + (py - cy) ** 2 <= R * R:
                    img[py, px] = col[i]
    return img


def view_cells(X, tri, uv, frame, labels=None, weights=None, colours=None, levels=None, outline=True, wire=False,
               points=None, point_colours=None, point_radius=2):
    """-> (H, W, 3) uint8, B G R.  labels: (n_layers, H, W) or (H, W) or None (no cells)."""
    frame = np.asarray(frame, np.uint8)
    H, W = frame.shape
    ch = np.repeat(frame[:, :, None], 3, axis=2).astype(np.uint64)
    if labels is not None:
        lab = np.asarray(labels, np.int64)
        lab = lab[None] if lab.ndim == 2 else lab
        col = np.asarray(colours, np.uint8).reshape(-1, 3).astype(np.uint64)
        wts = np.full(lab.shape, 65535, np.uint64) if weights is None else np.asarray(weights, np.uint16).reshape(lab.shape).astype(np.uint64)
        lev = np.full(col.shape[0], 255, np.uint64) if levels is None else np.asarray(levels, np.uint8).astype(np.uint64)
        row, colm, ok = body_pixel(uv, *map_at(X, tri, W, H, len(uv)))
        for j in range(lab.shape[0]):
            s = lab[j][row, colm]
            on = ok & (s >= 0)
            s0 = np.where(on, s, 0)
            a = np.where(on, wts[j][row, colm] * lev[s0], np.uint64(0)).astype(np.uint64)
            for q in range(3):
                ch[:, :, q] = (ch[:, :, q] * (D - a) + col[s0, q] * a + D // np.uint64(2)) // D
        if outline:
            s = lab[0][row, colm]
            on = ok & outline_plane(lab[0])[row, colm]
            ch[on] = col[s[on]]
    img = ch.astype(np.uint8)
    if wire:
        pos = np.asarray(X, np.float64).reshape(-1)[:2 * len(uv)]
        with np.errstate(invalid="ignore"):
            img[:, :, 0] = view_ref._blue(img[:, :, 0], view_ref.wire_count(tri, pos, W, H))
    return markers(img, points, point_colours, point_radius)
