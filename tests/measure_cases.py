"""Meshes shared by the CPU and GPU tests of the measurement kernels at their structural limits (k_star_regions,
k_measure_vertex, k_measure_edge, k_render_iter, k_render, k_solve_prep, k_body_map).

Each limit changes a code path, and every case here sits on one side of one of them:
  EKF_MAX_STAR = 24 triangles around a vertex: star setups padded to an even count, one bit per star triangle in the
      tile words (hubs with 7 .. 24 triangles; a vertex in 25 is refused);
  PREP_MAX_ENTRIES = 104 terms of a row of k_solve_prep, i.e. at most 25 neighbours (a border fan of 24 triangles has
      exactly 25; a pinched vertex of 24 triangles in two fans has 26 and is refused);
  TMASK_STRIDE = 1024 tiles of 8 x 8 px per star region: above it no tile list is built and k_measure_vertex walks every
      tile of the region with the per-triangle boxes (`ubox`);
  EKF_MAX_TRI = 4096 triangles: the LDS triangle masks of k_render, k_render_iter and k_body_map are full (4097: refused);
  RI_CHUNK = 32 candidates of a 64 x 16 strip of k_render_iter set up at a time (strips of 31, 32, 33, 64, 65 and
      4096 candidates).

Every case is a dict: name, mesh (mesh.Mesh), W, H, tex (uint8, seeded by the name), hub (the vertex the case is about,
or None) and states (name -> X of 4N doubles).  The host restatements below -- the star region of k_star_regions and
the candidates of a k_render_iter strip -- let the CPU test hold each case to the count its name promises."""
import zlib

import numpy as np

from hydra_mi import mesh
from oracle import ekf_ref

EKF_MAX_STAR = 24
PREP_MAX_ENTRIES = 4 * (EKF_MAX_STAR + 2)
TMASK_STRIDE = 1024
EKF_MAX_TRI = 4096
RI_CHUNK = 32
RI_W, RI_H = 64, 16
DELTA = 2.0                        # deltaX of the measurement (Renderer.measure's default)
SUB = ekf_ref.SUB

HUB_DEGREES = (7, 12, 13, 16, 17, 23, 24)
STRIP_COUNTS = (31, 32, 33, 64, 65)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def texture(name, W, H):
    """uniform noise, seeded by the case name"""
    return _rng("tex:" + name).integers(0, 256, (H, W)).astype(np.uint8)


def with_velocities(name, P, sigma=1.0):
    """positions P (N x 2) and velocities drawn with the case's seed -> X (4N)"""
    P = np.asarray(P, np.float64)
    return np.concatenate((P.reshape(-1), _rng("vel:" + name).normal(0, sigma, P.size)))


def case(name, p, t, W, H, hub=None, states=None):
    p, t = np.asarray(p, np.float64), np.array(t, np.int64)
    a = (p[t[:, 1], 0] - p[t[:, 0], 0]) * (p[t[:, 2], 1] - p[t[:, 0], 1]) - \
        (p[t[:, 1], 1] - p[t[:, 0], 1]) * (p[t[:, 2], 0] - p[t[:, 0], 0])
    t[a < 0] = t[a < 0][:, [0, 2, 1]]          # one orientation at rest, as the filter's fold test expects
    m = mesh.Mesh(p, t)
    st = {"rest": with_velocities(name, m.p)}
    for k, P in (states or {}).items():
        st[k] = with_velocities(name, P)
    return dict(name=name, mesh=m, W=W, H=H, tex=texture(name, W, H), hub=hub, states=st)


# ---- counts ---------------------------------------------------------------------------------------------------------
def star(t, v):
    return np.nonzero((np.asarray(t) == v).any(axis=1))[0]


def neighbours(t, v):
    s = np.asarray(t)[star(t, v)].reshape(-1)
    return np.unique(s[s != v])


def prep_entries(t, v):
    """terms of the k_solve_prep rows of vertex v: its own 4x4 block and one per neighbour"""
    return 4 * (len(neighbours(t, v)) + 1)


def tri_box(P, W, H):
    """d_tri_bbox of three snapped vertices (3 x 2 int64) -> (cmin, cmax, rmin, rmax); cmin > cmax: empty"""
    (x0, y0), (x1, y1), (x2, y2) = [(int(a), int(b)) for a, b in P]
    lim = 1 << 32
    if not all(-lim < q < lim for q in (x0, y0, x1, y1, x2, y2)):
        return (1, 0, 1, 0)
    if (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) == 0:
        return (1, 0, 1, 0)
    cl, ch = (min(x0, x1, x2) - 128) // SUB, (max(x0, x1, x2) - 128) // SUB + 1
    rl, rh = (min(y0, y1, y2) - 128) // SUB, (max(y0, y1, y2) - 128) // SUB + 1
    return (max(cl, 0), min(ch, W - 1), max(rl, 0), min(rh, H - 1))


def configurations(X, N, v, d=DELTA):
    """the five states of k_star_regions: reference, +x, -x, +y, -y of vertex v"""
    out = []
    for dx, dy in ((0, 0), (d, 0), (-d, 0), (0, d), (0, -d)):
        Xc = np.array(X, np.float64).reshape(-1).copy()
        Xc[2 * v] += dx
        Xc[2 * v + 1] += dy
        out.append(Xc)
    return out


def star_region(X, N, t, v, W, H, d=DELTA):
    """The region of vertex v as k_star_regions forms it (csrc/ekf_kernels.h, d_star_regions): the union over the five
    configurations of the pixel boxes of the star triangles (a box counts when cmin <= cmax), the first column and row
    rounded down to the 8 x 8 grid of the frame, width and height rounded up to whole tiles -> (c0, r0, rw, rh)"""
    t = np.asarray(t)
    c0, c1, r0, r1 = W, -1, H, -1
    for Xc in configurations(X, N, v, d):
        P = ekf_ref.snap(Xc[:2 * N].reshape(N, 2))
        for tr in t[star(t, v)]:
            b = tri_box(P[tr], W, H)
            if b[0] > b[1]:
                continue
            c0, c1, r0, r1 = min(c0, b[0]), max(c1, b[1]), min(r0, b[2]), max(r1, b[3])
    if c1 >= c0:
        c0, r0 = c0 & ~7, r0 & ~7
    rw = (c1 - c0 + 8) & ~7 if c1 >= c0 else 0
    rh = (r1 - r0 + 8) & ~7 if (c1 >= c0 and r1 >= r0) else 0
    return c0, r0, rw, rh


def region_tiles(X, N, t, v, W, H, d=DELTA):
    _, _, rw, rh = star_region(X, N, t, v, W, H, d)
    return (rw // 8) * (rh // 8)


def strip_candidates(X, N, t, W, H, rows=RI_H):
    """Candidates of every strip of k_render_iter (csrc/ekf_kernels.h): the triangles that pass the extent test (the
    vertices' extent widened by 2 px) and whose d_tri_bbox meets the strip -> (tiles_y, tiles_x) int array"""
    X = np.asarray(X, np.float64).reshape(-1)
    Q = X[:2 * N].reshape(N, 2)
    P = ekf_ref.snap(Q)
    tx, ty = -(-W // RI_W), -(-H // rows)
    out = np.zeros((ty, tx), np.int64)
    for tr in np.asarray(t):
        cmin, cmax, rmin, rmax = tri_box(P[tr], W, H)
        if cmin > cmax:
            continue
        lo, hi = Q[tr].min(axis=0) - 2.0, Q[tr].max(axis=0) + 2.0
        for sy in range(max(0, rmin // rows - 1), min(ty, rmax // rows + 2)):
            r0 = sy * rows
            if not (rmax >= r0 and rmin < r0 + rows):
                continue
            for sx in range(max(0, cmin // RI_W - 1), min(tx, cmax // RI_W + 2)):
                c0 = sx * RI_W
                if hi[0] < c0 or lo[0] > c0 + RI_W or hi[1] < r0 or lo[1] > r0 + rows:
                    continue
                if cmax >= c0 and cmin < c0 + RI_W:
                    out[sy, sx] += 1
    return out


# ---- hubs and fans --------------------------------------------------------------------------------------------------
def _ring(c, R, k, a0, a1, closed, rx=None, ry=None):
    rx = R if rx is None else rx
    ry = R if ry is None else ry
    a = a0 + (a1 - a0) * np.arange(k) / (k if closed else k - 1)
    return np.column_stack((c[0] + rx * np.cos(a), c[1] - ry * np.sin(a)))


def wheel_mesh(k, c, R, R2=None, rx=None, ry=None):
    """hub 0 at c joined to a closed rim 1..k (k triangles around the hub), and with R2 an outer ring k+1..2k of two
    triangles per rim edge (the hub then has non-neighbours) -> p, t"""
    rim = _ring(c, R, k, 0.0, 2 * np.pi, True, rx, ry)
    t = [(0, 1 + j, 1 + (j + 1) % k) for j in range(k)]
    pts = [np.asarray(c, np.float64)[None], rim]
    if R2 is not None:
        pts.append(_ring(c, R2, k, np.pi / k, 2 * np.pi + np.pi / k, True))
        for j in range(k):
            r, rn, o, on = 1 + j, 1 + (j + 1) % k, 1 + k + j, 1 + k + (j + 1) % k
            t += [(r, o, rn), (o, on, rn)]
    return np.vstack(pts), np.array(t, np.int64)


def fan_mesh(k, c, R, R2, a0, a1):
    """hub 0 at c joined to an open arc of k + 1 rim vertices from angle a0 to a1 (k triangles, k + 1 neighbours: the
    hub lies on the mesh border), an outer arc of k vertices beyond it -> p, t"""
    rim = _ring(c, R, k + 1, a0, a1, False)
    step = (a1 - a0) / k
    outer = _ring(c, R2, k, a0 + step / 2, a1 - step / 2, False)
    t = [(0, 1 + j, 2 + j) for j in range(k)]
    o0 = k + 2
    for j in range(k):
        t.append((1 + j, o0 + j, 2 + j))
        if j + 1 < k:
            t.append((o0 + j, o0 + j + 1, 2 + j))
    return np.vstack((np.asarray(c, np.float64)[None], rim, outer)), np.array(t, np.int64)


def hub_states(p, hub, R):
    """perturbed (every vertex by ~0.5 px) and folded (the hub pulled across its rim: its triangles turn over)"""
    rng = _rng("perturb:%d:%d" % (len(p), hub))
    pert = p + rng.normal(0, 0.5, p.shape)
    fold = p.copy()
    fold[hub] += (1.35 * R, 0.4 * R)
    return {"perturbed": pert, "folded": fold}


def hub_cases():
    out = []
    for k in HUB_DEGREES:
        c, R = (47.3, 48.6), 19.0
        p, t = wheel_mesh(k, c, R, R2=38.0)
        out.append(case("hub%d" % k, p, t, 96, 96, hub=0, states=hub_states(p, 0, R)))
    return out


def border_fan_case():
    """a fan of 24 triangles on the border: 25 neighbours, 104 k_solve_prep terms"""
    c, R = (48.4, 66.7), 22.0
    p, t = fan_mesh(EKF_MAX_STAR, c, R, 40.0, 0.0, np.pi)
    return case("fan24", p, t, 96, 96, hub=0, states=hub_states(p, 0, R))


def refused_cases():
    """meshes hm_ctx_create must refuse: a hub in 25 triangles; a pinched vertex (two fans of 12 triangles meeting in
    it: 24 triangles, 26 neighbours); the 33 x 65 grid with one triangle more (grid_case(extra=True))"""
    p, t = wheel_mesh(EKF_MAX_STAR + 1, (47.3, 48.6), 20.0)
    over = case("hub25", p, t, 96, 96, hub=0)
    c = np.array([48.2, 47.9])
    up = _ring(c, 24.0, 13, np.radians(8), np.radians(172), False)
    down = _ring(c, 24.0, 13, np.radians(188), np.radians(352), False)
    p = np.vstack((c[None], up, down))
    t = [(0, 1 + j, 2 + j) for j in range(12)] + [(0, 14 + j, 15 + j) for j in range(12)]
    pinch = case("pinched", p, np.array(t, np.int64), 96, 96, hub=0)
    return [over, pinch, grid_case(extra=True)]


# ---- coarse meshes: star regions at and above TMASK_STRIDE tiles ----------------------------------------------------
def _coarse_wheel(R, c, k=8):
    return wheel_mesh(k, c, R)


def search_region_radius(c, W, H, lo, hi, k=8, step=1.0 / SUB):
    """the hub radius R (a multiple of 1/256 px) of a k-wheel at c whose hub region has exactly TMASK_STRIDE tiles, and
    the smallest R above it whose region has more -> (R_at, tiles_at, R_above, tiles_above)"""
    def tiles(R):
        p, t = _coarse_wheel(R, c, k)
        return region_tiles(with_velocities("search", p), len(p), t, 0, W, H)
    # coarse scan for the first radius past the limit, then the last 1/256 steps before it
    n = int(round((hi - lo) / step))
    a, b = 0, n
    assert tiles(lo) <= TMASK_STRIDE < tiles(hi)
    while b - a > 1:                       # tiles(R) does not decrease with R: the rim moves outwards
        m = (a + b) // 2
        if tiles(lo + m * step) > TMASK_STRIDE:
            b = m
        else:
            a = m
    Ra, Rb = lo + a * step, lo + b * step
    return Ra, tiles(Ra), Rb, tiles(Rb)


COARSE_C, COARSE_W = (160.37, 158.81), 320


def coarse_cases():
    """regions of exactly 1024 tiles and the smallest count above; one far above on a 4096 x 64 frame; one on a 517 x 300
    frame clipped by its right edge (the last tile column sticks out of the frame)"""
    out = []
    Ra, ta, Rb, tb = search_region_radius(COARSE_C, COARSE_W, COARSE_W, 120.0, 132.0)
    for name, R in (("region_at", Ra), ("region_above", Rb)):
        p, t = _coarse_wheel(R, COARSE_C)
        cs = case(name, p, t, COARSE_W, COARSE_W, hub=0)
        cs["R"] = R
        out.append(cs)
    p, t = wheel_mesh(8, (2048.4, 31.7), 0.0, rx=2000.0, ry=27.0)
    out.append(case("region_wide", p, t, 4096, 64, hub=0))
    p, t = wheel_mesh(8, (470.6, 151.3), 0.0, rx=240.0, ry=140.0)
    out.append(case("region_clipped", p, t, 517, 300, hub=0))
    return out


# ---- triangle-count meshes: the 4096-bit masks and chunked strips ---------------------------------------------------
def grid(rows, cols, h, x0, y0):
    """rows x cols vertices, every cell split by the same diagonal (degree <= 6) -> p, t"""
    jj, ii = np.meshgrid(np.arange(cols), np.arange(rows))
    p = np.column_stack((x0 + h * jj.ravel(), y0 + h * ii.ravel()))
    t = []
    for i in range(rows - 1):
        for j in range(cols - 1):
            a, b, c, d = i * cols + j, i * cols + j + 1, (i + 1) * cols + j, (i + 1) * cols + j + 1
            t += [(a, b, d), (a, d, c)]
    return p, np.array(t, np.int64)


def tri_wave(x, m):
    """0 .. m and back, period 2m: folds a line onto itself every m units"""
    return np.abs(np.mod(x + m, 2 * m) - m)


GRID_ROWS, GRID_COLS, GRID_H = 33, 65, 3.5


def grid_case(extra=False):
    """the 33 x 65 grid: 4096 triangles (extra: one more, a fan triangle below the border -> refused).  States: shrunk
    (all of it inside the strip [64, 128) x [16, 32): 4096 candidates, 128 chunks) and folded (the columns folded every
    4, the rows every 4: ~128 triangles over every pixel of a 14 x 14 px patch across two strips)"""
    x0, y0 = 8.3, 7.6
    p, t = grid(GRID_ROWS, GRID_COLS, GRID_H, x0, y0)
    W, H = 240, 128
    if extra:
        v = len(p)
        p = np.vstack((p, [[x0 + GRID_H * 31.5, y0 - 3.0]]))
        t = np.vstack((t, [[v, 32, 31]]))
        return case("grid4097", p, t, W, H)
    jj, ii = (p[:, 0] - x0) / GRID_H, (p[:, 1] - y0) / GRID_H
    shrunk = np.column_stack((66.0 + jj * (58.0 / 64), 17.0 + ii * (13.5 / 32)))
    folded = np.column_stack((100.2 + GRID_H * tri_wave(jj, 4), 40.3 + GRID_H * tri_wave(ii, 4)))
    return case("grid4096", p, t, W, H, states={"shrunk": shrunk, "folded": folded})


def ribbon_case(n):
    """a ribbon of n triangles (vertices alternating between two rows) inside strip (0, 1) of a 128 x 48 frame: that
    strip has n candidates, no other one has any.  Folded: the ribbon concertinaed onto itself, so that every pixel
    it covers is covered by triangles of several chunks"""
    j = np.arange(n + 2)
    x = 4.0 + 54.0 * j / (n + 1)
    y = np.where(j % 2 == 0, 19.3, 28.6)
    t = np.array([(i, i + 1, i + 2) for i in range(n)], np.int64)
    folded = np.column_stack((20.0 + 1.7 * tri_wave(j + 0.5, 6), y))
    return case("ribbon%d" % n, np.column_stack((x, y)), t, 128, 48, states={"folded": folded})


def strip_cases():
    return [ribbon_case(n) for n in STRIP_COUNTS]
