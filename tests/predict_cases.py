"""Spring topologies shared by the CPU and GPU tests of the mass-spring prediction (hm_ms_newton, k_ms_newton4 through
hm_newton_dev_start, k_ms_newton through hm_ms_predict, k_fw_rows / k_pft_cols through hm_cov_predict).

The device kernels change their work split at the shapes built here: k_ms_newton4 gives a vertex to each of the 256
lanes of four waves (N = 64 fills one wave, 65 starts the second, 193 the fourth, 256 fills all, 257 is refused) and
pads every vertex to DEG = 8 or 12 neighbour slots (a vertex with more than 12 springs is refused); k_ms_newton strides
vectors of 2N and 4N over 512 threads (one pass up to N = 128 / 256).  Both keep the problem in LDS, with the footprints
of lds_newton4 / lds_newton below; a mesh over the limit takes the host loop.

Every case is a dict: name, p (N x 2), t (triangles, or None for a graph of bars only), bars (I x 2 int32), l0 (rest
lengths at p), X (4N float64: p perturbed by ~0.4 px, velocities ~1.5 px/frame, seeded by the name)."""
import ctypes
import os
import zlib

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# IteratedMSKalmanFilter's parameters of the prediction (kappa, M, deltat, maxiter, tol)
DEFAULTS = dict(kappa=-1.0, M=1.0, dt=0.05, maxiter=1000, tol=1e-4)

# LDS limits of the two launchers (csrc/predict_dev.hip: hm_newton_dev_start, hm_ms_predict)
NEWTON4_LDS_MAX = 64 * 1024
NEWTON_LDS_MAX = 160 * 1024


def lds_newton4(I):
    """bytes of LDS k_ms_newton4 asks for: (6 * 256 + 4 (I + 1) + 4 * 4) doubles + 2I ints"""
    return 12448 + 40 * I


def lds_newton(N, I):
    """bytes of LDS k_ms_newton asks for: (34N + 7I + 8) doubles + (N + 1 + 4I) ints"""
    return 276 * N + 72 * I + 68


def bars_of(t):
    """the springs of a triangulation as IteratedMSKalmanFilter gets them (mesh.Mesh: unique sorted edges)"""
    t = np.asarray(t, np.int64)
    e = np.vstack((t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]))
    return np.ascontiguousarray(np.unique(np.sort(e, axis=1), axis=0), np.int32)


def degrees(N, bars):
    return np.bincount(np.asarray(bars).reshape(-1), minlength=N)


def rest_lengths(p, bars):
    d = p[bars[:, 0]] - p[bars[:, 1]]
    return np.ascontiguousarray(np.sqrt((d * d).sum(1)), np.float64)


def state(p, name, pos_sigma=0.4, vel_sigma=1.5):
    """positions perturbed, velocities drawn: springs both stretched and compressed"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n2 = 2 * p.shape[0]
    return np.concatenate((p.reshape(-1) + rng.normal(0, pos_sigma, n2), rng.normal(0, vel_sigma, n2)))


def case(name, p, t, bars=None):
    p = np.ascontiguousarray(p, np.float64)
    if bars is None:
        bars = bars_of(t)
    bars = np.ascontiguousarray(bars, np.int32)
    return dict(name=name, p=p, t=None if t is None else np.ascontiguousarray(t, np.int64), bars=bars,
                l0=rest_lengths(p, bars), X=state(p, name), N=p.shape[0], I=bars.shape[0])


# ---- triangulations ------------------------------------------------------------------------------------------------
def grid(rows, cols, h=6.0, x0=0.0, y0=0.0):
    """rows x cols vertices, row-major, the cells split by alternating diagonals (a vertex with i + j even takes the
    diagonals of all four cells around it: degree 8 inside, 4 for the others) -> p, t"""
    jj, ii = np.meshgrid(np.arange(cols), np.arange(rows))
    p = np.column_stack((x0 + h * jj.ravel(), y0 + h * ii.ravel()))
    t = []
    for i in range(rows - 1):
        for j in range(cols - 1):
            a, b, c, d = i * cols + j, i * cols + j + 1, (i + 1) * cols + j, (i + 1) * cols + j + 1
            if (i + j) % 2 == 0:
                t += [(a, b, d), (a, d, c)]
            else:
                t += [(a, b, c), (b, d, c)]
    return p, np.array(t, np.int64)


def fan_onto_border(p, t, cols, m=3):
    """one more vertex below row 0 of a grid, joined to the m border vertices in the middle of that row (a fan of m - 1
    triangles): N + 1 vertices"""
    j0 = (cols - m) // 2
    h = p[1, 0] - p[0, 0]
    q = np.array([p[j0, 0] + h * (m - 1) / 2.0, p[0, 1] - h])
    v = p.shape[0]
    ft = [(v, j0 + k + 1, j0 + k) for k in range(m - 1)]
    return np.vstack((p, q)), np.vstack((t, np.array(ft, np.int64)))


def wheel(rows, cols, r0, c0, size, extra=False, h=6.0):
    """a grid whose cells [r0, r0 + size) x [c0, c0 + size) are replaced by a wheel: the block's inner vertices go, a hub
    at its centre is joined to the 4 size vertices of its outline (the rim).  extra: the rim also gets the midpoint of
    its first edge, which must lie on the grid's border (r0 = 0), so that no triangle outside needs it.  The hub has
    degree 4 size (+ 1); every other vertex keeps at most 8."""
    p, t = grid(rows, cols, h)
    r1, c1 = r0 + size, c0 + size
    # the rim in order around the block, starting along row r0
    rim = [r0 * cols + c for c in range(c0, c1)] + [r * cols + c1 for r in range(r0, r1)] + \
          [r1 * cols + c for c in range(c1, c0, -1)] + [r * cols + c0 for r in range(r1, r0, -1)]
    cen = p[t].mean(axis=1)
    inside = (cen[:, 1] > r0 * h) & (cen[:, 1] < r1 * h) & (cen[:, 0] > c0 * h) & (cen[:, 0] < c1 * h)
    t = t[~inside]
    hub = np.array([(c0 + c1) / 2.0 * h, (r0 + r1) / 2.0 * h])
    pts = [p, hub[None]]
    hub_i = p.shape[0]
    if extra:
        assert r0 == 0, "the extra rim vertex must lie on the grid's border"
        pts.append(((p[rim[0]] + p[rim[1]]) / 2.0)[None])
        rim = [rim[0], hub_i + 1] + rim[1:]
    p = np.vstack(pts)
    t = np.vstack((t, np.array([(hub_i, rim[k], rim[(k + 1) % len(rim)]) for k in range(len(rim))], np.int64)))
    # drop the block's inner vertices (no triangle uses them any more) and renumber
    used = np.unique(t)
    remap = -np.ones(p.shape[0], np.int64)
    remap[used] = np.arange(used.size)
    return p[used], remap[t]


def grid_case(rows, cols):
    p, t = grid(rows, cols)
    return case("grid_%dx%d" % (rows, cols), p, t)


def fan_case(rows, cols):
    p, t = fan_onto_border(*grid(rows, cols), cols)
    return case("grid_%dx%d_fan" % (rows, cols), p, t)


def config4_case():
    g = np.load(os.path.join(GOLD, "config4_track.npz"))
    return case("config4", g["p"], g["t"])


GRIDS = [(8, 8), (5, 13), (8, 16), (3, 43), (12, 16), (15, 17), (16, 16), (15, 20)]
WHEELS = {8: dict(r0=3, c0=2, size=2), 9: dict(r0=0, c0=3, size=2, extra=True),
          12: dict(r0=2, c0=2, size=3), 13: dict(r0=0, c0=2, size=3, extra=True)}


def wheel_case(k):
    """a wheel in an 8 x 8 grid whose hub has exactly k springs, the most of any vertex"""
    p, t = wheel(8, 8, **WHEELS[k])
    return case("wheel_%d" % k, p, t)


def grid_cases():
    """the triangulations of the grids (N = 64, 65, 128, 129, 192, 255, 256, 300), the fans (193, 257) and config 4
    (201), ascending in N"""
    cs = [grid_case(r, c) for r, c in GRIDS] + [fan_case(12, 16), fan_case(16, 16), config4_case()]
    return sorted(cs, key=lambda c: c["N"])


# ---- graphs of bars only (for the C-ABI: any springs whose N is the handle's) ----------------------------------------
def circulant(N, r):
    """vertex i joined to i +- 1 .. i +- r (mod N): degree 2r everywhere"""
    i = np.arange(N)
    return np.concatenate([np.column_stack((i, (i + s) % N)) for s in range(1, r + 1)])


def circulant_case(rows=8, cols=8, r=6):
    p, _ = grid(rows, cols)
    return case("circulant_%d_r%d" % (rows * cols, r), p, None, circulant(rows * cols, r))


def pendant_case():
    """the 8 x 8 grid plus vertex 64 hanging from vertex 63 by one spring (N = 65)"""
    p, t = grid(8, 8)
    p = np.vstack((p, p[63] + [4.0, 3.0]))
    return case("pendant_65", p, None, np.vstack((bars_of(t), [[63, 64]])))


def isolated_case():
    """the 8 x 8 grid plus vertex 64 without a spring (N = 65)"""
    p, t = grid(8, 8)
    p = np.vstack((p, p[63] + [4.0, 3.0]))
    return case("isolated_65", p, None, bars_of(t))


def graph_cases():
    return [circulant_case(), pendant_case(), isolated_case()]


def newton4_lds_case(I):
    """N = 256 (the 16 x 16 grid's vertices), I springs of degree <= 12: a circulant of radius 5 (1280 springs) plus
    i -- i + 6 for the first I - 1280 vertices.  I = 1327 is the largest footprint k_ms_newton4 takes, 1328 the first
    it refuses."""
    N = 256
    assert 1280 <= I <= 1280 + N
    p, _ = grid(16, 16)
    i = np.arange(I - 1280)
    b = np.vstack((circulant(N, 5), np.column_stack((i, (i + 6) % N))))
    return case("lds4_256_%d" % I, p, None, b)


def newton_lds_case(I):
    """N = 300 (the 15 x 20 grid's vertices), I springs: a circulant of radius 3 (900 springs) plus i -- i + 4 for the
    first I - 900 vertices.  I = 1124 is the largest footprint k_ms_newton takes at N = 300, 1125 the first it refuses
    (the grid's own triangulation has 831 springs)."""
    N = 300
    assert 900 <= I <= 900 + N
    p, _ = grid(15, 20)
    i = np.arange(I - 900)
    b = np.vstack((circulant(N, 3), np.column_stack((i, (i + 4) % N))))
    return case("lds_300_%d" % I, p, None, b)


def handle_mesh(N):
    """a triangulation with N vertices for the handle a graph of bars only is run on (the C-ABI calls take the springs
    as arguments; the handle's mesh only fixes N)"""
    shapes = {r * c: (r, c) for r, c in GRIDS}
    if N in shapes:
        return grid(*shapes[N])
    raise KeyError(N)


# ---- the host loop and the oracle on a case --------------------------------------------------------------------------
def host_newton(c, kappa, M, dt, maxiter, tol):
    """hm_ms_newton on the case -> (X advanced, Newton iterations)"""
    from hydra_mi import _lib
    X = c["X"].copy()
    its = ctypes.c_int()
    _lib.check(_lib.lib().hm_ms_newton(int(c["N"]), int(c["I"]), _lib.ptr(c["bars"]), _lib.ptr(c["l0"]), float(kappa),
                                       float(M), float(dt), int(maxiter), float(tol), _lib.ptr(X), ctypes.byref(its)),
               "hm_ms_newton")
    return X, its.value


def oracle_newton(c, kappa, M, dt, maxiter, tol):
    """oracle/ekf_ref.ms_predict (a dense inverse per Newton iteration) on the case -> X advanced"""
    from oracle import ekf_ref
    n4 = 4 * c["N"]
    K = ekf_ref.incidence(c["N"], c["bars"])
    X, _ = ekf_ref.ms_predict(c["X"], np.eye(n4), np.zeros((n4, n4)), K, c["l0"], kappa, M, dt, maxiter, tol)
    return X.reshape(-1)
