"""Scenes, states and palettes shared by the CPU and GPU tests of the tracker's views at their limits
(tests/test_view_cases_cpu.py, tests/test_view_limits_gpu.py): frame clipping, the 2^20 rule, non-finite vertices and
velocities, the byte-wise tail of k_view_compose, the mask palette.

A scene is a dict: name, W, H, mesh (a box mesh), frame (uint8, bright: two triangles over a pixel sum past 255), and
`scene()` builds nothing on a device; `make_filter` does.  A state is X of 4N doubles.  `check_state` asserts on the host
that a state has the property it is named for, so that a test that passes has really been at that limit."""
import zlib

import numpy as np

import view_ref

SCENES = ("33x17", "34x17", "35x17", "90x72")
ODD_SCENES = SCENES[:3]
POSITION_STATES = ("inside", "half", "straddle", "far", "nonfinite", "collapsed", "folded")
VELOCITY_STATES = ("vel0", "velnan", "velallnan", "velinf", "velulp")
STATES = POSITION_STATES + VELOCITY_STATES
MASK_STATES = ("inside", "half", "straddle", "collapsed", "folded")
PALETTES = ("mixed", "high", None)
C20 = 1048576.0
STRADDLE_SCALE = {"33x17": 3.0, "34x17": 3.0, "35x17": 3.0, "90x72": 16.0}
COVER_SCALE = 2.2          # velulp: the box mesh scaled about the frame centre until it covers the whole frame


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def scene(name):
    from hydra_mi import mesh
    rng = _rng("scene:" + name)
    if name == "90x72":
        W, H = 90, 72
        dm = mesh.box_mesh(20.0, 14.0, 70.0, 57.0, 9.0)
    else:
        W, H = int(name.split("x")[0]), 17
        dm = mesh.box_mesh(3.0, 2.0, 30.0, 14.5, 5.0)
    frame = rng.integers(130, 256, (H, W)).astype(np.uint8)
    flow = rng.normal(0, 2, (H, W, 2)).astype(np.float32)
    assert (W * H) % 4 == {"33x17": 1, "34x17": 2, "35x17": 3, "90x72": 0}[name]
    assert W * H < 4 * 256 or name == "90x72"              # the odd scenes: one, partly filled workgroup of k_view_compose
    return dict(name=name, W=W, H=H, mesh=dm, frame=frame, flow=flow, mask=(frame > 0).astype(np.uint8))


def make_filter(sc):
    """the filter of a scene as bodystats_cases.make_filter builds it, with the observation the overlay shows"""
    import bodystats_cases
    kf = bodystats_cases.make_filter(sc["mesh"], sc["frame"])
    kf.state.renderer.set_observation(sc["frame"], sc["flow"], sc["mask"])
    return kf


def _tri(sc):
    return np.asarray(sc["mesh"].t, np.int64)


def _interior(sc, k):
    """k vertices of the highest degree, no two of them in one triangle"""
    t = _tri(sc)
    N = sc["mesh"].size()
    deg = np.bincount(t.reshape(-1), minlength=N)
    out = []
    for v in np.argsort(-deg, kind="stable"):
        if all(not ((t == v).any(axis=1) & (t == u).any(axis=1)).any() for u in out):
            out.append(int(v))
        if len(out) == k:
            return out
    raise AssertionError("mesh too small for %d separate vertices" % k)


def _disjoint_triangles(sc, k):
    """k triangles that share no vertex"""
    out, used = [], set()
    for i, tr in enumerate(_tri(sc)):
        if not used & set(int(v) for v in tr):
            out.append(i)
            used |= set(int(v) for v in tr)
        if len(out) == k:
            return out
    raise AssertionError("mesh too small for %d disjoint triangles" % k)


def special(sc, state):
    """the vertices / triangles a state is about, in the order its description names them"""
    if state in ("far", "nonfinite", "velinf"):
        return _interior(sc, 3)
    if state in ("velnan", "velulp", "folded"):
        return _interior(sc, 1)
    if state == "collapsed":
        return _disjoint_triangles(sc, 2)
    return []


def signed_areas(P, t):
    a, b, c = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def state(sc, name):
    W, H = sc["W"], sc["H"]
    p = np.asarray(sc["mesh"].p, np.float64)
    t = _tri(sc)
    N = p.shape[0]
    rng = _rng("state:" + sc["name"])                       # `inside` is the same whatever state is built from it
    P = p + rng.uniform(-0.45, 0.45, p.shape) + 0.013
    V = rng.normal(0, 1.0, p.shape)
    c = np.array([W / 2.0, H / 2.0])
    sp = special(sc, name)
    if name == "half":
        P = np.floor(p) + 0.5 - (np.floor(p.min(axis=0)) + 1.0)          # the box's corner at (-0.5, -0.5)
    elif name == "straddle":
        P = c + STRADDLE_SCALE[sc["name"]] * (P - c)
    elif name == "far":
        P[sp[0]] = (C20, -C20)
        P[sp[1]] = (C20 + 0.5, 0.0)
        P[sp[2]] = (C20 + 0.6, 0.0)
    elif name == "nonfinite":
        P[sp[0], 0] = np.nan
        P[sp[1]] = (np.inf, P[sp[1], 1])
        P[sp[2]] = (P[sp[2], 0], -np.inf)
    elif name == "collapsed":
        a, b = t[sp[0]], t[sp[1]]
        q = np.floor(P[a].mean(axis=0))
        P[a[0]], P[a[1]], P[a[2]] = q + (0.1, 0.2), q + (-0.2, 0.3), q + (0.3, -0.1)
        P[b[1]] = np.floor(P[b[0]]) + (0.2, -0.3)
        P[b[0]] = np.floor(P[b[0]]) + (-0.1, 0.4)
    elif name == "folded":
        v = sp[0]
        ring = np.unique(t[(t == v).any(axis=1)])
        far_side = ring[np.argmax(np.hypot(*(p[ring] - p[v]).T))]
        P[v] = P[v] + 2.2 * (p[far_side] - p[v])                        # through the ring and out on the other side
    elif name == "vel0":
        V[:] = 0.0
    elif name == "velnan":
        V[sp[0], 0] = np.nan
        V[sp[0], 1] = np.nan
    elif name == "velallnan":
        V[:] = np.nan
    elif name == "velinf":
        V[sp[0]] = (1e39, 1e39)
        V[sp[1]] = (-1e39, -1e39)
    elif name == "velulp":
        P = c + COVER_SCALE * (P - c)
        V[:] = (0.75, -0.625)
        V[sp[0]] = (np.nextafter(np.float32(0.75), np.float32(1)), np.nextafter(np.float32(-0.625), np.float32(0)))
    elif name != "inside":
        raise KeyError(name)
    return np.concatenate((P.reshape(-1), V.reshape(-1)))


def palette(sc, name):
    """the mask view's label per triangle -> (T,) int64, None: no palette (-1 everywhere)"""
    T = _tri(sc).shape[0]
    if name is None:
        return None
    if name == "high":
        return np.full(T, 65534, np.int64)
    assert name == "mixed" and T >= 8
    lab = (2503 * np.arange(T, dtype=np.int64) + 77) % 65535
    lab[:5] = (-1, 0, 255, 256, 65534)
    g, b = lab[5:] // 256, lab[5:] % 256
    assert ((g != 0) & (g != 255) & (g != b)).any()
    return lab


# ---- what the CPU test holds every state to -------------------------------------------------------------------------
def segments(sc, X):
    """the wireframe's segments at X: (x0, y0, x1, y1) after rint, None for one that is not drawn"""
    N = sc["mesh"].size()
    with np.errstate(invalid="ignore"):
        P = np.rint(np.asarray(X, np.float64)[:2 * N]).reshape(N, 2)
    out = []
    for tr in _tri(sc):
        for k in range(3):
            a, b = P[tr[k]], P[tr[(k + 1) % 3]]
            q = (a[0], a[1], b[0], b[1])
            out.append(tuple(int(v) for v in q) if all(np.isfinite(v) and abs(v) <= C20 for v in q) else None)
    return out


def unclipped_count(sc, X, pad):
    """pixels of the wireframe (with multiplicity) on the frame padded by `pad` on every side, and on the frame itself"""
    W, H = sc["W"], sc["H"]
    N = sc["mesh"].size()
    Xp = np.array(X, np.float64)
    Xp[:2 * N] += pad
    big = view_ref.wire_count(_tri(sc), Xp[:2 * N], W + 2 * pad, H + 2 * pad)
    return int(big.sum()), int(view_ref.wire_count(_tri(sc), X[:2 * N], W, H).sum()), big[pad:pad + H, pad:pad + W]


def check_state(sc, name, X):
    """assert that X is at the limit `name` stands for"""
    W, H = sc["W"], sc["H"]
    N = sc["mesh"].size()
    t = _tri(sc)
    P, V = X[:2 * N].reshape(N, 2), X[2 * N:].reshape(N, 2)
    sp = special(sc, name)
    segs = segments(sc, X)
    if name in ("inside",) + VELOCITY_STATES and name != "velulp":
        R = np.rint(P)
        assert (R[:, 0] >= 0).all() and (R[:, 0] < W).all() and (R[:, 1] >= 0).all() and (R[:, 1] < H).all()
        assert (P != R).all()
    if name == "inside":
        assert (V != 0).all() and np.isfinite(X).all()
    elif name == "half":
        assert (np.mod(2 * P, 2) == 1).all() and (P < 0).any()
        k = np.floor(P)
        assert (np.mod(k, 2) == 0).any() and (np.mod(k, 2) == 1).any()        # half to even goes both ways
        assert (P == -0.5).any()                                             # rint -> -0: drawn; floor(x + .5) as well
        assert (np.rint(P) != np.trunc(P)).any() and (np.rint(P) != np.floor(P + 0.5)).any()
    elif name == "straddle":
        sides = {"left": False, "right": False, "top": False, "bottom": False}
        outside = 0
        for tr in t:
            Q = np.rint(P[tr])
            lo, hi = Q.min(axis=0), Q.max(axis=0)
            if hi[0] < 0 or lo[0] >= W or hi[1] < 0 or lo[1] >= H:
                outside += 1
        for s in segs:
            pad = int(max(abs(v) for v in s)) + 1
            px = view_ref.segment(s[0] + pad, s[1] + pad, s[2] + pad, s[3] + pad, W + 2 * pad, H + 2 * pad)
            x, y = px % (W + 2 * pad) - pad, px // (W + 2 * pad) - pad
            ins = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            if not ins.any():
                continue
            sides["left"] |= bool((x < 0).any())
            sides["right"] |= bool((x >= W).any())
            sides["top"] |= bool((y < 0).any())
            sides["bottom"] |= bool((y >= H).any())
        assert all(sides.values()), sides
        assert outside >= 1
        if sc["name"] == "90x72":                      # several trips of the lane loop of d_segment
            n = [max(abs(s[2] - s[0]), abs(s[3] - s[1])) for s in segs]
            assert max(n) > 128
    elif name == "far":
        assert tuple(P[sp[0]]) == (C20, -C20) and tuple(P[sp[1]]) == (C20 + 0.5, 0.0) and tuple(P[sp[2]]) == (C20 + 0.6, 0.0)
        assert np.rint(P[sp[1], 0]) == C20 and np.rint(P[sp[2], 0]) == C20 + 1
        k = 0
        for tr in t:
            for e in range(3):
                ends = (tr[e], tr[(e + 1) % 3])
                assert (segs[k] is None) == (sp[2] in ends), (k, ends)
                k += 1
    elif name == "nonfinite":
        assert np.isnan(P[sp[0]]).any() and (P[sp[1]] == np.inf).any() and (P[sp[2]] == -np.inf).any()
        k = 0
        for tr in t:
            for e in range(3):
                ends = (tr[e], tr[(e + 1) % 3])
                assert (segs[k] is None) == bool(set(sp) & set(int(v) for v in ends))
                k += 1
        assert sum(s is not None for s in segs) > 0
    elif name == "collapsed":
        a, b = t[sp[0]], t[sp[1]]
        R = np.rint(P)
        assert (R[a] == R[a[0]]).all() and len({tuple(q) for q in R[b]}) == 2
        assert not (P[a[0]] == P[a[1]]).all()
        k0 = 3 * sp[0]
        assert all(s is not None and s[:2] == s[2:] for s in segs[k0:k0 + 3])           # three segments with n == 0
        x, y = int(R[a[0], 0]), int(R[a[0], 1])
        assert 0 <= x < W and 0 <= y < H
        assert view_ref.wire_count(t, X[:2 * N], W, H)[y, x] >= 3
    elif name == "folded":
        rest = signed_areas(np.asarray(sc["mesh"].p, np.float64), t)
        now = signed_areas(P, t)
        assert (np.sign(rest) != np.sign(now)).any() and (np.sign(rest) == np.sign(now)).any()
        assert coverage(sc, X).max() >= 2
    elif name == "vel0":
        assert (V == 0).all()
    elif name == "velnan":
        assert np.isnan(V[sp[0]]).all() and np.isfinite(np.delete(V, sp[0], axis=0)).all()
    elif name == "velallnan":
        assert np.isnan(V).all()
    elif name == "velinf":
        with np.errstate(over="ignore"):
            V32 = V.astype(np.float32)
        assert np.isfinite(V).all()                                      # finite in binary64 ...
        assert (V32[sp[0]] == np.inf).all() and (V32[sp[1]] == -np.inf).all()      # ... and not in the flow targets
    elif name == "velulp":
        V32 = V.astype(np.float32)
        assert (V32 == V).all()
        for k in range(2):
            u = np.unique(V32[:, k])
            assert len(u) == 2 and np.nextafter(u[0], np.float32(np.inf)) == u[1]
            assert np.count_nonzero(V32[:, k] == u[1]) == 1
        assert coverage(sc, X).min() >= 1                                 # no pixel is left at the cleared 0
        _, fx, fy, _ = oracle_render(sc, X)
        for plane in (fx, fy):                                            # the rendered planes: two values, an ulp apart
            u = np.unique(plane)
            assert len(u) == 2 and np.nextafter(u[0], np.float32(np.inf)) == u[1], u


def oracle_render(sc, X):
    from oracle import ekf_ref
    dm = sc["mesh"]
    return ekf_ref.render(X, dm.size(), _tri(sc), np.asarray(dm.p, np.float32), sc["frame"], sc["W"], sc["H"])


def coverage(sc, X):
    """triangles over every pixel centre by the oracle's raster rule (labels 1: the id image counts)"""
    from oracle import ekf_ref
    dm = sc["mesh"]
    N = dm.size()
    t = _tri(sc)
    assert t.shape[0] < 255
    uv = np.asarray(dm.p, np.float32)
    return ekf_ref.render(X, N, t, uv, sc["frame"], sc["W"], sc["H"], labels=np.ones(t.shape[0], np.int64))[4]


def oracle_ids(sc, X, pal):
    """the id image (256 G + B) of the mask render at X under palette `pal` (None: -1), by the project's oracle"""
    from oracle import ekf_ref
    dm = sc["mesh"]
    t = _tri(sc)
    lab = np.full(t.shape[0], -1, np.int64) if pal is None else pal
    return ekf_ref.render(X, dm.size(), t, np.asarray(dm.p, np.float32), sc["frame"], sc["W"], sc["H"], labels=lab)[4]
