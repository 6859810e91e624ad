"""The tracker's views at their limits on the GPU (`pytest -m gpu`): k_view_wire, k_view_minmax, k_view_compose,
k_view_arrows and k_flow_preview (csrc/view_kernels.h) against the NumPy restatement of tests/view_ref.py at the scenes
and states of tests/view_cases.py -- segments clipped by every frame side, end points at and past 2^20, non-finite
vertices and velocities, the byte-wise tail of the compose kernel (W H % 4 = 1, 2, 3), the mask palette channel by
channel against the oracle's id image, arrows of length 0 and off the frame, hm_view_dev into a caller's buffer and what
it refuses.  Every comparison is an equality on all H x W x 3 bytes unless it says otherwise.  The states are inputs
whose result include/hydra_mi.h defines (segments skipped, triangles refused), as in test_body_gpu.py."""
import ctypes

import numpy as np
import pytest

import view_cases
import view_ref

pytestmark = pytest.mark.gpu
C20 = view_cases.C20
HM_ERR_ARG = -1


@pytest.fixture(scope="module")
def rigs(hm):
    """scene name -> (scene, filter): one filter per scene for the whole module"""
    made = {}

    def get(name):
        if name not in made:
            sc = view_cases.scene(name)
            made[name] = (sc, view_cases.make_filter(sc))
        return made[name]
    yield get
    for _, kf in made.values():
        kf.close()


_expected = {}


def _at(rigs, scene, state):
    """-> (scene, renderer, X, Renderer.render() at X, the restated wireframe counts); computed once per (scene, state)"""
    sc, kf = rigs(scene)
    r = kf.state.renderer
    key = (scene, state)
    if key not in _expected:
        X = view_cases.state(sc, state)
        N = r.n
        r.update_vertex_buffer(X[:2 * N], X[2 * N:])
        render = tuple(a.copy() for a in r.render())
        _expected[key] = (X, render, view_ref.wire_count(r.tri, X[:2 * N], r.nx, r.ny))
    X, render, wire = _expected[key]
    return sc, r, X, render, wire


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist(), got[got != want][:5], want[got != want][:5])


CASES = [(s, st) for s in view_cases.SCENES for st in view_cases.STATES if st != "far" or s == "33x17"]


@pytest.mark.parametrize("scene,state", CASES)
def test_views_at_every_state(rigs, scene, state):
    sc, r, X, render, wire = _at(rigs, scene, state)
    for which in ("raw", "overlay", "texture", "flowx", "flowy"):
        got = r.view(X, which)
        want = view_ref.view(which, render, r.tri, X, obs=sc["frame"], wire=wire)
        _same(got, want, (scene, state, which))
    W, H, N = r.nx, r.ny, r.n
    if state == "inside":
        assert wire.max() >= 2                                            # interior edges are drawn twice
    if state == "far":
        # the two vertices that round to 2^20 are drawn: without them the frame's wireframe is another
        sp = view_cases.special(sc, state)
        Xn = X.copy()
        Xn[2 * sp[0]] = Xn[2 * sp[1]] = np.nan
        assert not np.array_equal(wire, view_ref.wire_count(r.tri, Xn[:2 * N], W, H))
    if state == "nonfinite":
        assert wire.any()                                                 # only their segments vanish
    if state == "collapsed":
        assert (wire >= 3).any()
    if state == "folded":
        assert (render[0] == 255).any()


@pytest.mark.parametrize("scene", view_cases.SCENES)
@pytest.mark.parametrize("state", view_cases.MASK_STATES)
def test_mask_view_channel_by_channel(rigs, scene, state):
    """G, B and R of the mask view against the oracle's id image (oracle/ekf_ref.render(labels=palette)) at the state"""
    sc, r, X, render, wire = _at(rigs, scene, state)
    keep = r.labels_hess
    seen = dict(g_mid=False, g_ne_b=False, wire_sat=False, overlap_sat=False)
    try:
        for pname in view_cases.PALETTES:
            pal = view_cases.palette(sc, pname)
            r.labels_hess = None if pal is None else np.stack((pal, pal), axis=1)
            got = r.view(X, "mask")
            ids = view_cases.oracle_ids(sc, X, pal)
            want = view_ref.ids_view(ids, wire, render[3])
            _same(got, want, (scene, state, pname))
            b, g = want[:, :, 0].astype(int), want[:, :, 1].astype(int)
            seen["g_mid"] |= bool(((g != 0) & (g != 255)).any())
            seen["g_ne_b"] |= bool((g != b).any())
            seen["wire_sat"] |= bool(((ids % 256 < 255) & (wire > 0) & (b == 255)).any())
            if pname == "high":                                           # 65534: B = 254; two of them over a pixel: 508 -> 255
                cover = view_cases.coverage(sc, X)
                seen["overlap_sat"] |= bool(((cover >= 2) & (wire == 0) & (b == 255)).any())
    finally:
        r.labels_hess = keep
    assert seen["g_mid"] and seen["g_ne_b"] and seen["wire_sat"], seen
    if state == "folded":
        assert seen["overlap_sat"], seen


@pytest.mark.parametrize("scene", view_cases.SCENES)
def test_flow_views_at_degenerate_planes(rigs, scene):
    """The non-finite rule of hm_view: a pixel that is not finite takes no part in min / max and shows 0; no finite
    pixel or max == min: every pixel 0."""
    for state in ("vel0", "velallnan"):
        sc, r, X, render, _ = _at(rigs, scene, state)
        for which in ("flowx", "flowy"):
            assert not r.view(X, which).any(), (scene, state, which)
    sc, r, X, render, _ = _at(rigs, scene, "velallnan")
    assert np.isnan(render[1]).any() and not np.isfinite(render[1][render[3] > 0]).any()
    sc, r, X, render, _ = _at(rigs, scene, "velulp")
    for which, plane in (("flowx", render[1]), ("flowy", render[2])):
        u = np.unique(plane)
        assert len(u) == 2 and np.nextafter(u[0], np.float32(np.inf)) == u[1]
        got = r.view(X, which)
        assert set(np.unique(got).tolist()) == {0, 255}
        assert np.array_equal(got[:, :, 0] == 255, plane == u[1])
    for state in ("velnan", "velinf"):
        sc, r, X, render, _ = _at(rigs, scene, state)
        for which, plane in (("flowx", render[1]), ("flowy", render[2])):
            bad = ~np.isfinite(plane)
            assert bad.any() and (~bad).any()
            if state == "velinf":
                assert np.isinf(plane).any() or np.isnan(plane).any()
            got = r.view(X, which)
            _same(got, view_ref.view(which, render, r.tri, X), (scene, state, which))
            assert not got[bad].any()
            fin = plane[~bad].astype(np.float64)
            lo, hi = fin.min(), fin.max()
            assert hi > lo
            assert np.array_equal(got[:, :, 0][~bad], np.floor(255.0 * (fin - lo) / (hi - lo)).astype(np.uint8))
            assert got.max() == 255                                       # the finite maximum, not an infinity, is white


def _force_inputs(sc, r, X):
    """orig, pred, tv, fv, mv of one force plot with every arrow case of hm_view_forces in it, and the vertex of each"""
    W, H, N = r.nx, r.ny, r.n
    assert N >= 14
    rng = np.random.default_rng(11)
    pred = X[:2 * N].reshape(N, 2).copy()
    orig = pred + rng.normal(0, 2, pred.shape)
    tv, fv, mv = (rng.normal(0, 0.8, pred.shape) for _ in range(3))
    orig[0], orig[1] = pred[0], pred[1]                                   # zero-length shafts and heads
    pred[2] = (-0.7, 3.2)                                                 # C truncation: pixel (0, 3); a floor would drop it
    pred[3] = (5.3, -0.4)
    orig[3] = (-0.9, -0.2)                                                # (0, 0) -> (5, 0)
    tv[4] = (-float(W), 0.3)                                              # tips off the left, right, top, bottom side
    fv[5] = (float(W), -0.2)
    mv[6] = (0.1, -float(H))
    tv[7] = (-0.3, float(H))
    tv[8] = (np.nan, 0.4)                                                 # no arrow of tv at vertex 8
    fv[9] = (C20 / 10.0 + 5.0, 0.0)                                       # pred + 10 fv past 2^20: the whole arrow absent
    orig[10] = (-C20, C20)                                                # exactly at the limit: drawn
    orig[11] = (C20, -C20)
    orig[12] = pred[12]                                                   # four arrows on one pixel: the last layer stays
    tv[12] = fv[12] = mv[12] = (0.01, 0.01)
    mv[13] = (np.inf, 0.0)
    return orig, pred, tv, fv, mv


@pytest.mark.parametrize("scene", view_cases.SCENES)
def test_forces_at_arrow_limits(rigs, scene):
    sc, r, X, render, wire = _at(rigs, scene, "inside")
    W, H, N = r.nx, r.ny, r.n
    orig, pred, tv, fv, mv = _force_inputs(sc, r, X)
    assert (pred[9] + 10.0 * fv[9])[0] > C20 and abs(orig[10]).max() == C20
    assert -1 < pred[2, 0] < 0 and -1 < pred[3, 1] < 0 and (-1 < orig[3]).all() and (orig[3] < 0).all()
    for v, vec, side in ((4, tv, 0), (5, fv, 1), (6, mv, 2), (7, tv, 3)):
        tip = pred[v] + 10.0 * vec[v]
        assert [tip[0] < 0, tip[0] >= W, tip[1] < 0, tip[1] >= H][side]
    overlay = view_ref.view("overlay", render, r.tri, X, obs=sc["frame"], wire=wire)
    want = view_ref.forces(overlay, orig, pred, tv, fv, mv, N)
    got = r.view_forces(X, orig, pred, tv, fv, mv)
    _same(got, want, (scene, "forces"))
    # in the expected image: the last layer (0, 0, 255) is what remains where the four arrows of vertex 12 meet
    x, y = int(pred[12, 0]), int(pred[12, 1])
    assert want[y, x].tolist() == [0, 0, 255]
    assert want[3, 0].tolist() != (overlay[3, 0] >> 1).tolist()           # the start in (-1, 0) is on pixel (0, 3)
    if scene == "33x17":
        # the arrows from exactly +-2^20 are visible: without them the picture is another; the one past 2^20 is absent:
        # with its vector zeroed (a dot at pred, below the red layer's own dot) the picture is the same
        o2 = orig.copy()
        o2[10] = o2[11] = np.nan
        assert not np.array_equal(view_ref.forces(overlay, o2, pred, tv, fv, mv, N), want)
        f2 = fv.copy()
        f2[9] = 0.0
        assert np.array_equal(view_ref.forces(overlay, orig, pred, tv, f2, mv, N), want)


@pytest.mark.parametrize("scene", view_cases.ODD_SCENES)
def test_view_dev_into_a_callers_buffer(rigs, scene):
    """hm_view_dev at W H % 4 = 1, 2, 3: byte for byte hm_view, the buffer overwritten completely"""
    import torch
    sc, r, X, render, wire = _at(rigs, scene, "inside")
    n = 3 * r.nx * r.ny
    stream = torch.cuda.Stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    keep = r.labels_hess
    try:
        r.labels_hess = None                                              # the mask view: every byte 0 or 255
        want = {w: r.view(X, w) for w in ("overlay", "mask", "flowx")}
        assert not (want["mask"] == 0xAA).any()
        buf = torch.empty(n + 8, dtype=torch.uint8, device="cuda")      # 8 bytes behind the view: the tail writes bytes, no dword
        assert buf.data_ptr() % 4 == 0 and n % 4 != 0
        for first in ("overlay", "flowx", "mask"):
            buf.fill_(0xAA)
            torch.cuda.synchronize()
            r.view_dev(X, first, buf.data_ptr(), sp)
            with torch.cuda.stream(stream):
                got = buf.cpu().numpy()
            _same(got[:n].reshape(r.ny, r.nx, 3), want[first], (scene, first))
            assert (got[n:] == 0xAA).all()
            # a second view into the same buffer, not refilled: nothing of the first, nothing of the fill survives
            torch.cuda.synchronize()
            r.view_dev(X, "mask", buf.data_ptr(), sp)
            with torch.cuda.stream(stream):
                got = buf.cpu().numpy()
            _same(got[:n].reshape(r.ny, r.nx, 3), want["mask"], (scene, first, "then mask"))
            assert not (got[:n] == 0xAA).any() and (got[n:] == 0xAA).all()
        torch.cuda.synchronize()
    finally:
        r.labels_hess = keep


def test_refusals_launch_nothing_and_leave_the_handle_usable(rigs):
    import torch
    from hydra_mi import _lib
    sc, r, X, render, wire = _at(rigs, "35x17", "inside")
    L = _lib.lib()
    n = 3 * r.nx * r.ny
    x = np.ascontiguousarray(X, np.float64)
    out = np.empty((r.ny, r.nx, 3), np.uint8)
    buf = torch.full((n + 4,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for off in (1, 2, 3):
        rc = L.hm_view_dev(r._h, _lib.ptr(x), 1, None, ctypes.c_void_p(buf.data_ptr() + off), None)
        assert rc == HM_ERR_ARG
        msg = L.hm_last_error().decode()
        assert "hm_view_dev" in msg and "4-byte aligned" in msg, msg
    for which in (-1, 6, 7, 1 << 20):
        assert L.hm_view_dev(r._h, _lib.ptr(x), which, None, ctypes.c_void_p(buf.data_ptr()), None) == HM_ERR_ARG
        assert "outside 0..5" in L.hm_last_error().decode()
        assert L.hm_view(r._h, _lib.ptr(x), which, None, _lib.ptr(out)) == HM_ERR_ARG
        assert "outside 0..5" in L.hm_last_error().decode()
    assert L.hm_view_dev(None, _lib.ptr(x), 1, None, ctypes.c_void_p(buf.data_ptr()), None) == HM_ERR_ARG
    assert L.hm_view_dev(r._h, None, 1, None, ctypes.c_void_p(buf.data_ptr()), None) == HM_ERR_ARG
    assert L.hm_view_dev(r._h, _lib.ptr(x), 1, None, None, None) == HM_ERR_ARG
    assert L.hm_view(r._h, None, 1, None, _lib.ptr(out)) == HM_ERR_ARG
    assert L.hm_view(r._h, _lib.ptr(x), 1, None, None) == HM_ERR_ARG
    assert L.hm_view(None, _lib.ptr(x), 1, None, _lib.ptr(out)) == HM_ERR_ARG
    assert "NULL" in L.hm_last_error().decode()
    zeros = [np.zeros(2 * r.n) for _ in range(5)]
    f = [_lib.ptr(a) for a in zeros]
    assert L.hm_view_forces(r._h, _lib.ptr(x), f[0], f[1], None, f[3], f[4], _lib.ptr(out)) == HM_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == 0xAA).all())                                      # nothing was launched
    # afterwards the same handle produces a correct view, into the same buffer at an aligned address
    stream = torch.cuda.Stream()
    r.view_dev(X, "overlay", buf.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    with torch.cuda.stream(stream):
        got = buf.cpu().numpy()
    want = view_ref.view("overlay", render, r.tri, X, obs=sc["frame"], wire=wire)
    _same(got[:n].reshape(r.ny, r.nx, 3), want, "after the refusals")
    assert (got[n:] == 0xAA).all()                                        # and nothing past W H 3 bytes
    _same(r.view(X, "overlay"), want, "hm_view after the refusals")
    torch.cuda.synchronize()


@pytest.mark.parametrize("channels", [1, 3])
def test_flow_preview_at_the_wheels_edges(hm, channels):
    """k_flow_preview on three 35 x 17 frames (1785 pixels: seven workgroups, the last one partly filled): exact where the
    wheel is defined black or the flow is zero, within the existing bound elsewhere, and every difference within one
    level of the binary64 wheel."""
    from hydra_mi import videoio
    n, H, W = 3, 17, 35
    assert (n * H * W) % 256 != 0
    rng = np.random.default_rng(channels)
    fx = rng.uniform(-30, 30, (n, H, W)).astype(np.float32)
    fy = rng.uniform(-30, 30, (n, H, W)).astype(np.float32)
    f32 = np.float32
    nan, inf, e9 = f32(np.nan), f32(np.inf), f32(1e9)
    assert float(e9) == 1e9
    above15 = np.nextafter(f32(15), inf)
    below9 = np.nextafter(e9, f32(0))
    black = [(nan, 0), (0, nan), (nan, nan), (inf, 0), (-inf, 0), (0, inf), (0, -inf), (inf, -inf), (e9, 0), (-e9, 0), (0, e9),
             (0, -e9), (e9, e9), (f32(3e38), 1), (nan, inf), (e9, 3), (-2, -e9)]
    zero = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (f32(1e-30), 0), (0, f32(-1e-42))]         # (the last two: rad underflows to 0)
    coloured = [(15, 0), (-15, 0), (0, 15), (0, -15), (15, -0.0), (above15, 0), (-above15, 0), (0, above15), (0, -above15),
                (below9, 0), (0, -below9), (-below9, below9), (6, 7), (-20, 3)]
    vec = black + zero + coloured
    # the list at the start of the first frame, across the workgroup seam at pixel 256 and at the very end (the tail)
    flat_x, flat_y = fx.reshape(-1), fy.reshape(-1)
    spots = {}
    for base in (0, 256 - len(black) - 1, flat_x.size - len(vec)):
        for k, (a, b) in enumerate(vec):
            flat_x[base + k], flat_y[base + k] = a, b
            spots[base + k] = "black" if k < len(black) else "zero" if k < len(black) + len(zero) else "coloured"
    shape = (n, H, W) if channels == 1 else (n, H, W, 3)
    frames = rng.integers(0, 256, shape).astype(np.uint8)
    got = videoio.flow_preview(frames, fx, fy)
    assert got.shape == (n, H, W, 3) and got.dtype == np.uint8
    want = view_ref.flow_preview(frames, fx, fy)
    want64 = view_ref.flow_preview(frames, fx, fy, wheel_fn=view_ref.wheel64)
    f3 = (frames if channels == 3 else np.repeat(frames[..., None], 3, axis=-1)).astype(np.int64)
    plain = ((4 * f3 + 5) // 10).astype(np.uint8).reshape(-1, 3)
    g, w, w64 = got.reshape(-1, 3), want.reshape(-1, 3), want64.reshape(-1, 3)
    exact = np.array(sorted(p for p, kind in spots.items() if kind != "coloured"))
    assert np.array_equal(w[exact], plain[exact]) and np.array_equal(w64[exact], plain[exact])
    assert np.array_equal(g[exact], plain[exact]), [p for p in exact if not np.array_equal(g[p], plain[p])][:5]
    col = np.array(sorted(p for p, kind in spots.items() if kind == "coloured"))
    assert (view_ref.wheel(flat_x[col], flat_y[col]).max(axis=1) > 0).all()             # coloured: not black
    assert (np.abs(g[col].astype(int) - plain[col].astype(int)).max(axis=1) > 0).all()
    # (15, 0) is full saturation, the next binary32 above it three quarters
    assert view_ref.wheel(f32([15]), f32([0])).max() == 255 and view_ref.wheel(f32([above15]), f32([0])).max() == 191
    # elsewhere: at most one level, in at most the share of pixels test_views_gpu.py allows its grid of vectors
    d = np.abs(g.astype(int) - w.astype(int))
    assert d.max() <= 1, d.max()
    assert np.count_nonzero(d) <= (n * H * W) // 100, np.count_nonzero(d)
    # the restatement itself, and every pixel where the kernel differs from it, within one level of the binary64 wheel
    assert np.abs(w.astype(int) - w64.astype(int)).max() <= 1
    assert (np.abs(g.astype(int) - w64.astype(int))[d > 0] <= 1).all()
