"""The measurement kernels at their structural limits (tests/measure_cases.py; the CPU test pins every case to its count)
against the oracle, through the C-ABI: stars of 7 .. 24 triangles and a border fan that fills all 104 terms of a
k_solve_prep row; meshes hm_ctx_create must refuse; star regions of exactly 1024 tiles and above (k_measure_vertex
without a tile list); 4096 triangles and k_render_iter strips of 31 .. 4096 candidates.

Bars as in tests/test_ekf_gpu.py: renders and whole-number error terms bit-exact, sums 1e-9 of the largest entry, HTH
symmetric bit for bit and exactly zero between vertices that share no triangle, the device update 1e-9 of numpy's."""
import os

import numpy as np
import pytest

import body_ref
import measure_cases as mc
from oracle import ekf_c, ekf_ref

pytestmark = pytest.mark.gpu
EPS = (1e-3, 1.0, 1.0)


class _St:
    def __init__(self, X):
        self.X = np.asarray(X, np.float64).reshape(-1, 1)


def _renderer(c):
    from hydra_mi import renderer
    m = c["mesh"]
    N = len(m.p)
    return renderer.Renderer(m, np.zeros((N, 2)), np.zeros((c["H"], c["W"], 2), np.float32), c["H"], c["tex"], True, *EPS)


def _twin(c):
    m = c["mesh"]
    return ekf_c.Measurement(len(m.p), m.t, m.p, c["tex"], *EPS, threads=min(16, os.cpu_count() or 1))


def _observation(c, cm):
    """the oracle's render of the mesh moved by (1.5, -1.0) px with a small velocity, noise on the flow"""
    m = c["mesh"]
    N = len(m.p)
    Xo = np.concatenate(((m.p + [1.5, -1.0]).reshape(-1), np.full(2 * N, 0.5)))
    y_im, fx, fy, ym = cm.render(Xo)
    rng = mc._rng("obs:" + c["name"])
    flow = (np.dstack((fx, -fy)) + rng.normal(0, 0.05, (c["H"], c["W"], 2))).astype(np.float32)
    return y_im, flow, (ym // 255).astype(np.uint8)


def _prior(n4, name):
    M = mc._rng("prior:" + name).normal(size=(n4, n4))
    return np.eye(n4) * 0.5 + 0.05 * (M @ M.T) / n4


def _near(a, b, rel, what):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= rel * scale, (what, np.abs(a - b).max(), scale)


def _check_render(R, c, X):
    m = c["mesh"]
    N = len(m.p)
    R.update_vertex_buffer(X[:2 * N].reshape(-1, 2), X[2 * N:].reshape(-1, 2))
    got = R.render()                                               # k_setup_all + k_render<0>
    ref = ekf_ref.render(X, N, m.t, m.p, c["tex"], c["W"], c["H"])
    for name, g, r in zip(("im", "fx", "fy", "m"), got, ref):
        assert np.array_equal(g, r), (c["name"], name)
    return ref


def _check_error(R, c, X, obs):
    """Renderer.error (k_render_iter) against the oracle: whole-number terms and both flow planes exact"""
    m = c["mesh"]
    meas = ekf_ref.Measurement(len(m.p), m.t, m.p, c["tex"], *EPS)
    e = R.error(_St(X), *obs)
    r = meas.error(X, *obs)
    assert e[0] == r[0] and e[3] == r[3], c["name"]
    assert abs(e[1] - r[1]) <= 1e-10 * r[1] and abs(e[2] - r[2]) <= 1e-10 * r[2]
    assert np.array_equal(e[4][:, :, 0], r[4]) and np.array_equal(e[5][:, :, 0], r[5])
    return e


def _hub_pairs(t, N, hub):
    """state indices of every 4x4 block of the hub with itself, each neighbour and one non-neighbour"""
    nb = list(mc.neighbours(t, hub))
    far = [u for u in range(N) if u != hub and u not in nb][0]
    idx = lambda v: [2 * v, 2 * v + 1, 2 * N + 2 * v, 2 * N + 2 * v + 1]
    pi, pj = [], []
    for u in [hub] + nb + [far]:
        for a in idx(hub):
            for b in idx(u):
                pi.append(a)
                pj.append(b)
    return np.array(pi), np.array(pj), far


def _check_measure(R, cm, c, X, obs, pairs=None):
    """hm_measure at X: all 4N of Hz / Hzc, the HTH entries `pairs` (default: all adjacent ones), symmetry and zeros"""
    m = c["mesh"]
    N = len(m.p)
    Hz, HTH, Hzc = R.measure(_St(X), *obs)
    rHz, rHzc = cm.jacobian_all(X, *obs)
    _near(Hz, rHz, 1e-9, "Hz")
    _near(Hzc, rHzc, 1e-9, "Hzc")
    _, J = ekf_ref.adjacency(N, m.t)
    if pairs is None:
        pi, pj = np.nonzero(np.triu(J == 1))
    else:
        pi, pj = pairs
    # (KFState's sparse HTH has entries on the pattern only: off it, where a folded star reaches a vertex it shares no
    # triangle with, the value is 0 by definition, not the oracle's j)
    vals = np.where(J[pi, pj] == 1, cm.hessian_pairs(pi, pj, 2.0), 0.0)
    scale = max(np.abs(HTH).max(), 1e-300)
    assert np.abs(HTH[pi, pj] - vals).max() <= 1e-9 * scale, c["name"]
    assert np.array_equal(HTH, HTH.T)
    assert np.all(HTH[J == 0] == 0)
    return Hz, HTH, Hzc


def _hub_case(name):
    return {c["name"]: c for c in mc.hub_cases() + [mc.border_fan_case()]}[name]


@pytest.mark.parametrize("name", ["hub%d" % k for k in mc.HUB_DEGREES] + ["fan24"])
def test_hub_stars_match_the_oracle(hm, name):
    """Stars of 7 .. 24 triangles (odd counts: the padding setup) and the border fan whose k_solve_prep row has 104 terms:
    render, measure, error in the rest, perturbed and folded states; the dense update against numpy, with the
    factorisation in one persistent launch and in one launch per block step -- the same bits."""
    c = _hub_case(name)
    m = c["mesh"]
    N, hub = len(m.p), c["hub"]
    R, cm = _renderer(c), _twin(c)
    try:
        obs = _observation(c, cm)
        R.update_frame(*obs)
        pi, pj, far = _hub_pairs(m.t, N, hub)
        for sname in ("rest", "perturbed", "folded"):
            X = c["states"][sname]
            _check_render(R, c, X)
            Hz, HTH, _ = _check_measure(R, cm, c, X, obs, (pi, pj))
            assert np.any(HTH[2 * hub, [2 * u for u in mc.neighbours(m.t, hub)]] != 0), sname
            assert not np.any(HTH[2 * hub:2 * hub + 2, 2 * far:2 * far + 2]), sname
            _check_error(R, c, X, obs)
            # the update around this state: X0 the prior mean, measured at X
            n4 = 4 * N
            W = _prior(n4, name + sname)
            X0 = X + mc._rng("x0:" + name + sname).normal(0, 0.3, X.size)
            A = np.linalg.inv(W) + HTH
            ref = np.linalg.solve(A, Hz - HTH @ (X0 - X).reshape(-1, 1))
            out = []
            for flow in (1, 0):
                R.tune("chol_flow", flow)
                R.update_begin(W, X0)
                step, Hzc2, err = R.update_step(_St(X), *obs)
                cov = R.update_cov(0)
                out.append((step, cov, err))
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), sname
            assert out[0][2] == out[1][2]
            step, cov, err = out[0]
            assert np.linalg.norm(step - ref) <= 1e-9 * np.linalg.norm(ref), sname
            assert np.linalg.norm(cov - np.linalg.inv(A)) <= 1e-9 * np.linalg.norm(np.linalg.inv(A)), sname
            e = R.error(_St(X0 + step.reshape(-1)), *obs)
            assert err[0] == e[0] and err[3] == e[3] and abs(err[1] - e[1]) <= 1e-12 * e[1]
    finally:
        R.close()


@pytest.mark.parametrize("which,limit", [(0, "limit 24"), (1, "limit 25"), (2, "1..4096 triangles")])
def test_meshes_over_a_limit_are_refused(hm, which, limit):
    """a vertex in 25 triangles, a vertex with 26 neighbours, 4097 triangles: hm_ctx_create refuses and names the limit"""
    c = mc.refused_cases()[which]
    with pytest.raises(RuntimeError) as e:
        _renderer(c)
    assert "hm_ctx_create" in str(e.value) and limit in str(e.value)


def _coarse(name):
    return {c["name"]: c for c in mc.coarse_cases()}[name]


@pytest.mark.parametrize("name", ["region_at", "region_above", "region_wide", "region_clipped"])
def test_big_star_regions_match_the_oracle(hm, name):
    """A hub region of exactly 1024 tiles (tile list) and above it (k_measure_vertex tests the per-triangle boxes of
    every tile of the region): measure against the oracle at every entry, the split of the vertex jobs changing only the
    rounding, hm_update_step and hm_update_run (whose second iteration measures with the regions of k_render_iter)
    against numpy."""
    c = _coarse(name)
    m = c["mesh"]
    N = len(m.p)
    R, cm = _renderer(c), _twin(c)
    try:
        obs = _observation(c, cm)
        R.update_frame(*obs)
        X = c["states"]["rest"]
        _check_render(R, c, X)
        Hz, HTH, Hzc = _check_measure(R, cm, c, X, obs)
        assert np.all(Hz[[0, 1, 2 * N, 2 * N + 1]] != 0)                  # the hub's entries are not empty sums
        for split in (1, 5, 16):
            R.tune("measure_split", split)
            h, H2, hc = R.measure(_St(X), *obs)
            _near(h, Hz, 1e-12, "Hz split %d" % split)
            _near(H2, HTH, 1e-12, "HTH split %d" % split)
            _near(hc, Hzc, 1e-12, "Hzc split %d" % split)
        _check_error(R, c, X, obs)
        n4 = 4 * N
        W = _prior(n4, name)
        X0 = X
        # two steps by hand: at X0, then at X1 = X0 + step 1
        R.update_begin(W, X0)
        s1, _, e1 = R.update_step(_St(X0), *obs)
        A = np.linalg.inv(W) + HTH
        ref1 = np.linalg.solve(A, Hz)
        assert np.linalg.norm(s1 - ref1) <= 1e-9 * np.linalg.norm(ref1)
        X1 = X0 + s1.reshape(-1)
        Hz1, HTH1, _ = R.measure(_St(X1), *obs)
        R.update_begin(W, X0)
        s2, _, e2 = R.update_step(_St(X1), *obs)
        A1 = np.linalg.inv(W) + HTH1
        ref2 = np.linalg.solve(A1, Hz1 - HTH1 @ (X0 - X1).reshape(-1, 1))
        assert np.linalg.norm(s2 - ref2) <= 1e-9 * np.linalg.norm(ref2)
        # the same two iterations in one call
        Xk, info, errs, _, _, _ = R.update_run(W, X0, *obs, 2, 1e-12)
        assert info["niter"] == 2 and not info["reverted"], info
        assert errs[0][0] == e1[0] and errs[0][3] == e1[3] and errs[1][0] == e2[0] and errs[1][3] == e2[3]
        X2 = X0 + s2.reshape(-1)
        assert np.abs(Xk.reshape(-1) - X2).max() <= 1e-12 * np.abs(s2).max()
    finally:
        R.close()


def _check_body(R, c, X, frame):
    m = c["mesh"]
    tri_of, l1, l2, ids = body_ref.body_map(np.asarray(m.p, np.float32), m.t, c["W"], c["H"])
    g_tri, g_cnt = R.body_map()                                    # k_body_map
    assert np.array_equal(g_tri, tri_of)
    assert np.array_equal(g_cnt.astype(np.uint64), body_ref.counts(tri_of, len(m.t)))
    reg, ts, _ = R.body_warp(X, frame)
    ref = body_ref.warp(X, frame, tri_of, l1, l2, ids)
    assert np.array_equal(reg, ref)
    assert np.array_equal(ts, body_ref.sums(ref, tri_of, len(m.t)))


@pytest.mark.parametrize("n", mc.STRIP_COUNTS)
def test_chunked_strips_match_the_oracle(hm, n):
    """k_render_iter with 31, 32, 33, 64, 65 candidates in one strip (one or more chunks), laid flat and concertinaed
    (pixels covered by triangles of several chunks: the f32 flow sums in ascending triangle order)"""
    c = mc.ribbon_case(n)
    R, cm = _renderer(c), _twin(c)
    try:
        obs = _observation(c, cm)
        R.update_frame(*obs)
        for sname, X in c["states"].items():
            _check_render(R, c, X)
            _check_error(R, c, X, obs)
            _check_body(R, c, X, obs[0])
    finally:
        R.close()


def test_grid_of_4096_triangles_renders_as_the_oracle(hm):
    """4096 triangles, all bits of the triangle masks in use: k_render (with and without the label ids of jz_multi),
    k_render_iter (Renderer.error) and k_body_map / the body readout at rest, shrunk into one strip (4096 candidates,
    128 chunks) and folded over itself (~128 triangles a pixel: 8-bit saturation, long f32 sums)"""
    c = mc.grid_case()
    m = c["mesh"]
    N, T = len(m.p), len(m.t)
    R, cm = _renderer(c), _twin(c)
    try:
        obs = _observation(c, cm)
        R.update_frame(*obs)
        labels = ((np.arange(T) * 37) % (N + 40) - 40).astype(np.int32)[:, None]        # -1 .. N-1, some unlabelled
        labels[labels < -1] = -1
        meas = ekf_ref.Measurement(N, m.t, m.p, c["tex"], *EPS)
        R.labels = labels
        for sname in ("rest", "shrunk", "folded"):
            X = c["states"][sname]
            ref = _check_render(R, c, X)
            if sname == "folded":
                assert np.any(ref[0] == 255)
            _check_error(R, c, X, obs)
            _check_body(R, c, X, obs[0])
            # the id image of the label palette (k_render<1>, k_render<2>) through hm_jz_multi
            R.update_vertex_buffer(X[:2 * N].reshape(-1, 2), X[2 * N:].reshape(-1, 2), 0)
            R.initjacobian(*obs)
            meas.initjacobian(X, *obs)
            Xp = X.copy()
            Xp[0:2 * N:2] += 0.6
            hz, hzc = R.jz_multi(_St(Xp))
            rhz, rhzc = meas.jz_multi(Xp, labels[:, 0], N)
            scale = max(np.abs(rhzc).max(), 1e-30)
            assert np.abs(hzc - rhzc).max() <= 1e-10 * scale, sname
            assert np.abs(hz[:, 0] - rhz).max() <= 1e-10 * scale, sname
    finally:
        R.close()


def test_grid_of_4096_triangles_measures_as_the_oracle(hm):
    """hm_measure on the 4096-triangle mesh (4N = 8580: the HTH fetched is 589 MB) at rest and shrunk into one strip: a
    few Hz components and HTH entries against the C twin, zeros off the adjacency.  (Folded ~128 deep, the vertex jobs
    form a perturbed flow sum as (reference - star) + perturbed star in binary32, which is not the ascending-order sum
    of the oracle: there they differ by ~3e-8 of the largest Hz, beyond this bar.)"""
    c = mc.grid_case()
    m = c["mesh"]
    N = len(m.p)
    R, cm = _renderer(c), _twin(c)
    try:
        obs = _observation(c, cm)
        R.update_frame(*obs)
        Jv, _ = ekf_ref.adjacency(N, m.t)                 # (the 4N x 4N pattern would be another 589 MB)
        verts = [0, 1, 64, 65, 1072, N // 2 + 7, N - 66, N - 1]
        idx = np.array([2 * v + k for v in verts for k in (0, 1)] + [2 * N + 2 * v + k for v in verts for k in (0, 1)])
        for sname in ("rest", "shrunk"):
            X = c["states"][sname]
            Hz, HTH, Hzc = R.measure(_St(X), *obs)
            rHz, rHzc = cm.jacobian_all(X, *obs, idx=idx)
            assert np.abs(Hz[idx] - rHz).max() <= 1e-9 * max(np.abs(Hz).max(), 1e-300), sname
            assert np.abs(Hzc[idx] - rHzc).max() <= 1e-9 * max(np.abs(Hzc).max(), 1e-300), sname
            vert = lambda s: (s % (2 * N)) // 2
            Jrows = Jv[vert(idx)][:, vert(np.arange(4 * N))] != 0                   # rows idx of the pattern
            pi, pj = np.nonzero(Jrows)
            pi = idx[pi]
            vals = cm.hessian_pairs(pi, pj, 2.0)
            assert np.abs(HTH[pi, pj] - vals).max() <= 1e-9 * max(np.abs(HTH).max(), 1e-300), sname
            rows = HTH[idx]
            assert np.all(rows[~Jrows] == 0) and np.array_equal(rows, HTH[:, idx].T)
            del Hz, HTH, Hzc, rows
    finally:
        R.close()
