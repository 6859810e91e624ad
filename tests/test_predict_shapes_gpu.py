"""The mass-spring prediction kernels at the launch shapes where their work split changes (tests/predict_cases.py):

A  k_ms_newton4 (hm_newton_dev_start / _finish): one to four waves, 256 lanes full, DEG = 8 and 12 with and without
   padding slots, more springs than lanes, the LDS limit; against the host loop (hm_ms_newton) -- same Newton
   iterations, 1e-12 -- and against the oracle's dense Newton (1e-9) where it is affordable; refusals; the table cache.
B  the same through the worker (hm_ms_newton_start / _finish) and through whole IteratedMSKalmanFilter tracks, device
   prediction (chained predict -> projectmask -> update) against the host loop.
C  k_ms_newton (hm_ms_predict) with more vector entries than threads, at and past its LDS limit.
D  k_fw_rows / k_pft_cols (hm_cov_predict) against the dense F W F^T + Weps of the oracle's dfdy.

The device sums over the whole vector in another order than the host: the two agree to rounding, not to the bit.  Where
no device kernel runs (a refused mesh) the numbers are the host's, bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

import predict_cases as pc
from predict_cases import host_newton, oracle_newton
from oracle import ekf_ref

pytestmark = pytest.mark.gpu

PARAMS = {"defaults": pc.DEFAULTS, "dt_0.12": dict(pc.DEFAULTS, dt=0.12), "maxiter_2": dict(pc.DEFAULTS, maxiter=2)}

_BUILD = {c: (lambda c=c: next(x for x in pc.grid_cases() if x["name"] == c))
          for c in ("grid_8x8", "grid_5x13", "grid_8x16", "grid_3x43", "grid_12x16", "grid_12x16_fan", "config4",
                    "grid_15x17", "grid_16x16", "grid_16x16_fan", "grid_15x20")}
_BUILD.update({"wheel_%d" % k: (lambda k=k: pc.wheel_case(k)) for k in pc.WHEELS})
_BUILD.update({"circulant_64_r6": pc.circulant_case, "pendant_65": pc.pendant_case, "isolated_65": pc.isolated_case,
               "lds4_256_1327": lambda: pc.newton4_lds_case(1327), "lds4_256_1328": lambda: pc.newton4_lds_case(1328)})
FITS = ["grid_8x8", "grid_5x13", "grid_8x16", "grid_3x43", "grid_12x16", "grid_12x16_fan", "config4", "grid_15x17",
        "grid_16x16", "wheel_8", "wheel_9", "wheel_12", "circulant_64_r6", "pendant_65", "isolated_65", "lds4_256_1327"]
# a vertex with 13 springs; 40 bytes of LDS over 64 KiB; N = 257 and 300 > 256 lanes
REFUSED = ["wheel_13", "lds4_256_1328", "grid_16x16_fan", "grid_15x20"]


@functools.lru_cache(maxsize=None)
def _case(name):
    return _BUILD[name]()


def _renderer(p, t, n=64):
    from hydra_mi import mesh, renderer, synth
    N = p.shape[0]
    tex = synth.noise_texture(n, 1).astype(np.uint8)
    return renderer.Renderer(mesh.Mesh(p, t), np.zeros((N, 2)), np.zeros((n, n, 2), np.float32), n, tex, True, 1e-3, 1.0, 1.0)


@pytest.fixture(scope="module")
def handles(hm):
    """a filter handle per vertex count (the prediction calls take the springs as arguments: the handle fixes N)"""
    hs = {}

    def get(c):
        N = c["N"]
        if N not in hs:
            p, t = (c["p"], c["t"]) if c["t"] is not None else pc.handle_mesh(N)
            hs[N] = _renderer(p, t)
        return hs[N]
    yield get
    for R in hs.values():
        R.close()


@pytest.fixture(scope="module")
def worker(hm):
    from hydra_mi import _lib
    w = _lib.c_vp()
    _lib.check(_lib.lib().hm_ms_worker_create(ctypes.byref(w)), "hm_ms_worker_create")
    yield w
    _lib.lib().hm_ms_worker_destroy(w)


def dev_newton(R, c, kappa, M, dt, maxiter, tol, bars=None, l0=None):
    """hm_newton_dev_start / _finish -> (rc of the start, X, Newton iterations); X None when refused"""
    from hydra_mi import _lib
    L = _lib.lib()
    bars = c["bars"] if bars is None else bars
    l0 = c["l0"] if l0 is None else l0
    X = c["X"].copy()
    rc = L.hm_newton_dev_start(R._h, int(c["N"]), int(bars.shape[0]), _lib.ptr(bars), _lib.ptr(l0), float(kappa), float(M),
                               float(dt), int(maxiter), float(tol), _lib.ptr(X))
    assert rc in (0, 1), _lib.lib().hm_last_error()
    if rc:
        return rc, None, None
    its = ctypes.c_int()
    _lib.check(L.hm_newton_dev_finish(R._h, _lib.ptr(X), ctypes.byref(its)), "hm_newton_dev_finish")
    return 0, X, its.value


def _close(X, ref, rel):
    return np.abs(X - ref).max() <= rel * np.abs(ref).max()


# ---- A: k_ms_newton4 directly ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FITS)
def test_newton4_matches_host_loop(handles, name):
    c = _case(name)
    R = handles(c)
    for param, par in PARAMS.items():
        rc, Xd, itd = dev_newton(R, c, **par)
        assert rc == 0, (name, param)
        Xh, ith = host_newton(c, **par)
        assert itd == ith, (name, param, itd, ith)
        assert _close(Xd, Xh, 1e-12), (name, param, np.abs(Xd - Xh).max())
        assert np.abs(Xd - c["X"]).max() > 1.0
    if c["N"] <= 129:
        rc, Xd, _ = dev_newton(R, c, **pc.DEFAULTS)
        ref = oracle_newton(c, **pc.DEFAULTS)
        assert _close(Xd, ref, 1e-9), (name, np.abs(Xd - ref).max())


@pytest.mark.parametrize("name", REFUSED)
def test_newton4_refuses(handles, name):
    c = _case(name)
    rc, _, _ = dev_newton(handles(c), c, **pc.DEFAULTS)
    assert rc == 1


def test_newton4_table_cache(hm):
    """one handle, the springs changing between calls: A, B (more springs: new buffers), a graph it refuses (13 springs
    at two vertices), A again (tables rebuilt in the buffers of B), A with other rest lengths (tables kept, rest lengths
    uploaded).  Every result is the host's for the springs of that call."""
    a, b = _case("grid_8x8"), _case("circulant_64_r6")
    R = _renderer(a["p"], a["t"])
    try:
        par = pc.DEFAULTS
        _, Xa, ia = dev_newton(R, a, **par)
        for c in (a, b):
            Xh, ih = host_newton(c, **par)
            rc, Xd, idv = dev_newton(R, c, **par)
            assert rc == 0 and idv == ih and _close(Xd, Xh, 1e-12), c["name"]
        deg13 = np.ascontiguousarray(np.vstack((b["bars"], [[0, 32]])), np.int32)
        assert pc.degrees(64, deg13).max() == 13
        assert dev_newton(R, b, **par, bars=deg13, l0=pc.rest_lengths(b["p"], deg13))[0] == 1
        rc, Xd, idv = dev_newton(R, a, **par)
        assert rc == 0 and idv == ia and np.array_equal(Xd, Xa)                 # deterministic: the first A, bit for bit
        a2 = dict(a, l0=np.ascontiguousarray(a["l0"] * 1.05))
        Xh, ih = host_newton(a2, **par)
        rc, Xd, idv = dev_newton(R, a2, **par)
        assert rc == 0 and idv == ih and _close(Xd, Xh, 1e-12)
        assert np.abs(Xd - Xa).max() > 1e-3                                      # (the rest lengths do matter)
    finally:
        R.close()


# ---- B: through the worker and the filter ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", FITS + REFUSED)
def test_worker_routes_to_device_or_host(handles, worker, name):
    from hydra_mi import _lib
    L = _lib.lib()
    c = _case(name)
    R = handles(c)
    par = pc.DEFAULTS
    R.attach_worker(worker)
    try:
        X = c["X"].copy()
        _lib.check(L.hm_ms_newton_start(worker, int(c["N"]), int(c["I"]), _lib.ptr(c["bars"]), _lib.ptr(c["l0"]),
                                        par["kappa"], par["M"], par["dt"], par["maxiter"], par["tol"], _lib.ptr(X)),
                   "hm_ms_newton_start")
        its = ctypes.c_int()
        _lib.check(L.hm_ms_newton_finish(worker, _lib.ptr(X), ctypes.byref(its)), "hm_ms_newton_finish")
    finally:
        R.detach_worker(worker)
    if name in REFUSED:
        want, wits = host_newton(c, **par)
    else:
        _, want, wits = dev_newton(R, c, **par)
    assert its.value == wits and np.array_equal(X, want)


# The tracks run on synth.test_data(384, 384): on the 128-px frame the box is 43 px wide, and with 64 or 256 vertices on it
# (6 or 2.8 px apart) hm_update_run already fails in frame 1 -- "inv(W) + HTH is not positive definite" -- with the host
# prediction as with the device one.  Here the vertices are 8.5 px apart and more; the prediction is what is compared.
TRACK_PX = 384


def _track(p, t, h0, on_device, frames=3):
    """IteratedMSKalmanFilter on synth.test_data, the observations in device memory (so that the chained path may be
    taken) -> [(X, niter, newton_iterations)], the results of hm_chain_project"""
    from hydra_mi import kalman, mesh, synth
    from hydra_mi.pipeline import DeviceBuffer
    from hydra_mi.renderer import DeviceObservation
    n = TRACK_PX
    video, flow = synth.test_data(n, n)
    bufs, obs = [], []
    for k in range(1, frames + 1):
        b = [DeviceBuffer(n * n), DeviceBuffer(4 * n * n), DeviceBuffer(4 * n * n), DeviceBuffer(n * n)]
        b[0].upload(np.ascontiguousarray(video[:, :, k]))
        b[1].upload(np.ascontiguousarray(flow[:, :, 0, k]))
        b[2].upload(np.ascontiguousarray(flow[:, :, 1, k]))
        b[3].upload((video[:, :, k] > 0).astype(np.uint8))
        bufs += b
        obs.append(DeviceObservation(*[x.ptr for x in b]))
    kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(p, t, h0), video[:, :, 0], flow[:, :, :, 0], True)
    kf.newton_on_device = on_device
    r = kf.state.renderer
    chained = []
    chain_project = r.chain_project

    def counted():
        chained.append(chain_project())
        return chained[-1]
    r.chain_project = counted
    out = []
    try:
        for o in obs:
            kf.compute(o, None, None)
            out.append((kf.state.X.copy(), kf.niter, kf.newton_iterations))
    finally:
        kf.close()
        for b in bufs:
            b.close()
    return out, chained


def _on_the_box(p, n=TRACK_PX):
    """a mesh of tests/predict_cases.py moved onto the box of synth.test_data(n, n) (rows / columns n/3 .. 2n/3)"""
    lo, hi = p.min(0), p.max(0)
    start, end = n // 3, 2 * n // 3
    return start + 0.5 + (p - lo) * ((end - start - 1.0) / (hi - lo).max())


def test_filter_track_device_prediction_at_256(hm):
    """N = 256, every lane busy: the device prediction is chained into the next update (frames 2 and 3) and gives the
    host loop's iterations and states to 1e-9"""
    p, t = pc.grid(16, 16)
    p = _on_the_box(p)
    dev, chained = _track(p, t, 8.5, True)
    host, none = _track(p, t, 8.5, False)
    assert chained == [True, True] and none == []
    for a, b in zip(dev, host):
        assert a[1:] == b[1:]
        assert _close(a[0], b[0], 1e-9), np.abs(a[0] - b[0]).max()


@pytest.mark.parametrize("which", ["fan_257", "wheel_13"])
def test_filter_track_refused_mesh_declines_the_chain(hm, which):
    """a mesh the kernel refuses: the worker takes the host loop, hm_chain_project declines, and the track is the one
    without the device prediction, bit for bit"""
    if which == "fan_257":
        p, t = pc.fan_onto_border(*pc.grid(16, 16), 16)
    else:
        p, t = pc.wheel(8, 8, **pc.WHEELS[13])
    assert p.shape[0] == 257 or pc.degrees(p.shape[0], pc.bars_of(t)).max() == 13
    p = _on_the_box(p)
    dev, chained = _track(p, t, 8.0, True)
    host, none = _track(p, t, 8.0, False)
    assert chained == [False, False] and none == []
    for a, b in zip(dev, host):
        assert a[1:] == b[1:] and np.array_equal(a[0], b[0])


# ---- C: k_ms_newton through hm_ms_predict ----------------------------------------------------------------------------
def _spd(n4, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n4, n4))
    return np.eye(n4) * 0.3 + 0.02 * (A @ A.T) / n4


def _blocks(c, X, kappa=-1.0):
    """per spring (Bxx, Bxy, Byy) of dfdy at the positions of X (IteratedMSKalmanFilter._spring_blocks)"""
    y = X[:2 * c["N"]].reshape(-1, 2)
    d = y[c["bars"][:, 0]] - y[c["bars"][:, 1]]
    l = np.sqrt((d * d).sum(1))
    k, cc = kappa * (1 - c["l0"] / l), kappa * c["l0"] / (l * l * l)
    return np.column_stack((k + cc * d[:, 0] * d[:, 0], cc * d[:, 0] * d[:, 1], k + cc * d[:, 1] * d[:, 1]))


def _dense_prediction(c, X, W, dt=0.05, M=1.0, eps_F=0.1, kappa=-1.0):
    """F W F^T + Weps with F = [[I, dt I], [dt/M dfdy, I]] from the oracle's dense dfdy at the positions of X"""
    N = c["N"]
    K = ekf_ref.incidence(N, c["bars"])
    dfdy = ekf_ref.ms_dfdy(K, c["l0"], X[:2 * N], kappa)
    e = np.eye(2 * N)
    F = np.block([[e, dt * e], [(dt / M) * dfdy, e]])
    _, Weps, _ = ekf_ref.initial_covariances(N, eps_F)
    return F @ W @ F.T + Weps


@pytest.mark.parametrize("name", ["grid_3x43", "grid_16x16", "lds_300_1124", "lds_300_1125"])
def test_ms_predict_past_one_pass(handles, name):
    """k_ms_newton strides 2N and 4N over 512 threads: one pass at N = 129 (4N > 512 already), two at 256 and 300; at
    I = 1124 its LDS footprint is the largest that fits 160 KiB, at 1125 hm_ms_predict takes the host loop"""
    if name.startswith("lds"):
        c = pc.newton_lds_case(int(name[-4:]))
    else:
        c = _case(name)
    R = handles(c)
    N = c["N"]
    on_device = pc.lds_newton(N, c["I"]) <= pc.NEWTON_LDS_MAX
    assert on_device == (name != "lds_300_1125")
    W = _spd(4 * N, N)
    tok = R.cov_predict(W, None, None, 0.0, 0.0, 0.0, fetch=False)
    par = pc.DEFAULTS
    Xp, its, tokp = R.ms_predict(tok, c["X"], c["bars"], c["l0"], par["kappa"], par["M"], par["dt"], par["maxiter"],
                                 par["tol"], 0.1)
    Xh, ith = host_newton(c, **par)
    assert its == ith
    if on_device:
        assert _close(Xp[:, 0], Xh, 1e-12), np.abs(Xp[:, 0] - Xh).max()
    else:
        assert np.array_equal(Xp[:, 0], Xh)
    if N <= 129:
        ref = _dense_prediction(c, c["X"], W)
        Wp = tokp.fetch()
        assert np.linalg.norm(Wp - ref) <= 1e-11 * np.linalg.norm(ref)


# ---- D: k_fw_rows / k_pft_cols through hm_cov_predict ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid_3x43", "grid_16x16", "wheel_12"])
def test_cov_predict_shapes(handles, name):
    c = _case(name)
    R = handles(c)
    N = c["N"]
    W = _spd(4 * N, N + 1)
    blk = _blocks(c, c["X"])
    ref = _dense_prediction(c, c["X"], W)
    got = R.cov_predict(W, c["bars"], blk, 0.05, 0.05, 0.1)                          # W uploaded
    assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref)
    tok = R.cov_predict(W, None, None, 0.0, 0.0, 0.0, fetch=False)                   # W itself, resident on the device
    assert np.array_equal(tok.fetch(), W)
    res = R.cov_predict(tok, c["bars"], blk, 0.05, 0.05, 0.1)                        # propagated where it is
    assert np.array_equal(res, got)
