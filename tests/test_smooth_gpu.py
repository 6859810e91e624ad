"""The RTS smoother on the device (hydra_mi.smooth, hm_smooth_*, csrc/smooth_kernels.h), `pytest -m gpu`:

  - recording changes nothing of the forward track (config 1, config 3), which still matches its golden;
  - what is recorded is what the filter kept (P_k bit for bit, m_k = the prior mean of the update), and the Pp_{k+1}
    the backward pass recomputes is the forward prior bit for bit -- on the fused, cov_ahead and chained paths;
  - xs, var and Ps_k against the NumPy restatement (tests/smooth_ref.py) on the same recorded inputs, one step and whole
    runs (config 1, config 3, 201 vertices at 1024^2), plus the smoother's invariants;
  - the three f64 matrix-core products alone against numpy on integer data (exact), edge tiles included;
  - the pipeline hook, the CLI's --smooth and a record past its capacity.
"""
import os
import sys

import numpy as np
import pytest

import smooth_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# relative Frobenius bounds against smooth_ref: one backward step / a whole run (the issue's starting figures)
TOL_STEP = 1e-10
TOL_RUN = 1e-8


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def _config1():
    from hydra_mi import mesh, synth
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    video, flow = synth.test_data(128, 128)
    return g, video, flow, lambda: mesh.Mesh(g["p"], g["t"], 15.0)


def _make_config1(path="chained"):
    from hydra_mi import kalman
    g, video, flow, dm = _config1()
    kf = kalman.IteratedMSKalmanFilter(dm(), video[:, :, 0], flow[:, :, :, 0], True)
    if path in ("fused", "cov_ahead"):
        kf.chain = False
        kf.cov_ahead = path == "cov_ahead"
    return kf


def _track_config1(kf, sm=None, frames=None, probe=None):
    g, video, flow, _ = _config1()
    out = []
    for k in range(g["X"].shape[0] if frames is None else frames):
        frame = video[:, :, k]
        e = kf.compute(frame, flow[:, :, :, k], (frame > 0).astype(np.uint8))
        if sm is not None:
            sm.record()
        if probe is not None:
            probe(k)
        out.append((kf.state.X.reshape(-1).copy(), kf.niter, tuple(e[:4])))
    return out


def _capture_priors(kf):
    """the prior covariance every update starts from, fetched from the device just before the update is called"""
    from hydra_mi.renderer import DeviceCovariance
    r = kf.state.renderer
    priors = []
    for name in ("update_run", "update_begin"):
        orig = getattr(r, name)

        def wrapped(W, *a, _orig=orig, **kw):
            priors.append(r.cov_fetch() if isinstance(W, DeviceCovariance) else np.array(W, np.float64))
            return _orig(W, *a, **kw)
        setattr(r, name, wrapped)
    return priors


def _ref_inputs(sm, K):
    bars, l0, kappa, a, s, eps_F = sm.model()
    P, x, m = [], [], []
    for k in range(K):
        Pk, xk, mk = sm.fetch(k)
        P.append(Pk); x.append(xk); m.append(mk)
    N = sm.N
    F = [smooth_ref.model_F(N, bars, l0, kappa, a, s, x[k]) for k in range(K - 1)]
    return P, np.array(x), np.array(m), F, smooth_ref.Weps(N, eps_F)


def _check_run(sm, K, tol, label):
    """run the smoother (means only, then with covariances) and hold it against smooth_ref and the invariants"""
    P, x, m, F, Q = _ref_inputs(sm, K)
    xs_ref, Ps_ref, _ = smooth_ref.smooth(P, x, m, F, Q)
    xs0, var0 = sm.run(covariances=False)
    assert var0 is None
    xs, var = sm.run(covariances=True)
    assert np.array_equal(xs0, xs), label                           # mean-only and full runs: the same bits
    assert np.array_equal(xs[K - 1], x[K - 1]), label               # the last frame is the filter's
    worst = 0.0
    for k in range(K):
        Ps = sm.cov(k)
        assert np.array_equal(Ps, Ps.T), (label, k)                 # exactly symmetric
        assert np.array_equal(np.diag(Ps), var[k]), (label, k)
        d, d0 = np.diag(Ps), np.diag(P[k])
        assert np.all(d <= d0 + 1e-12 * np.abs(d0) + 1e-300), (label, k)   # smoothing never adds uncertainty
        if k == K - 1:
            assert np.array_equal(Ps, P[k]), label
        worst = max(worst, _rel(xs[k], xs_ref[k]), _rel(Ps, Ps_ref[k]))
    print("%s: %d frames, worst relative difference to smooth_ref %.2e" % (label, K, worst))
    assert worst <= tol, (label, worst)
    return xs, var


# ---- the products alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [36, 100, 128, 804])
def test_products_against_numpy_exactly(hm, n):
    """Integer-valued operands: every sum is exact in f64, so a wrong element (a fragment-layout or edge-tile slip) is an
    exact mismatch.  n = 36, 100, 804 are not multiples of 16 or 32; 128 is a multiple of 32."""
    from hydra_mi import smooth
    rng = np.random.default_rng(n)
    A, B, C = (rng.integers(-4, 5, (n, n)).astype(np.float64) for _ in range(3))
    assert np.array_equal(smooth.gemm("tn", A, B), A.T @ B)
    assert np.array_equal(smooth.gemm("nnd", A, B, C), A @ (B - C))
    S = C + C.T
    want = np.tril(S + A @ B.T)
    want = want + np.tril(want, -1).T                              # the lower triangle, mirrored
    got = smooth.gemm("sym", A, B, S)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [20, 32, 36, 100, 260])
def test_triangular_products_against_numpy_exactly(hm, n):
    """The two products G = (T F P)^T T is formed by, on integer data (exact): only the lower triangle of the triangular
    operand counts -- what lies right of its diagonal is NaN here, as the factorisation may leave it, and must not reach
    the result.  n = 20: one partial tile; 32: one tile; 36: a 4-row last tile; 100, 260: several tiles, none full at the
    edge, so slabs left and right of the diagonal exist and the skipped ones are the right ones."""
    from hydra_mi import smooth
    rng = np.random.default_rng(1000 + n)
    T, B = (rng.integers(-4, 5, (n, n)).astype(np.float64) for _ in range(2))
    Tl = np.tril(T)
    Tnan = np.where(np.tri(n, dtype=bool), T, np.nan)
    assert np.array_equal(smooth.gemm("ln", Tnan, B), Tl @ B)
    assert np.array_equal(smooth.gemm("tl", B, Tnan), B.T @ Tl)


# ---- the forward track is untouched ---------------------------------------------------------------------------
def test_recording_changes_nothing_config1(hm):
    from hydra_mi.smooth import RTSSmoother
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    K = g["X"].shape[0]
    off = _track_config1(_make_config1())
    kf = _make_config1()
    with RTSSmoother(kf, K) as sm:
        on = _track_config1(kf, sm)
        assert len(sm) == K
    for k in range(K):
        assert np.array_equal(on[k][0], off[k][0]) and on[k][1] == off[k][1] and on[k][2] == off[k][2], k
        rel = np.linalg.norm(on[k][0] - g["X"][k]) / np.linalg.norm(g["X"][k])
        assert rel <= 1e-5 and on[k][1] == int(g["iters"][k]), k          # still the golden track


def _config3():
    from hydra_mi import brox, mesh, synth
    g = np.load(os.path.join(GOLD, "config3_track.npz"))
    n, frames = int(g["n"]), int(g["frames"])
    video, masks, centre, radius = synth.disk_video(n, frames, "warp", 0)
    bf = brox.BroxOpticalFlow(n, n)
    flows = [bf.calc(video[k - 1], video[k]) for k in range(1, frames)]
    bf.close()

    def make():
        from hydra_mi import kalman
        dm = mesh.disk_mesh(centre[0], centre[1], radius - 1.0, float(g["h0"]) * n)
        return kalman.IteratedMSKalmanFilter(dm, video[0], np.zeros((n, n, 2), np.float32), True)
    return g, video, masks, flows, make


def _track_config3(kf, video, masks, flows, sm=None):
    out = []
    for k in range(1, len(flows) + 1):
        u, v = flows[k - 1]
        e = kf.compute(video[k], np.dstack((u, v)), masks[k])
        if sm is not None:
            sm.record()
        out.append((kf.state.X.reshape(-1).copy(), kf.niter, tuple(e[:4])))
    return out


def test_config3_recording_changes_nothing_and_smooths(hm):
    from hydra_mi.smooth import RTSSmoother
    g, video, masks, flows, make = _config3()
    off = _track_config3(make(), video, masks, flows)
    kf = make()
    K = len(flows)
    with RTSSmoother(kf, K) as sm:
        on = _track_config3(kf, video, masks, flows, sm)
        for k in range(K):
            assert np.array_equal(on[k][0], off[k][0]) and on[k][1:] == off[k][1:], k
            Xg = g["X"][k]
            assert np.linalg.norm(on[k][0] - Xg) / np.linalg.norm(Xg) <= 1e-5, k
        _check_run(sm, K, TOL_RUN, "config 3")


# ---- what is recorded ----------------------------------------------------------------------------------------
def _disk_pipeline_filter():
    """a disk video at 128^2 through FlowEKFPipeline: the observations are in device memory, so compute() chains"""
    from hydra_mi import kalman, mesh, synth
    from hydra_mi.pipeline import FlowEKFPipeline
    n, frames = 128, 8
    video, masks, c, r = synth.disk_video(n, frames, "translate_leftup", 0)
    dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.12 * n)
    kf = kalman.IteratedMSKalmanFilter(dm, video[0], np.zeros((n, n, 2), np.float32), True)
    return kf, FlowEKFPipeline(kf, video, masks, flow_batch=4), frames - 1


@pytest.mark.parametrize("path", ["fused", "cov_ahead", "chained"])
def test_recorded_inputs_are_the_filters(hm, path):
    """P_k = the covariance the update kept (hm_cov_fetch) bit for bit, m_k = the prior mean of the update, x_k = the
    state; the Pp_{k+1} the backward pass recomputes = the prior the forward update k+1 started from, bit for bit.
    Fused and cov_ahead: config 1 in a compute() loop; chained: the pipeline (observations in device memory)."""
    from hydra_mi.smooth import RTSSmoother
    if path == "chained":
        kf, pipe, K = _disk_pipeline_filter()
    else:
        kf, pipe, K = _make_config1(path), None, 6
    priors = _capture_priors(kf)
    posts, means, chained_frames, states = [], [], [], []
    r = kf.state.renderer
    kf._chained_last = False
    orig_chained = kf._compute_chained

    def chained(*a, **kw):
        kf._chained_last = orig_chained(*a, **kw)
        return kf._chained_last
    kf._compute_chained = chained

    def probe(k, e=None):
        posts.append(r.cov_fetch())
        states.append(kf.state.X.reshape(-1).copy())
        chained_frames.append(kf._chained_last)
        if kf._chained_last:
            means.append(np.array(r.chain_states()[1]).reshape(-1))
        else:
            means.append(np.array(kf.proj_x, np.float64).reshape(-1))
    with RTSSmoother(kf, K) as sm:
        if pipe is None:
            _track_config1(kf, sm, frames=K, probe=probe)
        else:
            pipe.run(on_frame=probe, smoother=sm)
            pipe.close()
        assert any(chained_frames) == (path == "chained"), chained_frames
        assert len(priors) == K and len(sm) == K
        for k in range(K):
            P, x, m = sm.fetch(k)
            assert np.array_equal(P, posts[k]), (path, k)
            assert np.array_equal(x, states[k]), (path, k)
            assert np.array_equal(m, means[k]), (path, k)
            if k >= 1:
                assert np.array_equal(sm.prior(k), priors[k]), (path, k)
        # one backward step from identical inputs: the last two frames' values against smooth_ref
        P, x, m, F, Q = _ref_inputs(sm, K)
        xs, var = sm.run()
        xs_ref, Ps_ref, _ = smooth_ref.smooth(P[K - 2:], x[K - 2:], m[K - 2:], F[K - 2:], Q)
        assert _rel(xs[K - 2], xs_ref[0]) <= TOL_STEP, _rel(xs[K - 2], xs_ref[0])
        assert _rel(sm.cov(K - 2), Ps_ref[0]) <= TOL_STEP, _rel(sm.cov(K - 2), Ps_ref[0])


# ---- parity of whole runs --------------------------------------------------------------------------------------
def test_whole_run_config1(hm):
    from hydra_mi.smooth import RTSSmoother
    g = np.load(os.path.join(GOLD, "config1_track.npz"))
    K = g["X"].shape[0]
    kf = _make_config1()
    with RTSSmoother(kf, K) as sm:
        _track_config1(kf, sm)
        _check_run(sm, K, TOL_RUN, "config 1")


def _fullsize(frames):
    from hydra_mi import mesh, synth
    n = 1024
    video, masks, c, r = synth.disk_video(n, frames, "translate_leftup", 0)
    dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
    assert dm.size() == 201
    return n, video, masks, dm


def test_whole_run_201_vertices_and_pipeline(hm):
    """201 vertices at 1024^2 over a few frames: parity of the whole run, and FlowEKFPipeline.run(smoother=) records
    the same as the compute() loop."""
    from hydra_mi import brox, kalman, mesh
    from hydra_mi.pipeline import FlowEKFPipeline
    from hydra_mi.smooth import RTSSmoother
    frames = 5
    n, video, masks, dm = _fullsize(frames)

    def make():
        return kalman.IteratedMSKalmanFilter(mesh.Mesh(dm.p, dm.t, dm.h0), video[0], np.zeros((n, n, 2), np.float32), True)
    K = frames - 1
    kf, bf = make(), brox.BroxOpticalFlow(n, n)
    with RTSSmoother(kf, K) as sm:
        for k in range(K):
            u, v = bf.calc(video[k], video[k + 1])
            kf.compute(video[k + 1], np.dstack((u, v)), masks[k + 1])
            sm.record()
        xs_loop, var_loop = _check_run(sm, K, TOL_RUN, "201 vertices")
    kf2 = make()
    with RTSSmoother(kf2, K) as sm2:
        pipe = FlowEKFPipeline(kf2, video, masks, flow_batch=8)
        pipe.run(smoother=sm2)
        pipe.close()
        assert len(sm2) == K
        xs, var = sm2.run()
    assert np.array_equal(xs, xs_loop) and np.array_equal(var, var_loop)


# ---- the record's limits and the CLI ---------------------------------------------------------------------------
def test_record_past_capacity_is_refused_and_the_record_stays_usable(hm):
    from hydra_mi.smooth import RTSSmoother
    kf = _make_config1()
    with RTSSmoother(kf, 3) as sm:
        _track_config1(kf, sm, frames=3)
        before = [sm.fetch(k) for k in range(3)]
        g, video, flow, _ = _config1()
        frame = video[:, :, 3]
        kf.compute(frame, flow[:, :, :, 3], (frame > 0).astype(np.uint8))
        with pytest.raises(RuntimeError, match="the record is full"):
            sm.record()
        assert len(sm) == 3
        for k in range(3):
            after = sm.fetch(k)
            assert all(np.array_equal(a, b) for a, b in zip(after, before[k])), k
        xs, var = sm.run()
        assert xs.shape == (3, 4 * kf.N) and np.all(np.isfinite(var))
        assert np.array_equal(xs[2], before[2][1])
        with pytest.raises(RuntimeError, match="smoothed"):
            sm.record()
    kf2 = _make_config1()
    with RTSSmoother(kf2, 4) as sm2:
        _track_config1(kf2, sm2, frames=1)
        kf2.kappa = -2.0
        with pytest.raises(RuntimeError, match="springs or parameters changed"):
            sm2.record()
        assert len(sm2) == 1


def test_cli_smooth_keeps_every_key(hm, tmp_path):
    from hydra_mi import synth
    sys.path.insert(0, ROOT)
    import run_kalmanfilter
    n, F = 96, 5
    video, masks, c, r = synth.disk_video(n, F, "translate_leftup", 0)
    vid = str(tmp_path / "video.npy")
    np.save(vid, video)
    a, b = str(tmp_path / "plain.npz"), str(tmp_path / "smooth.npz")
    assert run_kalmanfilter.main([vid, str(tmp_path / "noflow"), a, "-s", "14"]) == 0
    assert run_kalmanfilter.main([vid, str(tmp_path / "noflow"), b, "-s", "14", "--smooth"]) == 0
    ra, rb = np.load(a), np.load(b)
    assert set(rb.files) == set(ra.files) | {"Xs", "Xs_std"}
    for key in ra.files:
        assert ra[key].dtype == rb[key].dtype and ra[key].tobytes() == rb[key].tobytes(), key
    K = ra["X"].shape[0]
    assert rb["Xs"].shape == ra["X"].shape == rb["Xs_std"].shape
    assert np.array_equal(rb["Xs"][K - 1], ra["X"][K - 1]) and np.all(rb["Xs_std"] > 0)
    # a video beyond the budget fails before tracking starts, with RTSSmoother's message
    with pytest.raises(ValueError, match="a record of 4 frames at .* vertices needs"):
        run_kalmanfilter.main([vid, str(tmp_path / "noflow"), str(tmp_path / "c.npz"), "-s", "14", "--smooth",
                               "--smooth-max-gb", "0.00001"])
    assert not os.path.exists(str(tmp_path / "c.npz"))
