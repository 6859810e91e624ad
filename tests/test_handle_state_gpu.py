"""State a filter handle carries from one call to the next, out of the happy path's order.

A streaming caller queues the outline of the NEXT frame's mask a frame early (hm_update_arm_mask / hm_prepare_mask); the
preparation is matched to the next observation by device address, and frame ring slots are reused.  An update takes a
one-shot arm and leaves a tail block (Hz components, gains) for hm_update_tail.  Each test here sets up the case in which
stale state would give other numbers and asserts that it does (the aliasing precondition and a projection onto the stale
mask that differs from the one onto the right mask, both against oracle/ekf_ref.project_mask), then that the numbers are
the right ones: the pipeline bit for bit those of the sequential loop of host-observation calls, the handle's projection
that of the mask in place, and no tail after a failed update.
"""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

from oracle import ekf_ref

pytestmark = pytest.mark.gpu

N_PX, FRAMES, ERODE_FROM = 64, 24, 8


def _device_sync():
    """hipDeviceSynchronize of the HIP runtime the library uses: nothing queued on the handle's streams (the second one
    prepares outlines) still reads a device buffer the test rewrites next."""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64.so" in line:
                path = line.split()[-1]
                break
    assert path is not None, "the HIP runtime is not loaded"
    assert ctypes.CDLL(path).hipDeviceSynchronize() == 0


# ---- A: FlowEKFPipeline against the sequential loop when ring slots are reused ------------------------------------------
_VIDEO = {}


def _video():
    """A textured disk turning in place; the masks of frames ERODE_FROM.. are eroded by 5 px, so that the outline of a
    mask from before that frame and of one after it put the mesh's border vertices in different places.  The flow of
    every pair from single calls (the pipeline's flow is the same bits, test_pipeline_equals_sequential_calls)."""
    if not _VIDEO:
        from hydra_mi import brox, synth
        video, masks, c, r = synth.disk_video(N_PX, FRAMES, "rotate", 2)
        masks = masks.copy()
        for f in range(ERODE_FROM, FRAMES):
            masks[f] = ndimage.binary_erosion(masks[f], iterations=5).astype(np.uint8)
        bf = brox.BroxOpticalFlow(N_PX, N_PX)
        flows = [np.dstack(bf.calc(video[k], video[k + 1])) for k in range(FRAMES - 1)]
        bf.close()
        _VIDEO.update(video=video, masks=masks, c=c, r=r, flows=flows)
    return _VIDEO


def _new_filter(v):
    from hydra_mi import kalman, mesh
    zero = np.zeros((N_PX, N_PX, 2), np.float32)
    dm = mesh.disk_mesh(v["c"][0], v["c"][1], v["r"] - 1.0, 12.0)
    return kalman.IteratedMSKalmanFilter(dm, v["video"][0], zero, True, nI=2)


def _record(kf, e):
    return dict(X=kf.state.X.copy(), pred=np.array(kf.pred_x, np.float64).reshape(-1),
                proj=np.array(kf.proj_x, np.float64).reshape(-1), moved=int(kf.moved),
                err=tuple(float(x) for x in e[:4]), niter=int(kf.niter))


def _sequential(v, frames):
    """A fresh filter through the same observations by host calls: kf.compute(frame f, flow of (f-1, f), mask)."""
    kf = _new_filter(v)
    out = []
    for f, mask in frames:
        e = kf.compute(v["video"][f], v["flows"][f - 1], mask)
        out.append(_record(kf, e))
    W = np.array(kf.state.W)
    kf.close()
    return out, W


def _watch_next_mask(kf):
    """-> list of the next_mask address every compute() of kf is given (None: nothing queued ahead)."""
    seen = []
    compute = kf.compute

    def watched(y_im, *a, **kw):
        seen.append(getattr(y_im, "next_mask", None))
        return compute(y_im, *a, **kw)

    kf.compute = watched
    return seen


def _assert_teeth(rec, stale, right):
    """The frame's sequential projection is the oracle's onto the right mask, and one onto the stale mask differs."""
    N = rec["pred"].shape[0] // 4
    on_right = ekf_ref.project_mask(rec["pred"], N, right)[:, 0]
    on_stale = ekf_ref.project_mask(rec["pred"], N, stale)[:, 0]
    assert np.array_equal(rec["proj"], on_right)
    assert not np.array_equal(on_stale, on_right), "the stale and the right mask project the predicted state alike"


def _assert_same_track(got, want, W, Wref):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for key in ("X", "pred", "proj"):
            assert np.array_equal(g[key], w[key]), (i, key, np.abs(g[key] - w[key]).max())
        for key in ("moved", "err", "niter"):
            assert g[key] == w[key], (i, key, g[key], w[key])
    assert np.array_equal(W, Wref)


@pytest.mark.parametrize("concurrent", [True, False])
def test_phase_restart_onto_the_slot_of_a_prepared_mask(hm, concurrent):
    """A first phase run(0, 3) with flow_batch 4: calibrate() has frames 0..4 in the ring, so the last step could queue
    frame 4's outline; the next phase's first observation lands in frame 4's slot."""
    from hydra_mi.pipeline import FlowEKFPipeline
    v = _video()
    kf = _new_filter(v)
    got, pre = [], {}
    with FlowEKFPipeline(kf, v["video"], v["masks"], flow_batch=4, concurrent_series=concurrent) as pipe:
        ring = pipe.ring
        R = ring.R
        first2 = R + 3
        assert R < FRAMES and (first2 + 1) % R == 4 % R and first2 + 3 <= FRAMES - 1

        def on_frame(k, e):
            got.append(_record(kf, e))
            if k == 2:
                pre.update(synced=ring.lo <= 4 < ring.synced_hi, ptr=ring.ptr(1, 4))

        pipe.run(0, 3, on_frame=on_frame)
        pipe.run(first2, first2 + 3, on_frame=on_frame)
        assert pre["synced"], "frame 4's mask was not in the ring at the end of the first phase"
        assert ring.ptr(1, first2 + 1) == pre["ptr"]
        W = np.array(kf.state.W)
    kf.close()
    frames = [1, 2, 3, first2 + 1, first2 + 2, first2 + 3]
    want, Wref = _sequential(v, [(f, v["masks"][f]) for f in frames])
    _assert_teeth(want[3], stale=v["masks"][4], right=v["masks"][first2 + 1])
    _assert_same_track(got, want, W, Wref)


@pytest.mark.parametrize("concurrent", [True, False])
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_random_access_onto_the_slot_of_a_prepared_mask(hm, direction, concurrent):
    """step(0 .. k), where step(k) queued the outline of frame k + 2, then step(j) with frame j + 1 in the same slot:
    j = k + 1 + R (forward) or k + 1 - R (backward), then one step more."""
    from hydra_mi.pipeline import FlowEKFPipeline
    v = _video()
    kf = _new_filter(v)
    seen = _watch_next_mask(kf)
    got, frames = [], []
    with FlowEKFPipeline(kf, v["video"], v["masks"], flow_batch=2, concurrent_series=concurrent) as pipe:
        ring = pipe.ring
        R = ring.R
        assert R < FRAMES
        # forward: frame k + 2 before the eroded masks, k + 2 + R after; backward: k + 2 after, k + 2 - R before
        ks = range(1, ERODE_FROM - 2) if direction == "forward" else range(R - 1, ERODE_FROM + R - 2)
        jump = None
        for k in range(ks[-1] + 1):
            got.append(_record(kf, pipe.step(k)))
            frames.append(k + 1)
            if k in ks and seen[-1] is not None:
                jump = k + 1 + R if direction == "forward" else k + 1 - R
                break
        assert jump is not None, "no step queued the outline of the frame after next"
        assert seen[-1] == ring.ptr(1, k + 2) and ring.lo <= k + 2 < ring.synced_hi
        assert ring.ptr(1, jump + 1) == ring.ptr(1, k + 2) and jump + 2 <= FRAMES - 1
        for j in (jump, jump + 1):
            got.append(_record(kf, pipe.step(j)))
            frames.append(j + 1)
        W = np.array(kf.state.W)
    kf.close()
    want, Wref = _sequential(v, [(f, v["masks"][f]) for f in frames])
    _assert_teeth(want[k + 1], stale=v["masks"][k + 2], right=v["masks"][jump + 1])
    _assert_same_track(got, want, W, Wref)


@pytest.mark.parametrize("concurrent", [True, False])
def test_second_pipeline_on_the_same_filter(hm, concurrent):
    """A pipeline closed after a step that queued the outline of frame k + 2, then a new one on the same filter with other
    masks that goes on from frame k + 2.  Whether the new ring got the old one's memory is the allocator's business: it is
    printed, not asserted."""
    from hydra_mi.pipeline import FlowEKFPipeline
    v = _video()
    plain = (v["video"] > 20).astype(np.uint8)                  # (synth.disk_video's masks, none eroded)
    eroded = np.stack([ndimage.binary_erosion(m, iterations=5).astype(np.uint8) for m in plain])
    kf = _new_filter(v)
    seen = _watch_next_mask(kf)
    got, frames = [], []
    with FlowEKFPipeline(kf, v["video"], plain, flow_batch=2, concurrent_series=concurrent) as pipe:
        for k in range(FRAMES - 4):
            got.append(_record(kf, pipe.step(k)))
            frames.append((k + 1, plain[k + 1]))
            if k >= 1 and seen[-1] is not None:
                break
        old = pipe.ring.ptr(1, k + 2)
        assert seen[-1] == old and pipe.ring.lo <= k + 2 < pipe.ring.synced_hi
    with FlowEKFPipeline(kf, v["video"], eroded, flow_batch=2, concurrent_series=concurrent) as pipe:
        same = pipe.ring.ptr(1, k + 2) == old
        print("second pipeline's mask of frame %d at the first one's address: %s" % (k + 2, same))
        for j in (k + 1, k + 2):
            got.append(_record(kf, pipe.step(j)))
            frames.append((j + 1, eroded[j + 1]))
        W = np.array(kf.state.W)
    kf.close()
    want, Wref = _sequential(v, frames)
    _assert_teeth(want[k + 1], stale=plain[k + 2], right=eroded[k + 2])
    _assert_same_track(got, want, W, Wref)


# ---- B: the handle through the C-ABI -----------------------------------------------------------------------------------
class _Handle:
    """A renderer handle (the disk mesh of test_ekf_gpu._setup), an observation in device memory whose mask lives in the
    buffer `m`, two masks A and B, and a state whose projections onto A and onto B (the oracle's) differ."""

    def __init__(self, n=64, seed=11):
        from hydra_mi import mesh, renderer, synth
        from hydra_mi.pipeline import DeviceBuffer
        self.n = n
        dm = mesh.disk_mesh((n - 1) / 2.0, (n - 1) / 2.0, 0.31 * n, 11.0)
        self.N = N = dm.size()
        tex = synth.noise_texture(n, seed).astype(np.uint8)
        eps = (1e-3, 1.0, 1.0)
        self.R = renderer.Renderer(dm, np.zeros((N, 2)), np.zeros((n, n, 2), np.float32), n, tex, True, *eps)
        meas = ekf_ref.Measurement(N, dm.t, dm.p, tex, *eps)
        rng = np.random.default_rng(seed)
        Xobs = np.concatenate((dm.p.reshape(-1) + 1.5, np.full(2 * N, 0.5)))
        y_im, yfx, yfy, ym = meas.render(Xobs)
        self.y_im = y_im
        self.y_m = (ym // 255).astype(np.uint8)
        self.flow = (np.dstack((yfx, -yfy)) + rng.normal(0, 0.05, (n, n, 2))).astype(np.float32)
        self.X = np.concatenate((dm.p.reshape(-1) + rng.normal(0, 4.0, 2 * N), rng.normal(0, 1.0, 2 * N)))
        yy, xx = np.mgrid[:n, :n]
        self.A = ((xx - 0.5 * n) ** 2 + (yy - 0.45 * n) ** 2 < (0.3 * n) ** 2).astype(np.uint8)
        self.B = np.roll(self.A, 6, axis=1)
        self.want_A = ekf_ref.project_mask(self.X, N, self.A)[:, 0]
        self.want_B = ekf_ref.project_mask(self.X, N, self.B)[:, 0]
        assert not np.array_equal(self.want_A, self.want_B)
        self.bufs = [DeviceBuffer(n * n), DeviceBuffer(4 * n * n), DeviceBuffer(4 * n * n), DeviceBuffer(n * n)]
        d_im, d_fx, d_fy, self.m = self.bufs
        d_im.upload(np.ascontiguousarray(y_im, np.uint8))
        d_fx.upload(np.ascontiguousarray(self.flow[:, :, 0]))
        d_fy.upload(np.ascontiguousarray(self.flow[:, :, 1]))
        self.obs = renderer.DeviceObservation(d_im.ptr, d_fx.ptr, d_fy.ptr, self.m.ptr)

    def put(self, mask):
        """Rewrite the mask buffer (after everything queued that may still read it)."""
        _device_sync()
        self.m.upload(np.ascontiguousarray(mask, np.uint8))

    def host_observation(self):
        self.R.set_observation(self.y_im, self.flow, self.y_m)

    def projection_in_place(self):
        """projectmask of X onto the mask of the observation in place (the outline the handle holds for it)."""
        got, _ = self.R.project_mask(self.X)
        return got

    def close(self):
        _device_sync()
        self.R.close()
        for b in self.bufs:
            b.close()


def test_prepared_mask_then_host_observation_is_dropped(hm):
    """B1: a host observation between hm_prepare_mask(p) and hm_set_observation_dev(p) drops the preparation (the
    documented behaviour): p rewritten in between, the projection follows what p holds at the observation."""
    h = _Handle()
    try:
        h.put(h.A)
        h.R.prepare_mask(h.m.ptr)
        h.host_observation()
        h.put(h.B)
        h.R.set_observation_dev(h.obs)
        assert np.array_equal(h.projection_in_place(), h.want_B)
    finally:
        h.close()


def test_prepared_mask_discarded_with_null(hm):
    """B2: hm_prepare_mask(h, NULL) discards the preparation.  Without it the preparation stands by contract (the mask
    must not change until the observation that names it): rewriting p shows, so the discard is what the B result says."""
    h = _Handle()
    try:
        h.put(h.A)
        h.R.prepare_mask(h.m.ptr)
        h.R.set_observation_dev(h.obs)                      # the fast path: the outline prepared ahead is used
        assert np.array_equal(h.projection_in_place(), h.want_A)
        h.R.prepare_mask(h.m.ptr)
        h.put(h.B)
        h.R.set_observation_dev(h.obs)                      # not discarded: the outline of what p held when prepared
        assert np.array_equal(h.projection_in_place(), h.want_A)
        h.put(h.A)
        h.R.prepare_mask(h.m.ptr)
        h.R.prepare_mask(None)
        h.put(h.B)
        h.R.set_observation_dev(h.obs)
        assert np.array_equal(h.projection_in_place(), h.want_B)
        h.R.prepare_mask(None)                              # nothing prepared: a no-op
        h.R.set_observation_dev(h.obs)
        assert np.array_equal(h.projection_in_place(), h.want_B)
    finally:
        h.close()


def test_mask_arm_is_used_up_by_a_failed_update(hm):
    """B3: hm_update_arm_mask(p) is for the next hm_update_run only, whether that call succeeds or not.  A successful
    update prepares p (shown by rewriting p afterwards: the projection follows what p held); an update that fails on its
    arguments leaves nothing armed for the next, unrelated one."""
    h = _Handle()
    try:
        W = np.eye(4 * h.N) * 0.5
        h.host_observation()
        h.put(h.A)
        h.R.arm_mask(h.m.ptr)
        h.R.update_run(W, h.X, h.y_im, h.flow, h.y_m, 2, 1e-4)
        h.put(h.B)
        h.R.set_observation_dev(h.obs)
        assert np.array_equal(h.projection_in_place(), h.want_A)    # the armed outline, prepared by that update
        h.host_observation()
        h.put(h.A)
        h.R.arm_mask(h.m.ptr)
        with pytest.raises(RuntimeError):
            h.R.update_run(W, h.X, h.y_im, h.flow, h.y_m, 2, 1e-4, deltaX=0.0)
        h.R.update_run(W, h.X, h.y_im, h.flow, h.y_m, 2, 1e-4)       # a host observation, nothing armed
        h.put(h.B)
        h.R.set_observation_dev(h.obs)
        assert np.array_equal(h.projection_in_place(), h.want_B)
    finally:
        h.close()


def test_update_tail_only_after_a_successful_update(hm):
    """B4: hm_update_tail hands out the block of the last hm_update_run when that one succeeded -- the values the call
    would have returned itself, zeros without iterations -- and HM_ERR_STATE after one that failed."""
    h = _Handle()
    try:
        R, n4 = h.R, 4 * h.N
        good = np.eye(n4) * 0.5
        bad = good.copy()
        bad[5, 5] = -1.0
        h.host_observation()
        with pytest.raises(RuntimeError, match="code -3"):
            R.update_tail()                                 # no update yet
        X1, info, errs, Hzc, gains, _ = R.update_run(good, h.X, h.y_im, h.flow, h.y_m, 3, 1e-4)
        assert info["niter"] >= 1 and np.abs(gains).max() > 0 and np.all(np.isfinite(gains))
        X2, info2, _, Hz_none, g_none, _ = R.update_run(good, h.X, h.y_im, h.flow, h.y_m, 3, 1e-4, tail=False)
        assert Hz_none is None and g_none is None and np.array_equal(X2, X1) and info2 == info
        for _ in range(2):                                  # (until the next update_run)
            Hz_t, g_t = R.update_tail()
            assert np.array_equal(Hz_t, Hzc) and np.array_equal(g_t, gains)
        with pytest.raises(FloatingPointError):
            R.update_run(bad, h.X, h.y_im, h.flow, h.y_m, 3, 1e-4, tail=False)
        with pytest.raises(RuntimeError, match="code -3"):
            R.update_tail()
        R.update_run(good, h.X, h.y_im, h.flow, h.y_m, 3, 1e-4, tail=False)
        with pytest.raises(RuntimeError):
            R.update_run(good, h.X, h.y_im, h.flow, h.y_m, 3, 1e-4, deltaX=0.0, tail=False)
        with pytest.raises(RuntimeError, match="code -3"):
            R.update_tail()                                 # (an argument error counts as well)
        R.update_run(good, h.X, h.y_im, h.flow, h.y_m, 0, 1e-4, tail=False)
        Hz0, g0 = R.update_tail()
        assert not Hz0.any() and not g0.any()
        R.update_run(good, h.X, h.y_im, h.flow, h.y_m, 3, 1e-4, tail=False)
        Hz_t, g_t = R.update_tail()
        assert np.array_equal(Hz_t, Hzc) and np.array_equal(g_t, gains)
    finally:
        h.close()


def test_filter_gains_after_a_failed_compute(hm):
    """The same at the filter: after a compute() whose update fails, kf.tv / fv / mv raise instead of handing out the
    gains of the frame before; from the first frame's state again, compute() gives that frame's gains again."""
    from hydra_mi import kalman, mesh, synth
    video, flow = synth.test_data(64, 64)
    dm = mesh.box_mesh(21.0, 22.0, 42.0, 43.0, 10.0)
    kf = kalman.IteratedKalmanFilter(dm, video[:, :, 0], flow[:, :, :, 0], True, nI=2)
    frame = video[:, :, 1]
    mask = (frame > 0).astype(np.uint8)
    try:
        n4 = 4 * kf.state.N
        X0, W0 = kf.state.X.copy(), np.array(kf.state.W)
        kf.compute(frame, flow[:, :, :, 1], mask)
        tv = np.array(kf.tv)
        assert tv.shape == (n4,) and np.all(np.isfinite(tv)) and np.abs(tv).max() > 0
        assert np.all(np.isfinite(kf.fv)) and np.all(np.isfinite(kf.mv))
        bad = np.eye(n4) * 0.5
        bad[5, 5] = -1e3                                    # stays indefinite through the prediction
        kf.state.W = bad
        with pytest.raises(FloatingPointError):
            kf.compute(frame, flow[:, :, :, 1], mask)
        for name in ("tv", "fv", "mv"):
            with pytest.raises(RuntimeError, match="hm_update_tail"):
                getattr(kf, name)
        kf.state.X, kf.state.W = X0.copy(), W0.copy()
        kf.compute(frame, flow[:, :, :, 1], mask)
        assert np.array_equal(kf.tv, tv)
    finally:
        kf.close()
