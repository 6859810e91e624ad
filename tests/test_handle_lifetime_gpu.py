"""Handle lifetime: a filter handle and a flow handle give back every buffer, stream and event they build.

Each cycle, at the bench's frame size and mesh (1024^2, mesh.disk_mesh at h0 0.047: 201 vertices), builds a filter and
a flow handle and drives every group of resources the filter handle builds on first use: a short chained track through
the streaming pipeline with its Newton worker attached (the prediction's stream and blocks, the tail's stream and event,
the armed mask, the covariance prediction queued ahead), a projection onto a host mask and onto the mask in place,
contour pruning, the multi-perturbation operators, two covariance predictions of which the second has more springs than
any before it (the spring arrays grow), the views and the force plot, the body-frame readout -- the body map, a label
image of a few discs, three warps with the statistics and a record of a few frames both on, the summary images, the
peaks and one reduction of the record over a seed -- and a flow handle whose CU mask is changed and dropped.  Then
everything is closed, the filter handle with its statistics and its record still open.  Free device memory after the last
cycle is what it was after the first, or more: earlier tests of the same process may still give memory back (objects the
collector frees late), which the collections here bring forward but cannot rule out; a handle that keeps what it built
shows as less.  The statistics' sums and images are 48 MiB per handle at this size, more than the slack in one cycle; the
record's few frames are less than the slack, so for the record this covers faults when the handle is destroyed, not
leaks.
"""
import ctypes
import gc
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PX, FRAMES, CYCLES = 1024, 6, 6
SLACK = 32 << 20


def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the library uses (the device the handles were built on is current)."""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64.so" in line:
                path = line.split()[-1]
                break
    assert path is not None, "the HIP runtime is not loaded"
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert ctypes.CDLL(path).hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _cycle(video, masks, centre, radius):
    from hydra_mi import body, brox, kalman, mesh
    from hydra_mi.pipeline import FlowEKFPipeline
    from oracle import partitions_ref

    dm = mesh.disk_mesh(centre[0], centre[1], radius - 1.0, 0.047 * N_PX)
    kf = kalman.IteratedMSKalmanFilter(dm, video[0], np.zeros((N_PX, N_PX, 2), np.float32), True)
    pipe = FlowEKFPipeline(kf, video, masks, flow_batch=2)
    try:
        pipe.run(0, FRAMES - 1)
        pipe.flow_sync()
        R, st = kf.state.renderer, kf.state
        N = R.n
        X = np.asarray(st.X, np.float64).reshape(-1)
        assert N == 201
        assert R.project_mask(X)[0].shape == X.shape                  # the mask in place
        assert R.project_mask(X, masks[1])[0].shape == X.shape        # a host mask
        assert R.prune_mask(masks[2]).shape == (N_PX, N_PX)

        R.initjacobian(video[1], np.zeros((N_PX, N_PX, 2), np.float32), masks[1])
        E, labels = partitions_ref.jacobian_partitions(N, dm.t)
        Q, EH, _, lh = partitions_ref.hessian_partitions(N, dm.t)
        R.labels, R.labels_hess, R.Q = labels, lh, Q
        v = types.SimpleNamespace(X=X.reshape(-1, 1))
        R.update_vertex_buffer(X[:2 * N].reshape(-1, 2), X[2 * N:].reshape(-1, 2), 0)
        hz, _ = R.jz_multi(v)
        assert hz.shape == (N, 1)
        e = np.asarray(EH[0]).reshape(-1, 2)
        h, _, _ = R.j_multi(v, 2.0, np.column_stack((2 * e[:, 0], 2 * e[:, 1])), 0)
        assert h.shape == (1, len(Q))

        W = np.eye(4 * N)
        bars = np.asarray(dm.bars, np.int32)
        R.cov_predict(W, bars, np.ones((len(bars), 3)), 0.05, 0.05, 0.1)
        more = np.vstack((bars, bars))                                # more springs than the track has had
        assert R.cov_predict(W, more, np.ones((len(more), 3)), 0.05, 0.05, 0.1).shape == W.shape

        assert R.view(X, "overlay").shape == (N_PX, N_PX, 3)
        assert R.view_forces(X, X, X, X, X, X).shape == (N_PX, N_PX, 3)

        tri_of, _ = R.body_map()
        cx, cy = centre
        pts = np.array([(cx, cy), (cx - 0.3 * radius, cy), (cx, cy + 0.3 * radius)])
        R.body_set_labels(body.disc_labels(tri_of, pts, 3.0), len(pts))
        R.body_stats_begin()
        R.body_rec_begin(body.record_bytes(tri_of, 4))
        for k in range(3):
            reg, _, ls = R.body_warp(X, video[k])
            assert reg.shape == (N_PX, N_PX) and ls.shape == (len(pts),)
        assert R.body_stats_images()[0].shape == (N_PX, N_PX)
        assert R.body_stats_peaks("corr", 6)[2] >= 0
        seed = np.array([[int(cx), int(cy)]], np.int32)
        assert tri_of[seed[0, 1], seed[0, 0]] >= 0
        assert R.body_rec_seed_sums(seed, 3.0, 6.0, 8.5, 4)["T"].shape == (3, 1)
        assert R.body_stats_count() == 3 and R.body_rec_count() == 3     # (both still open when the handle is closed)
    finally:
        pipe.close()
        kf.close()

    bf = brox.BroxOpticalFlow(N_PX, N_PX)
    try:
        bf.tune("cu_reserve", 32)
        u, _ = bf.calc(video[0], video[1])
        assert np.isfinite(u).all()
        bf.tune("cu_reserve", 16)
        bf.tune("cu_reserve", 0)
    finally:
        bf.close()


def test_handles_give_back_their_device_memory(hm):
    from hydra_mi import synth
    video, masks, centre, radius = synth.disk_video(N_PX, FRAMES, "translate_leftup", 0)
    gc.collect()
    free = []
    for _ in range(CYCLES):
        _cycle(video, masks, centre, radius)
        gc.collect()
        free.append(_free_device_memory())
    assert free[0] - free[-1] <= SLACK, "free device memory after each cycle (MiB): %s" % [f >> 20 for f in free]
