"""Scenes for the GPU tests of the statistics of the registered video: the meshes, states and frames of
tests/test_body_gpu.py (the same builder), and the filter they run on."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ["16", "33x17", "96x160", "config1", "config4"]


def make_filter(dm, frame):
    from hydra_mi import kalman
    H, W = frame.shape
    return kalman.IteratedMSKalmanFilter(dm, frame, np.zeros((H, W, 2), np.float32), True)


def scene(name):
    """-> (mesh, states, frames, frame 0)"""
    from hydra_mi import mesh, synth
    rng = np.random.default_rng(len(name))
    if name == "16":
        dm = mesh.box_mesh(2.0, 3.0, 13.0, 12.5, 4.0)
        frames = [rng.integers(0, 256, (16, 16), dtype=np.uint8) for _ in range(3)]
    elif name == "33x17":                                   # an odd pixel count, rows that are no multiple of 4 pixels
        dm = mesh.box_mesh(3.0, 2.0, 30.0, 14.5, 5.0)
        frames = [rng.integers(0, 256, (17, 33), dtype=np.uint8) for _ in range(3)]
    elif name == "96x160":
        dm = mesh.disk_mesh(80.0, 47.5, 40.0, 9.0)
        frames = [rng.integers(0, 256, (96, 160), dtype=np.uint8) for _ in range(3)]
    elif name == "config1":
        g = np.load(os.path.join(GOLD, "config1_track.npz"))
        video, _ = synth.test_data(128, 128)
        return mesh.Mesh(g["p"], g["t"], 15.0), list(g["X"]), [video[:, :, k] for k in range(10)], video[:, :, 0]
    else:
        g = np.load(os.path.join(GOLD, "config4_track.npz"))
        n = int(g["n"])
        video, _, _, _ = synth.disk_video(n, int(g["frames"]), "translate_leftup", 0)
        return mesh.Mesh(g["p"], g["t"], float(g["h0"]) * n), list(g["X"]), [video[k + 1] for k in range(3)], video[0]
    N = dm.size()
    Xs = []
    for s in (0.0, 0.7, 2.5):
        X = np.concatenate((np.asarray(dm.p, np.float64).reshape(-1) + rng.normal(0, s, 2 * N), rng.normal(0, 1, 2 * N)))
        Xs.append(X)
    return dm, Xs, frames, frames[0]
