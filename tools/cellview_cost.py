#!/usr/bin/env python
"""What the cell view costs at 1024^2 with the bench's 201-vertex mesh, 32 cells in two layers and 32 markers.

  python tools/cellview_cost.py [--frames 64] [--views 200] [--video-dir /dev/shm] [--kernel-stats FILE] [--out profiles/..]

1. `--views` cell views (outline and wireframe on) and as many overlay views, the yardstick, queued back to back on the
   filter's stream (hm_view_cells_dev / hm_view_dev, no copies): wall time per view.  The kernel times come from a run of
   this tool under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/cellview_cost.py --kernels-only`
   (KERNEL_CMD, a run of its own, no counters with it); --kernel-stats names the kernel_stats.csv it wrote, whose
   k_view_cells, k_view_cell_marks, k_view_cell_outline and k_view_wire rows and the overlay's k_setup_all, k_render and
   k_view_compose rows go into the record, with the ratio of the two views' kernel sums.
2. cellview.write_video over `--frames` frames of bench.py's video at one state: wall time per frame.
The record is one JSON file (default profiles/cellview_cost.json).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

KERNEL_CMD = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/cellview_cost.py --views 200 --kernels-only"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELL_KERNELS = ("k_view_cells", "k_view_cell_marks")
OVERLAY_KERNELS = ("k_setup_all", "k_render", "k_view_compose")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--video-dir", default="/dev/shm")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cellview_cost.json"))
    a = ap.parse_args()
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, cellview, kalman, mesh
    from hydra_mi.pipeline import DeviceBuffer
    import bench

    n = 1024
    video = bench.BenchVideo(n, a.frames + 1, 0)
    c, r = video.centre, video.radius
    dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
    f0 = video.frame_at(0)[0]
    kf = kalman.IteratedMSKalmanFilter(dm, f0, np.zeros((n, n, 2), np.float32), True)
    rd = kf.state.renderer
    rec = {"size": n, "vertices": int(dm.size()), "cells": 32, "layers": 2, "markers": 32}
    # 32 cells of radius 9 on a ring inside the animal, neighbours overlapping: two layers
    ang = 2 * np.pi * np.arange(32) / 32
    seeds = np.column_stack((c[0] + 0.18 * r * np.cos(ang), c[1] + 0.18 * r * np.sin(ang))).astype(np.int32)
    R = 9
    d = np.arange(-R, R + 1)
    disc = np.where(d[:, None] ** 2 + d[None, :] ** 2 <= R * R, 65535 - 3000 * np.hypot(d[:, None], d[None, :]), 0)
    shapes = np.repeat(disc.astype(np.uint16)[None], 32, axis=0)
    step = float(np.hypot(*(seeds[1] - seeds[0])))
    lab, w, dropped = cellview.layers_from_shapes(shapes, seeds, R, (n, n), n_layers=2)
    rec["cell_radius"], rec["cell_spacing_px"], rec["dropped"] = R, step, dropped
    col = cellview.palette(32)
    rd.view_set_cells(lab, w, col)
    fr, mk, _ = video.frame_at(1)
    rd.set_observation(fr, np.zeros((n, n, 2), np.float32), mk)
    X = np.array(kf.state.X, np.float64).reshape(-1)
    lev = np.linspace(20, 255, 32).astype(np.uint8)
    pts = seeds.astype(np.float64) + 0.5
    d_frame, buf = DeviceBuffer(n * n), DeviceBuffer(3 * n * n)
    d_frame.upload(fr)

    def timed(queue):
        for _ in range(5):
            queue()
        _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
        t0 = time.perf_counter()
        for _ in range(a.views):
            queue()
        _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
        return 1e6 * (time.perf_counter() - t0) / a.views
    rec["cell_view_wall_us"] = timed(lambda: rd.view_cells_dev(X, d_frame.ptr, buf.ptr, lev, True, True, pts, col, 2))
    rec["overlay_view_wall_us"] = timed(lambda: rd.view_dev(X, "overlay", buf.ptr))
    d_frame.close()
    buf.close()
    print("cell view %.1f us, overlay view %.1f us wall per view" % (rec["cell_view_wall_us"], rec["overlay_view_wall_us"]))
    if a.kernels_only:
        kf.close()
        return
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rec["kernel_stats_from"] = KERNEL_CMD
        for row in csv.DictReader(open(a.kernel_stats)):
            for kernel in CELL_KERNELS + OVERLAY_KERNELS + ("k_view_wire", "k_view_cell_outline"):
                name = row.get("Name", "")
                if name.startswith(kernel + "(") or name.startswith("void " + kernel + "<"):
                    rec[kernel] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
                    rec[kernel + "_us"] = float(row["AverageNs"]) / 1e3
        if all(k + "_us" in rec for k in CELL_KERNELS + OVERLAY_KERNELS + ("k_view_wire",)):
            # both views draw the wireframe with the same launch
            rec["cell_view_kernels_us"] = sum(rec[k + "_us"] for k in CELL_KERNELS) + rec["k_view_wire_us"]
            rec["overlay_view_kernels_us"] = sum(rec[k + "_us"] for k in OVERLAY_KERNELS) + rec["k_view_wire_us"]
            rec["cell_over_overlay_kernels"] = rec["cell_view_kernels_us"] / rec["overlay_view_kernels_us"]

    # 2. the video
    states = [X] * a.frames
    levels = np.tile(lev, (a.frames, 1))
    path = os.path.join(a.video_dir, "hydra_mi_cellview_cost_%d.avi" % os.getpid())
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        frames = cellview.write_video(kf, states, video, path, cells=(lab, w), levels=levels, points=pts, wire=True)
        runs.append(1e3 * (time.perf_counter() - t0) / frames)
        os.remove(path)
    rec["write_video_frames"] = a.frames
    rec["write_video_ms_per_frame"] = runs
    kf.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
