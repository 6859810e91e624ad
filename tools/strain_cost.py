#!/usr/bin/env python
"""What the deformation readout costs at 1024^2 with the bench's 201-vertex mesh.

  python tools/strain_cost.py [--frames 2000] [--views 200] [--kernel-stats FILE] [--pipeline PARENT_TREE] [--out profiles/..]

1. hm_strain_tri over `--frames` states in one call (a few calls), and `--views` strain views (wireframe on) queued back to
   back on the filter's stream (hm_view_strain_dev, no copies): wall time per call / per view.  The kernel times come from a
   run of this tool under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/strain_cost.py
   --kernels-only` (KERNEL_CMD, a run of its own, no counters with it); --kernel-stats names the kernel_stats.csv it wrote,
   whose k_strain_tri, k_view_strain and k_view_wire rows go into the record, with k_view_strain over the k_view_cells
   figure of profiles/cellview_cost.json (the expectation: about 1; DESIGN.md section 16 says why if it is beyond 1.5).
2. --pipeline PARENT_TREE: run_kalmanfilter.py on 65 frames of bench.py's video (64 tracked), with --strain-video in this
   tree against the same command without it in a built checkout of the parent commit, alternating, two runs each:
   frames/s of the whole command, process start to exit.
The record is one JSON file (default profiles/strain_cost.json).
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

KERNEL_CMD = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/strain_cost.py --kernels-only"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_strain_tri", "k_view_strain", "k_view_wire")


def pipeline_runs(parent, frames, shm):
    import bench
    n = 1024
    video = bench.BenchVideo(n, frames + 1, 0)
    vid = os.path.join(shm, "hydra_mi_strain_cost_%d.npy" % os.getpid())
    np.save(vid, np.stack([video.frame_at(k)[0] for k in range(frames + 1)]))
    out = os.path.join(shm, "hydra_mi_strain_cost_%d" % os.getpid())
    runs = {"parent": [], "strain_video": []}
    try:
        for _ in range(2):
            for name, tree, extra in (("parent", parent, []), ("strain_video", ROOT, ["--strain-video", out + ".avi"])):
                cmd = [sys.executable, os.path.join(tree, "run_kalmanfilter.py"), vid, out + "_noflow", out + ".npz", "-s", "48"] + extra
                t0 = time.perf_counter()
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree)
                dt = time.perf_counter() - t0
                if res.returncode != 0 or "Finished: %d frames" % frames not in res.stdout:
                    raise RuntimeError("%s failed: %s" % (" ".join(cmd), res.stderr[-2000:]))
                runs[name].append(frames / dt)
    finally:
        for f in (vid, out + ".npz", out + ".avi", out + "_points.txt"):
            if os.path.exists(f):
                os.remove(f)
    return {"command": "run_kalmanfilter.py VIDEO noflow OUT.npz -s 48 [--strain-video OUT.avi]", "tracked_frames": frames,
            "frames_per_s": runs, "strain_video_over_parent": float(np.mean(runs["strain_video"]) / np.mean(runs["parent"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--pipeline", default=None, metavar="PARENT_TREE")
    ap.add_argument("--pipeline-frames", type=int, default=64)
    ap.add_argument("--shm", default="/dev/shm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strain_cost.json"))
    a = ap.parse_args()
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, kalman, mesh, strain
    from hydra_mi.pipeline import DeviceBuffer
    import bench

    n = 1024
    video = bench.BenchVideo(n, 2, 0)
    c, r = video.centre, video.radius
    dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
    kf = kalman.IteratedMSKalmanFilter(dm, video.frame_at(0)[0], np.zeros((n, n, 2), np.float32), True)
    rd = kf.state.renderer
    N, T = int(dm.size()), int(rd.tri.shape[0])
    rec = {"size": n, "vertices": N, "triangles": T, "strain_frames": a.frames}
    rng = np.random.default_rng(0)
    X = np.array(kf.state.X, np.float64).reshape(-1)
    states = np.tile(X, (a.frames, 1))
    states[:, :2 * N] += rng.normal(0, 0.5, (a.frames, 2 * N))
    # bytes the kernel moves per call: the positions read once (whole 64-byte lines of the 2N doubles of a row), 7 doubles out
    rec["strain_tri_bytes"] = {"positions_read": a.frames * 2 * N * 8, "written": a.frames * T * 7 * 8}
    rd.strain_tri(states)                          # (every call of the run has all the frames: the kernel's average is theirs)
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        rd.strain_tri(states)
        runs.append(1e3 * (time.perf_counter() - t0))
    rec["strain_tri_call_ms"] = runs               # with the copies of the states in and the result out
    fr = video.frame_at(1)[0]
    d_frame, buf = DeviceBuffer(n * n), DeviceBuffer(3 * n * n)
    d_frame.upload(fr)
    lut = strain.default_lut()

    def timed(queue):
        for _ in range(5):
            queue()
        _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
        t0 = time.perf_counter()
        for _ in range(a.views):
            queue()
        _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
        return 1e6 * (time.perf_counter() - t0) / a.views
    rec["strain_view_wall_us"] = timed(lambda: rd.view_strain_dev(states[1], d_frame.ptr, buf.ptr, "J", 256.0, 128, lut, True))
    d_frame.close()
    buf.close()
    kf.close()
    print("hm_strain_tri of %d frames %.2f ms per call, strain view %.1f us wall per view" % (a.frames, min(runs), rec["strain_view_wall_us"]))
    if a.kernels_only:
        return
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rec["kernel_stats_from"] = KERNEL_CMD
        for row in csv.DictReader(open(a.kernel_stats)):
            for kernel in KERNELS:
                if row.get("Name", "").startswith(kernel + "("):
                    rec[kernel] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
                    rec[kernel + "_us"] = float(row["AverageNs"]) / 1e3
        if "k_strain_tri" in rec:
            b = rec["strain_tri_bytes"]
            rec["k_strain_tri_gb_per_s"] = (b["positions_read"] + b["written"]) / float(rec["k_strain_tri"]["AverageNs"])
        cv = os.path.join(ROOT, "profiles", "cellview_cost.json")
        if "k_view_strain_us" in rec and os.path.exists(cv):
            rec["k_view_cells_us_of_cellview_cost"] = json.load(open(cv))["k_view_cells_us"]
            rec["view_strain_over_view_cells"] = rec["k_view_strain_us"] / rec["k_view_cells_us_of_cellview_cost"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for part in (None, a.pipeline):                     # (the kernels' record is written before the long runs start)
        if part:
            rec["pipeline"] = pipeline_runs(os.path.abspath(part), a.pipeline_frames, a.shm)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
