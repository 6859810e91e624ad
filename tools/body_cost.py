#!/usr/bin/env python
"""What the body-frame readout costs at 1024^2 with the bench's 201-vertex mesh.

  python tools/body_cost.py [--frames 64] [--warps 200] [--warps-only] [--video-dir /dev/shm] [--kernel-stats CSV]
                            [--out profiles/body_cost.json]

1. `--warps` warps queued back to back on the filter's stream (hm_body_warp_dev: 3 channels, triangle and 32-label
   sums, no copies): wall time per warp.  The kernel time of one warp comes from a run of this tool under
   `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/body_cost.py --warps-only` (KERNEL_CMD);
   --kernel-stats names the kernel_stats.csv it wrote, whose k_body_warp and k_body_map (once per handle) rows go
   into the record.
2. The 64-frame 1024^2 pipeline (bench.py's video) without the readout and with it (triangle sums, 32 point discs,
   the registered AVI written to --video-dir), alternated after one run that is not recorded: frames/s of each.
The record is one JSON file (default profiles/body_cost.json).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

# the run whose kernel_stats.csv --kernel-stats names (the body map is built once per handle in it, the warp --warps + 5
# times)
KERNEL_CMD = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/body_cost.py --frames 8 --warps 200 --warps-only"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warps", type=int, default=200)
    ap.add_argument("--warps-only", action="store_true")
    ap.add_argument("--video-dir", default="/dev/shm")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_cost.json"))
    a = ap.parse_args()
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, body, kalman, mesh
    from hydra_mi.pipeline import DeviceBuffer, FlowEKFPipeline
    from hydra_mi.videoio import AviWriter
    import bench

    n = 1024
    video = bench.BenchVideo(n, a.frames + 1, 0)
    c, r = video.centre, video.radius
    rng = np.random.default_rng(0)

    def new_filter():
        dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
        f0 = video.frame_at(0)[0]
        return dm, kalman.IteratedMSKalmanFilter(dm, f0, np.zeros((n, n, 2), np.float32), True)

    def points():
        ang = rng.uniform(0, 2 * np.pi, 32)
        rad = (r - 20.0) * np.sqrt(rng.uniform(0, 1, 32))
        return np.stack((c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)), 1)

    rec = {"size": n}
    # 1. warps back to back
    dm, kf = new_filter()
    rec["vertices"] = int(dm.size())
    rec["triangles"] = int(dm.t.shape[0])
    rd = kf.state.renderer
    b = body.BodyReadout(kf, points=points())
    fr = video.frame_at(1)[0]
    X = np.array(kf.state.X, np.float64).reshape(-1)
    X[:2 * dm.size()] += rng.normal(0, 1.0, 2 * dm.size())
    d_f, d_o, d_s = DeviceBuffer(n * n), DeviceBuffer(3 * n * n), DeviceBuffer(8 * (b.T + b.L))
    d_f.upload(np.ascontiguousarray(fr))
    for _ in range(5):
        rd.body_warp_dev(X, d_f.ptr, d_o.ptr, 3, d_s.ptr, d_s.ptr + 8 * b.T)
    _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
    t0 = time.perf_counter()
    for _ in range(a.warps):
        rd.body_warp_dev(X, d_f.ptr, d_o.ptr, 3, d_s.ptr, d_s.ptr + 8 * b.T)
    _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
    rec["warp_wall_us"] = 1e6 * (time.perf_counter() - t0) / a.warps
    for buf in (d_f, d_o, d_s):
        buf.close()
    kf.close()
    print("warp: %.1f us wall per call" % rec["warp_wall_us"])
    if a.warps_only:
        return
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rec["kernel_stats_from"] = KERNEL_CMD
        for row in csv.DictReader(open(a.kernel_stats)):
            for kernel, key in (("k_body_warp", "warp_kernel"), ("k_body_map", "body_map_kernel")):
                if row.get("Name", "").startswith(kernel + "("):
                    rec[key] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
                    rec[key + "_us"] = float(row["AverageNs"]) / 1e3

    # 2. the pipeline with and without the readout
    def run(with_body):
        _, kf = new_filter()
        pipe = FlowEKFPipeline(kf, video)
        path = os.path.join(a.video_dir, "hydra_mi_body_cost_%d.avi" % os.getpid())
        w = AviWriter(path, n, n) if with_body else None
        bd = body.BodyReadout(kf, points=points(), video=w) if with_body else None
        t0 = time.perf_counter()
        pipe.run(body=bd)
        dt = time.perf_counter() - t0
        pipe.close()
        frames = w.frames if w is not None else None
        if w is not None:
            w.close()
            os.remove(path)
        kf.close()
        return a.frames / dt, frames

    run(False)                                  # (first-use costs of the process: not recorded)
    runs = []
    for mode in (False, True, False, True, False, True):
        fps, frames = run(mode)
        runs.append({"readout": mode, "frames_per_s": fps, "video_frames": frames})
        print("pipeline %s readout: %.1f frames/s" % ("with" if mode else "without", fps))
    rec["pipeline_runs"] = runs
    off = [x["frames_per_s"] for x in runs if not x["readout"]]
    on = [x["frames_per_s"] for x in runs if x["readout"]]
    rec["on_over_off"] = float(np.mean(on) / np.mean(off))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
