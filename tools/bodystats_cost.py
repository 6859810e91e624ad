#!/usr/bin/env python
"""What the statistics of the registered video cost at 1024^2 with the bench's 201-vertex mesh.

  python tools/bodystats_cost.py [--frames 64] [--warps 200] [--kernels-only] [--video-dir /dev/shm] [--kernel-stats CSV]
                                 [--out profiles/bodystats_cost.json]

1. `--warps` warps queued back to back on the filter's stream with the statistics on (hm_body_warp_dev as the pipeline's
   readout queues it: 3 channels, triangle and 32-label sums), then the summary images and the peaks of the three scores
   at radius 6: wall time per warp.  The kernel times come from a run of this tool under
   `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bodystats_cost.py --kernels-only` (KERNEL_CMD, a
   run of its own, no counters with it); --kernel-stats names the kernel_stats.csv it wrote, whose k_body_stats_add,
   k_body_stats_images, k_body_peaks and k_body_warp rows go into the record, with the bytes k_body_stats_add has to
   move (50 per map pixel for its sums, 4 per pixel of map, about 2 per map pixel of registered values) over its time.
2. The 64-frame 1024^2 pipeline (bench.py's video) with the readout of tools/body_cost.py (triangle sums, 32 point
   discs, the registered AVI written to --video-dir) without the statistics and with them, alternated after one run that
   is not recorded: frames/s of each, all six runs, and the ratio of the means.
The record is one JSON file (default profiles/bodystats_cost.json).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

KERNEL_CMD = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bodystats_cost.py --frames 8 --warps 200 --kernels-only"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warps", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--video-dir", default="/dev/shm")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bodystats_cost.json"))
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
    # 1. warps with the statistics on, back to back; then the images and the peaks
    dm, kf = new_filter()
    rec["vertices"] = int(dm.size())
    rec["triangles"] = int(dm.t.shape[0])
    rd = kf.state.renderer
    b = body.BodyReadout(kf, points=points(), stats=True)
    map_px = int((b.tri_of_pixel >= 0).sum())
    rec["map_pixels"] = map_px
    X = np.array(kf.state.X, np.float64).reshape(-1)
    d_f, d_o, d_s = DeviceBuffer(n * n), DeviceBuffer(3 * n * n), DeviceBuffer(8 * (b.T + b.L))
    d_f.upload(np.ascontiguousarray(video.frame_at(1)[0]))

    def warp():                                      # (the state jitters: the registered frames differ, the images are not flat)
        Xk = X.copy()
        Xk[:2 * dm.size()] += rng.normal(0, 1.0, 2 * dm.size())
        rd.body_warp_dev(Xk, d_f.ptr, d_o.ptr, 3, d_s.ptr, d_s.ptr + 8 * b.T)
    for _ in range(5):
        warp()
    _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
    t0 = time.perf_counter()
    for _ in range(a.warps):
        warp()
    _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
    rec["warp_with_stats_wall_us"] = 1e6 * (time.perf_counter() - t0) / a.warps
    t0 = time.perf_counter()
    sm = b.summary()
    rec["images_call_ms"] = 1e3 * (time.perf_counter() - t0)
    rec["frames_accumulated"] = sm["frames"]
    for score in ("corr", "std", "range"):
        t0 = time.perf_counter()
        _, _, found = rd.body_stats_peaks(score, 6)
        rec["peaks_%s_call_ms" % score] = 1e3 * (time.perf_counter() - t0)
        rec["peaks_%s_found" % score] = found
    for buf in (d_f, d_o, d_s):
        buf.close()
    kf.close()
    print("warp with statistics: %.1f us wall per call; images %.2f ms, peaks %.2f ms per call (host copies included)"
          % (rec["warp_with_stats_wall_us"], rec["images_call_ms"], rec["peaks_corr_call_ms"]))
    if a.kernels_only:
        return
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rec["kernel_stats_from"] = KERNEL_CMD
        for row in csv.DictReader(open(a.kernel_stats)):
            for kernel in ("k_body_stats_add", "k_body_stats_images", "k_body_peaks", "k_body_warp"):
                if row.get("Name", "").startswith(kernel + "("):
                    rec[kernel] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
                    rec[kernel + "_us"] = float(row["AverageNs"]) / 1e3
        if "k_body_stats_add_us" in rec:
            # what the kernel has to move: its sums read and written (2 x 25 B per map pixel), the map (4 B per pixel of
            # the threads that stay; counted for every pixel) and the registered rows (about 2 B per map pixel)
            nbytes = 52 * map_px + 4 * n * n
            rec["k_body_stats_add_bytes"] = nbytes
            rec["k_body_stats_add_gb_per_s"] = nbytes / rec["k_body_stats_add_us"] / 1e3

    # 2. the pipeline with the readout, without and with the statistics
    def run(stats):
        _, kf = new_filter()
        pipe = FlowEKFPipeline(kf, video)
        path = os.path.join(a.video_dir, "hydra_mi_bodystats_cost_%d.avi" % os.getpid())
        w = AviWriter(path, n, n)
        bd = body.BodyReadout(kf, points=points(), video=w, stats=stats)
        t0 = time.perf_counter()
        pipe.run(body=bd)
        dt = time.perf_counter() - t0
        added = kf.state.renderer.body_stats_count() if stats else None
        pipe.close()
        w.close()
        os.remove(path)
        kf.close()
        return a.frames / dt, added

    run(False)                                  # (first-use costs of the process: not recorded)
    runs = []
    for mode in (False, True, False, True, False, True):
        fps, added = run(mode)
        runs.append({"statistics": mode, "frames_per_s": fps, "frames_added": added})
        print("pipeline with the readout, %s statistics: %.1f frames/s" % ("with" if mode else "without", fps))
    rec["pipeline_runs"] = runs
    off = [x["frames_per_s"] for x in runs if not x["statistics"]]
    on = [x["frames_per_s"] for x in runs if x["statistics"]]
    rec["on_over_off"] = float(np.mean(on) / np.mean(off))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
