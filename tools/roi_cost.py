#!/usr/bin/env python
"""What keeping the registered video on the device costs at 1024^2 with the bench's 201-vertex mesh, and what the
reductions over it take.

  python tools/roi_cost.py [--frames 64] [--warps 200] [--kernels-only] [--video-dir /dev/shm] [--kernel-stats CSV]
                           [--out profiles/roi_cost.json]

1. `--warps` warps queued back to back on the filter's stream with the record on (hm_body_warp_dev as the pipeline's
   readout queues it: 3 channels, triangle and 32-label sums), then seed_sums (R = 8), label_sums (32 discs) and
   weighted_sums (the 32 rings) over the recorded frames: wall time per call.  The kernel times come from a run of this
   tool under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/roi_cost.py --kernels-only`
   (KERNEL_CMD, a run of its own, no counters with it); --kernel-stats names the kernel_stats.csv it wrote, whose
   k_rec_copy, k_rec_seed_traces, k_rec_window_sums, k_rec_label_sums, k_rec_weighted_sums and k_body_warp rows go into
   the record.
2. The 64-frame 1024^2 pipeline (bench.py's video) with the readout of tools/body_cost.py (triangle sums, 32 point
   discs, the registered AVI written to --video-dir) without the record and with it, alternated after one run that is
   not recorded: frames/s of each, all six runs, and the ratio of the means.
The record is one JSON file (default profiles/roi_cost.json).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

KERNEL_CMD = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/roi_cost.py --frames 8 --warps 200 --kernels-only"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warps", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--video-dir", default="/dev/shm")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_cost.json"))
    a = ap.parse_args()
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, body, kalman, mesh, roi
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
    # 1. warps with the record on, back to back; then the reductions over the recorded frames
    dm, kf = new_filter()
    rec["vertices"] = int(dm.size())
    rec["triangles"] = int(dm.t.shape[0])
    rd = kf.state.renderer
    pts = points()
    b = body.BodyReadout(kf, points=pts, keep=True)
    map_px = int((b.tri_of_pixel >= 0).sum())
    rec["map_pixels"] = map_px
    rec["record_bytes_per_frame"] = body.record_bytes(b.tri_of_pixel, 1)
    X = np.array(kf.state.X, np.float64).reshape(-1)
    d_f, d_o, d_s = DeviceBuffer(n * n), DeviceBuffer(3 * n * n), DeviceBuffer(8 * (b.T + b.L))
    d_f.upload(np.ascontiguousarray(video.frame_at(1)[0]))

    def warp():                                      # (the state jitters: the registered frames differ)
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
    rec["warp_with_record_wall_us"] = 1e6 * (time.perf_counter() - t0) / a.warps
    rec["frames_recorded"] = rd.body_rec_count()
    seeds = roi.seeds_of(pts[~b.outside])
    rec["seeds"] = int(len(seeds))
    labels = body.disc_labels(b.tri_of_pixel, pts, 3.0)
    ring, _, Rg = roi.ring_weights(labels, b.tri_of_pixel >= 0, seeds, 6.0, 8.5)
    for name, call in (("seed_sums", lambda: rd.body_rec_seed_sums(seeds, 3.0, 6.0, 8.5, 8)),
                       ("label_sums", lambda: rd.body_rec_label_sums(labels, len(pts))),
                       ("weighted_sums", lambda: rd.body_rec_weighted_sums(seeds, ring, Rg))):
        call()
        t0 = time.perf_counter()
        for _ in range(5):
            call()
        rec[name + "_call_ms"] = 1e3 * (time.perf_counter() - t0) / 5
    t0 = time.perf_counter()
    roi.extract(b, pts[~b.outside])
    rec["extract_call_ms"] = 1e3 * (time.perf_counter() - t0)
    rd.body_rec_end()
    for buf in (d_f, d_o, d_s):
        buf.close()
    kf.close()
    print("warp with the record: %.1f us wall per call; seed_sums %.2f ms, label_sums %.2f ms, weighted_sums %.2f ms, "
          "extract %.1f ms per call over %d frames (host copies included)"
          % (rec["warp_with_record_wall_us"], rec["seed_sums_call_ms"], rec["label_sums_call_ms"],
             rec["weighted_sums_call_ms"], rec["extract_call_ms"], rec["frames_recorded"]))
    if a.kernels_only:
        return
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rec["kernel_stats_from"] = KERNEL_CMD
        for row in csv.DictReader(open(a.kernel_stats)):
            for kernel in ("k_rec_copy", "k_rec_seed_traces", "k_rec_window_sums", "k_rec_label_sums", "k_rec_box_labels",
                           "k_rec_weighted_sums", "k_body_warp"):
                if row.get("Name", "").startswith(kernel + "("):
                    rec[kernel] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
                    rec[kernel + "_us"] = float(row["AverageNs"]) / 1e3

    # 2. the pipeline with the readout, without and with the record
    def run(keep):
        _, kf = new_filter()
        pipe = FlowEKFPipeline(kf, video)
        path = os.path.join(a.video_dir, "hydra_mi_roi_cost_%d.avi" % os.getpid())
        w = AviWriter(path, n, n)
        bd = body.BodyReadout(kf, points=points(), video=w, keep=keep)
        t0 = time.perf_counter()
        pipe.run(body=bd)
        dt = time.perf_counter() - t0
        added = kf.state.renderer.body_rec_count() if keep else None
        pipe.close()
        w.close()
        os.remove(path)
        kf.close()
        return a.frames / dt, added

    run(False)                                  # (first-use costs of the process: not recorded)
    runs = []
    for mode in (False, True, False, True, False, True):
        fps, added = run(mode)
        runs.append({"record": mode, "frames_per_s": fps, "frames_recorded": added})
        print("pipeline with the readout, %s the record: %.1f frames/s" % ("with" if mode else "without", fps))
    rec["pipeline_runs"] = runs
    off = [x["frames_per_s"] for x in runs if not x["record"]]
    on = [x["frames_per_s"] for x in runs if x["record"]]
    rec["on_over_off"] = float(np.mean(on) / np.mean(off))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
