#!/usr/bin/env python
"""What demixing costs at 1024^2 with the bench's 201-vertex mesh, 32 seeds (16 pairs 4 px apart) and R = 8, on records
of 64 and of 1024 frames.

  python tools/demix_cost.py [--out profiles/demix_cost.json]
  python tools/demix_cost.py --kernels-only --frames N          (what the profiler runs)

For each record length the tool starts `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/demix_cost.py --kernels-only --frames N` (a run of its own, no counters with it) and reads from its
kernel_stats.csv the time of k_rec_trace_products and, on the same record in the same run, of k_rec_window_sums: the
kernel hm_body_rec_seed_sums forms c = sum v U with, the comparable reduction before the trace products existed.  Then,
without the profiler, the wall time of demix.extract(iters=6) and of one trace_products call (host copies included).
The video is the bench's frame with 32 planted cells (the model of tests/roi_ref.py in windows round the seeds), the mesh
at rest.  The record is one JSON file (default profiles/demix_cost.json).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_rec_trace_products", "k_rec_window_sums", "k_rec_weighted_sums", "k_rec_seed_traces")


def record(frames):
    """-> (filter, readout with `frames` frames recorded, points (32, 2))"""
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, body, kalman, mesh
    from hydra_mi.pipeline import DeviceBuffer
    import bench
    n = 1024
    video = bench.BenchVideo(n, 2, 0)
    c, r = video.centre, video.radius
    dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
    base = (video.frame_at(1)[0] // 2).astype(np.float64)
    kf = kalman.IteratedMSKalmanFilter(dm, video.frame_at(0)[0], np.zeros((n, n, 2), np.float32), True)
    rng = np.random.default_rng(0)
    pts = []
    for i in range(16):                              # pairs on a 4 x 4 grid inside the disk, the partner 4 px away
        cx = int(c[0]) + 60 * (i % 4) - 90 + int(rng.integers(-4, 5))
        cy = int(c[1]) + 60 * (i // 4) - 90 + int(rng.integers(-4, 5))
        th = rng.uniform(0, 2 * np.pi)
        pts += [(cx, cy), (cx + int(np.rint(4 * np.cos(th))), cy + int(np.rint(4 * np.sin(th))))]
    pts = np.array(pts)
    K, W = len(pts), 16
    yy, xx = np.mgrid[-W:W + 1, -W:W + 1]
    blobs = []
    for _ in range(K):
        sa, sb = rng.uniform(1.5, 2.5, 2)
        blobs.append(np.exp(-(xx * xx / (2 * sa * sa) + yy * yy / (2 * sb * sb))))
    act = np.zeros((K, frames))
    for i in range(K):
        ev, a = rng.random(frames) < 0.06, 0.0
        for k in range(frames):
            a = a * 0.8 + (1.0 if ev[k] else 0.0)
            act[i, k] = min(a, 1.0)
    npil = 15.0 + 15.0 * np.sin(np.arange(frames) / 17.0)
    b = body.BodyReadout(kf, keep=True)
    rd = kf.state.renderer
    X = np.array(kf.state.X, np.float64).reshape(-1)
    d_f = DeviceBuffer(n * n)
    for k in range(frames):
        f = base + npil[k]
        for i, (cx, cy) in enumerate(pts):
            f[cy - W:cy + W + 1, cx - W:cx + W + 1] += 50.0 * act[i, k] * blobs[i] + rng.integers(-8, 9, (2 * W + 1, 2 * W + 1))
        d_f.upload(np.ascontiguousarray(np.clip(np.rint(f), 0, 255).astype(np.uint8)))
        rd.body_warp_dev(X, d_f.ptr, None, 1, None, None)
        _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")          # (the next upload overwrites the frame)
    d_f.close()
    assert rd.body_rec_count() == frames
    return kf, b, pts + 0.5


def kernels_only(frames):
    from hydra_mi import roi
    kf, b, pts = record(frames)
    rd = kf.state.renderer
    seeds = roi.seeds_of(pts)
    q = np.random.default_rng(1).integers(-2 ** 20, 2 ** 20 + 1, (frames, len(seeds))).astype(np.int32)
    for _ in range(5):
        rd.body_rec_seed_sums(seeds, 3.0, 6.0, 8.5, 8)
        rd.body_rec_trace_products(seeds, q, 8)
    rd.body_rec_end()
    kf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demix_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.frames)
        return
    rec = {"size": 1024, "seeds": 32, "R": 8, "records": {}}
    for frames in (64, 1024):
        one = {}
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                   os.path.abspath(__file__), "--kernels-only", "--frames", str(frames)]
            one["kernel_stats_from"] = ("rocprofv3 --kernel-trace --stats --output-format csv -- python tools/demix_cost.py "
                                        "--kernels-only --frames %d" % frames)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                raise RuntimeError("the profiled run failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if len(found) != 1:
                raise RuntimeError("expected one kernel_stats.csv under the profiler's directory, found %r" % found)
            for row in csv.DictReader(open(found[0])):
                for kernel in KERNELS:
                    if row.get("Name", "").startswith(kernel + "("):
                        one[kernel] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
                        one[kernel + "_us"] = float(row["AverageNs"]) / 1e3
        rec["records"][str(frames)] = one
    from hydra_mi import demix, roi                  # (the profiled runs are over: this process opens the GPU only now)
    for frames in (64, 1024):
        one = rec["records"][str(frames)]
        kf, b, pts = record(frames)
        rd = kf.state.renderer
        seeds = roi.seeds_of(pts)
        q = np.random.default_rng(1).integers(-2 ** 20, 2 ** 20 + 1, (frames, len(seeds))).astype(np.int32)
        rd.body_rec_trace_products(seeds, q, 8)
        t0 = time.perf_counter()
        for _ in range(5):
            rd.body_rec_trace_products(seeds, q, 8)
        one["trace_products_call_ms"] = 1e3 * (time.perf_counter() - t0) / 5
        t0 = time.perf_counter()
        roi.extract(b, pts, alpha=1.0)
        one["roi_extract_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        try:
            t0 = time.perf_counter()
            e = demix.extract(b, pts, iters=6, alpha=1.0)
            one["demix_extract_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            one["demix_change"] = [float(x) for x in e["demix_change"]]
            one["shapes_kept"] = int(e["demix_kept"].sum())
        except (np.linalg.LinAlgError, ValueError) as err:
            one["demix_extract_error"] = str(err)
        rd.body_rec_end()
        kf.close()
        print("%d frames: %s" % (frames, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
