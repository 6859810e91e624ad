#!/usr/bin/env python
"""What the full-depth second pass costs at 1024^2 with the bench's 201-vertex mesh and 100 cells.

  python tools/deeptrace_cost.py [--frames 64] [--passes 5] [--kernels-only] [--kernel-stats DIR_OR_CSV]
                                 [--bench LABEL=LOG ...] [--out profiles/deeptrace_cost.json]

The scene: bench.py's video as 16-bit frames (16 v + 100), one state per frame (the mesh at rest plus N(0, 1) px per
vertex and frame: nothing is tracked here), 100 cells inside the disk with an ROI (a disc of 5 px), a ring
(roi.ring_weights, 6..8.5 px) and a 17 x 17 shape of random weights each: 300 columns.

1. Kernel times: k_deep_cols and k_body_warp16 per launch -- a run of 8 frames -- from a run of this tool under
   `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/deeptrace_cost.py --kernels-only`
   (KERNEL_CMD; no counters in that run); --kernel-stats names DIR or the kernel_stats.csv in it.
2. The wall time of the pass over the video (hm_deep_body_run, sums only; then with the planes too) against uploading the
   same runs alone: the frames copied into two page-locked blocks in turn and from there to the device on a copy stream.
3. --bench: the output of `python bench.py --gpus 1 --steps 64 --warmup 2` runs of the same session, in the order they
   were made, each as LABEL=LOG (a library build of the parent commit against this one: bench.py does not reach this
   code); the frames/s of every log's JSON line go into the record as they are.
The record is one JSON file (default profiles/deeptrace_cost.json).
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

KERNEL_CMD = "rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/deeptrace_cost.py --kernels-only"
BODY_WARP_US = 15.3                      # k_body_warp per frame at this size (README; profiles/body_cost.json)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--bench", nargs="*", default=[], metavar="LABEL=LOG")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deeptrace_cost.json"))
    a = ap.parse_args()
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, deepio, deeptrace, kalman, mesh, roi
    from hydra_mi.pipeline import DeviceBuffer
    import bench

    n, F, RUN = 1024, a.frames, 8
    video = bench.BenchVideo(n, F, 0)
    c, r = video.centre, video.radius
    rng = np.random.default_rng(0)
    deep = np.stack([video.frame_at(f)[0] for f in range(F)]).astype(np.uint16) * 16 + 100
    dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
    kf = kalman.IteratedMSKalmanFilter(dm, video.frame_at(0)[0], np.zeros((n, n, 2), np.float32), True)
    rd = kf.state.renderer
    N = dm.size()
    X = np.repeat(np.array(kf.state.X, np.float64).reshape(1, -1), F, axis=0)
    X[:, :2 * N] += rng.normal(0, 1.0, (F, 2 * N))
    tri_of = rd.body_map()[0]
    inmap = tri_of >= 0
    ang, rad = rng.uniform(0, 2 * np.pi, 100), (r - 30.0) * np.sqrt(rng.uniform(0, 1, 100))
    seeds = np.floor(np.stack((c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)), 1)).astype(np.int32)
    labels = np.full((n, n), -1, np.int32)
    yy, xx = np.mgrid[-5:6, -5:6]
    for s, (cx, cy) in enumerate(seeds):
        disc = (xx * xx + yy * yy <= 25) & inmap[cy - 5:cy + 6, cx - 5:cx + 6] & (labels[cy - 5:cy + 6, cx - 5:cx + 6] < 0)
        labels[cy - 5:cy + 6, cx - 5:cx + 6][disc] = s
    w, _, Rg = roi.ring_weights(labels, inmap, seeds, 6.0, 8.5)
    shapes = rng.integers(1, 65536, (100, 17, 17)).astype(np.uint16)
    cols = deeptrace.columns(labels, 100, [(seeds, w, Rg), (seeds, shapes, 8)])
    C, M = len(cols.col_ptr) - 1, int(cols.col_ptr[-1])
    rec = {"size": n, "vertices": int(N), "frames": F, "run_frames": RUN, "cells": 100, "columns": C, "entries": M,
           "map_pixels": int(inmap.sum()), "longest_column": int(np.diff(cols.col_ptr).max())}
    print("%d columns, %d entries, %d map pixels" % (C, M, rec["map_pixels"]))

    L = _lib.lib()
    h = deepio._Handle(n, n, RUN, 0)
    _lib.check(L.hm_deep_body_set_columns(h._h, rd._h, C, _lib.ptr(cols.col_ptr), _lib.ptr(cols.pix), _lib.ptr(cols.wt)),
               "hm_deep_body_set_columns")
    sums = np.zeros((F, C), np.uint64)
    planes = np.zeros((F, n, n), np.uint16)

    def second_pass(with_planes):
        t0 = time.perf_counter()
        _lib.check(L.hm_deep_body_run(h._h, rd._h, F, _lib.ptr(deep), 0, _lib.ptr(X), _lib.ptr(sums),
                                      _lib.ptr(planes) if with_planes else None), "hm_deep_body_run")
        return 1e3 * (time.perf_counter() - t0)

    second_pass(True)                            # (first use: buffers, the body map)
    host = deeptrace.run(rd, deep[:2], X[:2], cols, device=None, first=0)
    assert np.array_equal(host, sums[:2]), "the device's sums differ from the host path's"
    if a.kernels_only:
        for _ in range(a.passes):
            second_pass(True)
        h.close()
        kf.close()
        return
    rec["pass_sums_ms"] = [second_pass(False) for _ in range(a.passes)]
    rec["pass_sums_planes_ms"] = [second_pass(True) for _ in range(a.passes)]

    # the same runs uploaded alone
    run_bytes = RUN * n * n * 2
    pins = []
    for _ in range(2):
        p = _lib.c_vp()
        _lib.check(L.hm_host_alloc(run_bytes, ctypes.byref(p)), "hm_host_alloc")
        pins.append(p)
    dev = [DeviceBuffer(run_bytes), DeviceBuffer(run_bytes)]
    stream = _lib.c_vp()
    _lib.check(L.hm_copy_stream_create(0, ctypes.byref(stream)), "hm_copy_stream_create")

    def upload_alone():
        t0 = time.perf_counter()
        for i, f0 in enumerate(range(0, F, RUN)):
            k = min(RUN, F - f0)
            if i >= 2:                           # (the block is free once its copy has run: as the handle's events say)
                _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
            ctypes.memmove(pins[i & 1].value, deep[f0:f0 + k].ctypes.data, k * n * n * 2)
            _lib.check(L.hm_dev_upload_async(0, ctypes.c_void_p(dev[i & 1].ptr), pins[i & 1], k * n * n * 2, stream),
                       "hm_dev_upload_async")
        _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
        return 1e3 * (time.perf_counter() - t0)

    upload_alone()
    rec["upload_alone_ms"] = [upload_alone() for _ in range(a.passes)]
    L.hm_copy_stream_destroy(0, stream)
    for p in pins:
        L.hm_host_free(p)
    for d in dev:
        d.close()
    h.close()
    kf.close()
    med = lambda v: float(np.median(v))
    rec["pass_over_upload"] = med(rec["pass_sums_ms"]) / med(rec["upload_alone_ms"])
    # the frames' bytes over the median time: of the stand-alone upload, and of the whole pass (sums only)
    rec["upload_alone_GBps"] = F * n * n * 2 / med(rec["upload_alone_ms"]) / 1e6
    rec["pass_GBps"] = F * n * n * 2 / med(rec["pass_sums_ms"]) / 1e6
    if a.bench:
        rec["bench_command"] = "python bench.py --gpus 1 --steps 64 --warmup 2"
        rec["bench_frames_per_s"] = []
        for item in a.bench:
            label, path = item.split("=", 1)
            line = [ln for ln in open(path) if ln.startswith("{")][-1]
            rec["bench_frames_per_s"].append({"library": label, "frames_per_s": json.loads(line)["value"]})

    stats = a.kernel_stats
    if stats and os.path.isdir(stats):
        found = sorted(glob.glob(os.path.join(stats, "**", "*kernel_stats.csv"), recursive=True))
        stats = found[0] if found else None
    if stats and os.path.exists(stats):
        rec["kernel_stats_from"] = KERNEL_CMD
        for row in csv.DictReader(open(stats)):
            for kernel in ("k_deep_cols", "k_body_warp16"):
                if row.get("Name", "").startswith(kernel + "("):
                    rec[kernel] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
                    rec[kernel + "_us_per_run"] = float(row["AverageNs"]) / 1e3
                    rec[kernel + "_us_per_frame"] = float(row["AverageNs"]) / 1e3 / RUN
        if "k_deep_cols_us_per_run" in rec:
            runs = (F + RUN - 1) // RUN
            rec["k_body_warp_us_per_frame"] = BODY_WARP_US
            rec["kernels_of_a_pass_ms"] = runs * rec["k_deep_cols_us_per_run"] / 1e3
            # the overlap shows when the pass takes less than the upload and the kernels one after the other
            rec["pass_minus_upload_ms"] = med(rec["pass_sums_ms"]) - med(rec["upload_alone_ms"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
