#!/usr/bin/env python
"""What the 16-bit input costs at 1024^2.

  python tools/deep_cost.py [--frames 64] [--reps 20] [--rounds 3] [--only map|hist_random|hist_constant]
                            [--kernel-stats map=kernel_stats.csv ...] [--bench-line FILE] [--out profiles/deep_cost.json]

1. A run of 8 frames through hm_deep_map_run_dev (three planes written, one stream) and through hm_deep_hist_add, on
   random 12-bit data and on a constant frame: wall time per run, upload included.  Kernel times come from runs of their
   own under `rocprofv3 --kernel-trace --stats -- python tools/deep_cost.py --only map` (no counters alongside; --only
   runs that one part and writes no record); --kernel-stats map=.../kernel_stats.csv puts that run's k_deep_* rows into the
   record under its name.  Where rocprofv3 writes a database and no CSV, map=.../map_results.db is read instead (its
   dispatch table).
2. The 64-frame pipeline (FlowEKFPipeline.run on bench.py's video, made 16-bit as 40 v + 1000 + noise) from a DeepSource
   against an ArraySource of the same mapped frames, in turn --rounds times after one run that is not counted: frames/s of
   each and the bytes per frame that were queued host-to-device, as the ring counted them.
3. --bench-line: a file of `LABEL {json}` lines, the label (parent, change) in front of what bench.py printed in the same
   session; label, frames/s, steps and warmup of each go into the record, in the file's order.
4. --merge RECORD: no GPU work; adds --kernel-stats and --bench-line to a record written before and writes it to --out.
Nothing here has a bar in advance; the record says what came out.
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THRESHOLD = 9
MODES = ("array", "deep")


def kernel_rows(path, run):
    """the k_deep_* launches of a `rocprofv3 --kernel-trace --stats` run: from its kernel_stats.csv or, where rocprofv3
    writes a database instead, from the dispatch table of its results .db"""
    if path.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(path)
        found = {}
        for name, start, end in db.execute("select s.kernel_name, d.start, d.end from rocpd_kernel_dispatch d join "
                                           "rocpd_info_kernel_symbol s on d.kernel_id = s.id where s.kernel_name like '%k_deep%'"):
            found.setdefault(name.split("(")[0], []).append((end - start) / 1e3)
        stats = [(name, len(v), sum(v) / len(v), min(v), max(v)) for name, v in sorted(found.items())]
    else:
        with open(path) as f:
            stats = [(row["Name"].split("(")[0], int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3,
                      float(row["MaxNs"]) / 1e3) for row in csv.DictReader(f) if "k_deep" in row.get("Name", "")]
    return [{"name": name, "calls": calls, "average_us": avg, "average_us_per_frame": avg / run, "min_us": lo, "max_us": hi}
            for name, calls, avg, lo, hi in stats]


def merge(a, rec, run):
    """--kernel-stats and --bench-line into the record"""
    rec.setdefault("kernels", {})                       # per part: a run of 8 frames per call
    for item in a.kernel_stats:
        label, _, path = item.partition("=")
        if os.path.exists(path):
            rec["kernels"][label] = kernel_rows(path, run)
    if a.bench_line and os.path.exists(a.bench_line):
        rec["bench"] = []
        for ln in open(a.bench_line).read().splitlines():
            label, brace, rest = ln.partition("{")
            if brace:
                line = json.loads(brace + rest)
                rec["bench"].append({"build": label.strip(), "frames_per_s": line["value"], "steps": line["steps"], "warmup": line["warmup"]})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("bench", "pipeline_runs")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", default=None, metavar="RECORD", help="no GPU work: add --kernel-stats / --bench-line to this record")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("map", "hist_random", "hist_constant"))
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="PART=CSV")
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_cost.json"))
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            rec = json.load(f)
        return merge(a, rec, rec["run"])
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, deepio, kalman, mesh
    from hydra_mi.pipeline import ArraySource, DeviceBuffer, FlowEKFPipeline, threshold_mask
    import bench

    L = _lib.lib()
    n, run = 1024, 8
    rec = {"size": n, "run": run, "frame_bytes_16": 2 * n * n, "frame_bytes_8": n * n}
    rng = np.random.default_rng(0)
    random12 = rng.integers(0, 4096, (run, n, n)).astype(np.uint16)
    constant = np.full((run, n, n), 1234, np.uint16)
    lo, hi = 100, 4000
    stream = _lib.c_vp()
    _lib.check(L.hm_copy_stream_create(0, ctypes.byref(stream)), "hm_copy_stream_create")
    planes = [DeviceBuffer(run * n * n) for _ in range(3)]
    h = deepio._Handle(n, n, run, 0)
    h.set_lut(deepio.make_lut(lo, hi), lo, hi)

    def timed(call):
        for _ in range(2):
            call()
        _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
        t0 = time.perf_counter()
        for _ in range(a.reps):
            call()
        _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
        return 1e6 * (time.perf_counter() - t0) / a.reps

    parts = {"map": lambda: h.map_run_dev(random12, 0, planes[0].ptr, planes[1].ptr, planes[2].ptr, n * n, THRESHOLD, None, stream),
             "hist_random": lambda: h.hist_add(random12, 0),
             "hist_constant": lambda: h.hist_add(constant, 0)}
    rec["wall_us_per_run"] = {}
    for name, call in parts.items():
        if a.only and a.only != name:
            continue
        rec["wall_us_per_run"][name] = timed(call)
        print("%s: %.0f us per run of %d frames (upload of %d bytes included)" % (name, rec["wall_us_per_run"][name], run, 2 * run * n * n))
    h.close()
    for b in planes:
        b.close()
    L.hm_copy_stream_destroy(0, stream)
    if a.only:
        return

    # 2. the pipeline from the 16-bit pixels and from the mapped arrays, alternating
    video = bench.BenchVideo(n, a.frames + 1, 0)
    grey = np.stack([np.ascontiguousarray(video.frame_at(k)[0]) for k in range(a.frames + 1)])
    deep = (40 * grey.astype(np.int64) + 1000 + rng.integers(0, 40, grey.shape)).astype(np.uint16)
    t0 = time.perf_counter()
    win = deepio.resolve(deep, None, device=0)
    t1 = time.perf_counter()
    mapped, clipped = deepio.map_video(deep, win["lut"], win["lo"], win["hi"], device=0)
    t2 = time.perf_counter()
    rec["window"] = {"lo": win["lo"], "hi": win["hi"], "frames": a.frames + 1, "histogram_and_window_s": t1 - t0, "map_video_s": t2 - t1,
                     "clipped_below": int(clipped[:, 0].sum()), "clipped_above": int(clipped[:, 1].sum())}
    masks = threshold_mask(mapped, THRESHOLD)
    shown = mapped * masks
    c, rad = video.centre, video.radius

    def once(mode):
        dm = mesh.disk_mesh(c[0], c[1], rad - 1.0, 0.047 * n)
        kf = kalman.IteratedMSKalmanFilter(dm, mapped[0], np.zeros((n, n, 2), np.float32), True)
        src = ArraySource(mapped, masks, shown) if mode == "array" else \
            deepio.DeepSource(deep, win["lut"], win["lo"], win["hi"], THRESHOLD, frames=mapped)
        pipe = FlowEKFPipeline(kf, src)
        t0 = time.perf_counter()
        pipe.run()
        dt = time.perf_counter() - t0
        out = {"source": mode, "frames_per_s": a.frames / dt, "bus_bytes_per_frame": pipe.ring.bytes_uploaded / float(a.frames + 1)}
        pipe.close()
        kf.close()
        if mode != "array":
            src.close()
        return out

    once("array")                                   # the session's first run warms up and is not counted
    runs = []
    for _ in range(a.rounds):
        for mode in MODES:
            runs.append(once(mode))
            print("pipeline from %s: %.1f frames/s, %.0f bytes a frame over the bus"
                  % (mode, runs[-1]["frames_per_s"], runs[-1]["bus_bytes_per_frame"]))
    rec["pipeline_runs"] = runs
    rec["pipeline"] = {}
    for mode in MODES:
        v = [x["frames_per_s"] for x in runs if x["source"] == mode]
        rec["pipeline"][mode] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                                 "bus_bytes_per_frame": [x["bus_bytes_per_frame"] for x in runs if x["source"] == mode][0]}
    merge(a, rec, run)


if __name__ == "__main__":
    main()
