#!/usr/bin/env python
"""What decoding Motion-JPEG on the device costs at 1024^2, grey, quality 90.

  python tools/mjpeg_decode_cost.py [--frames 64] [--reps 20] [--rounds 3] [--only FILE:ENTROPY]
                                    [--kernel-stats FILE:ENTROPY=kernel_stats.csv ...]
                                    [--bench-line FILE] [--video-dir /dev/shm] [--out profiles/mjpeg_decode_cost.json]

1. A run of 8 frames (hm_mjpeg_decode_run_dev on one stream, three planes written) by each entropy path, wall time per
   run, for a file of this library's encoder (restart_rows 1: 128 intervals), a PIL file without restart markers and a
   4:2:0 colour file of PIL; then the same grey frames cut by PIL into 128 ... 4096 restart intervals, to find the number
   of intervals from which the device path is the faster one (the "auto_intervals" tune).  With every figure goes what
   the decoder queued host-to-device per frame (hm_mjpeg_dec_uploaded).  Kernel times come from runs of their own, one
   per kind of file and entropy path, under `rocprofv3 --kernel-trace --stats -- python tools/mjpeg_decode_cost.py --only
   encoder_rows1:device` (no counters alongside; --only decodes that one combination and writes no record);
   --kernel-stats encoder_rows1:device=.../kernel_stats.csv puts that run's k_mjdec_* rows into the record under its name.
2. The 64-frame pipeline (FlowEKFPipeline.run, bench.py's video coded as an MJPEG AVI of restart_rows 1) from an
   ArraySource of the decoded frames, masks and shown frames, from an AviSource as it is by default (entropy "auto": the
   host pool for these 128-interval frames, so coefficients cross the bus) and from an AviSource with the device entropy
   path forced (the JPEG bytes cross), in turn --rounds times after one run that is not counted: frames/s of each and the
   bytes per frame that were queued host-to-device, as the ring counted them.  Nothing is downloaded in either.
3. --bench-line: the JSON lines bench.py printed in the same session, copied into the record.
No speed-up is promised; the record says what came out.
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
MODES = ("array", "avi", "avi_device")


def pil_file(frame, **kw):
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", **kw)
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--only", default=None, metavar="FILE:ENTROPY")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="FILE:ENTROPY=CSV")
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--video-dir", default="/dev/shm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mjpeg_decode_cost.json"))
    a = ap.parse_args()
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, kalman, mesh, videoio
    from hydra_mi.pipeline import ArraySource, DeviceBuffer, FlowEKFPipeline, threshold_mask
    import bench

    L = _lib.lib()
    n, run = 1024, 8
    video = bench.BenchVideo(n, a.frames + 1, 0)
    rec = {"size": n, "quality": a.quality, "run": run, "raw_frame_bytes": n * n}

    # 1. a run of 8 frames by each entropy path
    grey = [np.ascontiguousarray(video.frame_at(k)[0]) for k in range(run)]
    enc = videoio.MjpegEncoder(n, n, 1, a.quality, 1)
    files = {"encoder_rows1": [enc.encode(f) for f in grey],
             "pil_no_restart": [pil_file(f, quality=a.quality) for f in grey],
             "pil_420_colour": [pil_file(np.stack([f, f[::-1], f.T], 2), quality=a.quality, subsampling=2) for f in grey]}
    enc.close()
    stream = _lib.c_vp()
    _lib.check(L.hm_copy_stream_create(0, ctypes.byref(stream)), "hm_copy_stream_create")
    planes = [DeviceBuffer(run * n * n) for _ in range(3)]
    rec["decode"] = {}
    for name, chunks in files.items():
        if a.only and a.only.split(":")[0] != name:
            continue
        info = videoio.mjpeg_probe(chunks[0])
        item = {"file_bytes": float(np.mean([len(c) for c in chunks])), "intervals": info["intervals"], "components": info["components"]}
        for entropy in ("host", "device"):
            if a.only and a.only.split(":")[1] != entropy:
                continue
            reps = 2 if entropy == "device" and info["ri"] == 0 else a.reps      # (one lane decodes a whole frame: not twenty times)
            dec = videoio.MjpegDecoder(n, n, run, entropy=entropy)
            for _ in range(2):
                dec.decode_run_dev(chunks, planes[0].ptr, planes[1].ptr, planes[2].ptr, threshold=THRESHOLD, stream=stream)
            _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
            t0 = time.perf_counter()
            for _ in range(reps):
                sent = dec.decode_run_dev(chunks, planes[0].ptr, planes[1].ptr, planes[2].ptr, threshold=THRESHOLD, stream=stream)
            _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
            item["wall_us_per_run_%s" % entropy] = 1e6 * (time.perf_counter() - t0) / reps
            item["h2d_bytes_per_frame_%s" % entropy] = sent / float(run)
            dec.close()
        rec["decode"][name] = item
        print("%s: %d bytes a frame, %d intervals; a run of %d: %s" % (name, item["file_bytes"], item["intervals"], run, ", ".join(
            "%s %.0f us and %.0f bytes a frame over the bus" % (e, item["wall_us_per_run_" + e], item["h2d_bytes_per_frame_" + e])
            for e in ("host", "device") if "wall_us_per_run_" + e in item)))
    if a.only:
        for b in planes:
            b.close()
        L.hm_copy_stream_destroy(0, stream)
        return
    # where the device path overtakes the host pool: the same frames cut into ever more restart intervals
    rec["sweep"] = []
    for blocks in (128, 64, 32, 16, 8, 4):
        chunks = [pil_file(f, quality=a.quality, restart_marker_blocks=blocks) for f in grey]
        row = {"intervals": videoio.mjpeg_probe(chunks[0])["intervals"], "file_bytes": float(np.mean([len(c) for c in chunks]))}
        for entropy in ("host", "device"):
            dec = videoio.MjpegDecoder(n, n, run, entropy=entropy)
            for _ in range(2):
                dec.decode_run_dev(chunks, planes[0].ptr, planes[1].ptr, planes[2].ptr, threshold=THRESHOLD, stream=stream)
            _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
            t0 = time.perf_counter()
            for _ in range(a.reps):
                sent = dec.decode_run_dev(chunks, planes[0].ptr, planes[1].ptr, planes[2].ptr, threshold=THRESHOLD, stream=stream)
            _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
            row["wall_us_per_run_%s" % entropy] = 1e6 * (time.perf_counter() - t0) / a.reps
            row["h2d_bytes_per_frame_%s" % entropy] = sent / float(run)
            dec.close()
        rec["sweep"].append(row)
        print("%d intervals a frame: host %.0f us, device %.0f us" % (row["intervals"], row["wall_us_per_run_host"], row["wall_us_per_run_device"]))
    for b in planes:
        b.close()
    L.hm_copy_stream_destroy(0, stream)
    rec["kernels"] = {}                                 # per kind of file and entropy path: a run of 8 frames per call
    for item in a.kernel_stats:
        label, _, path = item.partition("=")
        if not os.path.exists(path):
            continue
        with open(path) as f:
            rows = [row for row in csv.DictReader(f) if "k_mjdec" in row.get("Name", "")]
        rec["kernels"][label] = [{"name": row["Name"].split("(")[0], "calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                  "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3} for row in rows]

    # 2. the pipeline from the JPEG bytes and from the decoded arrays, alternating
    path = os.path.join(a.video_dir, "hydra_mi_mjpeg_decode_cost_%d.avi" % os.getpid())
    with videoio.AviWriter(path, n, n, codec="mjpeg", channels=1, quality=a.quality, restart_rows=1) as w:
        for k in range(a.frames + 1):
            w.write(np.ascontiguousarray(video.frame_at(k)[0]))
    with videoio.AviReader(path) as r:
        decoded = videoio.decode_avi(r)
        rec["avi_bytes_per_frame"] = float(np.mean([len(r.chunk(f)) for f in range(len(r))]))
    masks = threshold_mask(decoded, THRESHOLD)
    shown = decoded * masks
    c, rad = video.centre, video.radius

    def once(mode):
        dm = mesh.disk_mesh(c[0], c[1], rad - 1.0, 0.047 * n)
        kf = kalman.IteratedMSKalmanFilter(dm, decoded[0], np.zeros((n, n, 2), np.float32), True)
        src = ArraySource(decoded, masks, shown) if mode == "array" else \
            videoio.AviSource(path, THRESHOLD, frames=decoded, entropy="device" if mode == "avi_device" else "auto")
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
    os.remove(path)
    rec["pipeline_runs"] = runs
    rec["pipeline"] = {}
    for mode in MODES:
        v = [x["frames_per_s"] for x in runs if x["source"] == mode]
        rec["pipeline"][mode] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                                 "bus_bytes_per_frame": [x["bus_bytes_per_frame"] for x in runs if x["source"] == mode][0]}
    if a.bench_line and os.path.exists(a.bench_line):
        lines = [ln for ln in open(a.bench_line).read().splitlines() if ln.startswith("{")]
        rec["bench"] = [json.loads(ln) for ln in lines]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("bench", "pipeline_runs")}))


if __name__ == "__main__":
    main()
