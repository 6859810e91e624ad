#!/usr/bin/env python
"""What the Motion-JPEG video costs at 1024^2 with the bench's 201-vertex mesh, quality 90.

  python tools/mjpeg_cost.py [--frames 64] [--encodes 200] [--rounds 3] [--video-dir /dev/shm] [--encode-only]
                             [--only overlay|registered] [--kernel-stats KIND=FILE.csv ...] [--bench-line FILE]
                             [--out profiles/mjpeg_cost.json]

1. An overlay frame (B G R, three components) and a registered frame (grey, one component) of the tracker encoded
   `--encodes` times back to back (hm_mjpeg_encode_dev on one stream, stream and size word left on the device): wall
   time per encode, the stream's bytes against the raw frame's 3 145 728.  The kernel time of every launch comes from a
   run of its own per kind of frame under `rocprofv3 --kernel-trace --stats -- python tools/mjpeg_cost.py --encode-only
   --only KIND` (no counters alongside); --kernel-stats KIND=FILE takes that run's kernel_stats.csv and puts the
   k_mjpeg_* rows into the record.
2. The 64-frame 1024^2 pipeline (bench.py's video) with no video, with a raw video and with an MJPEG video written to
   --video-dir, alternating, `--rounds` times after one run that is not counted: frames/s of each, their spread, and the bytes the MJPEG video copied
   over the bus per frame (VideoTap.bus_bytes).
3. The arithmetic bound of the encoder: the frame read once and the stream written against the DCT's multiply-adds.
4. --bench-line: the JSON line bench.py printed in the same session, copied into the record.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12        # MI355X: 8 TB/s
INT_OPS_PER_S = 256 * 4 * 16 * 2.4e9 / 1.0      # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz 32-bit integer multiply-adds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--encodes", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--video-dir", default="/dev/shm")
    ap.add_argument("--encode-only", action="store_true")
    ap.add_argument("--only", default=None, choices=("overlay", "registered"))
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="KIND=FILE")
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mjpeg_cost.json"))
    a = ap.parse_args()
    import ctypes
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, kalman, mesh
    from hydra_mi.pipeline import DeviceBuffer, FlowEKFPipeline
    from hydra_mi.videoio import AviWriter, MjpegEncoder
    import bench

    L = _lib.lib()
    n = 1024
    video = bench.BenchVideo(n, a.frames + 1, 0)
    c, r = video.centre, video.radius

    def new_filter():
        dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
        f0 = video.frame_at(0)[0]
        return dm, kalman.IteratedMSKalmanFilter(dm, f0, np.zeros((n, n, 2), np.float32), True)

    rec = {"size": n, "quality": a.quality, "raw_frame_bytes": 3 * n * n}
    # 1. the two kinds of frame, encoded back to back
    dm, kf = new_filter()
    rec["vertices"] = int(dm.size())
    fr, mk, _ = video.frame_at(1)
    rd = kf.state.renderer
    rd.set_observation(fr, np.zeros((n, n, 2), np.float32), mk)
    X = np.array(kf.state.X, np.float64).reshape(-1)
    frames = {"overlay": rd.view(X, "overlay"), "registered": rd.body_warp(X, fr)[0]}
    stream = _lib.c_vp()
    _lib.check(L.hm_copy_stream_create(0, ctypes.byref(stream)), "hm_copy_stream_create")
    rec["encode"] = {}
    for name, frame in frames.items():
        if a.only not in (None, name):
            continue
        ch = 3 if frame.ndim == 3 else 1
        enc = MjpegEncoder(n, n, ch, a.quality, 1)
        d_frame, d_out, d_word = DeviceBuffer(frame.nbytes), DeviceBuffer(enc.max_stream), DeviceBuffer(16)
        d_frame.upload(frame)
        for _ in range(5):
            enc.encode_dev(d_frame.ptr, d_out.ptr, enc.max_stream, d_word.ptr, stream)
        _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
        t0 = time.perf_counter()
        for _ in range(a.encodes):
            enc.encode_dev(d_frame.ptr, d_out.ptr, enc.max_stream, d_word.ptr, stream)
        _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
        wall = 1e6 * (time.perf_counter() - t0) / a.encodes
        size = int(d_word.download(np.empty(4, np.uint32))[0])
        blocks = (n // 8) ** 2 * ch
        macs = blocks * 2 * 8 * 64                      # two passes of eight 8-point transforms of 8 multiply-adds
        traffic = frame.nbytes + size
        rec["encode"][name] = {
            "components": ch, "wall_us_per_encode": wall, "stream_bytes": size, "file_bytes": size + len(enc.header),
            "of_raw_frame": (size + len(enc.header)) / (3.0 * n * n), "max_stream_bytes": enc.max_stream,
            "bound": {"bytes_read_once_plus_stream": traffic, "us_at_hbm_rate": 1e6 * traffic / HBM_BYTES_PER_S,
                      "dct_multiply_adds": macs, "us_at_integer_rate": 1e6 * macs / INT_OPS_PER_S}}
        print("%s: %.1f us per encode (wall), %d bytes of %d" % (name, wall, size + len(enc.header), 3 * n * n))
        for b in (d_frame, d_out, d_word):
            b.close()
        enc.close()
    L.hm_copy_stream_destroy(0, stream)
    kf.close()
    for item in a.kernel_stats:
        kind, _, path = item.partition("=")
        if os.path.exists(path):
            with open(path) as f:
                rows = [row for row in csv.DictReader(f) if "k_mjpeg" in row.get("Name", "")]
            rec.setdefault("kernels", {})[kind] = [
                {"name": row["Name"].split("(")[0], "calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                 "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3} for row in rows]

    # 2. the pipeline with no video, a raw one and an MJPEG one, alternating
    def run(mode):
        _, kf = new_filter()
        pipe = FlowEKFPipeline(kf, video)
        path = os.path.join(a.video_dir, "hydra_mi_mjpeg_cost_%d.avi" % os.getpid())
        w = None
        if mode == "raw":
            w = AviWriter(path, n, n)
        elif mode == "mjpeg":
            w = AviWriter(path, n, n, codec="mjpeg", quality=a.quality)
        t0 = time.perf_counter()
        pipe.run(video=w)
        dt = time.perf_counter() - t0
        copied = pipe.video_tap.bus_bytes if w is not None else 0
        pipe.close()
        out = {"video": mode, "frames_per_s": a.frames / dt, "bus_bytes_per_frame": copied / float(a.frames)}
        if w is not None:
            w.close()
            out["file_bytes_per_frame"] = os.path.getsize(path) / float(a.frames)
            os.remove(path)
        kf.close()
        return out

    if not a.encode_only:
        run("none")                                     # the session's first run warms up and is not counted
        runs = []
        for _ in range(a.rounds):
            for mode in ("none", "raw", "mjpeg"):
                runs.append(run(mode))
                print("pipeline, %s video: %.1f frames/s" % (mode, runs[-1]["frames_per_s"]))
        rec["pipeline_runs"] = runs
        rec["pipeline"] = {}
        for mode in ("none", "raw", "mjpeg"):
            v = [x["frames_per_s"] for x in runs if x["video"] == mode]
            rec["pipeline"][mode] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    if a.bench_line and os.path.exists(a.bench_line):
        lines = [ln for ln in open(a.bench_line).read().splitlines() if ln.startswith("{")]
        rec["bench"] = [json.loads(ln) for ln in lines]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("bench", "pipeline_runs")}))


if __name__ == "__main__":
    main()
