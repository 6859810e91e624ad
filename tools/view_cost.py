#!/usr/bin/env python
"""What the overlay video costs at 1024^2 with the bench's 201-vertex mesh.

  python tools/view_cost.py [--frames 64] [--views 200] [--video-dir /dev/shm] [--bench-line FILE] [--out profiles/..]

1. `--views` overlay views queued back to back on the filter's stream (hm_view_dev, no copies): wall time per view.
   The kernel time of one view comes from a run under `rocprofv3 --kernel-trace --stats -- python tools/view_cost.py`
   (k_setup_all + k_render<0> + k_view_wire + k_view_compose and the wireframe memset).
2. The 64-frame 1024^2 pipeline (bench.py's video) without video, with video= writing an AVI to --video-dir, and
   without again: frames/s of each.
3. --bench-line: the JSON line bench.py printed in the same session, copied into the record.
The record is one JSON file (default profiles/views_cost.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--video-dir", default="/dev/shm")
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_cost.json"))
    a = ap.parse_args()
    import hydra_mi  # noqa: F401
    from hydra_mi import _lib, kalman, mesh
    from hydra_mi.pipeline import DeviceBuffer, FlowEKFPipeline
    from hydra_mi.videoio import AviWriter
    import bench

    n = 1024
    video = bench.BenchVideo(n, a.frames + 1, 0)
    c, r = video.centre, video.radius

    def new_filter():
        dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
        f0 = video.frame_at(0)[0]
        return dm, kalman.IteratedMSKalmanFilter(dm, f0, np.zeros((n, n, 2), np.float32), True)

    rec = {"size": n}
    # 1. views back to back
    dm, kf = new_filter()
    rec["vertices"] = int(dm.size())
    fr, mk, _ = video.frame_at(1)
    rd = kf.state.renderer
    rd.set_observation(fr, np.zeros((n, n, 2), np.float32), mk)
    X = np.array(kf.state.X, np.float64).reshape(-1)
    buf = DeviceBuffer(3 * n * n)
    for _ in range(5):
        rd.view_dev(X, "overlay", buf.ptr)
    _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
    t0 = time.perf_counter()
    for _ in range(a.views):
        rd.view_dev(X, "overlay", buf.ptr)
    _lib.check(_lib.lib().hm_ctx_sync(rd._h), "hm_ctx_sync")
    rec["overlay_view_wall_us"] = 1e6 * (time.perf_counter() - t0) / a.views
    buf.close()
    kf.close()

    # 2. the pipeline with and without the video
    def run(with_video):
        _, kf = new_filter()
        pipe = FlowEKFPipeline(kf, video)
        path = os.path.join(a.video_dir, "hydra_mi_view_cost_%d.avi" % os.getpid())
        w = AviWriter(path, n, n) if with_video else None
        t0 = time.perf_counter()
        pipe.run(video=w)
        dt = time.perf_counter() - t0
        pipe.close()
        frames = w.frames if w is not None else None
        if w is not None:
            w.close()
            os.remove(path)
        kf.close()
        return (a.frames) / dt, frames

    runs = []
    for mode in (False, True, False, True):
        fps, frames = run(mode)
        runs.append({"video": mode, "frames_per_s": fps, "video_frames": frames})
        print("pipeline %s video: %.1f frames/s" % ("with" if mode else "without", fps))
    rec["pipeline_runs"] = runs
    without = [x["frames_per_s"] for x in runs if not x["video"]]
    withv = [x["frames_per_s"] for x in runs if x["video"]]
    rec["with_over_without"] = float(np.mean(withv) / np.mean(without))
    if a.bench_line and os.path.exists(a.bench_line):
        lines = [ln for ln in open(a.bench_line).read().splitlines() if ln.startswith("{")]
        rec["bench"] = json.loads(lines[-1]) if lines else None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k != "bench"}))


if __name__ == "__main__":
    main()
