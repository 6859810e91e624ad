#!/usr/bin/env python
"""What the events per pixel cost at 1024^2 with the bench's 201-vertex mesh on records of 300 and of 2 000 frames: AR(1)
deconvolution of the dF/F bytes (half = 20, q = 10, floor 16, gain 255) with g = 0.8, lam = 8, s_min = 8.

  python tools/events_cost.py [--out profiles/events_cost.json]
  python tools/events_cost.py --kernels-only --frames N            (what the profiler runs)

For each record length the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/events_cost.py --kernels-only --frames N` (a run of its own, no counters with it; the first run that fails ends the
tool): one hm_body_rec_event_stats_add and one hm_body_rec_event_sums of the whole record.  From its kernel_stats.csv: the
times of k_rec_ev_push, k_rec_ev_read, k_rec_running, k_rec_paste and k_body_stats_add.  Then, without the profiler, the
wall time of each call (event_planes on 64 frames; event_sums also at hm_ctx_tune "rec_ev_bytes" 2^28 .. 2^34), and the restatement in Python floats (tests/events_ref.py) on a cut of
the box on this host, extrapolated to the box by the time per pixel -- labelled so.  Beside the times, the bytes the
arithmetic of DESIGN.md section 19 predicts: 20 B of pool stack per frame and pixel, written once, plus the source plane's
byte read and the event byte written; the achieved bytes/s are those over the time of k_rec_ev_push and k_rec_ev_read.
The video and the record are those of tools/demix_cost.py.  The result is one JSON file (default
profiles/events_cost.json).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KERNELS = ("k_rec_ev_push", "k_rec_ev_read", "k_rec_running", "k_rec_paste", "k_body_stats_add")
RECORDS = (300, 2000)
DET = dict(what="dff", half=20, q=10, floor=16, gain=255)
G, LAM, SMIN, CUT, SIDE = 0.8, 8.0, 8.0, 64, 24


def kernels_only(frames):
    from demix_cost import record
    kf, b, _ = record(frames)
    rd = kf.state.renderer
    rd.body_stats_begin()
    rd.body_rec_event_stats_add(g=G, lam=LAM, **DET)
    rd.body_stats_end()
    rd.body_rec_event_sums(g=G, lam=LAM, s_min=SMIN, **DET)
    rd.body_rec_end()
    kf.close()


def profiled(frames):
    one = {}
    with tempfile.TemporaryDirectory() as tmp:
        tail = ["--kernels-only", "--frames", str(frames)]
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, os.path.abspath(__file__)] + tail
        one["kernel_stats_from"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/events_cost.py " + " ".join(tail)
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                       # (nothing more is started on the GPU after a run that failed)
            raise RuntimeError("the profiled run failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if len(found) != 1:
            raise RuntimeError("expected one kernel_stats.csv under the profiler's directory, found %r" % found)
        for row in csv.DictReader(open(found[0])):
            for kernel in KERNELS:
                if row.get("Name", "").startswith(kernel + "("):
                    one[kernel + "_launches"] = int(row["Calls"])
                    one[kernel + "_total_ms"] = float(row["AverageNs"]) * int(row["Calls"]) / 1e6
    return one


def wall(call):
    call()
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def measure(F):
    one = profiled(F)                                 # (two calls in it: both push all F frames, one reads E, one the sums)
    from demix_cost import record                     # (the profiled run is over: this process opens the GPU only now)
    import detrend_ref
    import events_ref
    kf, b, _ = record(F)
    rd = kf.state.renderer
    m = b.tri_of_pixel >= 0
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    pitch = (bw + 3) // 4 * 4
    fs = ((pitch * bh + 15) // 16) * 16
    npx = -(-pitch * bh // 64) * 64
    passes = -(-(npx // 64) // max(1, min(npx // 64, (1 << 34) // (20 * 64 * F))))
    one.update(frames=F, map_pixels=int(m.sum()), box=[bw, bh], frame_bytes=fs, stack_pixels=npx, passes=passes)
    # per call: the stack's 20 B per frame and pixel written once (re-read on merges: not counted), the source byte read
    stack, src = 20 * F * npx, F * fs
    one.update(stack_bytes=stack, source_bytes=src, event_bytes=F * fs)
    t = one.get("k_rec_ev_push_total_ms", 0.0) + one.get("k_rec_ev_read_total_ms", 0.0)
    if t:
        one["bytes_per_s"] = (2 * (stack + src) + F * fs) / (t * 1e-3)          # (the profiled run holds two calls, one writes E)

    def stats_add():
        rd.body_stats_begin()
        rd.body_rec_event_stats_add(g=G, lam=LAM, **DET)
        rd.body_stats_end()
    k0, n = F // 2, min(CUT, F - F // 2)
    one["event_stats_add_wall_ms"] = wall(stats_add)
    one["event_sums_wall_ms"] = wall(lambda: rd.body_rec_event_sums(g=G, lam=LAM, s_min=SMIN, **DET))
    one["event_sums_wall_ms_by_rec_ev_bytes"] = {}       # the pass size: fewer, larger passes have more waves to wait with
    for bits in (28, 30, 32, 34):
        rd.tune("rec_ev_bytes", 1 << bits)
        one["event_sums_wall_ms_by_rec_ev_bytes"]["2^%d" % bits] = wall(lambda: rd.body_rec_event_sums(g=G, lam=LAM, s_min=SMIN, **DET))
    one["event_planes_%d_frames_wall_ms" % CUT] = wall(lambda: rd.body_rec_event_planes(g=G, lam=LAM, k0=k0, n=n, **DET))
    got = rd.body_rec_event_planes(g=G, lam=LAM, k0=k0, n=n, **DET)
    # the restatement on the same host: a cut of SIDE x SIDE pixels in the middle of the box, all frames
    r0, c0 = int(rows[0]) + bh // 2, int(cols[0]) + bw // 2
    sl = (slice(None), slice(r0, r0 + SIDE), slice(c0, c0 + SIDE))
    y = detrend_ref.planes(rd.body_rec_fetch()[sl], m[sl[1:]], 3, DET["half"], DET["q"], DET["floor"], DET["gain"])
    t0 = time.perf_counter()
    E = events_ref.video(y, (0, SIDE, 0, SIDE), G, LAM, SMIN)[0]
    sec = time.perf_counter() - t0
    one["restatement"] = {"pixels_computed": SIDE * SIDE, "seconds": sec, "extrapolated_to_box_s": sec / (SIDE * SIDE) * bw * bh,
                          "note": "Python floats on %d x %d pixels of the box over all %d frames (the dF/F bytes given), "
                                  "extrapolated to the %d x %d box by the time per pixel" % (SIDE, SIDE, F, bw, bh)}
    one["cut_equals_restatement"] = bool(np.array_equal(got[sl], E[k0:k0 + n]))
    one["events_in_cut"] = int((E > 0).sum())
    rd.body_rec_end()
    kf.close()
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.frames)
        return
    rec = {"size": 1024, "g": G, "lam": LAM, "s_min": SMIN, "planes": DET, "records": {}}
    for F in ((a.frames,) if a.frames else RECORDS):
        rec["records"][str(F)] = measure(F)
        print("%d frames: %s" % (F, json.dumps(rec["records"][str(F)])), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
