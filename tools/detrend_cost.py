#!/usr/bin/env python
"""What the running baseline per pixel costs at 1024^2 with the bench's 201-vertex mesh on a record of 2 000 frames,
half = 100, q = 10.

  python tools/detrend_cost.py [--out profiles/detrend_cost.json]
  python tools/detrend_cost.py --kernels-only stats|planes --run N       (what the profiler runs)

For each of three run lengths (hm_ctx_tune "rec_bl_frames") the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace
--stats --output-format csv -- python tools/detrend_cost.py --kernels-only stats --run N` (a run of its own, no counters
with it; the first run that fails ends the tool): one hm_body_rec_stats_add of the excess planes of the whole record.  From
its kernel_stats.csv: the time of k_rec_running per launch, per frame and per call, and of k_rec_paste and
k_body_stats_add.  One more such run with `--kernels-only planes` at the default run length: one hm_body_rec_planes of
64 frames.  Then, without the profiler, the wall time of both calls, and the NumPy restatement (tests/detrend_ref.py) on a
cut of 64 frames of the record's box with their full windows, on this host, extrapolated to the record -- labelled so.
Beside the times, the bytes the arithmetic of DESIGN.md section 14 predicts.  The video and the record are those of
tools/demix_cost.py.  The result is one JSON file (default profiles/detrend_cost.json).
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
KERNELS = ("k_rec_running", "k_rec_paste", "k_body_stats_add")
FRAMES, HALF, Q, CUT = 2000, 100, 10, 64
RUNS = (8, 16, 64)
SCRATCH = 16 << 20


def kernels_only(mode, run, frames):
    from demix_cost import record
    kf, b, _ = record(frames)
    rd = kf.state.renderer
    if run:
        rd.tune("rec_bl_frames", run)
    if mode == "stats":
        rd.body_stats_begin()
        rd.body_rec_stats_add("excess", HALF, Q)
        rd.body_stats_end()
    else:
        rd.body_rec_planes("excess", HALF, Q, k0=frames // 2, n=min(CUT, frames - frames // 2))
    rd.body_rec_end()
    kf.close()


def profiled(mode, run, frames):
    one = {}
    with tempfile.TemporaryDirectory() as tmp:
        tail = ["--kernels-only", mode, "--run", str(run), "--frames", str(frames)]
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, os.path.abspath(__file__)] + tail
        one["kernel_stats_from"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/detrend_cost.py " + " ".join(tail)
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                       # (nothing more is started on the GPU after a run that failed)
            raise RuntimeError("the profiled run failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if len(found) != 1:
            raise RuntimeError("expected one kernel_stats.csv under the profiler's directory, found %r" % found)
        for row in csv.DictReader(open(found[0])):
            for kernel in KERNELS:
                if row.get("Name", "").startswith(kernel + "("):
                    one[kernel] = {k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in row}
                    one[kernel + "_launches"] = int(row["Calls"])
                    one[kernel + "_total_ms"] = float(row["AverageNs"]) * int(row["Calls"]) / 1e6
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--kernels-only", choices=("stats", "planes"), default=None)
    ap.add_argument("--run", type=int, default=0, help="rec_bl_frames (0: the default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detrend_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.kernels_only, a.run, a.frames)
        return
    F = a.frames
    rec = {"size": 1024, "frames": F, "half": HALF, "q": Q, "stats_add_by_run_length": {}}
    for run in RUNS:
        one = profiled("stats", run, F)
        if "k_rec_running_total_ms" in one:
            one["k_rec_running_us_per_frame"] = 1e3 * one["k_rec_running_total_ms"] / F
        rec["stats_add_by_run_length"][str(run)] = one
        print("run %d: %s" % (run, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})), flush=True)
    rec["planes_%d_frames" % CUT] = profiled("planes", 0, F)
    from demix_cost import record                     # (the profiled runs are over: this process opens the GPU only now)
    import detrend_ref
    kf, b, _ = record(F)
    rd = kf.state.renderer
    m = b.tri_of_pixel >= 0
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    fs = ((((bw + 3) // 4 * 4) * bh + 15) // 16) * 16
    per = max(1, min(F, SCRATCH // fs))
    rec.update(map_pixels=int(m.sum()), box=[bw, bh], frame_bytes=fs, frames_per_scratch=per)
    # the arithmetic to check the times against: every record byte read entering, leaving and as the current frame; a
    # run reads 2 half + 1 frames more; one byte written per pixel and frame (runs never reach beyond a scratch batch)
    for run in RUNS:
        runs = sum(-(-min(per, F - k) // run) for k in range(0, F, per))
        read = (3 * F + runs * (2 * HALF + 1)) * fs
        one = rec["stats_add_by_run_length"][str(run)]
        one.update(runs=runs, bytes_read=read, bytes_written=F * fs)
        if one.get("k_rec_running_total_ms"):
            one["bytes_per_s"] = (read + F * fs) / (one["k_rec_running_total_ms"] * 1e-3)
    rd.body_stats_begin()
    rd.body_rec_stats_add("excess", HALF, Q)
    t0 = time.perf_counter()
    rd.body_rec_stats_add("excess", HALF, Q)
    rec["stats_add_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    rd.body_stats_end()
    k0 = F // 2
    n = min(CUT, F - k0)
    rd.body_rec_planes("excess", HALF, Q, k0=k0, n=n)
    t0 = time.perf_counter()
    got = rd.body_rec_planes("excess", HALF, Q, k0=k0, n=n)
    rec["planes_%d_frames_wall_ms" % CUT] = 1e3 * (time.perf_counter() - t0)
    # the restatement on the same host: the frames the cut's windows reach, cropped to the box
    a0, b0 = max(0, k0 - HALF), min(F, k0 + n + HALF)
    sl = (slice(None), slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1))
    regs = rd.body_rec_fetch(a0, b0 - a0)[sl]
    t0 = time.perf_counter()
    want = detrend_ref.planes(regs, m[sl[1:]], 2, HALF, Q, k0=k0 - a0, n=n)
    sec = time.perf_counter() - t0
    rec["numpy_restatement"] = {"frames_computed": n, "seconds": sec, "seconds_per_frame": sec / n,
                                "extrapolated_to_record_s": sec / n * F,
                                "note": "measured on %d frames of the box with their full windows, extrapolated to %d by the "
                                        "time per frame" % (n, F)}
    rec["cut_equals_restatement"] = bool(np.array_equal(got[sl], want))
    rd.body_rec_end()
    kf.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
