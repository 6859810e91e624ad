#!/usr/bin/env python
"""What the correction for tissue compression (hydra_mi.deform) costs at 1024^2 with the bench's 201-vertex mesh on records
of 300 and of 2000 frames.

  python tools/deform_cost.py [--out profiles/deform_cost.json]
  python tools/deform_cost.py --kernels-only --frames N [--run R]         (what the profiler runs)

For each record length, and for the longer one at runs of 16, 64 and 256 frames (hm_ctx_tune "rec_tm_frames": the shorter
the run, the more 64-bit atomics meet in the sums), the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace --stats
--output-format csv -- python tools/deform_cost.py --kernels-only --frames N` (a run of its own, no counters with it; the
first run that fails ends the tool): three hm_body_rec_tri_maps and three hm_body_rec_tri_gain calls over the whole
record (neither kernel's work depends on the values).  From its kernel_stats.csv: the time of k_rec_tri_maps and
k_rec_tri_gain per launch, beside the bytes of the record they read (and, the gain, write) and the bytes per second that
follow.  Then, without the profiler: the wall time of each call, copies included, and of deform.correct as a whole.
The video and the record are those of tools/demix_cost.py.  The result is one JSON file (default
profiles/deform_cost.json).
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
KERNELS = ("k_rec_tri_maps", "k_rec_tri_gain")
FRAMES = (300, 2000)
RUNS = (16, 64, 256)
CALLS = 3


def tables(frames, T):
    rng = np.random.default_rng(1)
    return (rng.integers(-32767, 32768, (frames, T)).astype(np.int32), np.full((frames, T), 4096, np.uint16))


def states_of(kf, frames):
    """the state at rest breathing by 10 % in area: something for the fit to look at"""
    X = np.array(kf.state.X, np.float64).reshape(-1)
    N = len(X) // 4
    p = X[:2 * N].reshape(N, 2)
    c = p.mean(0)
    out = np.tile(X, (frames, 1))
    for k in range(frames):
        out[k, :2 * N] = (c + (p - c) * (1.0 - 0.05 * (1.0 - np.cos(k / 12.0)) / 2.0)).reshape(-1)
    return out


def kernels_only(frames, run):
    from demix_cost import record
    kf, b, pts = record(frames)
    rd = kf.state.renderer
    if run:
        rd.tune("rec_tm_frames", run)
    q, m = tables(frames, rd.tri.shape[0])
    for _ in range(CALLS):
        rd.body_rec_tri_maps(q)
        rd.body_rec_tri_gain(m)
    rd.body_rec_end()
    kf.close()


def profiled(frames, run=0):
    one = {}
    with tempfile.TemporaryDirectory() as tmp:
        tail = ["--kernels-only", "--frames", str(frames)] + (["--run", str(run)] if run else [])
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, os.path.abspath(__file__)] + tail
        one["kernel_stats_from"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/deform_cost.py " + " ".join(tail)
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                       # (nothing more is started on the GPU after a run that failed)
            raise RuntimeError("the profiled run failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if len(found) != 1:
            raise RuntimeError("expected one kernel_stats.csv under the profiler's directory, found %r" % found)
        for row in csv.DictReader(open(found[0])):
            for kernel in KERNELS:
                name = row.get("Name", "")                         # ("k_rec_tri_gain(...)", "void k_rec_tri_maps<1>(...)")
                if name.startswith(kernel + "(") or name.startswith("void " + kernel + "<"):
                    one[kernel] = {k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in row}
                    one[kernel + "_launches"] = int(row["Calls"])
                    one[kernel + "_total_ms_per_call"] = float(row["TotalDurationNs"]) / 1e6 / CALLS
                    one[kernel + "_min_ms"] = float(row["MinNs"]) / 1e6
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=FRAMES[0])
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--run", type=int, default=0, help="rec_tm_frames (0: the default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.frames, a.run)
        return
    rec = {"size": 1024, "calls_per_profiled_run": CALLS, "rec_tm_frames": 64, "records": {}, "by_run_length": {"frames": FRAMES[-1]}}
    for F in FRAMES:
        rec["records"][str(F)] = profiled(F)
        print("%d frames: %s" % (F, json.dumps({k: v for k, v in rec["records"][str(F)].items() if not isinstance(v, dict)})), flush=True)
    for run in RUNS:
        one = profiled(FRAMES[-1], run)
        one.update(runs=-(-FRAMES[-1] // run))
        rec["by_run_length"][str(run)] = one
        print("run %d: %s" % (run, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})), flush=True)
    from demix_cost import record                     # (the profiled runs are over: this process opens the GPU only now)
    from hydra_mi import deform
    for F in FRAMES:
        one = rec["records"][str(F)]
        kf, b, pts = record(F)
        rd = kf.state.renderer
        m = b.tri_of_pixel >= 0
        rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
        fs = ((((bw + 3) // 4 * 4) * bh + 15) // 16) * 16
        T = int(rd.tri.shape[0])
        one.update(triangles=T, map_pixels=int(m.sum()), box=[bw, bh], frame_bytes=fs, record_bytes=F * fs)
        # the arithmetic to check the times against: the maps read the record once, the gain reads and writes it once
        for kernel, passes in (("k_rec_tri_maps", 1), ("k_rec_tri_gain", 2)):
            if one.get(kernel + "_total_ms_per_call"):
                one[kernel + "_record_bytes_per_s"] = passes * F * fs / (one[kernel + "_total_ms_per_call"] * 1e-3)
        if F == FRAMES[-1]:
            for run in RUNS:
                o = rec["by_run_length"][str(run)]
                o.update(atomics=3 * int(m.sum()) * o["runs"])
                o["k_rec_tri_maps_record_bytes_per_s"] = F * fs / (o["k_rec_tri_maps_total_ms_per_call"] * 1e-3)
        q, gain = tables(F, T)
        rd.body_rec_tri_maps(q)
        t0 = time.perf_counter()
        rd.body_rec_tri_maps(q)
        one["tri_maps_call_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        rd.body_rec_tri_gain(gain)
        t0 = time.perf_counter()
        rd.body_rec_tri_gain(gain)
        one["tri_gain_call_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        d = deform.correct(b, states_of(kf, F))
        one["correct_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        one["correct_gamma"] = d["gamma"]
        rd.body_rec_end()
        kf.close()
        print("%d frames: %s" % (F, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
