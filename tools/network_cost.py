#!/usr/bin/env python
"""What the trace maps of hydra_mi.network cost at 1024^2 with the bench's 201-vertex mesh on a record of 300 frames.

  python tools/network_cost.py [--out profiles/network_cost.json]
  python tools/network_cost.py --kernels-only --traces L                  (what the profiler runs)

For L = 8, 32 and 128 traces the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv --
python tools/network_cost.py --kernels-only --traces L` (a run of its own, no counters with it; the first run that fails
ends the tool): three hm_body_rec_trace_maps calls over the whole record with random traces (the kernel's work does not
depend on the values), and the same for 32 traces at runs of 16, 64 and 256 frames (hm_ctx_tune "rec_map_frames": the
shorter the run, the more 64-bit atomics meet in the sums).  From its kernel_stats.csv: the time of k_rec_trace_maps per
launch, beside the bytes of the record it reads (once per group of 8 traces) and the bytes per second that follow.  Then, without the profiler: the wall time of
one such call, copies included, and the same maps made the only way there was before -- body_rec_fetch plus an int64 NumPy
product on the same box (L = 8 only: the host's time grows with L as the product does) -- and the ratio of the two.
The video and the record are those of tools/demix_cost.py.  The result is one JSON file (default
profiles/network_cost.json).
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
KERNEL = "k_rec_trace_maps"
FRAMES = 300
TRACES = (8, 32, 128)
HOST_TRACES = 8
RUNS = (16, 64, 256)
RUN_TRACES = 32
CALLS = 3


def traces(frames, L):
    return np.random.default_rng(1).integers(-32767, 32768, (frames, L)).astype(np.int32)


def kernels_only(L, frames, run):
    from demix_cost import record
    kf, b, pts = record(frames)
    rd = kf.state.renderer
    if run:
        rd.tune("rec_map_frames", run)
    q = traces(frames, L)
    for _ in range(CALLS):
        rd.body_rec_trace_maps(q)
    rd.body_rec_end()
    kf.close()


def profiled(L, frames, run=0):
    one = {}
    with tempfile.TemporaryDirectory() as tmp:
        tail = ["--kernels-only", "--traces", str(L), "--frames", str(frames)] + (["--run", str(run)] if run else [])
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, os.path.abspath(__file__)] + tail
        one["kernel_stats_from"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/network_cost.py " + " ".join(tail)
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                       # (nothing more is started on the GPU after a run that failed)
            raise RuntimeError("the profiled run failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if len(found) != 1:
            raise RuntimeError("expected one kernel_stats.csv under the profiler's directory, found %r" % found)
        for row in csv.DictReader(open(found[0])):
            if row.get("Name", "").startswith(KERNEL + "("):
                one[KERNEL] = {k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in row}
                one[KERNEL + "_launches"] = int(row["Calls"])
                one[KERNEL + "_ms"] = float(row["AverageNs"]) / 1e6
                one[KERNEL + "_min_ms"] = float(row["MinNs"]) / 1e6
    return one


def host_maps(rd, q, box):
    """the same sums from the fetched frames: an int64 product on the box of the map, frame by frame"""
    r0, r1, c0, c1 = box
    F, L = q.shape
    c = np.zeros((L, r1 - r0, c1 - c0), np.int64)
    w1, w2 = np.zeros(c.shape[1:], np.int64), np.zeros(c.shape[1:], np.int64)
    q64 = q.astype(np.int64)
    for k0 in range(0, F, 50):
        v = rd.body_rec_fetch(k0, min(50, F - k0))[:, r0:r1, c0:c1].astype(np.int64)
        for j in range(v.shape[0]):
            c += q64[k0 + j][:, None, None] * v[j][None]
            w1 += v[j]
            w2 += v[j] * v[j]
    return c, w1, w2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--traces", type=int, default=8)
    ap.add_argument("--run", type=int, default=0, help="rec_map_frames (0: the default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "network_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.traces, a.frames, a.run)
        return
    F = a.frames
    rec = {"size": 1024, "frames": F, "calls_per_profiled_run": CALLS, "by_traces": {}, "by_run_length": {"traces": RUN_TRACES}}
    for L in TRACES:
        one = profiled(L, F)
        rec["by_traces"][str(L)] = one
        print("L %d: %s" % (L, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})), flush=True)
    for run in RUNS:                                  # the run length decides how many atomics meet in `c`
        one = profiled(RUN_TRACES, F, run)
        one.update(runs=-(-F // run))
        rec["by_run_length"][str(run)] = one
        print("run %d: %s" % (run, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})), flush=True)
    from demix_cost import record                     # (the profiled runs are over: this process opens the GPU only now)
    kf, b, pts = record(F)
    rd = kf.state.renderer
    m = b.tri_of_pixel >= 0
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    fs = ((((bw + 3) // 4 * 4) * bh + 15) // 16) * 16
    rec.update(map_pixels=int(m.sum()), box=[bw, bh], frame_bytes=fs, rec_map_frames=64)
    # the arithmetic to check the times against: the record is read once per group of 8 traces; the atomics write
    # 8 bytes per (trace, map pixel, run), and w1, w2 once more per run
    runs = -(-F // 64)
    for run in RUNS:
        one = rec["by_run_length"][str(run)]
        one.update(atomics=int(m.sum()) * one["runs"] * (RUN_TRACES + 2))
    for L in TRACES:
        one = rec["by_traces"][str(L)]
        groups = -(-L // 8)
        one.update(groups=groups, record_bytes_read=groups * F * fs, atomic_bytes=8 * int(m.sum()) * runs * (L + 2))
        if one.get(KERNEL + "_ms"):
            one["record_bytes_per_s"] = one["record_bytes_read"] / (one[KERNEL + "_ms"] * 1e-3)
            one["multiply_adds_per_s"] = groups * F * (fs // 4) * 32 / (one[KERNEL + "_ms"] * 1e-3)
        q = traces(F, L)
        rd.body_rec_trace_maps(q)
        t0 = time.perf_counter()
        got = rd.body_rec_trace_maps(q)
        one["call_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        if L == HOST_TRACES:
            box = (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1)
            t0 = time.perf_counter()
            c, w1, w2 = host_maps(rd, q, box)
            one["host_fetch_and_product_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            one["host_over_device_call"] = one["host_fetch_and_product_wall_ms"] / one["call_wall_ms"]
            r0, r1, c0, c1 = box
            one["host_equals_device"] = bool(np.array_equal(c, got["c"][:, r0:r1, c0:c1]) and
                                             np.array_equal(w1.astype(np.uint64), got["w1"][r0:r1, c0:c1]) and
                                             np.array_equal(w2.astype(np.uint64), got["w2"][r0:r1, c0:c1]))
        del got
    rd.body_rec_end()
    kf.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
