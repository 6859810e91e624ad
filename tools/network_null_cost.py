#!/usr/bin/env python
"""What the surrogate reduction of hydra_mi.network.map_null costs at 1024^2 with the bench's 201-vertex mesh on a record
of 300 frames.

  python tools/network_null_cost.py [--out profiles/network_null_cost.json]
  python tools/network_null_cost.py --kernels-only --columns L --run R        (what the profiler runs)

For L = 129, 513 and 1025 columns (the trace and 128, 512, 1024 surrogates), each at runs of 64 and 256 frames (hm_ctx_tune
"rec_null_frames"), the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/network_null_cost.py --kernels-only --columns L --run R` (a run of its own per row, no counters with it; the first
run that fails ends the tool): three hm_body_rec_trace_null calls over the whole record with random columns (the kernel's
work does not depend on the values).  From its kernel_stats.csv: the time of k_rec_trace_null per launch, and of the
k_rec_trace_maps launch for column 0 that goes before it, beside the bytes of the record the kernel reads (once per group
of 8 columns) and its multiply-adds, and the rates that follow.  Then, without the profiler: the wall time of one such
call, copies included, and for L = 129 the same numbers made the only way there was before -- hm_body_rec_trace_maps in
calls of 128 columns, every 8-byte plane copied out and reduced in NumPy on the box of the map -- and the ratio of the
two; the larger L are not run that way (the planes of a call are 1 GB on the host; the time grows with L).  The video
and the record are those of tools/demix_cost.py.  The result is one JSON file (default profiles/network_null_cost.json).
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
KERNELS = ("k_rec_trace_null", "k_rec_trace_maps")
FRAMES = 300
COLUMNS = (129, 513, 1025)
RUNS = (64, 256)
OLD_COLUMNS = 129
CALLS = 3


def columns(frames, L):
    q = np.random.default_rng(1).integers(-32767, 32768, (frames, L)).astype(np.int32)
    q64 = q.astype(np.int64)
    return q, (frames * (q64 * q64).sum(0) - q64.sum(0) ** 2).astype(np.float64)


def kernels_only(L, frames, run):
    from demix_cost import record
    kf, b, pts = record(frames)
    rd = kf.state.renderer
    rd.tune("rec_null_frames", run)
    q, vb = columns(frames, L)
    for _ in range(CALLS):
        rd.body_rec_trace_null(q, vb)
    rd.body_rec_end()
    kf.close()


def profiled(L, frames, run):
    one = {}
    with tempfile.TemporaryDirectory() as tmp:
        tail = ["--kernels-only", "--columns", str(L), "--frames", str(frames), "--run", str(run)]
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, os.path.abspath(__file__)] + tail
        one["kernel_stats_from"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/network_null_cost.py " + " ".join(tail)
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
                    one[kernel + "_ms"] = float(row["AverageNs"]) / 1e6
                    one[kernel + "_min_ms"] = float(row["MinNs"]) / 1e6
    return one


def old_way(rd, q, vb, m, box):
    """tmax, tmin, ge, le from hm_body_rec_trace_maps in calls of 128 columns, reduced in NumPy on the box of the map"""
    r0, r1, c0, c1 = box
    F, L = q.shape
    mb = m[r0:r1, c0:c1]
    u1 = q.astype(np.int64).sum(0)
    w = rd.body_rec_trace_maps(q[:, :1].copy(), want=("c", "w1", "w2"))
    w1 = w["w1"][r0:r1, c0:c1].astype(np.int64)[mb]
    va = (F * w["w2"][r0:r1, c0:c1].astype(np.int64)[mb] - w1 * w1).astype(np.float64)
    num0 = F * w["c"][0, r0:r1, c0:c1][mb] - w1 * u1[0]
    tmax, tmin = np.empty(L), np.empty(L)
    ge, le = np.zeros(len(w1), np.int64), np.zeros(len(w1), np.int64)
    for s0 in range(0, L, 128):
        c = rd.body_rec_trace_maps(np.ascontiguousarray(q[:, s0:s0 + 128]), want=("c",))["c"]
        for j in range(c.shape[0]):
            s = s0 + j
            num = F * c[j, r0:r1, c0:c1][mb] - w1 * u1[s]
            with np.errstate(invalid="ignore", divide="ignore"):
                rho = np.where((va == 0.0) | (vb[s] == 0.0), 0.0, num.astype(np.float64) / np.sqrt(va * vb[s]))
            tmax[s], tmin[s] = rho.max(), rho.min()
            if s >= 1:
                ge += num >= num0
                le += num <= num0
        del c
    out = dict(tmax=tmax, tmin=tmin, ge=np.zeros(m.shape, np.uint32), le=np.zeros(m.shape, np.uint32))
    out["ge"][r0:r1, c0:c1][mb] = ge
    out["le"][r0:r1, c0:c1][mb] = le
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--columns", type=int, default=COLUMNS[0])
    ap.add_argument("--run", type=int, default=256, help="rec_null_frames")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "network_null_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.columns, a.frames, a.run)
        return
    F = a.frames
    rec = {"size": 1024, "frames": F, "calls_per_profiled_run": CALLS, "rows": {}}
    for L in COLUMNS:
        for run in RUNS:
            one = profiled(L, F, run)
            one.update(columns=L, rec_null_frames=run)
            rec["rows"]["%d/%d" % (L, run)] = one
            print("L %d run %d: %s" % (L, run, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})), flush=True)
    from demix_cost import record                     # (the profiled runs are over: this process opens the GPU only now)
    kf, b, pts = record(F)
    rd = kf.state.renderer
    m = b.tri_of_pixel >= 0
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    fs = ((((bw + 3) // 4 * 4) * bh + 15) // 16) * 16
    wgs = -(-(((bw + 3) // 4) * bh) // 256)
    rec.update(map_pixels=int(m.sum()), box=[bw, bh], frame_bytes=fs, workgroups_per_group=wgs)
    for L in COLUMNS:
        groups = -(-L // 8)
        q, vb = columns(F, L)
        for run in RUNS:
            one = rec["rows"]["%d/%d" % (L, run)]
            # the arithmetic to check the times against: every group of 8 columns reads the record once (1 KiB per
            # workgroup and frame) and does 4 x 8 multiply-adds per dword and frame
            one.update(groups=groups, workgroups=groups * wgs, record_bytes_read=groups * F * wgs * 1024,
                       multiply_adds=groups * F * wgs * 256 * 32)
            if one.get(KERNELS[0] + "_ms"):
                one["record_bytes_per_s"] = one["record_bytes_read"] / (one[KERNELS[0] + "_ms"] * 1e-3)
                one["multiply_adds_per_s"] = one["multiply_adds"] / (one[KERNELS[0] + "_ms"] * 1e-3)
            rd.tune("rec_null_frames", run)
            rd.body_rec_trace_null(q, vb)
            t0 = time.perf_counter()
            got = rd.body_rec_trace_null(q, vb)
            one["call_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            one["bytes_in"], one["bytes_out"] = int(q.nbytes + vb.nbytes), int(sum(v.nbytes for v in got.values()))
        if L == OLD_COLUMNS:
            box = (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1)
            t0 = time.perf_counter()
            old = old_way(rd, q, vb, m, box)
            ms = 1e3 * (time.perf_counter() - t0)
            rec["trace_maps_and_numpy"] = dict(
                columns=L, calls_of=128, wall_ms=ms, over_device_call=ms / rec["rows"]["%d/256" % L]["call_wall_ms"],
                bytes_copied_out=8 * (L + 3) * 1024 * 1024,
                equals_device=bool(all(old[k].tobytes() == got[k].tobytes() for k in ("tmax", "tmin", "ge", "le"))),
                larger_columns="not run: 513 and 1025 columns would copy 4.3 and 8.6 GB out in calls of 128")
            print("the old way, L %d: %s" % (L, json.dumps(rec["trace_maps_and_numpy"])), flush=True)
    rd.body_rec_end()
    kf.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
