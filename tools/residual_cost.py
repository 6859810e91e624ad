#!/usr/bin/env python
"""What the residual video of the demixed model costs at 1024^2 with the bench's 201-vertex mesh on a record of 2 000
frames with 32 cells as 16 pairs.

  python tools/residual_cost.py [--out profiles/residual_cost.json]
  python tools/residual_cost.py --kernels-only --run N                    (what the profiler runs)

For each of four run lengths (hm_ctx_tune "rec_res_frames") the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace
--stats --output-format csv -- python tools/residual_cost.py --kernels-only --run N` (a run of its own, no counters with
it; the first run that fails ends the tool): one hm_body_rec_residual_stats_add over the whole record, with a model made
up for the purpose (Gaussian shapes in the 17 x 17 windows of the 32 planted cells, four layers, random traces: the
kernel's work does not depend on the values).  From its kernel_stats.csv: the time of k_rec_residual per launch, per
frame and per call, and of k_rec_paste and k_body_stats_add, beside the bytes the arithmetic of DESIGN.md section 15
predicts and k_rec_running's time per frame on the same record (profiles/detrend_cost.json).  Then, without the
profiler: the wall time of one such call, and of a whole residual.find_more from the 16 pair leaders to 32 points, split into the time inside the renderer's calls (each ends in a device synchronise) and the rest, on the host.
The video and the record are those of tools/demix_cost.py.  The result is one JSON file (default
profiles/residual_cost.json).
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
KERNELS = ("k_rec_residual", "k_rec_paste", "k_body_stats_add")
FRAMES = 2000
RUNS = (4, 8, 16, 64)
SCRATCH = 16 << 20


def made_up_model(pts, frames, shape):
    from hydra_mi import cellview, roi
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[-8:9, -8:9]
    a_q = np.array([np.rint(65535.0 * np.exp(-(xx * xx + yy * yy) / (2.0 * s * s))) for s in rng.uniform(1.5, 2.5, len(pts))])
    a_q = np.where(a_q >= 0.25 * 65535.0, a_q, 0).astype(np.uint16)
    lab, wt, _ = cellview.layers_from_shapes(a_q, roi.seeds_of(pts), 8, shape, 4)
    tr = rng.integers(-50 * 256, 50 * 256, (frames, len(pts))).astype(np.int32)
    return lab, wt, tr


def kernels_only(run, frames):
    from demix_cost import record
    kf, b, pts = record(frames)
    rd = kf.state.renderer
    if run:
        rd.tune("rec_res_frames", run)
    lab, wt, tr = made_up_model(pts, frames, (b.H, b.W))
    rd.body_stats_begin()
    rd.body_rec_residual_stats_add(lab, wt, tr, None, 64)
    rd.body_stats_end()
    rd.body_rec_end()
    kf.close()


def profiled(run, frames):
    one = {}
    with tempfile.TemporaryDirectory() as tmp:
        tail = ["--kernels-only", "--run", str(run), "--frames", str(frames)]
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, os.path.abspath(__file__)] + tail
        one["kernel_stats_from"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/residual_cost.py " + " ".join(tail)
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


class Clock:
    """the wall time spent inside the renderer's body_* calls (each returns after a device synchronise)"""

    def __init__(self, rd):
        self.inside, self.calls = 0.0, 0
        for name in dir(rd):
            if name.startswith(("body_rec_", "body_stats_")):
                setattr(rd, name, self._timed(getattr(rd, name)))

    def _timed(self, fn):
        def call(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.inside += time.perf_counter() - t0
                self.calls += 1
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--run", type=int, default=0, help="rec_res_frames (0: the default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.run, a.frames)
        return
    F = a.frames
    rec = {"size": 1024, "frames": F, "cells": 32, "layers": 4, "stats_add_by_run_length": {}}
    for run in RUNS:
        one = profiled(run, F)
        if "k_rec_residual_total_ms" in one:
            one["k_rec_residual_us_per_frame"] = 1e3 * one["k_rec_residual_total_ms"] / F
        rec["stats_add_by_run_length"][str(run)] = one
        print("run %d: %s" % (run, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})), flush=True)
    from demix_cost import record                     # (the profiled runs are over: this process opens the GPU only now)
    from hydra_mi import residual
    kf, b, pts = record(F)
    rd = kf.state.renderer
    m = b.tri_of_pixel >= 0
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    fs = ((((bw + 3) // 4 * 4) * bh + 15) // 16) * 16
    per = max(1, min(F, SCRATCH // fs))
    lab, wt, tr = made_up_model(pts, F, m.shape)
    yc, xc = np.nonzero((lab >= 0).any(0) & m)         # segments of 64 dwords of the box frame that hold a pixel with a cell
    with_cells = int(np.unique(((yc - rows[0]) * ((bw + 3) // 4 * 4) + xc - cols[0]) // 256).size)
    rec.update(map_pixels=int(m.sum()), box=[bw, bh], frame_bytes=fs, frames_per_scratch=per, segments=-(-(fs // 4) // 64),
               segments_with_cells=with_cells)
    try:
        ref = json.load(open(os.path.join(ROOT, "profiles", "detrend_cost.json")))
        rec["k_rec_running_us_per_frame"] = {k: v.get("k_rec_running_us_per_frame") for k, v in ref["stats_add_by_run_length"].items()}
    except (OSError, KeyError, ValueError):
        rec["k_rec_running_us_per_frame"] = None
    # the arithmetic to check the times against: one record byte read and one written per box pixel and frame; per run a
    # segment reads its live bytes (1 per pixel) and, where it has cells, 4 bytes per pixel and layer it needs
    for run in RUNS:
        runs = sum(-(-min(per, F - k) // run) for k in range(0, F, per))
        one = rec["stats_add_by_run_length"][str(run)]
        one.update(runs=runs, bytes_read=F * fs + runs * fs, bytes_written=F * fs, layer_bytes_at_most=runs * with_cells * 256 * 4 * 4)
        if one.get("k_rec_residual_total_ms"):
            one["bytes_per_s"] = (one["bytes_read"] + one["bytes_written"]) / (one["k_rec_residual_total_ms"] * 1e-3)
    rd.body_stats_begin()
    rd.body_rec_residual_stats_add(lab, wt, tr, None, 64)
    t0 = time.perf_counter()
    rd.body_rec_residual_stats_add(lab, wt, tr, None, 64)
    rec["stats_add_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    # a whole find_more, 16 points -> 32: from the 16 pair leaders, at most 16 more.  This video has no noise outside the
    # cells' windows, so its corr image is 1 there and its scores are no guide to min_score: the run measures the work
    # (two demix.extract, two residual statistics, 16 ROI checks); the recovery is tests/test_residual_cpu.py's
    first, min_score = pts[0::2], 0.8
    clock = Clock(rd)
    near = lambda p: int((np.sqrt(((np.floor(p)[:, None, :] + 0.5 - pts[None]) ** 2).sum(2)).min(0) <= 2.0).sum())
    rec["find_more"] = {"given_points": int(len(first)), "min_score": min_score, "max_new": 16,
                        "planted_within_2px_before": near(first),
                        "note": "this video has no noise outside the cells' windows, so its corr image is 1 there and its "
                                "scores are no guide to min_score; planted_within_2px_* count the planted cells with a "
                                "point within 2 px; the work of 16 -> 32 points is what is timed"}
    t0 = time.perf_counter()
    try:
        more = residual.find_more(b, first, min_score, max_new=16)
        wall = time.perf_counter() - t0
        rec["find_more"].update(points=int(len(more["points"])), planted_within_2px_after=near(more["points"]),
                                accepted=more["accepted"], ended=more["ended"], clipped=[int(c) for c in more["clipped"]],
                                refused=len(more["refused"]), wall_s=wall, inside_renderer_calls_s=clock.inside,
                                renderer_calls=clock.calls, host_s=wall - clock.inside)
    except (ValueError, np.linalg.LinAlgError) as ex:          # (the search gave up on this video: said, not hidden)
        rec["find_more"].update(error=repr(ex), wall_s=time.perf_counter() - t0)
    rd.body_stats_end()
    rd.body_rec_end()
    kf.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
