#!/usr/bin/env python
"""What stabilising the kept registered video costs at 1024^2 with the bench's 201-vertex mesh, B = 16, S = 3, on records
of 64 and of 1024 frames.

  python tools/stab_cost.py [--out profiles/stab_cost.json]
  python tools/stab_cost.py --kernels-only --frames N          (what the profiler runs)

For each record length the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/stab_cost.py --kernels-only --frames N` (a run of its own, no counters with it; the first run that fails ends the
tool) and reads from its kernel_stats.csv the times of k_stab_match, k_stab_frame_sums and k_stab_shift and, of the field
mode, k_stab_field_sums and k_stab_warp; warp_over_shift is the ratio of the two kernels that rewrite the record (the same
bytes written; the warp reads four source bytes per pixel instead of one, and the field).  Then, without the profiler, the
wall time of stabilize.estimate and stabilize.apply in both modes (host arithmetic and copies included) beside
roi.extract's on the same record.  From the match kernel's time: record bytes read per second (every patch reads its window, (B + 2S)^2 / B^2 of its
own bytes) and byte products per second, F x map pixels x (2S + 1)^2 x 3 sums.  The video and the record are those of
tools/demix_cost.py.  The result is one JSON file (default profiles/stab_cost.json).
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
KERNELS = ("k_stab_match", "k_stab_frame_sums", "k_stab_shift", "k_stab_field_sums", "k_stab_warp")
B, S = 16, 3


def kernels_only(frames):
    from demix_cost import record
    kf, b, pts = record(frames)
    rd = kf.state.renderer
    npx, npy = rd.body_rec_patches(B)
    rng = np.random.default_rng(1)
    sh = rng.integers(-S, S + 1, (frames, npx * npy, 2)).astype(np.int8)
    q = rng.integers(-16 * S, 16 * S + 1, (frames, npx * npy, 2)).astype(np.int16)
    valid = (rng.random((frames, npx * npy)) < 0.6).astype(np.uint8)          # (about the share that does not fall back)
    t = rd.body_rec_fetch(0, 1)[0]
    block = min(frames, 64)
    for _ in range(3):
        for k0 in range(0, frames, block):
            rd.body_rec_match(t, B, S, k0, min(block, frames - k0))
        rd.body_rec_frame_sums(sh, B)
        rd.body_rec_shift(sh, B)
        rd.body_rec_field_sums(q, valid, B)
        rd.body_rec_warp(q, valid, B)
    rd.body_rec_end()
    kf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stab_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.frames)
        return
    rec = {"size": 1024, "B": B, "S": S, "records": {}}
    for frames in (64, 1024):
        one = {}
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
                   "--", sys.executable, os.path.abspath(__file__), "--kernels-only", "--frames", str(frames)]
            one["kernel_stats_from"] = ("rocprofv3 --kernel-trace --stats --output-format csv -- python tools/stab_cost.py "
                                        "--kernels-only --frames %d" % frames)
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:                   # (nothing more is started on the GPU after a run that failed)
                raise RuntimeError("the profiled run failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if len(found) != 1:
                raise RuntimeError("expected one kernel_stats.csv under the profiler's directory, found %r" % found)
            for row in csv.DictReader(open(found[0])):
                for kernel in KERNELS:
                    if row.get("Name", "").startswith(kernel + "("):
                        one[kernel] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
                        one[kernel + "_us"] = float(row["AverageNs"]) / 1e3
            if "k_stab_warp_us" in one and "k_stab_shift_us" in one:
                # (both kernels are launched once per run of frames, the same runs: the averages compare like with like)
                one["warp_over_shift"] = one["k_stab_warp_us"] / one["k_stab_shift_us"]
        rec["records"][str(frames)] = one
    from demix_cost import record                     # (the profiled runs are over: this process opens the GPU only now)
    from hydra_mi import roi, stabilize
    for frames in (64, 1024):
        one = rec["records"][str(frames)]
        kf, b, pts = record(frames)
        rd = kf.state.renderer
        m = b.tri_of_pixel >= 0
        grid = stabilize.patch_grid(m, B)
        stabilize.estimate(b, B=B, S=S)
        t0 = time.perf_counter()
        est = stabilize.estimate(b, B=B, S=S)
        one["estimate_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        roi.extract(b, pts, alpha=1.0)
        one["roi_extract_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        est_f = stabilize.estimate(b, B=B, S=S, mode="field")
        one["estimate_field_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        stabilize.apply(b, est)
        one["apply_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        stabilize.apply(b, est_f)                     # (on the shifted record: the cost does not depend on what it holds)
        one["apply_field_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        one["fallback_share"] = float(est["fallback"].mean())
        core = int(est["n_core"].sum())
        calls = -(-frames // min(frames, 64))         # (the kernel's time is per call: blocks of 64 frames in kernels_only)
        per_call = min(frames, 64)
        if "k_stab_match_us" in one:
            sec = one["k_stab_match_us"] * 1e-6
            window = (B + 2 * S) ** 2 * grid["npx"] * grid["npy"]
            one["match_frames_per_call"], one["match_calls_per_record"] = per_call, calls
            one["match_window_bytes_per_s"] = per_call * window / sec
            one["match_byte_products_per_s"] = 3.0 * per_call * core * (2 * S + 1) ** 2 / sec
        rd.body_rec_end()
        kf.close()
        print("%d frames: %s" % (frames, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
