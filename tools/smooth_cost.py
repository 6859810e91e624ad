#!/usr/bin/env python
"""What the RTS smoother (hydra_mi.smooth) costs at 1024^2 with the bench's 201-vertex mesh.

  python tools/smooth_cost.py [--frames 64] [--kernel-stats CSV] [--out profiles/smooth_cost.json]

1. The 64-frame 1024^2 pipeline (bench.py's video) without a record and with one (FlowEKFPipeline.run(smoother=)),
   alternated after one run that is not recorded: frames/s of each.
2. The backward pass over the record of one more such run: ms per backward step without covariances (means only; the
   second of two runs) and with them (one run: it consumes the record).
3. The kernel times come from a run of this tool under
   `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/smooth_cost.py --frames 16` (KERNEL_CMD);
   --kernel-stats names the kernel_stats.csv it wrote, whose rows of the smoother's kernels go into the record with the
   achieved f64 rate of the products (2 n^3 flops each, n = 4N; about half where an operand is triangular) against the
   chip's f64 matrix peak.
The record is one JSON file (default profiles/smooth_cost.json).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

KERNEL_CMD = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/smooth_cost.py --frames 16"
F64_MATRIX_PEAK_TFLOPS = 78.6        # MI355X, f64 matrix (v_mfma_f64_16x16x4_f64), vendor figure
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_sm_gemm", "k_fw_rows", "k_pft_cols", "k_chol_flow", "k_flow_fill", "k_ttt", "k_sm_trmv", "k_sm_mvt",
           "k_sm_sub", "k_sm_diag", "k_sm_check")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_cost.json"))
    a = ap.parse_args()
    import hydra_mi  # noqa: F401
    from hydra_mi import kalman, mesh
    from hydra_mi.pipeline import FlowEKFPipeline
    from hydra_mi.smooth import RTSSmoother, record_bytes
    import bench

    n = 1024
    video = bench.BenchVideo(n, a.frames + 1, 0)
    c, r = video.centre, video.radius

    def new_filter():
        dm = mesh.disk_mesh(c[0], c[1], r - 1.0, 0.047 * n)
        return dm, kalman.IteratedMSKalmanFilter(dm, video.frame_at(0)[0], np.zeros((n, n, 2), np.float32), True)

    def run(with_record, keep=False):
        dm, kf = new_filter()
        pipe = FlowEKFPipeline(kf, video)
        sm = RTSSmoother(kf, a.frames) if with_record else None
        t0 = time.perf_counter()
        pipe.run(smoother=sm)
        dt = time.perf_counter() - t0
        pipe.close()
        if keep:
            return dm, kf, sm, a.frames / dt
        if sm is not None:
            sm.close()
        kf.close()
        return a.frames / dt

    rec = {"size": n, "frames": a.frames}
    run(False)                                  # (first-use costs of the process: not recorded)
    runs = []
    for mode in (False, True, False, True, False, True):
        fps = run(mode)
        runs.append({"record": mode, "frames_per_s": fps})
        print("pipeline %s record: %.1f frames/s" % ("with" if mode else "without", fps))
    rec["pipeline_runs"] = runs
    off = [x["frames_per_s"] for x in runs if not x["record"]]
    on = [x["frames_per_s"] for x in runs if x["record"]]
    rec["on_over_off"] = float(np.mean(on) / np.mean(off))

    # the backward pass over the record of one more pipeline run
    dm, kf, sm, _ = run(True, keep=True)
    N = dm.size()
    rec["vertices"] = int(N)
    rec["record_bytes"] = record_bytes(N, a.frames)
    rec["copy_bytes_per_frame"] = (4 * N) ** 2 * 8 + 4 * N * 8
    K = len(sm)
    for want in (False, False, True):           # (a run with covariances consumes the record: it goes last)
        t0 = time.perf_counter()
        sm.run(covariances=want)
        dt = time.perf_counter() - t0
        key = "backward_ms_per_frame_" + ("cov" if want else "mean")
        rec[key] = 1e3 * dt / max(K - 1, 1)      # (of the two means-only runs the second counts)
        print("%s: %.3f ms" % (key, rec[key]))
    sm.close()
    kf.close()

    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rec["kernel_stats_from"] = KERNEL_CMD
        ks = {}
        for row in csv.DictReader(open(a.kernel_stats)):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name.split("(")[0]:
                    ks[name] = {f: row[f] for f in ("Calls", "AverageNs", "MinNs", "MaxNs") if f in row}
        rec["kernels"] = ks
        n4 = 4 * N
        nb = -(-n4 // 32)
        for name, row in ks.items():
            if "k_sm_gemm" in name.split("(")[0]:
                # SM_SYM (k_sm_gemm<2>) forms the lower tiles only; SM_LN / SM_TL (<3>, <4>) skip the slabs right of
                # the triangular operand's diagonal
                flops = 2.0 * n4 ** 3 * ((nb + 1) / (2.0 * nb) if any(m in name for m in ("<2>", "<3>", "<4>")) else 1.0)
                ns = float(row["AverageNs"])
                row["tflops"] = flops / ns / 1e3
                row["of_f64_matrix_peak"] = row["tflops"] / F64_MATRIX_PEAK_TFLOPS
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
