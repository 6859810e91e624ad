#!/usr/bin/env python
"""What the Gram matrix of hydra_mi.pca costs at 1024^2 with the bench's 201-vertex mesh on records of 300 and 2048 frames.

  python tools/pca_cost.py [--out profiles/pca_cost.json] [--keep DIR]
  python tools/pca_cost.py --kernels-only --frames F                      (what the profiler runs)

Per record length the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/pca_cost.py --kernels-only --frames F` (a run of its own, no counters with it; the first run that fails ends the
tool): for every run length of RUNS (hm_ctx_tune "rec_gram_bytes": the shorter the run, the more waves and the more 64-bit
atomics) three hm_body_rec_gram calls over the whole record, in that order.  From its kernel_trace.csv: the time of
k_rec_gram and of k_rec_gram_fix per launch and run length, beside the multiply-adds and the bytes the kernel asks the caches
for and the rates that follow.  Then, without the profiler: the wall time of one call at the default run length, the copy of
G included, and the same matrix made the only way there was before -- body_rec_fetch plus a NumPy product of the box crop,
in float64 BLAS (exact here: 65025 x box bytes < 2^53) at both lengths and in int64 at 300 frames -- with
host_equals_device for each -- and what follows the call in pca.components (the centring and numpy.linalg.eigh).  The video and the record are those of tools/demix_cost.py.  The result is one JSON file
(default profiles/pca_cost.json); --keep copies the profiler's csv files to DIR.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
KERNELS = ("k_rec_gram", "k_rec_gram_fix")
FRAMES = (300, 2048)
RUNS = (4096, 16384, 32768, 65536, 131008)
CALLS = 3
INT64_FRAMES = 300


def kernels_only(frames):
    from demix_cost import record
    kf, b, pts = record(frames)
    rd = kf.state.renderer
    for run in RUNS:
        rd.tune("rec_gram_bytes", run)
        for _ in range(CALLS):
            rd.body_rec_gram()
    rd.body_rec_end()
    kf.close()


def _col(row, *words):
    for k in row:
        if all(w in k.lower() for w in words):
            return k
    raise KeyError("no column with %r among %r" % (words, list(row)))


def profiled(frames, keep):
    one = {}
    with tempfile.TemporaryDirectory() as tmp:
        tail = ["--kernels-only", "--frames", str(frames)]
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, os.path.abspath(__file__)] + tail
        src = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/pca_cost.py " + " ".join(tail)
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                       # (nothing more is started on the GPU after a run that failed)
            raise RuntimeError("the profiled run failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
        found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if keep:
            os.makedirs(keep, exist_ok=True)
            for fn in glob.glob(os.path.join(tmp, "**", "*.csv"), recursive=True):
                shutil.copy(fn, os.path.join(keep, "f%d_%s" % (frames, os.path.basename(fn))))
        if len(found) != 1:
            raise RuntimeError("expected one kernel_trace.csv under the profiler's directory, found %r" % found)
        rows = list(csv.DictReader(open(found[0])))
        name, t0, t1 = _col(rows[0], "kernel", "name"), _col(rows[0], "start"), _col(rows[0], "end")
        for kernel in KERNELS:
            mine = sorted((int(r[t0]), int(r[t1])) for r in rows if r[name].startswith(kernel + "("))
            if len(mine) != CALLS * len(RUNS):
                raise RuntimeError("%d launches of %s, expected %d" % (len(mine), kernel, CALLS * len(RUNS)))
            for i, run in enumerate(RUNS):            # (the launches in time order: CALLS per run length)
                ns = [b - a for a, b in mine[i * CALLS:(i + 1) * CALLS]]
                one.setdefault(str(run), {}).update({kernel + "_ms": sum(ns) / len(ns) / 1e6, kernel + "_min_ms": min(ns) / 1e6})
    return src, one


def box_frames(rd, F, box):
    r0, r1, c0, c1 = box
    X = np.empty((F, (r1 - r0) * (c1 - c0)), np.uint8)
    for k0 in range(0, F, 50):
        m = min(50, F - k0)
        X[k0:k0 + m] = rd.body_rec_fetch(k0, m)[:, r0:r1, c0:c1].reshape(m, -1)
    return X


def host_gram(rd, F, box, dtype):
    """the same matrix from the fetched frames: the product of the box crop in `dtype`, a block of pixels at a time"""
    X = box_frames(rd, F, box)
    G = np.zeros((F, F), dtype)
    step = 1 << 15
    for p0 in range(0, X.shape[1], step):
        Xb = X[:, p0:p0 + step].astype(dtype)
        G += Xb @ Xb.T
    return G.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--keep", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.frames)
        return
    rec = {"size": 1024, "calls_per_run_length": CALLS, "by_frames": {}}
    for F in FRAMES:
        src, by_run = profiled(F, a.keep)
        rec["by_frames"][str(F)] = {"kernel_trace_from": src, "by_run_bytes": by_run}
        print("F %d: %s" % (F, json.dumps(rec["by_frames"][str(F)])), flush=True)
    from demix_cost import record                     # (the profiled runs are over: this process opens the GPU only now)
    for F in FRAMES:
        one = rec["by_frames"][str(F)]
        kf, b, pts = record(F)
        rd = kf.state.renderer
        m = b.tri_of_pixel >= 0
        rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
        nb = (bw + 3) // 4 * 4 * bh
        rec.update(map_pixels=int(m.sum()), box=[bw, bh], box_bytes=nb)
        # the arithmetic to check the times against: a workgroup owns a pair of blocks of 128 frames; per 64 bytes its four
        # waves do 16 MFMAs of 16 x 16 x 64 each (on the diagonal two of them 4 more for the sums), and per byte column it asks
        # the caches for its 256 frames once (128 on the diagonal)
        nbk = -(-F // 128)
        pairs = nbk * (nbk + 1) // 2
        steps = -(-nb // 64)
        one.update(blocks=nbk, pairs=pairs, multiply_adds=(64 * pairs + 8 * nbk) * steps * 16 * 16 * 64,
                   bytes_asked=(256 * (pairs - nbk) + 128 * nbk) * nb, record_bytes=F * nb)
        for run, t in one["by_run_bytes"].items():
            runs = -(-nb // int(run))
            t.update(runs=runs, waves=4 * pairs * runs, atomics=runs * (2 * 16384 * (pairs - nbk) + 16384 * nbk),
                     ops_per_s=2 * one["multiply_adds"] / (t["k_rec_gram_ms"] * 1e-3),
                     bytes_asked_per_s=one["bytes_asked"] / (t["k_rec_gram_ms"] * 1e-3))
        rd.body_rec_gram()
        t0 = time.perf_counter()
        got = rd.body_rec_gram()
        one["call_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        box = (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1)
        t0 = time.perf_counter()
        G = host_gram(rd, F, box, np.float64)
        one["host_fetch_and_f64_product_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        one["host_f64_equals_device"] = bool(np.array_equal(G, got["G"]))
        one["host_f64_over_device_call"] = one["host_fetch_and_f64_product_wall_ms"] / one["call_wall_ms"]
        from hydra_mi import pca
        t0 = time.perf_counter()
        lam, U, share = pca.components(got["G"], 4)
        one["host_components_wall_ms"] = 1e3 * (time.perf_counter() - t0)      # (centre and numpy.linalg.eigh: what follows the call)
        one["share_of_4"] = [float(v) for v in share]
        if F == INT64_FRAMES:
            t0 = time.perf_counter()
            G = host_gram(rd, F, box, np.int64)
            one["host_fetch_and_int64_product_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            one["host_equals_device"] = bool(np.array_equal(G, got["G"]))
            one["host_int64_over_device_call"] = one["host_fetch_and_int64_product_wall_ms"] / one["call_wall_ms"]
        print("F %d: %s" % (F, json.dumps({k: v for k, v in one.items() if not isinstance(v, dict)})), flush=True)
        del got, G
        rd.body_rec_end()
        kf.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
