#!/usr/bin/env python
"""What the activity waves cost at 1024^2 with the bench's 201-vertex mesh on the record of 64 frames: one
hm_body_rec_waves call with 16 triggers and the command's defaults (bins of 5 x 5, pre 8, lead 8, post 24, min_rise 8, a
node every 8 pixels fitted within 6), on the frames as recorded (kind 0) and on their dF/F bytes (kind 3: half = 20,
q = 10, floor 16, gain 255).

  python tools/waves_cost.py [--out profiles/waves_cost.json]
  python tools/waves_cost.py --kernels-only --kind K               (what the profiler runs)

For each kind the tool starts `timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/waves_cost.py --kernels-only --kind K` (a run of its own, no counters with it; the first run that fails ends the
tool): one call with every output asked for, and one hm_body_rec_trace_maps call with 8 traces, the yardstick: another
full pass over the same record in the same session (tools/network_cost.py).  From its kernel_stats.csv: the microseconds
of k_rec_wv_lat, k_rec_wv_sums, k_rec_wv_fit, k_rec_wv_mask, k_rec_wv_nbin, k_rec_running and k_rec_trace_maps.  Then,
without the profiler, the wall time of the call.  The bytes the rule must read are E x frame reads x box frame bytes: a
baseline frame is read once and a search frame twice (the walk is done twice), so an event reads
pre + 2 (lead + post + 1) frames; the effective bytes/s are those over the time of k_rec_wv_lat, beside the record bytes
per second of k_rec_trace_maps.  The video and the record are those of tools/demix_cost.py.  The result is one JSON file
(default profiles/waves_cost.json).
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
KERNELS = ("k_rec_wv_lat", "k_rec_wv_sums", "k_rec_wv_fit", "k_rec_wv_mask", "k_rec_wv_nbin", "k_rec_running", "k_rec_trace_maps")
FRAMES, EVENTS, TRACES = 64, 16, 8
PAR = dict(b=2, pre=8, lead=8, post=24, min_rise=8, step=8, Rf=6)
DET = dict(half=20, q=10, floor=16, gain=255)


def triggers():
    first, last = PAR["lead"] + PAR["pre"], FRAMES - 1 - PAR["post"]
    return np.linspace(first, last, EVENTS).astype(np.int32)


def traces():
    return np.random.default_rng(1).integers(-32767, 32768, (FRAMES, TRACES)).astype(np.int32)


def kernels_only(kind):
    from demix_cost import record
    kf, b, _ = record(FRAMES)
    rd = kf.state.renderer
    rd.body_rec_waves(triggers(), kind, **DET, **PAR)
    rd.body_rec_trace_maps(traces())
    rd.body_rec_end()
    kf.close()


def profiled(kind):
    one = {}
    with tempfile.TemporaryDirectory() as tmp:
        tail = ["--kernels-only", "--kind", str(kind)]
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, os.path.abspath(__file__)] + tail
        one["kernel_stats_from"] = "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/waves_cost.py " + " ".join(tail)
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
                    one[kernel + "_total_us"] = float(row["AverageNs"]) * int(row["Calls"]) / 1e3
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waves_cost.json"))
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a.kind)
        return
    rec = {"size": 1024, "frames": FRAMES, "events": EVENTS, "triggers": triggers().tolist(), "parameters": PAR, "dff": DET, "kinds": {}}
    for kind in (0, 3):
        rec["kinds"][str(kind)] = profiled(kind)
    from demix_cost import record                     # (the profiled runs are over: this process opens the GPU only now)
    kf, b, _ = record(FRAMES)
    rd = kf.state.renderer
    m = b.tri_of_pixel >= 0
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    bw, bh = int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1
    fs = ((((bw + 3) // 4 * 4) * bh + 15) // 16) * 16
    reads = PAR["pre"] + 2 * (PAR["lead"] + PAR["post"] + 1)
    rec.update(map_pixels=int(m.sum()), box=[bw, bh], frame_bytes=fs, frame_reads_per_event=reads, passes_over_the_search_frames=2,
               bytes_the_rule_reads=EVENTS * reads * fs, yardstick_record_bytes=FRAMES * fs)
    for kind in (0, 3):
        one = rec["kinds"][str(kind)]
        if one.get("k_rec_wv_lat_total_us"):
            one["latency_kernel_bytes_per_s"] = rec["bytes_the_rule_reads"] / (one["k_rec_wv_lat_total_us"] * 1e-6)
        if one.get("k_rec_trace_maps_total_us"):
            one["trace_maps_record_bytes_per_s"] = rec["yardstick_record_bytes"] / (one["k_rec_trace_maps_total_us"] * 1e-6)
        call = lambda: rd.body_rec_waves(triggers(), kind, **DET, **PAR)
        call()
        t0 = time.perf_counter()
        got = call()
        one["call_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        rd.body_rec_waves(triggers(), kind, want=("cnt", "sum_lat", "sum_lat2", "fit"), **DET, **PAR)
        one["call_wall_ms_without_the_planes_per_event"] = 1e3 * (time.perf_counter() - t0)
        one["valid_share"] = float((got["why"] <= 1).sum()) / float(EVENTS * max(1, int(m.sum())))
        print("kind %d: %s" % (kind, json.dumps(one)), flush=True)
    rd.body_rec_end()
    kf.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
