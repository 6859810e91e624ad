#!/usr/bin/env python
"""The record behind tests/test_measure_precision_gpu.py: every case of tests/measure_exact_ref.py's table measured on
the device, one line per case and array (Hz, each channel of Hzc, the self blocks and the edge blocks of HTH) -- the
largest error / bound of the device and of the binary64 oracle against the exact reference, bound = (n + C) u M per
entry, and how many of the array's non-zero entries the suite's earlier bar, 1e-9 of the largest entry of the whole
array, held to worse than 1e-6 of their own size.  Then the split settings and the single operators on the golden case.

    python tools/measure_precision_table.py [--cases golden,hub7,...] [-o profiles/measure_precision.md]

Needs a GPU.  Markdown on stdout (or to -o), the largest ratio stated at the top."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import measure_exact_ref as mx  # noqa: E402


def _old_bar(case, sums):
    """per array of the table: entries the old bar holds to worse than 1e-6 relative / non-zero entries"""
    Hz, Hzc, HTH = sums
    N = len(case["p"])
    val = np.vectorize(lambda s: 0.0 if s is None else abs(float(s.S)), otypes=[float])
    aHz, aHzc, aHTH = val(Hz), val(Hzc), val(HTH)
    vert = (np.arange(4 * N) % (2 * N)) // 2
    own = vert[:, None] == vert[None, :]

    def count(a, top):
        return "%d / %d" % (np.count_nonzero((a > 0) & (1e-9 * top > 1e-6 * a)), np.count_nonzero(a))
    out = {"Hz": count(aHz, aHz.max())}
    for ch in range(4):
        out["Hzc " + mx.CHANNELS[ch]] = count(aHzc[:, ch], aHzc.max())
    out["HTH self"] = count(aHTH[own], aHTH.max())
    out["HTH edge"] = count(aHTH[~own], aHTH.max())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", default=",".join(mx.CASES))
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    rows, worst, over = [], (0.0, None), 0
    for name in a.cases.split(","):
        case = mx.make_case(name)
        ex, sums = mx.exact_of(case)
        dev, rep = mx.check_measure(case, mx.device_measure(case), sums)
        orc, _ = mx.check_measure(case, mx.oracle_measure(case), sums)
        over += len(rep)
        for r in rep:
            print(r, file=sys.stderr)
        old = _old_bar(case, sums)
        for k in dev:
            if dev[k] > worst[0]:
                worst = (dev[k], "%s, %s" % (name, k))
            rows.append("| %s | %d | %d x %d | %s | %.3f | %.3f | %s |" % (name, len(case["p"]), case["W"], case["H"], k, dev[k],
                                                                       orc[k], old[k]))
            print(rows[-1], file=sys.stderr, flush=True)
    split_rows = []
    for name in mx.SPLIT_CASES:
        case = mx.make_case(name)
        _, sums = mx.exact_of(case)
        for key, values in (("measure_split", mx.MEASURE_SPLITS), ("edge_split", mx.EDGE_SPLITS)):
            for v in values:
                dev, rep = mx.check_measure(case, mx.device_measure(case, {key: v}), sums)
                over += len(rep)
                k = max(dev, key=dev.get)
                if dev[k] > worst[0]:
                    worst = (dev[k], "%s, %s = %d, %s" % (name, key, v, k))
                split_rows.append("| %s | %s | %d | %.3f | %s |" % (name, key, v, dev[k], k))
                print(split_rows[-1], file=sys.stderr, flush=True)
    head = ["# Measurement sums: the device against the exact reference", "",
            "Largest error / bound of the device: **%.3f** (%s); the test's bar is 1.  %d entries beyond it." % (
                worst[0], worst[1], over), "",
            "bound = (n + C) u M per entry, u = 2^-53, C = %d (tests/measure_exact_ref.py): n the entry's non-zero terms, M "
            "their absolute mass.  `oracle` is the binary64 C twin of oracle/ekf_ref.py against the same reference.  `old "
            "bar` counts the non-zero entries of the array that 1e-9 of the largest entry of the whole array (Hz, Hzc, "
            "HTH) held to worse than 1e-6 of their own size." % mx.C, "",
            "| case | N | frame | array | device | oracle | old bar worse than 1e-6 |", "|---|---|---|---|---|---|---|"]
    head2 = ["", "The partial sums split over several workgroups, each setting against the exact reference (the largest "
             "ratio over the arrays):", "", "| case | setting | value | device | array |", "|---|---|---|---|---|"]
    text = "\n".join(head + rows + head2 + split_rows) + "\n"
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
