#!/usr/bin/env python
"""The record behind the bar of tests/test_dense_precision_gpu.py: every case of tests/dense_ref.py's table on the
device, one line each -- N, the prior, kappa_2 of the information matrix scaled to a unit diagonal, the error of
binary64 LAPACK and of the device against the extended-precision reference (step: position half, velocity half;
covariance), and the ratio e_device / max(e_lapack, u kappa_2), which the test holds to at most 8.

    python tools/dense_precision_table.py [--chol-flow 0|1] [--sizes 5,8,...] [-o profiles/dense_precision.md]

Needs a GPU.  Markdown on stdout (or to -o), the largest ratio stated at the top."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dense_ref as dr  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--chol-flow", type=int, default=1, choices=(0, 1))
    ap.add_argument("--sizes", default=",".join(str(n) for n in dr.SIZES))
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    if not dr.available():
        sys.exit(dr.SKIP_REASON)
    sizes = [int(s) for s in a.sizes.split(",")]
    rows, worst, worst_unc = [], (0.0, None), 0.0
    for N in sizes:
        dev = dr.Device(N)
        dev.R.tune("chol_flow", a.chol_flow)
        for n_, name, moved in dr.cases():
            if n_ != N:
                continue
            ref, got, e_l, e_d = dr.measured_case(dev, name, moved)
            base = [max(e, dr.U * ref["kappa"]) for e in e_l]
            ratio = [d / b for d, b in zip(e_d, base)]
            worst_unc = max([worst_unc] + [u / (dr.BOUND_FACTOR * b) for u, b in zip(dr.uncertainty(ref), base)])
            if max(ratio) > worst[0]:
                worst = (max(ratio), "N = %d, %s%s" % (N, name, ", X0 moved" if moved else ""))
            rows.append("| %d | %d | %s%s | %.2e | %s | %s | %s |" % (
                N, 4 * N, name, " (X0 moved)" if moved else "", ref["kappa"], " / ".join("%.1e" % e for e in e_l),
                " / ".join("%.1e" % e for e in e_d), " / ".join("%.2f" % r for r in ratio)))
            print(rows[-1], file=sys.stderr, flush=True)
        dev.R.close()
    head = ["# Dense update: the device against the extended-precision reference", "",
            "Largest ratio e_device / max(e_lapack, u kappa_2(A^)): **%.2f** (%s); the test's bar is %g." % (
                worst[0], worst[1], dr.BOUND_FACTOR),
            "", "chol_flow = %d.  Errors as step positions / step velocities / covariance, in the measures of "
            "tests/dense_ref.py (A scaled to a unit diagonal); u = 2^-53.  The reference's own uncertainty (raw against "
            "refined) is at most %.1e of the bar over these cases." % (a.chol_flow, worst_unc), "",
            "| N | 4N | prior | kappa_2(A^) | e_lapack | e_device | ratio |", "|---|---|---|---|---|---|---|"]
    text = "\n".join(head + rows) + "\n"
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
