#!/usr/bin/env python
"""The record behind the bar of tests/test_smooth_precision_gpu.py: every case of tests/smooth_cases.py's table on the
device, one line each -- N, the record (prior, measurement weight h, eps_F, model), the largest kappa_2 over the steps of
Pp scaled to a unit diagonal, the extended-precision reference's own uncertainty, the error of binary64 numpy
(tests/smooth_ref.smooth) and of the device against that reference (mean correction: position half, velocity half;
covariance -- the largest over the frames), the ratio e_device / max(e_numpy, u kappa_2), which the test holds to at
most 8 per frame, and hm_smooth_prior's error as a fraction of its componentwise bar.

    python tools/smooth_precision_table.py [--sizes 5,8,...] [-o profiles/smooth_precision.md]

Needs a GPU.  Markdown on stdout (or to -o), the largest ratio per measure stated at the top."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import dense_ref as dr  # noqa: E402
import smooth_cases as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default=",".join(str(n) for n in sc.SIZES))
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    if not dr.available():
        sys.exit(dr.SKIP_REASON)
    rows, worst, worst_unc, worst_prior = [], [(0.0, None)] * 3, 0.0, (0.0, None, 0)
    for N in (int(s) for s in a.sizes.split(",")):
        dev = dr.Device(N)
        for c in sc.cases_of(N):
            r = sc.reference(c)
            got = sc.run_on_device(dev, c)
            e_dev = sc.device_errors(c, got)
            e_prior, cp = sc.prior_errors(c, got)
            ratio = (e_dev / r["base"]).max(axis=0)              # per frame against that frame's bar, the largest
            for i in range(3):
                if ratio[i] > worst[i][0]:
                    worst[i] = (ratio[i], sc.label(c))
            worst_unc = max(worst_unc, (r["unc"] / r["bound"]).max())
            pr = max(e[0] for e in e_prior)
            if pr > worst_prior[0]:
                worst_prior = (pr, sc.label(c), cp)
            fmt = lambda v: " / ".join("%.1e" % e for e in v.max(axis=0))  # noqa: E731
            rows.append("| %d | %d | %s | %g | %g | %s | %.2e | %s | %s | %s | %s | %.2f |" % (
                N, 4 * N, c.prior, c.h, c.eps_F, "springs" if c.springs else "constant velocity", r["ref"]["kappa"],
                fmt(r["unc"]), fmt(r["e_numpy"]), fmt(e_dev), " / ".join("%.2f" % v for v in ratio), pr))
            print(rows[-1], file=sys.stderr, flush=True)
        dev.R.close()
    head = ["# RTS smoother: the device against the extended-precision reference", "",
            "Largest ratio e_device / max(e_numpy, u kappa_2) per measure; the test's bar is %g:" % dr.BOUND_FACTOR, ""]
    head += ["- %s: **%.2f** (%s)" % (what, w[0], w[1]) for what, w in zip(sc.WHAT, worst)]
    head += ["", "hm_smooth_prior against its componentwise bar c_p u (|F| |P| |F|^T + Weps), c_p = 2 d_max + 11, |F| spring by "
             "spring (tests/smooth_cases.prior_bound): at most "
             "**%.2f** of it (%s, c_p = %d)." % worst_prior, "",
             "Tracks of %d frames.  Errors as mean positions / mean velocities / covariance in the measures of "
             "tests/smooth_ref.py (the correction xs_k - x_k whitened by sqrt(diag Ps_k); Ps_k scaled to a unit diagonal), "
             "the largest over the frames; the ratio is taken per frame; u = 2^-53.  The reference's own uncertainty (raw "
             "against refined) is at most %.1e of the bar over these cases." % (sc.K, worst_unc), "",
             "| N | 4N | prior | h | eps_F | model | kappa_2 | reference's uncertainty | e_numpy | e_device | ratio | prior / bar |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    text = "\n".join(head + rows) + "\n"
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
