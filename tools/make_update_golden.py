#!/usr/bin/env python
"""The oracle's results for the cases of tests/update_cases.py -> tests/golden/update_paths.npz.

For every case oracle/ekf_ref.iekf_update is run on the CPU (its Jacobian and Hessian through the C twin
oracle/ekf_c.py, which tests/test_oracle_ekf_c.py and tests/test_update_cases_cpu.py hold to the NumPy oracle) and the
door it leaves by, its rounds, error sums, convergence figures, every iterate, the state, covariance and gains kept and
the condition numbers of the systems it solved are stored under '<case>/<key>'.

    python tools/make_update_golden.py            write the file
    python tools/make_update_golden.py --explore  print each case's figures without its reltol (never converging),
                                                  which is what reltol, max_iter and the sliver parameters are chosen from
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hydra_mi  # noqa: E402,F401  (the package's mesh builders)
import update_cases as uc  # noqa: E402
from oracle import ekf_c  # noqa: E402


def main():
    explore = "--explore" in sys.argv[1:]
    out = {}
    for name in uc.NAMES:
        case = uc.build(name)
        if explore:
            case = dict(case, reltol=0.0, max_iter=10)
        res = uc.run_oracle(case, ekf_c.Measurement)
        print("%-15s door %-12s info %s" % (name, res["door"], res["info"]))
        print("    figures    ", np.array2string(res["ratios"], precision=5))
        print("    min areas  ", np.array2string(res["min_area"], precision=4))
        print("    snap dist  ", np.array2string(res["snap_distance"], precision=7))
        print("    cond       ", np.array2string(res["cond_A"], precision=4))
        for k, v in res.items():
            out["%s/%s" % (name, k)] = v
    if not explore:
        path = os.path.join(ROOT, "tests", "golden", uc.GOLDEN)
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
