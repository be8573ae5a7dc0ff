#!/usr/bin/env python3
"""Sensitivity of the numpy PCQM restatement (tests/pcqm_ref.py) on the test clouds, CPU only: the per-point features, the
curvature field and the pooled score with the neighbour order reversed, and in np.longdouble, each against the plain float64
run.  The tolerance of tests/test_gpu_pcqm.py is 64 x the larger of the two, floored at 1e-10.

    python tools/pcqm_tolerances.py > profiles/pcqm_tolerances.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import pcqm_ref as P  # noqa: E402

CASES = (("shell20", 4.1, 8.2), ("sheet48", 4.1, 8.2), ("shell30", 8.19, 16.38))
MARGIN, FLOOR = 64.0, 1e-10


def main():
    print("PCQM restatement (tests/pcqm_ref.py): its own sensitivity on the test clouds, source against the seeded 70 % / sigma 12")
    print("reconstruction.  Columns: max over the points of |difference| per feature f1 .. f8, then of the curvature field (both")
    print("clouds), then |difference| of the pooled score.  np.longdouble where this ran: %s (eps %.3g)."
          % (np.dtype(np.longdouble).name, np.finfo(np.longdouble).eps))
    print("tolerance = %g x max(reversed, longdouble), floored at %g" % (MARGIN, FLOOR))
    print()
    table = {}
    for name, r, h in CASES:
        src = P.cloud(name)
        rec = P.reconstruction(src)
        base = P.pcqm(src, rec, r, h)
        rows = {}
        for label, kw in (("reversed", dict(reverse=True)), ("longdouble", dict(dtype=np.longdouble)),
                          ("reversed, no centre shift", dict(reverse=True, shift=False))):
            other = P.pcqm(src, rec, r, h, **kw)
            ref = P.pcqm(src, rec, r, h, shift=False) if "shift" in kw else base
            df = np.abs(other["features_native"] - ref["features"]).max(axis=0).astype(np.float64)
            dr = max(np.abs(other["rho_r"] - ref["rho_r"]).max(), np.abs(other["rho_d"] - ref["rho_d"]).max())
            ds = abs(float(other["pcqm_native"] - ref["pcqm"]))
            rows[label] = np.concatenate([df, [dr, ds]])
        tol = np.maximum(MARGIN * np.maximum(rows["reversed"], rows["longdouble"]), FLOOR)
        table[name] = tol
        print("%s  r = %g  h = %g  n = %d  PCQM = %.6f" % (name, r, h, len(base["features"]), base["pcqm"]))
        for label, v in rows.items():
            print("  %-26s %s" % (label, " ".join("%.2e" % x for x in v)))
        print("  %-26s %s" % ("tolerance", " ".join("%.2e" % x for x in tol)))
        print()
    print("TOLERANCES = {    # cloud: (f1 .. f8, curvature, score)")
    for name, tol in table.items():
        print('    "%s": (%s),' % (name, ", ".join("%.2e" % x for x in tol)))
    print("}")


if __name__ == "__main__":
    main()
