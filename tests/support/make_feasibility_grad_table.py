"""Writes tests/golden/G47_feasibility_grad_truth.npz: the two derivatives of the probability of feasibility in exact arithmetic
(mpmath, 60 digits) on the seeded draw `criteria_cases.draw("feasibility")`, stored as `_true` / `_rlo` / checksum like G46, and prints
the worst |reference expression - exact| / allowance over the full draw -- the figures tests/feasibility_grad_cases.py records as
REFERENCE_RATIO and takes F from.

    python tests/support/make_feasibility_grad_table.py            (from the repository root; about a minute)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import criteria_cases as CC  # noqa: E402
import feasibility_grad_cases as FG  # noqa: E402


def main():
    c = FG.draw()
    ex = FG.exact(c)
    out = {"checksum": np.float64(CC.checksum(c))}
    for name in FG.NAMES:
        true, rlo = ex[name]
        out[name + "_true"], out[name + "_rlo"] = true, rlo
        r, cmp = FG.ratios(FG.reference(name, c), true, rlo, FG.allowance(name, c))
        print("%s: reference expression, worst |value - exact| / allowance = %.4g over %d of %d rows" % (name, r.max(), cmp.sum(), len(cmp)))
    path = os.path.join(ROOT, "tests", "golden", "G47_feasibility_grad_truth.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
