"""The scalar criterion functions of csrc/bogp_device.h (ndtr, norm_pdf, ehvi_G, EI, EpsilonPI, UCB, MGFI, feasibility) at the seeded
draws of tests/criteria_cases.py: the EXACT value of each expression at the double inputs (mpmath, 60 digits)
-> tests/golden/G46_criteria_truth.npz.

Run (build container):  python oracle/make_criteria_table.py [processes]        (~2 min with 8 processes)

Per criterion the table holds `<name>_true` (the exact value rounded to double), `<name>_rlo` (float32: exact = true (1 + rlo)) and
`<name>_checksum` of the regenerated inputs; the inputs themselves are regenerated from the seed by the reader
(criteria_cases.draw).  With the table the GPU test needs no mpmath (tests/test_gpu_criteria.py); tests/test_criteria_host.py
regenerates a sub-sample with mpmath and holds the reference's expressions to it (ledger T20)."""
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "G46_criteria_truth.npz")


def _part(args):
    import criteria_cases as CC

    name, rows = args
    return CC.exact(name, CC.draw(name), rows)


def table(name, pool, nproc):
    import criteria_cases as CC

    n = CC.ROWS[name]
    res = pool.map(_part, [(name, np.arange(i, n, nproc)) for i in range(nproc)])
    true, rlo = np.empty(n), np.empty(n, dtype=np.float32)
    for i, (t, r) in enumerate(res):
        true[i::nproc], rlo[i::nproc] = t, r
    return true, rlo


if __name__ == "__main__":
    import mpmath
    import scipy

    import criteria_cases as CC

    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    out = dict(names=np.array(CC.NAMES), mpmath=mpmath.__version__, scipy=scipy.__version__, numpy=np.__version__)
    with Pool(nproc) as pool:
        for name in CC.NAMES:
            c = CC.draw(name)
            true, rlo = table(name, pool, nproc)
            out[name + "_true"], out[name + "_rlo"], out[name + "_checksum"] = true, rlo, CC.checksum(c)
            r, cmp = CC.ratios(CC.reference(name, c), true, rlo, CC.allowance(name, c, true))
            print("%-12s %6d rows, %6d compared; the reference's worst |value - exact| / allowance = %.4g" % (name, len(true), int(cmp.sum()), r.max()))
            for what, got, need in CC.draw_conditions(name, c, cmp):
                print("    %-22s %6d (>= %d)%s" % (what, got, need, "" if got >= need else "   <-- NOT MET"))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
