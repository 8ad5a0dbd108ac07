#!/usr/bin/env python3
"""One sha1 per configuration over everything bogp_point_eval_ehvi returns -- (ehvi, dehvi, mu, mse, dmu, dmse) -- for the 38
configurations of tests/test_gpu_ehvi_grad.py, and one over bogp_polish_ehvi's (points, values, evaluations) on the last of them.
Two builds compute the same EHVI gradient bit for bit exactly when their listings agree line for line:

    python tools/ehvi_point_bits.py                    > pr.txt       # the tree this file sits in
    python tools/ehvi_point_bits.py --root ../parent   > parent.txt   # another checkout with its own libbogp.so

Needs an MI355X."""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package, library and test shapes are loaded")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import numpy as np

    import test_gpu_ehvi_grad as T
    from bogp import _lib

    assert os.path.dirname(os.path.abspath(_lib.__file__)).startswith(root), _lib.__file__
    eng = _lib.Engine(0)
    cfgs = T._configs()
    for cfg in cfgs:  # all of them: every N, d, m (one kernel instantiation each), both B, the four kernels, noisy and noiseless
        kernel, noisy, N, d, m, kind, B = cfg
        par, mode, X, Y, lo, hi = T._problem(*cfg[:6], seed=N + d + m)
        T._commit(eng, kernel, par, mode, X, Y)
        rows = T._rows(np.random.default_rng(1), X, B, d)
        h = hashlib.sha1()
        for a in eng.point_eval_ehvi(rows, lo, hi, moments=True):
            h.update(np.ascontiguousarray(a).tobytes())
        print("BITS %-40s %s" % (T._id(cfg), h.hexdigest()), flush=True)
    h = hashlib.sha1()
    for a in eng.polish_ehvi(rows, np.full(d, T.BOX[0]), np.full(d, T.BOX[1]), lo, hi, max_evals=20):
        h.update(np.ascontiguousarray(a).tobytes())
    print("BITS %-40s %s" % ("polish/" + T._id(cfg), h.hexdigest()), flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
