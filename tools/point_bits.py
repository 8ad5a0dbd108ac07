#!/usr/bin/env python3
"""One sha1 per configuration over everything the one-point / B-point path returns, for its three families, and one per family over a
polish: the configurations and problems are those of the GPU tests.

  ehvi         bogp_point_eval_ehvi (ehvi, dehvi, mu, mse, dmu, dmse) for the 38 configurations of tests/test_gpu_ehvi_grad.py,
               bogp_polish_ehvi (points, values, evaluations) on the last of them
  constrained  bogp_point_eval_constrained (acq, dacq, pof, dpof, mu, mse, dmu, dmse) for the 38 configurations of
               tests/test_gpu_constrained_grad.py, bogp_polish_constrained on the last of them
  point        bogp_point_eval_batch (mu, mse, dmu, dmse, values, dvalues) and the one-point bogp_point_eval of row 0 for the five golden
               models tests/test_gpu_point.py names, VALU and MFMA flavour (BOGP_POINT_MFMA_MIN = 0 / 1), bogp_polish on that module's C3-like model

Two builds compute the same numbers bit for bit exactly when their listings agree line for line:

    python tools/point_bits.py                    > pr.txt       # the tree this file sits in
    python tools/point_bits.py --root ../parent   > parent.txt   # another checkout with its own libbogp.so

Needs an MI355X."""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def line(name, arrays):
    import numpy as np

    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print("BITS %-48s %s" % (name, h.hexdigest()), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package, library and test shapes are loaded")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import numpy as np

    import test_gpu_constrained_grad as TC
    import test_gpu_ehvi_grad as TE
    import test_gpu_point as TP
    from bogp import _lib

    assert os.path.dirname(os.path.abspath(_lib.__file__)).startswith(root), _lib.__file__
    eng = _lib.Engine(0)
    # all of them: every N, d, m (one kernel instantiation each), both B, the four kernels, noisy and noiseless
    for cfg in TE._configs():
        kernel, noisy, N, d, m, kind, B = cfg
        par, mode, X, Y, lo, hi = TE._problem(*cfg[:6], seed=N + d + m)
        TE._commit(eng, kernel, par, mode, X, Y)
        rows = TE._rows(np.random.default_rng(1), X, B, d)
        line("ehvi/" + TE._id(cfg), eng.point_eval_ehvi(rows, lo, hi, moments=True))
    line("ehvi/polish/" + TE._id(cfg), eng.polish_ehvi(rows, np.full(d, TE.BOX[0]), np.full(d, TE.BOX[1]), lo, hi, max_evals=20))
    for cfg in TC._configs():
        par, mode, X, Y, lo, hi, plugin, rows = TC._case(cfg)
        TC._commit(eng, cfg[0], par, mode, X, Y)
        line("constrained/" + TC._id(cfg), eng.point_eval_constrained(rows, TC.ACQ4, plugin, cfg[6], lo, hi, moments=True))
    d = cfg[3]
    box = np.full(d, TC.BOX[0]), np.full(d, TC.BOX[1])
    line("constrained/polish/" + TC._id(cfg), eng.polish_constrained(rows, *box, TC.ACQ4[0], plugin, cfg[6], lo, hi, max_evals=20))
    acq = [(i, p) for _, i, p in TP.DX_ACQ]
    for name in TP.DX_FILES:
        g = TP.load_golden(name)
        TP.commit_golden(eng, g)
        pl = float(g["plugin_eff"][0])
        for flavour, v in (("valu", "0"), ("mfma", "1")):
            os.environ["BOGP_POINT_MFMA_MIN"] = v
            line("point/%s/%s" % (name, flavour), eng.point_eval_batch(g["Xs"], acq, pl, True))
        del os.environ["BOGP_POINT_MFMA_MIN"]
        line("point/%s/one" % name, eng.point_eval(g["Xs"][0], acq, pl, True))
    X, y, rng = TP._c3_like(eng)
    d = X.shape[1]
    starts = rng.uniform(-5, 5, size=(32, d))
    line("point/polish/c3-like", eng.polish(starts, np.full(d, -5.0), np.full(d, 5.0), (_lib.ACQ_MGFI, 2.0), float(y.min()), True, max_evals=20))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
