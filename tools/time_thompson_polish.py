"""The Thompson polish (bogp_point_eval_path / bogp_polish_path, kernels_point_path.hip) on one MI355X: d = 20, Matern-5/2,
noiseless, q = 16 paths, n_starts = 8 (B = 128 starts), per N and L medians over `--reps` runs after a warm-up, in one process:
  eval        one bogp_point_eval_path at B = 1 and at B = 128, wall (upload of the operands, ONE launch, read-back)
  iteration   the time of a polish iteration: (polish of 41 evaluations - polish of 1 evaluation) / 40, pgtol = factr = 0 so no start stops
  polish      bogp_polish_path with the library's defaults (50 evaluations at most), beside bogp_polish (one EI) on the same shapes, starts
              and box from the same process
  best value  per path the best row of a 1e4-row sweep, that sweep + polish of its 8 best rows, and a 1e5-row sweep + polish: the mean
              over the 16 paths of the (minimised) path value -- lower is better
Nothing here was tuned."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, thompson  # noqa: E402

D, Q, STARTS = 20, 16, 8


def median_ms(fn, reps):
    ts = []
    for _ in range(reps + 1):  # run 0 warms up
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--features", type=int, nargs="+", default=[256, 1024, 4096])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    lo, hi = np.full(D, -5.0), np.full(D, 5.0)
    for N in args.sizes:
        rng = np.random.default_rng(N)
        X = rng.uniform(-5, 5, size=(N, D))
        y = np.sin(X @ rng.normal(size=D) / 4) + 0.05 * rng.normal(size=N)
        theta = np.full(D, 0.01)
        eng.set_train(X, y)
        eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0)
        st = SimpleNamespace(X=X, kernel=_lib.KERNEL_MATERN52, theta=theta, nu=None)  # what thompson.draw reads of a model
        members = np.repeat(np.arange(Q), STARTS)
        for L in args.features:
            dr = thompson.draw(st, Q, L, seed=L)
            best = {}
            for M in (10_000, 100_000):
                eng.generate_candidates(lo, hi, M, 7)
                out = eng.sweep_thompson(dr, k=STARTS)
                starts = out["best_x"].reshape(Q * STARTS, D)
                _, fp, ne = eng.polish_path(starts, lo, hi, dr, out["coef"], members)
                best[M] = (float(np.mean(-out["best_val"][:, 0])), float(np.mean(fp.reshape(Q, STARTS).min(axis=1))), float(ne.mean()))
                if M == 10_000:
                    coef, s10 = out["coef"], starts
            ev1 = median_ms(lambda: eng.point_eval_path(s10[:1], dr, coef, members[:1]), args.reps)
            ev128 = median_ms(lambda: eng.point_eval_path(s10, dr, coef, members), args.reps)
            p1 = median_ms(lambda: eng.polish_path(s10, lo, hi, dr, coef, members, max_evals=1, pgtol=0.0, factr=0.0), args.reps)
            p41 = median_ms(lambda: eng.polish_path(s10, lo, hi, dr, coef, members, max_evals=41, pgtol=0.0, factr=0.0), args.reps)
            whole = median_ms(lambda: eng.polish_path(s10, lo, hi, dr, coef, members), args.reps)
            crit = median_ms(lambda: eng.polish(s10, lo, hi, (_lib.ACQ_EI, 0.0), float(y.min()), True), args.reps)
            print("N=%d L=%d: eval B=1 %.3f ms, B=128 %.3f ms; iteration %.1f us; polish_path %.3f ms (mean %.1f evaluations), bogp_polish (EI) %.3f ms"
                  % (N, L, ev1, ev128, 1e3 * (p41 - p1) / 40, whole, best[10_000][2], crit))  # fmt: skip
            print("    mean best path value: 1e4-row sweep %.4f, + polish %.4f; 1e5-row sweep %.4f, + polish %.4f"
                  % (best[10_000][0], best[10_000][1], best[100_000][0], best[100_000][1]), flush=True)  # fmt: skip
    eng.close()


if __name__ == "__main__":
    main()
