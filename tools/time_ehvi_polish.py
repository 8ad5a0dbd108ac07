"""The input gradient of EHVI and the lock-step polish on it (bogp_point_eval_ehvi, bogp_polish_ehvi) against the EHVI sweep
(bogp_sweep_ehvi) on the same handle: Matern-5/2, d = 20, at N = 2048 (C3's shape) and N = 512; m = 2 targets with a front of 29
points (30 cells) and m = 3 with a front of 31 points (1024 cells).  Per shape, medians over `--reps` runs after a warm-up:
  us per one-point value + gradient call (the call of the reference-style BFGS loop; cells resident, completion polled)
  ms for a 32-start polish of 50 iterations (bogp_polish_ehvi from the sweep's 32 best rows; iterations actually used per start)
  per candidate count (1e6 and 1e5, drawn on the device): bogp_sweep_ehvi's time -- the yardstick -- and its best EHVI, then
  sweep (k = 32) + polish on the same state: time and the EHVI found."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib  # noqa: E402

D, K, ITERS = 20, 32, 50


def front_of(m, lo, hi):
    """mutually non-dominated rows with distinct coordinates inside [lo, hi] per objective: 29 rows for m = 2, 31 for m = 3"""
    n = 29 if m == 2 else 31
    t = (np.arange(n) + 0.5) / n
    return np.column_stack([lo[k] + (hi[k] - lo[k]) * (t if k < m - 1 else 1.0 - t) for k in range(m)])


def med_ms(fn, reps):
    out = []
    for rep in range(reps + 1):  # run 0 warms up
        t0 = time.perf_counter()
        r = fn()
        if rep:
            out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--targets", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--candidates", type=int, nargs="+", default=[1_000_000, 100_000])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    blo, bhi = np.full(D, -5.0), np.full(D, 5.0)
    for N in args.sizes:
        for m in args.targets:
            rng = np.random.default_rng(N + m)
            X = rng.uniform(-5, 5, size=(N, D))
            Y = np.sin(X @ rng.normal(size=(D, m)) / 4) * (1.0 + np.arange(m)) + 0.05 * rng.normal(size=(N, m))
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, np.r_[np.full(D, 0.01), 0.9], 0.0, False, 0.0)
            ref = Y.min(axis=0) - 0.1
            front = front_of(m, np.quantile(Y, 0.3, axis=0), np.quantile(Y, 0.9, axis=0))
            lo, hi = _lib.grid_cells(front, ref)
            print("N=%d d=%d m=%d cells=%d reps=%d" % (N, D, m, len(lo), args.reps))
            x1 = rng.uniform(-5, 5, size=(1, D))
            eng.point_eval_ehvi(x1, lo, hi)
            n_calls = 200
            t0 = time.perf_counter()
            for _ in range(n_calls):
                eng.point_eval_ehvi(x1, lo, hi)
            print("  one-point value + gradient call     %8.1f us" % (1e6 * (time.perf_counter() - t0) / n_calls))
            for M in args.candidates:
                eng.generate_candidates(blo, bhi, M, 7)
                t_sweep, (best, idx) = med_ms(lambda: eng.sweep_ehvi(lo, hi), args.reps)

                def hybrid():
                    bv, bi = eng.sweep_ehvi(lo, hi, k=K)
                    return eng.polish_ehvi(eng.read_candidates(bi), blo, bhi, lo, hi, max_evals=ITERS)

                t_hyb, (xs, fs, ne) = med_ms(hybrid, args.reps)
                starts = eng.read_candidates(eng.sweep_ehvi(lo, hi, k=K)[1])
                t_pol, _ = med_ms(lambda: eng.polish_ehvi(starts, blo, bhi, lo, hi, max_evals=ITERS), args.reps)
                print("  M=%-8d bogp_sweep_ehvi        %8.3f ms   best EHVI %.6g" % (M, t_sweep, best[0]))
                print("  M=%-8d sweep (k=%d) + polish  %8.3f ms   best EHVI %.6g   (polish alone %.3f ms, %d starts, "
                      "evaluations per start min %d / median %d / max %d)"
                      % (M, K, t_hyb, fs.max(), t_pol, len(starts), ne.min(), int(np.median(ne)), ne.max()), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
