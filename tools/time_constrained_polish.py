"""The input gradient of the feasibility-weighted criterion and the lock-step polish on it (bogp_point_eval_constrained,
bogp_polish_constrained) against the constrained sweep (bogp_sweep_constrained) on the same handle: Matern-5/2, d = 20, at N = 2048
(C3's shape) and N = 512; EI on target 0 with 1 and with 3 constraints (g <= median, an interval [q40, q60], an upper tail [q70, +inf)).
Per shape, medians over `--reps` runs after a warm-up:
  us per one-point value + gradient call (the call of the reference-style BFGS loop; completion polled)
  per candidate count (1e6 and 1e5, drawn on the device): bogp_sweep_constrained's time -- the yardstick -- and its best value, then
  sweep (k = 32) + polish of 50 iterations on the same state: time and the value found, and the polish alone."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib  # noqa: E402

D, K, ITERS = 20, 32, 50
INF = float("inf")


def med_ms(fn, reps):
    out = []
    for rep in range(reps + 1):  # run 0 warms up
        t0 = time.perf_counter()
        r = fn()
        if rep:
            out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), r


def bounds_of(Y, n_con):
    lo = [-INF, float(np.quantile(Y[:, 2], 0.4)) if n_con > 1 else 0.0, float(np.quantile(Y[:, 3], 0.7)) if n_con > 2 else 0.0]
    hi = [float(np.median(Y[:, 1])), float(np.quantile(Y[:, 2], 0.6)) if n_con > 1 else 0.0, INF]
    return np.array(lo[:n_con]), np.array(hi[:n_con])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--constraints", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--candidates", type=int, nargs="+", default=[1_000_000, 100_000])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    blo, bhi = np.full(D, -5.0), np.full(D, 5.0)
    acq = (_lib.ACQ_EI, 0.0)
    for N in args.sizes:
        for n_con in args.constraints:
            m = n_con + 1
            rng = np.random.default_rng(N + m)
            X = rng.uniform(-5, 5, size=(N, D))
            Y = np.sin(X @ rng.normal(size=(D, m)) / 4) * (1.0 + np.arange(m)) + 0.05 * rng.normal(size=(N, m))
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, np.r_[np.full(D, 0.01), 0.9], 0.0, False, 0.0)
            lo, hi = bounds_of(Y, n_con)
            feas = np.all((Y[:, 1:] >= lo) & (Y[:, 1:] <= hi), axis=1)
            plugin = float(Y[feas, 0].min()) if feas.any() else float(Y[:, 0].min())
            print("N=%d d=%d constraints=%d feasible training rows=%d reps=%d" % (N, D, n_con, feas.sum(), args.reps))
            x1 = rng.uniform(-5, 5, size=(1, D))
            eng.point_eval_constrained(x1, [acq], plugin, True, lo, hi)
            n_calls = 200
            t0 = time.perf_counter()
            for _ in range(n_calls):
                eng.point_eval_constrained(x1, [acq], plugin, True, lo, hi)
            print("  one-point value + gradient call         %8.1f us" % (1e6 * (time.perf_counter() - t0) / n_calls))
            for M in args.candidates:
                eng.generate_candidates(blo, bhi, M, 7)
                t_sweep, (best, idx) = med_ms(lambda: eng.sweep_constrained([acq], plugin, True, lo, hi), args.reps)

                def hybrid():
                    bv, bi = eng.sweep_constrained([acq], plugin, True, lo, hi, k=K)
                    return eng.polish_constrained(eng.read_candidates(bi[0]), blo, bhi, acq, plugin, True, lo, hi, max_evals=ITERS)

                t_hyb, (xs, fs, ne) = med_ms(hybrid, args.reps)
                starts = eng.read_candidates(eng.sweep_constrained([acq], plugin, True, lo, hi, k=K)[1][0])
                t_pol, _ = med_ms(lambda: eng.polish_constrained(starts, blo, bhi, acq, plugin, True, lo, hi, max_evals=ITERS), args.reps)
                print("  M=%-8d bogp_sweep_constrained     %8.3f ms   best value %.6g" % (M, t_sweep, best[0, 0]))
                print("  M=%-8d sweep (k=%d) + polish      %8.3f ms   best value %.6g   (polish alone %.3f ms, %d starts, "
                      "evaluations per start min %d / median %d / max %d)"
                      % (M, K, t_hyb, fs.max(), t_pol, len(starts), ne.min(), int(np.median(ne)), ne.max()), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
