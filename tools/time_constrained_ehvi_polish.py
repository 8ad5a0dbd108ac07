"""The input gradient of feasibility-weighted EHVI and the lock-step polish on it (bogp_point_eval_ehvi_constrained,
bogp_polish_ehvi_constrained) against the constrained EHVI sweep (bogp_sweep_ehvi_constrained) on the same handle: Matern-5/2, d = 20, at
N = 2048 (C3's shape) and N = 512; (m, c) = (2, 1), (2, 3) and (3, 1) objectives and constraints (g <= median, an interval [q40, q60], an
upper tail [q70, +inf)), the cells those of the front of the feasible training rows.  Per shape, medians over `--reps` runs after a warm-up:
  us per one-point value + gradient call (the call of the reference-style BFGS loop; cells resident, completion polled), and beside it
     bogp_point_eval_ehvi on the objectives-only model and bogp_point_eval_constrained (one criterion) on the same model
  per candidate count (1e6 and 1e5, drawn on the device): bogp_sweep_ehvi_constrained's time -- the yardstick -- and its best value, then
  sweep (k = 32) + polish of 50 iterations on the same state: time and the value found, and the polish alone."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, pareto  # noqa: E402

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


def bounds_of(Yc):
    c = Yc.shape[1]
    lo = [-INF, float(np.quantile(Yc[:, 1], 0.4)) if c > 1 else 0.0, float(np.quantile(Yc[:, 2], 0.7)) if c > 2 else 0.0]
    hi = [float(np.median(Yc[:, 0])), float(np.quantile(Yc[:, 1], 0.6)) if c > 1 else 0.0, INF]
    return np.array(lo[:c]), np.array(hi[:c])


def us_per_call(fn, n_calls=200):
    fn()
    t0 = time.perf_counter()
    for _ in range(n_calls):
        fn()
    return 1e6 * (time.perf_counter() - t0) / n_calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--shapes", type=str, nargs="+", default=["2,1", "2,3", "3,1"], help="objectives,constraints")
    ap.add_argument("--candidates", type=int, nargs="+", default=[1_000_000, 100_000])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    blo, bhi = np.full(D, -5.0), np.full(D, 5.0)
    par = np.r_[np.full(D, 0.01), 0.9]
    for N in args.sizes:
        for shape in args.shapes:
            m, c = (int(t) for t in shape.split(","))
            rng = np.random.default_rng(N + 10 * m + c)
            X = rng.uniform(-5, 5, size=(N, D))
            Y = np.sin(X @ rng.normal(size=(D, m + c)) / 4) * (1.0 + np.arange(m + c)) + 0.05 * rng.normal(size=(N, m + c))
            lo, hi = bounds_of(Y[:, m:])
            feas = np.all((Y[:, m:] >= lo) & (Y[:, m:] <= hi), axis=1)
            ref = Y[:, :m].min(axis=0) - 0.1
            front = pareto.pareto_front(Y[feas, :m], ref)[:31]  # (at most 32^2 cells for m = 3)
            lower, upper = pareto.hypercell_bounds(front, ref)
            x1 = rng.uniform(-5, 5, size=(1, D))
            # the two calls the new one sits next to: EHVI on the objectives-only model, one feasibility-weighted criterion on this model
            eng.set_train(X, Y[:, :m])
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, par, 0.0, False, 0.0)
            us_ehvi = us_per_call(lambda: eng.point_eval_ehvi(x1, lower, upper))
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, par, 0.0, False, 0.0)
            clo, chi = np.r_[np.full(m - 1, -INF), lo], np.r_[np.full(m - 1, INF), hi]
            us_con = us_per_call(lambda: eng.point_eval_constrained(x1, [(_lib.ACQ_EI, 0.0)], float(Y[:, 0].min()), True, clo, chi))
            us_new = us_per_call(lambda: eng.point_eval_ehvi_constrained(x1, lower, upper, lo, hi))
            print("N=%d d=%d objectives=%d constraints=%d cells=%d feasible training rows=%d reps=%d" % (N, D, m, c, len(lower), feas.sum(), args.reps))
            print("  one-point value + gradient call         %8.1f us   (bogp_point_eval_ehvi on the objectives alone %.1f us, "
                  "bogp_point_eval_constrained on this model %.1f us)" % (us_new, us_ehvi, us_con))  # fmt: skip
            for M in args.candidates:
                eng.generate_candidates(blo, bhi, M, 7)
                t_sweep, (best, idx) = med_ms(lambda: eng.sweep_ehvi_constrained(lower, upper, lo, hi), args.reps)

                def hybrid():
                    bv, bi = eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=K)
                    return eng.polish_ehvi_constrained(eng.read_candidates(bi), blo, bhi, lower, upper, lo, hi, max_evals=ITERS)

                t_hyb, (xs, fs, ne) = med_ms(hybrid, args.reps)
                starts = eng.read_candidates(eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=K)[1])
                t_pol, _ = med_ms(lambda: eng.polish_ehvi_constrained(starts, blo, bhi, lower, upper, lo, hi, max_evals=ITERS), args.reps)
                print("  M=%-8d bogp_sweep_ehvi_constrained %8.3f ms   best value %.6g" % (M, t_sweep, best[0]))
                print("  M=%-8d sweep (k=%d) + polish       %8.3f ms   best value %.6g   (polish alone %.3f ms, %d starts, "
                      "evaluations per start min %d / median %d / max %d)"
                      % (M, K, t_hyb, fs.max(), t_pol, len(starts), ne.min(), int(np.median(ne)), ne.max()), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
