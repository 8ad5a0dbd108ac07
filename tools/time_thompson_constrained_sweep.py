"""Thompson batches under modelled constraints (bogp_sweep_thompson_constrained, k = 8 ranks) beside bogp_sweep_thompson with q = 16
paths in the same process: C3's shape (N = 2048, d = 20, Matern-5/2, 1e6 candidates generated on the device) and N = 512, noiseless.
Both kernels issue the same matrix instructions for 16 columns, so the expectation is k_thompson's time plus the epilogue (the lane
gather, 2 q score rows stored where k > 1 instead of q path rows).  Per shape and L = 256 / 1024 / 4096, medians over `--reps` runs
after a warm-up, with the run-to-run spread (max - min) of each kernel time:
  thompson        bogp_sweep_thompson, q = 16: wall, producer, draw at X + solves, k_thompson
  constrained     (m, q) = (2, 8) and (4, 4), 16 columns each: wall, producer, draw at X + solves, k_thompson_constrained, and the
                  difference of the two kernel times
For scale, per shape: one constrained sweep (bogp_sweep_constrained, EI) and eight constrained-believer proposals
(bogp_sweep_believer_constrained) on the m = 2 model and the same candidates."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, thompson  # noqa: E402

D, M, K = 20, 1_000_000, 8


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def series(reps, call, last):
    rows = {k: [] for k in ("wall", "corr", "solve", "paths")}
    for rep in range(reps + 1):  # run 0 warms up (allocations, first launches)
        w, _ = timed(call)
        tl = last()
        if rep:
            for k, v in zip(rows, (w, tl["corr_ms"], tl["solve_ms"], tl["paths_ms"])):
                rows[k].append(v)
    med = {k: float(np.median(v)) for k, v in rows.items()}
    med["spread"] = float(np.max(rows["paths"]) - np.min(rows["paths"]))
    med["chunks"] = tl["n_chunks"]
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--features", type=int, nargs="+", default=[256, 1024, 4096])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    for N in args.sizes:
        rng = np.random.default_rng(N)
        X = rng.uniform(-5, 5, size=(N, D))
        Y = np.column_stack([np.sin(X @ rng.normal(size=D) / 4) + 0.05 * rng.normal(size=N) for _ in range(4)])
        theta = np.full(D, 0.01)
        st = SimpleNamespace(X=X, kernel=_lib.KERNEL_MATERN52, theta=theta, nu=None)  # what thompson.draw reads of a model
        print("N=%d d=%d M=%d k=%d reps=%d" % (N, D, M, K, args.reps))
        eng.set_train(X, Y[:, 0])
        eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0)
        eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
        base = {}
        for L in args.features:
            dr = thompson.draw(st, 16, L, seed=L)
            base[L] = series(args.reps, lambda: eng.sweep_thompson(dr, k=K), eng.thompson_last)
            b = base[L]
            print("  thompson q=16            L = %-4d  wall %8.3f ms   producer %7.3f ms  draw at X + solves %7.3f ms  k_thompson %7.3f ms (spread %.3f, %d chunks)"
                  % (L, b["wall"], b["corr"], b["solve"], b["paths"], b["spread"], b["chunks"]), flush=True)  # fmt: skip
        for m, q in ((2, 8), (4, 4)):
            eng.set_train(X, Y[:, :m])
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, theta, 0.0, False, 0.0)
            eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
            lo, hi = np.full(m - 1, -np.inf), np.median(Y[:, 1:m], axis=0)
            for L in args.features:
                dr = thompson.draw(st, q * m, L, seed=L)
                c = series(args.reps, lambda: eng.sweep_thompson_constrained(dr, q, lo, hi, k=K), eng.thompson_constrained_last)
                print("  constrained m=%d q=%d      L = %-4d  wall %8.3f ms   producer %7.3f ms  draw at X + solves %7.3f ms  k_thompson_constrained %7.3f ms "
                      "(spread %.3f, %d chunks)   kernel - k_thompson %+7.3f ms"
                      % (m, q, L, c["wall"], c["corr"], c["solve"], c["paths"], c["spread"], c["chunks"], c["paths"] - base[L]["paths"]), flush=True)  # fmt: skip
            if m == 2:  # for scale: the feasibility-weighted sweep and eight believer proposals on the same model and candidates
                ei = [(_lib.ACQ_EI, 0.0)]
                plugin = float(Y[:, 0].min())
                wall = [timed(lambda: eng.sweep_constrained(ei, plugin, True, lo, hi, k=K))[0] for _ in range(args.reps + 1)][1:]
                print("  bogp_sweep_constrained (EI), k = %d            wall %8.3f ms" % (K, np.median(wall)))
                wall = [timed(lambda: eng.sweep_believer_constrained(ei * 8, plugin, True, lo, hi))[0] for _ in range(args.reps + 1)][1:]
                print("  bogp_sweep_believer_constrained, q = 8          wall %8.3f ms" % np.median(wall), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
