"""Thompson batches for multi-objective runs (bogp_sweep_thompson_ehvi, k = 8 ranks) beside bogp_sweep_thompson_constrained at the same
column count in the same process: C3's shape (N = 2048, d = 20, Matern-5/2, 1e6 candidates generated on the device) and N = 512,
noiseless.  Both kernels issue the same matrix instructions, so the expectation is k_thompson_constrained's time plus the cell loop.
Per shape, (m, q) = (2, 8) with 30 cells and (3, 5) with 1024 cells, and L = 256 / 1024 / 4096, medians over `--reps` runs after a
warm-up with the run-to-run spread (max - min) of each kernel time:
  ehvi            wall, producer, draw at X + solves, k_thompson_ehvi; the same call over ONE cell, and from the two the share of the
                  kernel's time spent in the cell loop
  constrained     the other m - 1 targets as constraints: wall and k_thompson_constrained
For scale, per (m, q): one EHVI sweep (bogp_sweep_ehvi) and q Kriging-believer proposals (bogp_sweep_believer_ehvi) on the same model,
cells and candidates."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, pareto, thompson  # noqa: E402

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


def front_of(m, ref, top):
    """29 points on an arc (m = 2: 30 cells) or 31 on a staircase (m = 3: 32^2 = 1024 cells) between `ref` and `top`."""
    if m == 2:
        a = np.linspace(0.05, 0.95, 29) * np.pi / 2
        return ref + 0.6 * (top - ref) * np.column_stack([np.cos(a), np.sin(a)])
    s = np.linspace(0.1, 0.8, 31)
    return ref + (top - ref) * np.column_stack([s, s[::-1], 0.3 + 0.4 * np.abs(s - 0.45)])


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
        Y = np.column_stack([np.sin(X @ rng.normal(size=D) / 4) + 0.05 * rng.normal(size=N) for _ in range(3)])
        theta = np.full(D, 0.01)
        st = SimpleNamespace(X=X, kernel=_lib.KERNEL_MATERN52, theta=theta, nu=None)  # what thompson.draw reads of a model
        print("N=%d d=%d M=%d k=%d reps=%d" % (N, D, M, K, args.reps))
        for m, q in ((2, 8), (3, 5)):
            eng.set_train(X, Y[:, :m])
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, theta, 0.0, False, 0.0)
            eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
            ref = np.quantile(Y[:, :m], 0.3, axis=0)
            F = front_of(m, ref, Y[:, :m].max(axis=0))
            lower, upper = pareto.hypercell_bounds(F, ref)
            lo, hi = np.full(m - 1, -np.inf), np.median(Y[:, 1:m], axis=0)
            for L in args.features:
                dr = thompson.draw(st, q * m, L, seed=L)
                e = series(args.reps, lambda: eng.sweep_thompson_ehvi(dr, q, lower, upper, k=K), eng.thompson_ehvi_last)
                e1 = series(args.reps, lambda: eng.sweep_thompson_ehvi(dr, q, lower[:1], upper[:1], k=K), eng.thompson_ehvi_last)
                c = series(args.reps, lambda: eng.sweep_thompson_constrained(dr, q, lo, hi, k=K), eng.thompson_constrained_last)
                print("  ehvi m=%d q=%d C=%-4d  L = %-4d  wall %8.3f ms   producer %7.3f ms  draw at X + solves %7.3f ms  k_thompson_ehvi %7.3f ms "
                      "(spread %.3f, %d chunks)   one cell %7.3f ms (spread %.3f): cell loop %4.1f %% of the kernel"
                      % (m, q, len(lower), L, e["wall"], e["corr"], e["solve"], e["paths"], e["spread"], e["chunks"], e1["paths"], e1["spread"],
                         100.0 * (1.0 - e1["paths"] / e["paths"])), flush=True)  # fmt: skip
                print("  constrained m=%d q=%d   L = %-4d  wall %8.3f ms   k_thompson_constrained %7.3f ms (spread %.3f)   ehvi kernel - constrained %+7.3f ms"
                      % (m, q, L, c["wall"], c["paths"], c["spread"], e["paths"] - c["paths"]), flush=True)  # fmt: skip
            wall = [timed(lambda: eng.sweep_ehvi(lower, upper, k=K))[0] for _ in range(args.reps + 1)][1:]
            print("  bogp_sweep_ehvi, C = %d, k = %d                 wall %8.3f ms (spread %.3f)" % (len(lower), K, np.median(wall), max(wall) - min(wall)))
            wall = [timed(lambda: eng.sweep_believer_ehvi(F, ref, q))[0] for _ in range(args.reps + 1)][1:]
            print("  bogp_sweep_believer_ehvi, q = %d                 wall %8.3f ms (spread %.3f)" % (q, np.median(wall), max(wall) - min(wall)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
