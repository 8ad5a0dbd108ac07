"""Thompson-sampling batches (bogp_sweep_thompson, q = 16 paths, k = 8 ranks) beside the plain sweep (bogp_sweep, one EI, pruning on
and off) and 16 Kriging-believer proposals (bogp_sweep_believer) on the same handle and candidates: C3's shape (N = 2048, d = 20,
Matern-5/2, 1e6 candidates generated on the device) and N = 512, noiseless (the mode Thompson sampling serves).  Per shape, medians
over `--reps` runs after a warm-up:
  sweep      bogp_sweep, wall and device (bogp_last_timing: producer + contraction + criteria), pruning on / off
  believer   bogp_sweep_believer with q = 16, wall
  thompson   per L = 256 / 1024 / 4096: wall, and bogp_thompson_last's producer, draw-at-X + solves, and k_thompson times
  k_thompson's two terms: the prior paths (conditioned = 0) run the feature term alone -> cos per second; the rest of the conditioned
  run's kernel time is the r term, 8 N bytes per candidate -> bytes per second (peak HBM of an MI355X: 8 TB/s)"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, thompson  # noqa: E402

D, M, Q, K = 20, 1_000_000, 16, 8
HBM_PEAK = 8.0e12


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


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
        y = np.sin(X @ rng.normal(size=D) / 4) + 0.05 * rng.normal(size=N)
        theta = np.full(D, 0.01)
        eng.set_train(X, y)
        eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0)
        st = SimpleNamespace(X=X, kernel=_lib.KERNEL_MATERN52, theta=theta, nu=None)  # what thompson.draw reads of a model
        eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
        plugin = float(y.min())
        ei = [(_lib.ACQ_EI, 0.0)]
        print("N=%d d=%d M=%d q=%d k=%d reps=%d" % (N, D, M, Q, K, args.reps))
        for prune in (True, False):
            eng.set_prune(prune)
            wall, dev = [], []
            for rep in range(args.reps + 1):  # run 0 warms up (allocations, first launches)
                w, _ = timed(lambda: eng.sweep(ei, plugin, True))
                tm = eng.last_timing()
                if rep:
                    wall.append(w), dev.append(tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"])
            print("  bogp_sweep (EI), pruning %-3s        wall %8.3f ms   device %8.3f ms" % ("on" if prune else "off", np.median(wall), np.median(dev)))
        eng.set_prune(True)
        wall = [timed(lambda: eng.sweep_believer(ei * Q, plugin, True))[0] for _ in range(args.reps + 1)][1:]
        print("  bogp_sweep_believer, q = %d         wall %8.3f ms" % (Q, np.median(wall)), flush=True)
        for L in args.features:
            dr = thompson.draw(st, Q, L, seed=L)
            rows = {k: [] for k in ("wall", "corr", "solve", "paths", "prior")}
            for rep in range(args.reps + 1):
                w, out = timed(lambda: eng.sweep_thompson(dr, k=K))
                tl = eng.thompson_last()
                eng.sweep_thompson(dr, k=K, conditioned=False)
                pr = eng.thompson_last()["paths_ms"]
                if rep:
                    for k, v in zip(rows, (w, tl["corr_ms"], tl["solve_ms"], tl["paths_ms"], pr)):
                        rows[k].append(v)
            med = {k: float(np.median(v)) for k, v in rows.items()}
            assert out["best_idx"].shape == (Q, K) and np.all(out["best_idx"] >= 0)
            r_ms = max(med["paths"] - med["prior"], 1e-9)
            print("  bogp_sweep_thompson, L = %-4d        wall %8.3f ms   producer %7.3f ms  draw at X + solves %7.3f ms  k_thompson %7.3f ms (%d chunks)"
                  % (L, med["wall"], med["corr"], med["solve"], med["paths"], tl["n_chunks"]))  # fmt: skip
            print("      feature term alone %7.3f ms = %.3g cos/s;  r term %7.3f ms = %.3f TB/s (%.1f %% of %.1f TB/s)"
                  % (med["prior"], L * M / (1e-3 * med["prior"]), r_ms, 8.0 * N * M / (1e-3 * r_ms) / 1e12, 100 * 8.0 * N * M / (1e-3 * r_ms) / HBM_PEAK,
                     HBM_PEAK / 1e12), flush=True)  # fmt: skip
    eng.close()


if __name__ == "__main__":
    main()
