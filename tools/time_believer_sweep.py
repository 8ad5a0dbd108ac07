"""Kriging-believer batches (bogp_sweep_believer, q = 8) against the plain sweep (bogp_sweep, one EI) on the same handle and
candidates: C3's shape (N = 2048, d = 20, Matern-5/2, 1e6 candidates generated on the device) and N = 512.  Per shape, medians
over `--reps` runs after a warm-up:
  t1   bogp_sweep, wall and device (HIP events of bogp_last_timing: producer + contraction + criteria)
  t8   bogp_sweep_believer with q = 8, wall and device (pass 0's events + bogp_believer_last's: producer, solves, k_believer)
  the cost of one more believed point, (t8 - t1) / 7, and its split into producer, solve and k_believer from the events
  k_believer's achieved bytes/s: it reads the chunk once, 8 N bytes per candidate and pass (peak HBM of an MI355X: 8 TB/s)
The design holds if one more point costs less than t1 -- otherwise q plain sweeps would do."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib  # noqa: E402

D, M, Q = 20, 1_000_000, 8
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    for N in args.sizes:
        rng = np.random.default_rng(N)
        X = rng.uniform(-5, 5, size=(N, D))
        y = np.sin(X @ rng.normal(size=D) / 4) + 0.05 * rng.normal(size=N)
        eng.set_train(X, y)
        eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, np.r_[np.full(D, 0.01), 0.9], 1e-6, True, 0.0)
        eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
        plugin = float(y.min())
        ei = [(_lib.ACQ_EI, 0.0)]
        rows = {k: [] for k in ("t1_wall", "t1_dev", "t8_wall", "t8_dev", "corr", "solve", "kb")}
        for rep in range(args.reps + 1):  # run 0 warms up (allocations, first launches)
            t0 = time.perf_counter()
            eng.sweep(ei, plugin, True)
            t1w = 1e3 * (time.perf_counter() - t0)
            tm = eng.last_timing()
            t1d = tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"]
            t0 = time.perf_counter()
            out = eng.sweep_believer(ei * Q, plugin, True)
            t8w = 1e3 * (time.perf_counter() - t0)
            tm = eng.last_timing()
            bl = eng.believer_last()
            t8d = tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"] + bl["corr_ms"] + bl["solve_ms"] + bl["believer_ms"]
            if rep:
                for k, v in zip(rows, (t1w, t1d, t8w, t8d, bl["corr_ms"], bl["solve_ms"], bl["believer_ms"])):
                    rows[k].append(v)
        med = {k: float(np.median(v)) for k, v in rows.items()}
        n_pass = bl["n_passes"]
        assert n_pass == Q - 1 and len(set(out["best_idx"].tolist())) == Q
        per_wall, per_dev = (med["t8_wall"] - med["t1_wall"]) / (Q - 1), (med["t8_dev"] - med["t1_dev"]) / (Q - 1)
        bw = 8.0 * N * M / (1e-3 * med["kb"] / n_pass)
        print("N=%d d=%d M=%d q=%d reps=%d" % (N, D, M, Q, args.reps))
        print("  t1 bogp_sweep           wall %8.3f ms   device %8.3f ms" % (med["t1_wall"], med["t1_dev"]))
        print("  t8 bogp_sweep_believer  wall %8.3f ms   device %8.3f ms" % (med["t8_wall"], med["t8_dev"]))
        print("  one more believed point wall %8.3f ms (%.3f t1)   device %8.3f ms (%.3f t1)"
              % (per_wall, per_wall / med["t1_wall"], per_dev, per_dev / med["t1_dev"]))
        print("  split per point (events): producer %.3f ms, solve %.3f ms, k_believer %.3f ms"
              % (med["corr"] / n_pass, med["solve"] / Q, med["kb"] / n_pass))
        print("  k_believer: %.3f TB/s of the chunk read = %.1f %% of %.1f TB/s" % (bw / 1e12, 100 * bw / HBM_PEAK, HBM_PEAK / 1e12), flush=True)
        print("  condition (one more point < t1): %s" % ("holds" if per_wall < med["t1_wall"] and per_dev < med["t1_dev"] else "FAILS"), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
