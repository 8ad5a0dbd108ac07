"""Kriging-believer batches under EHVI (bogp_sweep_believer_ehvi, q = 8) against one EHVI sweep (bogp_sweep_ehvi) on the same handle,
candidates and cells: 1e6 candidates generated on the device, Matern-5/2, d = 20, at N = 2048 (C3's shape) and N = 512; m = 2 targets
with a front of 29 points (30 cells) and m = 3 with a front of 31 points (1024 cells).  Per shape, medians over `--reps` runs after
a warm-up:
  t1   bogp_sweep_ehvi with bogp_ehvi_grid_cells' cells, wall and device (HIP events of bogp_last_timing)
  t8   bogp_sweep_believer_ehvi with q = 8, wall and device (pass 0's events + bogp_believer_ehvi_last's)
  the cost of one more believed point, (t8 - t1) / 7, and its split into producer, solve, k_believer and k_believer_ehvi
Each shape runs twice: with believe_front (the believed means join the front: a winner's mean usually dominates much of it, so the later
steps see FEWER cells than step 0) and without (the front stays as given: every step evaluates step 0's cells, the dearest case).
The design holds if one more point costs less than t1 -- otherwise q EHVI sweeps would do."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib  # noqa: E402

D, M, Q = 20, 1_000_000, 8


def front_of(m, lo, hi):
    """mutually non-dominated rows with distinct coordinates inside [lo, hi] per objective: 29 rows for m = 2, 31 for m = 3"""
    n = 29 if m == 2 else 31
    t = (np.arange(n) + 0.5) / n
    return np.column_stack([lo[k] + (hi[k] - lo[k]) * (t if k < m - 1 else 1.0 - t) for k in range(m)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--targets", type=int, nargs="+", default=[2, 3])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    for N in args.sizes:
        for m in args.targets:
            rng = np.random.default_rng(N + m)
            X = rng.uniform(-5, 5, size=(N, D))
            Y = np.sin(X @ rng.normal(size=(D, m)) / 4) * (1.0 + np.arange(m)) + 0.05 * rng.normal(size=(N, m))
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, np.r_[np.full(D, 0.01), 0.9], 0.0, False, 0.0)
            eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
            ref = Y.min(axis=0) - 0.1
            front = front_of(m, np.quantile(Y, 0.3, axis=0), np.quantile(Y, 0.9, axis=0))
            lo, hi = _lib.grid_cells(front, ref)
            for bf in (True, False):
                rows = {k: [] for k in ("t1_wall", "t1_dev", "t8_wall", "t8_dev", "corr", "solve", "upd", "ehvi")}
                for rep in range(args.reps + 1):  # run 0 warms up (allocations, first launches)
                    t0 = time.perf_counter()
                    eng.sweep_ehvi(lo, hi)
                    t1w = 1e3 * (time.perf_counter() - t0)
                    tm = eng.last_timing()
                    t1d = tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"]
                    t0 = time.perf_counter()
                    out = eng.sweep_believer_ehvi(front, ref, Q, believe_front=bf)
                    t8w = 1e3 * (time.perf_counter() - t0)
                    tm = eng.last_timing()
                    bl = eng.believer_ehvi_last()
                    t8d = tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"] + bl["corr_ms"] + bl["solve_ms"] + bl["update_ms"] + bl["ehvi_ms"]
                    if rep:
                        for k, v in zip(rows, (t1w, t1d, t8w, t8d, bl["corr_ms"], bl["solve_ms"], bl["update_ms"], bl["ehvi_ms"])):
                            rows[k].append(v)
                med = {k: float(np.median(v)) for k, v in rows.items()}
                n_pass = bl["n_passes"]
                assert n_pass == Q - 1 and len(set(out["best_idx"].tolist())) == Q and out["n_cells"][0] == len(lo)
                per_wall, per_dev = (med["t8_wall"] - med["t1_wall"]) / (Q - 1), (med["t8_dev"] - med["t1_dev"]) / (Q - 1)
                print("N=%d d=%d M=%d m=%d q=%d reps=%d believe_front=%d cells per step %s" % (N, D, M, m, Q, args.reps, bf, out["n_cells"].tolist()))
                print("  t1 bogp_sweep_ehvi           wall %8.3f ms   device %8.3f ms" % (med["t1_wall"], med["t1_dev"]))
                print("  t8 bogp_sweep_believer_ehvi  wall %8.3f ms   device %8.3f ms" % (med["t8_wall"], med["t8_dev"]))
                print("  one more believed point      wall %8.3f ms (%.3f t1)   device %8.3f ms (%.3f t1)"
                      % (per_wall, per_wall / med["t1_wall"], per_dev, per_dev / med["t1_dev"]))
                print("  split per point (events): producer %.3f ms, solve %.3f ms, k_believer %.3f ms, k_believer_ehvi %.3f ms"
                      % (med["corr"] / n_pass, med["solve"] / Q, med["upd"] / n_pass, med["ehvi"] / n_pass))
                print("  condition (one more point < t1): %s" % ("holds" if per_wall < med["t1_wall"] and per_dev < med["t1_dev"] else "FAILS"), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
