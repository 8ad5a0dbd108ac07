"""Kriging-believer batches for constrained EHVI (bogp_sweep_believer_ehvi_constrained, q = 8) against one constrained EHVI sweep
(bogp_sweep_ehvi_constrained) on the same handle, candidates, cells and bounds: 1e6 candidates generated on the device, Matern-5/2,
d = 20, at N = 2048 (C3's shape) and N = 512; (m, c) = (2, 1), (2, 3) and (3, 1) objectives and constraints under quantile bounds of
the training columns; the front is tools/time_believer_ehvi_sweep.py's (29 points / 30 cells for m = 2, 31 points / 1024 cells for
m = 3).  Per shape, medians over `--reps` runs after a warm-up:
  t1   bogp_sweep_ehvi_constrained over the front's cells, wall and device (HIP events of bogp_last_timing)
  t8   bogp_sweep_believer_ehvi_constrained with q = 8, wall and device (pass 0's events + bogp_believer_ehvi_constrained_last's)
  the cost of one more believed point, (t8 - t1) / 7, and its split into producer, solve, k_believer and k_believer_ehvi_constrained
  f8   the same call feasibility-only (C = 0 in every step): k_believer_ehvi_constrained's own time a launch without a cell loop and
       the 8 (3 + 4 (m + c)) bytes a row it streams in TB/s
No time threshold is fixed: first measurements, to be read beside tools/time_believer_ehvi_sweep.py's and
tools/time_believer_constrained_sweep.py's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib  # noqa: E402

D, M, Q = 20, 1_000_000, 8
INF = float("inf")


def front_of(m, lo, hi):
    """mutually non-dominated rows with distinct coordinates inside [lo, hi] per objective: 29 rows for m = 2, 31 for m = 3"""
    n = 29 if m == 2 else 31
    t = (np.arange(n) + 0.5) / n
    return np.column_stack([lo[k] + (hi[k] - lo[k]) * (t if k < m - 1 else 1.0 - t) for k in range(m)])


def bounds_of(Yc):
    """(-inf, q50], [q25, q75], [q50, +inf) cycling over the constraint columns"""
    lo, hi = [], []
    for k in range(Yc.shape[1]):
        q25, q50, q75 = np.quantile(Yc[:, k], [0.25, 0.5, 0.75])
        a, b = ((-INF, q50), (q25, q75), (q50, INF))[k % 3]
        lo.append(a), hi.append(b)
    return np.array(lo), np.array(hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--shapes", type=str, nargs="+", default=["2,1", "2,3", "3,1"], help="objectives,constraints")
    args = ap.parse_args()
    eng = _lib.Engine(0)
    for N in args.sizes:
        for shape in args.shapes:
            m, c = (int(v) for v in shape.split(","))
            mt = m + c
            rng = np.random.default_rng(N + 10 * m + c)
            X = rng.uniform(-5, 5, size=(N, D))
            Y = np.sin(X @ rng.normal(size=(D, mt)) / 4) * (1.0 + np.arange(mt)) + 0.05 * rng.normal(size=(N, mt))
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, np.r_[np.full(D, 0.01), 0.9], 0.0, False, 0.0)
            eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
            ref = Y[:, :m].min(axis=0) - 0.1
            front = front_of(m, np.quantile(Y[:, :m], 0.3, axis=0), np.quantile(Y[:, :m], 0.9, axis=0))
            lower, upper = _lib.grid_cells(front, ref)
            lo, hi = bounds_of(Y[:, m:])
            rows = {k: [] for k in ("t1_wall", "t1_dev", "t8_wall", "t8_dev", "corr", "solve", "upd", "crit", "f8_wall", "f_crit")}
            for rep in range(args.reps + 1):  # run 0 warms up (allocations, first launches)
                t0 = time.perf_counter()
                eng.sweep_ehvi_constrained(lower, upper, lo, hi)
                t1w = 1e3 * (time.perf_counter() - t0)
                tm = eng.last_timing()
                t1d = tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"]
                t0 = time.perf_counter()
                out = eng.sweep_believer_ehvi_constrained(front, ref, Q, lo, hi)
                t8w = 1e3 * (time.perf_counter() - t0)
                tm = eng.last_timing()
                bl = eng.believer_ehvi_constrained_last()
                t8d = tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"] + bl["corr_ms"] + bl["solve_ms"] + bl["update_ms"] + bl["criterion_ms"]
                t0 = time.perf_counter()
                only = eng.sweep_believer_ehvi_constrained(None, ref, Q, lo, hi, feasibility_only=True)
                f8w = 1e3 * (time.perf_counter() - t0)
                fl = eng.believer_ehvi_constrained_last()
                if rep:
                    for k, v in zip(rows, (t1w, t1d, t8w, t8d, bl["corr_ms"], bl["solve_ms"], bl["update_ms"], bl["criterion_ms"], f8w, fl["criterion_ms"])):
                        rows[k].append(v)
            med = {k: float(np.median(v)) for k, v in rows.items()}
            n_pass = bl["n_passes"]
            assert n_pass == Q - 1 == fl["n_passes"] and len(set(out["best_idx"].tolist())) == Q and out["n_cells"][0] == len(lower)
            assert np.all(only["n_cells"] == 0) and len(set(only["best_idx"].tolist())) == Q
            per_wall, per_dev = (med["t8_wall"] - med["t1_wall"]) / (Q - 1), (med["t8_dev"] - med["t1_dev"]) / (Q - 1)
            kern = med["f_crit"] / n_pass
            nbytes = 8 * (3 + 4 * mt)
            print("N=%d d=%d M=%d objectives=%d constraints=%d q=%d reps=%d cells per step %s" % (N, D, M, m, c, Q, args.reps, out["n_cells"].tolist()))
            print("  t1 bogp_sweep_ehvi_constrained           wall %8.3f ms   device %8.3f ms" % (med["t1_wall"], med["t1_dev"]))
            print("  t8 bogp_sweep_believer_ehvi_constrained  wall %8.3f ms   device %8.3f ms" % (med["t8_wall"], med["t8_dev"]))
            print("  one more believed point                  wall %8.3f ms (%.3f t1)   device %8.3f ms (%.3f t1)"
                  % (per_wall, per_wall / med["t1_wall"], per_dev, per_dev / med["t1_dev"]))
            print("  split per point (events): producer %.3f ms, solve %.3f ms, k_believer %.3f ms, k_believer_ehvi_constrained %.3f ms"
                  % (med["corr"] / n_pass, med["solve"] / Q, med["upd"] / n_pass, med["crit"] / n_pass))
            print("  feasibility only (C = 0): f8 wall %8.3f ms; k_believer_ehvi_constrained %.3f ms a launch, %d B a row, %.2f TB/s"
                  % (med["f8_wall"], kern, nbytes, nbytes * M / (kern * 1e-3) / 1e12), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
