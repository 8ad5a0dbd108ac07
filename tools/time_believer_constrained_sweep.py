"""Kriging-believer batches under modelled constraints (bogp_sweep_believer_constrained, q = 8, EI) against one constrained sweep
(bogp_sweep_constrained) on the same handle and candidates: 1e6 candidates generated on the device, Matern-5/2, d = 20, at N = 2048
(C3's shape) and N = 512, with 1 and 3 constraints (m = 2 and 4 targets) under quantile bounds of the training columns.  Per shape,
medians over `--reps` runs after a warm-up:
  t1   bogp_sweep_constrained with one criterion, wall and device (HIP events of bogp_last_timing)
  t8   bogp_sweep_believer_constrained with q = 8, wall and device (pass 0's events + bogp_believer_constrained_last's)
  the cost of one more believed point, (t8 - t1) / 7, and its split into producer, solve, k_believer and k_believer_constrained;
  k_believer_constrained's own time a launch and the 8 (3 + 4 m) bytes a row it streams in TB/s
  s8   bogp_sweep_believer (the single-target believer, q = 8, EI) on column 0 of the same data, and ITS cost of one more point from the
       events of bogp_believer_last (producer + k_believer a pass, one solve), beside the same sum of this call
The design holds if one more point costs less than t1 -- otherwise q constrained sweeps would do."""
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


def bounds_of(Y):
    """(-inf, q50], [q25, q75], [q50, +inf) cycling over the constraint columns"""
    lo, hi = [], []
    for k in range(1, Y.shape[1]):
        q25, q50, q75 = np.quantile(Y[:, k], [0.25, 0.5, 0.75])
        a, b = ((-INF, q50), (q25, q75), (q50, INF))[(k - 1) % 3]
        lo.append(a), hi.append(b)
    return np.array(lo), np.array(hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--constraints", type=int, nargs="+", default=[1, 3])
    args = ap.parse_args()
    eng = _lib.Engine(0)
    acq = [(_lib.ACQ_EI, 0.0)] * Q
    par = np.r_[np.full(D, 0.01), 0.9]
    for N in args.sizes:
        for n_con in args.constraints:
            m = n_con + 1
            rng = np.random.default_rng(N + m)
            X = rng.uniform(-5, 5, size=(N, D))
            Y = np.sin(X @ rng.normal(size=(D, m)) / 4) * (1.0 + np.arange(m)) + 0.05 * rng.normal(size=(N, m))
            lo, hi = bounds_of(Y)
            ok = np.all((Y[:, 1:] >= lo) & (Y[:, 1:] <= hi), axis=1)
            plugin = float(Y[ok, 0].min())
            # the single-target believer on column 0, same data and candidates
            eng.set_train(X, Y[:, 0])
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, par, 0.0, False, 0.0)
            eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
            s8, sp = [], []  # (its pass 0 is the unpruned sweep, which bogp_sweep does not run here: the cost of a point is read from its events)
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                eng.sweep_believer(acq, plugin, True)
                b = 1e3 * (time.perf_counter() - t0)
                sl = eng.believer_last()
                if rep:
                    s8.append(b), sp.append((sl["corr_ms"] + sl["believer_ms"]) / sl["n_passes"] + sl["solve_ms"] / Q)
            single = float(np.median(sp))
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, par, 0.0, False, 0.0)
            eng.generate_candidates(np.full(D, -5.0), np.full(D, 5.0), M, 7)
            rows = {k: [] for k in ("t1_wall", "t1_dev", "t8_wall", "t8_dev", "corr", "solve", "upd", "crit")}
            for rep in range(args.reps + 1):  # run 0 warms up (allocations, first launches)
                t0 = time.perf_counter()
                eng.sweep_constrained(acq[:1], plugin, True, lo, hi)
                t1w = 1e3 * (time.perf_counter() - t0)
                tm = eng.last_timing()
                t1d = tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"]
                t0 = time.perf_counter()
                out = eng.sweep_believer_constrained(acq, plugin, True, lo, hi)
                t8w = 1e3 * (time.perf_counter() - t0)
                tm = eng.last_timing()
                bl = eng.believer_constrained_last()
                t8d = tm["corr_ms"] + tm["contract_ms"] + tm["acquisition_ms"] + bl["corr_ms"] + bl["solve_ms"] + bl["update_ms"] + bl["criterion_ms"]
                if rep:
                    for k, v in zip(rows, (t1w, t1d, t8w, t8d, bl["corr_ms"], bl["solve_ms"], bl["update_ms"], bl["criterion_ms"])):
                        rows[k].append(v)
            med = {k: float(np.median(v)) for k, v in rows.items()}
            n_pass = bl["n_passes"]
            assert n_pass == Q - 1 and len(set(out["best_idx"].tolist())) == Q
            per_wall, per_dev = (med["t8_wall"] - med["t1_wall"]) / (Q - 1), (med["t8_dev"] - med["t1_dev"]) / (Q - 1)
            kern = med["crit"] / n_pass
            print("N=%d d=%d M=%d constraints=%d (m=%d) q=%d reps=%d plugins %s" % (N, D, M, n_con, m, Q, args.reps, np.round(out["plugins"], 4).tolist()))
            print("  t1 bogp_sweep_constrained           wall %8.3f ms   device %8.3f ms" % (med["t1_wall"], med["t1_dev"]))
            print("  t8 bogp_sweep_believer_constrained  wall %8.3f ms   device %8.3f ms" % (med["t8_wall"], med["t8_dev"]))
            print("  one more believed point             wall %8.3f ms (%.3f t1)   device %8.3f ms (%.3f t1)"
                  % (per_wall, per_wall / med["t1_wall"], per_dev, per_dev / med["t1_dev"]))
            print("  split per point (events): producer %.3f ms, solve %.3f ms, k_believer %.3f ms, k_believer_constrained %.3f ms"
                  % (med["corr"] / n_pass, med["solve"] / Q, med["upd"] / n_pass, kern))
            print("  k_believer_constrained: %.3f ms a launch, %d B a row, %.2f TB/s" % (kern, 8 * (3 + 4 * m), 8 * (3 + 4 * m) * M / (kern * 1e-3) / 1e12))
            print("  single-target believer (bogp_sweep_believer, column 0): s8 wall %8.3f ms, one more point (events) %8.3f ms;  this call's (events) %8.3f ms"
                  % (float(np.median(s8)), single, (med["corr"] + med["upd"] + med["crit"]) / n_pass + med["solve"] / Q))
            print("  condition (one more point < t1): %s" % ("holds" if per_wall < med["t1_wall"] and per_dev < med["t1_dev"] else "FAILS"), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
