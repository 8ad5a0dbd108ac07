"""Constrained EHVI over the grid of the feasible front's cells (bogp_sweep_ehvi_constrained_grid, k_ehvi_constrained_grid) against the
cell loop (bogp_sweep_ehvi_constrained, k_ehvi_constrained) on the same handle, model and candidates, the two entries ALTERNATED call by
call: d = 20, Matern-5/2, candidates drawn on the device, N = 2048 and N = 512, (m, c) = (2, 1), (2, 3), (3, 1) with the 32-point
fronts of tools/time_constrained_ehvi_sweep.py and (4, 1) with a 20-point front (9261 columns).  Per shape and entry: median wall time
of `--reps` sweeps after one warm-up each and the median T_CRITERIA span (acquisition_ms of bogp_last_timing), each with its spread
(max - min), then the ratio grid / loop.  `--loop-rows`: candidates of the cell loop where the front has more than 2048 columns (the grid
entry always sweeps `--rows`); its figures are scaled to `--rows` in the ratio and marked.
The (3, 1) shape at N = 2048 runs three more times for the rows with P == 0 -- none, about half of them in the generated order (the
share printed), all (lo == hi) --, which the loop skips per wavefront and the grid kernel per row."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, pareto  # noqa: E402

d = 20
INF = float("inf")
SHAPES = [(2, 1, 32), (2, 3, 32), (3, 1, 32), (4, 1, 20)]  # (m, c, front points)


def front(m, P, rng):
    """P mutually non-dominated points above the origin: on the positive part of the unit sphere."""
    Z = np.abs(rng.normal(size=(P, m)))
    return Z / np.linalg.norm(Z, axis=1, keepdims=True)


def alternated(fns, eng, reps):
    """per function (median wall, spread, median criterion span, spread), the functions called in turn"""
    for fn in fns:
        fn()
    wall, crit = [[] for _ in fns], [[] for _ in fns]
    for _ in range(reps):
        for j, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            wall[j].append(1e3 * (time.perf_counter() - t0))
            crit[j].append(eng.last_timing()["acquisition_ms"])
    return [(np.median(w), max(w) - min(w), np.median(c), max(c) - min(c)) for w, c in zip(wall, crit)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--loop-rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    eng = _lib.Engine(0)
    box = np.full(d, -5.0), np.full(d, 5.0)
    for N in (2048, 512):
        X = rng.uniform(-5, 5, size=(N, d))
        for m, c, P in SHAPES:
            Y = np.column_stack([np.sin(X @ rng.normal(size=d) / 4) for _ in range(m + c)])
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, np.r_[np.full(d, 0.01), 0.9], 1e-6, False, 0.0)
            grid = pareto.hypercell_grid(front(m, P, rng), np.full(m, -0.1))
            lower, upper = pareto.expand_grid(grid)
            lo, hi = np.full(c, -INF), np.zeros(c)
            E = sum(grid.n_cells) + len(grid.last_val)
            eng.generate_candidates(*box, a.rows, 7)
            if len(lower) <= 2048:
                g, l = alternated([lambda: eng.sweep_ehvi_constrained_grid(grid, lo, hi), lambda: eng.sweep_ehvi_constrained(lower, upper, lo, hi)], eng, a.reps)
                rows = a.rows
            else:
                (g,) = alternated([lambda: eng.sweep_ehvi_constrained_grid(grid, lo, hi)], eng, a.reps)
                rows = min(a.rows, a.loop_rows)
                eng.generate_candidates(*box, rows, 7)
                (l,) = alternated([lambda: eng.sweep_ehvi_constrained(lower, upper, lo, hi)], eng, a.reps)
            s = a.rows / rows
            print("N=%d m=%d c=%d columns=%d E=%d | grid (%d rows): wall %.2f ms (spread %.2f) criterion %.3f ms (spread %.3f) | loop (%d rows): "
                  "wall %.2f ms (spread %.2f) criterion %.3f ms (spread %.3f) | grid / loop%s: wall %.3f criterion %.4f"
                  % (N, m, c, len(lower), E, a.rows, g[0], g[1], g[2], g[3], rows, l[0], l[1], l[2], l[3],
                     "" if s == 1 else " (loop x %g)" % s, g[0] / (s * l[0]), g[2] / (s * l[2])), flush=True)  # fmt: skip
            if (N, m, c) != (2048, 3, 1):
                continue
            # P == 0 exactly where (lo - mu) / sd exceeds about 38.5 (Phi underflows)
            _, _, _, mu, mse = eng.sweep_ehvi_constrained(np.zeros((0, m)), np.zeros((0, m)), lo, hi, return_pof=True, return_moments=True)
            reach = mu[:, m] + 38.6 * np.sqrt(mse[:, m])
            for name, slo, shi in [("no row", [-INF], [INF]), ("about half", [float(np.median(reach))], [INF]), ("every row (lo == hi)", [0.25], [0.25])]:
                g, l = alternated([lambda: eng.sweep_ehvi_constrained_grid(grid, slo, shi), lambda: eng.sweep_ehvi_constrained(lower, upper, slo, shi)], eng, a.reps)
                share = float(np.mean(eng.sweep_ehvi_constrained_grid(grid, slo, shi, return_pof=True)[2] == 0.0))
                print("  dead rows, %s at P == 0 (share %.3f, generated order): grid criterion %.3f ms (spread %.3f) | loop criterion %.3f ms "
                      "(spread %.3f)" % (name, share, g[2], g[3], l[2], l[3]), flush=True)  # fmt: skip
    eng.close()


if __name__ == "__main__":
    main()
