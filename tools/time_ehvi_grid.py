"""EHVI sweep over the grid of the front's cells (bogp_sweep_ehvi_grid) against the cell loop (bogp_sweep_ehvi) on the same handle,
model and candidates: d = 20, Matern-5/2, candidates drawn on the device, at N = 2048 and N = 512, for fronts of
(m, columns) = (2, 30), (3, 1024) and (4, 9261).  Per shape and entry: median wall time of `--reps` sweeps after one warm-up and
the median T_CRITERIA span (acquisition_ms of bogp_last_timing: k_ehvi or k_ehvi_grid), each with its spread (max - min), then the
ratio grid / loop of both.  `--loop-rows`: candidates of the cell loop where the front has more than 2048 columns (the grid entry
always sweeps `--rows`); its figures are scaled to `--rows` in the ratio and marked."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, pareto  # noqa: E402

d = 20
SHAPES = [(2, 29), (3, 31), (4, 20)]  # (m, front points): 30, 32^2 = 1024 and 21^3 = 9261 columns


def front(m, P, rng):
    """P mutually non-dominated points above the origin: on the positive part of the unit sphere."""
    Z = np.abs(rng.normal(size=(P, m)))
    return Z / np.linalg.norm(Z, axis=1, keepdims=True)


def timed(fn, eng, reps):
    fn()
    wall, crit = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        crit.append(eng.last_timing()["acquisition_ms"])
    return np.median(wall), max(wall) - min(wall), np.median(crit), max(crit) - min(crit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--loop-rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    eng = _lib.Engine(0)
    for N in (2048, 512):
        X = rng.uniform(-5, 5, size=(N, d))
        for m, P in SHAPES:
            Y = np.column_stack([np.sin(X @ rng.normal(size=d) / 4) for _ in range(m)])
            eng.set_train(X, Y)
            eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, np.r_[np.full(d, 0.01), 0.9], 1e-6, False, 0.0)
            F = front(m, P, rng)
            ref = np.full(m, -0.1)
            grid = pareto.hypercell_grid(F, ref)
            lo, hi = pareto.expand_grid(grid)
            eng.generate_candidates(np.full(d, -5.0), np.full(d, 5.0), a.rows, 7)
            g = timed(lambda: eng.sweep_ehvi_grid(grid), eng, a.reps)
            rows = a.rows if len(lo) <= 2048 else min(a.rows, a.loop_rows)
            if rows != a.rows:
                eng.generate_candidates(np.full(d, -5.0), np.full(d, 5.0), rows, 7)
            c = timed(lambda: eng.sweep_ehvi(lo, hi), eng, a.reps)
            s = a.rows / rows
            print("N=%d m=%d columns=%d E=%d | grid (%d rows): wall %.2f ms (spread %.2f) criterion %.3f ms (spread %.3f) | loop (%d rows): wall %.2f ms "
                  "(spread %.2f) criterion %.3f ms (spread %.3f) | grid / loop%s: wall %.3f criterion %.4f"
                  % (N, m, len(lo), sum(grid.n_cells) + len(grid.last_val), a.rows, g[0], g[1], g[2], g[3], rows, c[0], c[1], c[2], c[3],
                     "" if s == 1 else " (loop x %g)" % s, g[0] / (s * c[0]), g[2] / (s * c[2])), flush=True)  # fmt: skip
    eng.close()


if __name__ == "__main__":
    main()
