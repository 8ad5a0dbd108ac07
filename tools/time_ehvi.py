"""EHVI sweep (bogp_sweep_ehvi) against the single-target sweep (bogp_sweep, one EI) on the same handle and candidates, at the
C3 model size (N = 2048, d = 20, Matern-5/2, 1e6 candidates generated on the device): m = 2 (front of 32 points, 33 cells)
and m = 3 (front of 32 points, the grid decomposition's ~1 000 cells).  Prints one line per case: median wall time of
each sweep over 5 repetitions and the kernel-time split of the last EHVI sweep (bogp_last_timing: corr / contract /
acquisition = k_ehvi).  Kernel shares: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_ehvi.py`."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bogp import _lib, pareto  # noqa: E402

N, d, M, P = 2048, 20, 1_000_000, 32


def front(m, rng):
    """P mutually non-dominated points above the origin: on the positive part of the unit sphere."""
    Z = np.abs(rng.normal(size=(P, m)))
    return Z / np.linalg.norm(Z, axis=1, keepdims=True)


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    rng = np.random.default_rng(0)
    X = rng.uniform(-5, 5, size=(N, d))
    eng = _lib.Engine(0)
    for m in (2, 3):
        Y = np.column_stack([np.sin(X @ rng.normal(size=d) / 4) for _ in range(m)])
        eng.set_train(X, Y)
        eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, np.r_[np.full(d, 0.01), 0.9], 1e-6, False, 0.0)
        eng.generate_candidates(np.full(d, -5.0), np.full(d, 5.0), M, 7)
        F = front(m, rng)
        lo, hi = pareto.hypercell_bounds(F, np.full(m, -0.1))
        t_ei = timed(lambda: eng.sweep([(_lib.ACQ_EI, 0.0)], float(Y[:, 0].min()), True))
        t_eh = timed(lambda: eng.sweep_ehvi(lo, hi))
        tm = eng.last_timing()
        print("m=%d cells=%d  sweep(EI) %.2f ms  sweep_ehvi %.2f ms  ratio %.3f  | last EHVI: corr %.2f contract %.2f k_ehvi %.2f ms, %d chunks"
              % (m, len(lo), t_ei, t_eh, t_eh / t_ei, tm["corr_ms"], tm["contract_ms"], tm["acquisition_ms"], tm["n_chunks"]), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
