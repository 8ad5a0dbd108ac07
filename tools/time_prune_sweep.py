"""What the pruned sweep (csrc/kernels_prune.hip) costs and saves on ONE engine, three modes interleaved: pruning
off, the per-chunk path (Engine.set_prune("chunks")) and the automatic mode (one bounding pass where it applies, section 5.22.1):
  c3    the benchmark's C3 sweep (N = 2048, d = 20, M = 1e6, MGFI(t = 2) + EI): wall time of a step, the kernel split of
        bogp_last_timing and the rows that went through the contraction
  flat  the worst case: the same sizes with a criterion that prunes nothing (UCB, alpha = 50) -- every chunk is bounded, then
        contracted in place (the automatic mode gets there after its pilot estimate); what leaving the option on costs there
  bo    use, not benchmark: a BO trajectory on Rastrigin (d = 10, a 600-point design, 40 iterations, the model of
        tools/time_bo_loop.py re-fitted every tenth iteration, EI over 1e5 device-generated candidates): contracted fraction per
        iteration, path and time of each mode.  (Below N = 513 a sweep is ONE fused launch and never pruned: the trajectory starts above it.)
usage: python tools/time_prune_sweep.py [c3] [flat] [bo]   (default: all three)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bogp
from bogp import _lib


def c3_engine():
    rng = np.random.default_rng(0)  # bench.py's C3 model
    N, d, M = 2048, 20, 1_000_000
    X = rng.uniform(-5, 5, size=(N, d))
    y = np.sum(X**2, axis=1)
    y = ((y - y.mean()) / y.std()).reshape(-1, 1)
    eng = _lib.Engine(0)
    eng.set_train(X, y)
    eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISY, np.r_[np.full(d, 0.01), 0.9], 1e-6, False, 0.0)
    eng.generate_candidates(np.full(d, -5.0), np.full(d, 5.0), M, seed=1234)
    return eng, float(y.min()), M


MODES = (False, "chunks", True)
NAMES = {False: "off", "chunks": "chunks", True: "auto"}
PATHS = {_lib.PRUNE_PATH_NONE: "none", _lib.PRUNE_PATH_CHUNKS: "per-chunk", _lib.PRUNE_PATH_ONEPASS: "one-pass",
         _lib.PRUNE_PATH_ONEPASS_FALLBACK: "one-pass, a segment fell back"}  # fmt: skip


def timed(eng, acq, plugin, reps=10, warm=3):
    ms = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        best, idx = eng.sweep(acq, plugin, True)
        if r >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    return np.array(ms), best, idx, eng.last_timing(), eng.last_contracted_rows(), eng.last_prune_path()


def compare(eng, acq, plugin, M, label):
    rows = {}
    for mode in MODES + MODES:  # interleaved: drift of the clocks shows as a difference between the two runs of a setting
        eng.set_prune(mode)
        ms, best, idx, lt, n, (path, surv, rounds) = timed(eng, acq, plugin)
        rows.setdefault(mode, []).append((ms, best, idx))
        # (the kernel split is the last step's event times: wall minus their sum = launch gaps and host waits outside the first and last event)
        print("%s prune %-6s: step min / median / max %.2f / %.2f / %.2f ms; corr %.2f, contract %.2f, acquisition %.2f ms (%d contraction launches / chunks); "
              "contracted %d of %d rows (%.3f %%); path %s, %d survivors in %d rounds"
              % (label, NAMES[mode], ms.min(), np.median(ms), ms.max(), lt["corr_ms"], lt["contract_ms"], lt["acquisition_ms"], lt["n_chunks"], n, M,
                 100.0 * n / M, PATHS[path], surv, rounds))  # fmt: skip
    same = all(r[1].tobytes() == rows[False][0][1].tobytes() and np.array_equal(r[2], rows[False][0][2]) for v in rows.values() for r in v)
    print("%s winners identical (bits) in all three modes: %s" % (label, same))


def bo_trajectory(dim=10, n_doe=600, iters=40, M=100_000, seed=1):
    f = lambda x: float(10 * len(x) + np.sum(np.asarray(x) ** 2 - 10 * np.cos(2 * np.pi * np.asarray(x))))  # noqa: E731
    lo, hi = -5.12, 5.12
    rng = np.random.default_rng(seed)
    np.random.seed(seed)
    X = rng.uniform(lo, hi, size=(n_doe, dim))
    y = np.array([f(x) for x in X])
    rng_len = np.full(dim, hi - lo)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(dim), corr="matern", thetaL=1e-3 * rng_len, thetaU=1e3 * rng_len,
                                 nugget=1e-6, optimizer="BFGS", wait_iter=3, random_start=3, eval_budget=300)  # fmt: skip
    par = None
    for it in range(iters):
        ys = ((y - y.mean()) / y.std()).reshape(-1, 1)
        if it % 10 == 0:
            model.fit(X, ys)
            par = np.array(model._committed_par, dtype=float)  # what the fit committed: pinned until the next fit
        else:
            model.set_state(par, X, ys)
        eng = model.engine
        eng.generate_candidates(np.full(dim, lo), np.full(dim, hi), M, seed=100 + it)
        pl = float(ys.min())
        out = {}
        for mode in MODES:
            eng.set_prune(mode)
            t0 = time.perf_counter()
            best, idx = eng.sweep([(_lib.ACQ_EI, 0.0)], pl, True)
            out[mode] = (best, idx, (time.perf_counter() - t0) * 1e3, eng.last_contracted_rows(), eng.last_prune_path()[0])
        same = all(o[0].tobytes() == out[False][0].tobytes() and np.array_equal(o[1], out[False][1]) for o in out.values())
        print("bo iteration %2d, N = %d: contracted %6d (chunks) / %6d (auto: %s) of %d rows (%.2f %%), sweep %.2f (off) -> %.2f (chunks) -> %.2f ms (auto), same winner: %s"
              % (it, len(y), out["chunks"][3], out[True][3], PATHS[out[True][4]], M, 100.0 * out[True][3] / M, out[False][2], out["chunks"][2], out[True][2], same))  # fmt: skip
        x_new = eng.read_candidates(out[True][1])[0]
        X = np.vstack([X, x_new])
        y = np.append(y, f(x_new))


if __name__ == "__main__":
    what = sys.argv[1:] or ["c3", "flat", "bo"]
    if "c3" in what or "flat" in what:
        eng, pl, M = c3_engine()
        if "c3" in what:
            compare(eng, [(_lib.ACQ_MGFI, 2.0), (_lib.ACQ_EI, 0.0)], pl, M, "C3 (MGFI + EI)")
        if "flat" in what:
            compare(eng, [(_lib.ACQ_UCB, 50.0)], pl, M, "flat (UCB, alpha = 50)")
        eng.close()
    if "bo" in what:
        bo_trajectory()
