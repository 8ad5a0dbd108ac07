"""EHVI sweep over a forest with several outputs (bogp_forest_sweep_ehvi, csrc/kernels_forest_ehvi.hip) at M = 1e6 candidates of the
mixed space of tools/time_forest.py (4 reals, 2 integers, 2 categoricals of 5 levels) drawn on the device, against the 100-tree,
N = 200 forest shape of profiles/forest_sweep.txt refitted with m = 2 and m = 3 outputs (y MinMax-scaled and negated, as BaseMOBO.y),
with the cells of a 10-point front.  Beside it, in the same process and on the same rows, the one-output EI sweep
(bogp_forest_sweep_topk) of the forest fitted on the first output.  Per case one line: nodes, leaves, words of the largest tree, LDS
of a workgroup, cells; HIP-event time of the kernel inside the sweep call (bogp_last_timing) and of the moments alone
(bogp_forest_predict[_multi]), wall time of the whole call -- median [min .. max] over REPS repetitions after WARM warm-up calls; the
ratio to the one-output sweep, and what the time above the one-output sweep costs per evaluation of G (2 m C of them a row).
Kernel shares: `rocprofv3 --kernel-trace --stats -- python tools/time_forest_ehvi.py --quick`."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import time_forest as TF  # noqa: E402
from bogp import _lib, forest, pareto  # noqa: E402

M, REPS, WARM = 1_000_000, 15, 3
N, T = 200, 100


def objectives(X):
    f1 = TF.target(X)
    f2 = np.sum((X[:, :4] + 1.0) ** 2, 1) + 1.5 * X[:, 4] + 4.0 * (X[:, 6] == 1) - 2.0 * X[:, 7]
    f3 = np.sum(np.abs(X[:, :4]), 1) + 3 * np.sin(X[:, 0] * (1 + X[:, 6])) + 0.5 * (10 - X[:, 4]) + X[:, 5]
    Y = np.column_stack([f1, f2, f3])
    return -(Y - Y.min(0)) / (Y.max(0) - Y.min(0))  # mobo.py:66-76 with minimize=True


def fit(m, seed=1):
    from sklearn.ensemble import RandomForestRegressor

    rng = np.random.default_rng(seed)
    X = TF.rows(rng, N)
    y = objectives(X)[:, :m]
    model = RandomForestRegressor(n_estimators=T, max_features=5 / 6, min_samples_leaf=2, random_state=seed).fit(TF.encode(X), y[:, 0] if m == 1 else y)
    model._cat_idx, model._categories = [6, 7], [list(range(TF.LEVELS))] * 2
    return model, y


def front(m, P=10):
    """P mutually non-dominated points of [-1, 0]^m (maximised) and the cells of the region they do not dominate."""
    t = (np.arange(P) + 0.5) / P
    Y = -np.column_stack([t, 1.0 - t] if m == 2 else [t, (1.0 - t) * (0.3 + 0.7 * ((np.arange(P) * 7) % P) / P), 1.0 - t * t])[:, :m]
    assert pareto.is_non_dominated(Y).all()
    ref = np.full(m, -1.0) * 1.1
    return pareto.hypercell_bounds(Y, ref)


def timed(call, eng):
    k, wall = [], []
    for r in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        w = 1e3 * (time.perf_counter() - t0)
        if r >= WARM:
            k.append(eng.last_timing()["acquisition_ms"]), wall.append(w)
    return k, wall


def main():
    quick = "--quick" in sys.argv
    eng = _lib.Engine(0)
    L = TF.LEVELS
    kind, lo, hi, nl = [0] * 4 + [1] * 4, [-5.0] * 4 + [0, -3, 0, 0], [5.0] * 4 + [10, 3, L - 1, L - 1], [0] * 4 + [11, 7, L, L]
    base = None
    for m in ((2,) if quick else (1, 2, 3)):
        model, y = fit(m)
        pk = forest.pack(model, multi_output=True)
        f, t, test = pk.raw()
        if m == 1:
            eng.forest_set(pk.d_raw, pk.tree_offset, f, t, pk.left, pk.right, pk.value, test)
        else:
            eng.forest_set_multi(pk.d_raw, m, pk.tree_offset, f, t, pk.left, pk.right, pk.value, test)
        if eng.M != M:
            eng.generate_candidates_mixed(kind, lo, hi, nl, M, seed=7)  # the same rows for every case: a forest of the same d keeps them
        info = eng.forest_info()
        if m == 1:
            k_mom, _ = timed(lambda: eng.forest_predict(eval_MSE=False), eng)
            k_sw, wall = timed(lambda: eng.forest_sweep_topk([(_lib.ACQ_EI, 0.0)], float(y.min()), True, 1), eng)
            base = float(np.median(k_sw))
            print("m=1 EI (bogp_forest_sweep_topk): nodes %d leaves %d depth %d, LDS %d bytes/workgroup | kernel in the sweep %s ms, moments alone %s ms, "
                  "sweep call (wall) %s ms | %.3g candidates/s"
                  % (info["nodes"], info["leaves"], info["depth"], info["lds_bytes"], TF.stats(k_sw), TF.stats(k_mom), TF.stats(wall), M / (base * 1e-3)), flush=True)
            continue
        lower, upper = front(m)
        C = len(lower)
        k_mom, _ = timed(lambda: eng.forest_predict_multi(eval_MSE=False), eng)
        k_sw, wall = timed(lambda: eng.forest_sweep_ehvi(lower, upper, k=1), eng)
        ks = float(np.median(k_sw))
        line = ("m=%d EHVI (bogp_forest_sweep_ehvi): nodes %d leaves %d depth %d, LDS %d bytes/workgroup, %d cells (%d upper bounds +inf) | kernel in the sweep "
                "%s ms, moments alone %s ms, sweep call (wall) %s ms | %.3g candidates/s"
                % (m, info["nodes"], info["leaves"], info["depth"], info["lds_bytes"], C, int(np.isinf(upper).sum()), TF.stats(k_sw), TF.stats(k_mom),
                   TF.stats(wall), M / (ks * 1e-3)))
        if base is not None:
            line += (" | %.2f x the one-output EI sweep; the %.3f ms above it over 2 m C = %d evaluations of G a row: %.3g G/s"
                     % (ks / base, ks - base, 2 * m * C, M * 2.0 * m * C / max((ks - base) * 1e-3, 1e-12)))
        print(line, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
