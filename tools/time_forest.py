"""Forest sweep (bogp_forest_sweep_topk, csrc/kernels_forest.hip) at M = 1e6 candidates of a mixed space -- 4 reals, 2 integers,
2 categoricals of 5 levels: 8 raw / 16 encoded columns -- drawn on the device, q = 2 (MGFI + EI), for forests of T = 100 trees
from N = 50, 200, 1000, 2048 training rows and T = 500 at N = 200.  Per case one line: nodes, depth, encoded width, bytes of the
packed forest, LDS of a workgroup; HIP-event time of k_forest alone (moments only, bogp_forest_predict) and inside the sweep (moments +
2 criteria + block argmax), wall time of the whole sweep call -- median [min .. max] over REPS repetitions after WARM warm-up calls;
node visits per second (M x mean visits per row, counted by the CPU stand-in's traversal on 2000 of the device's own rows, over the
kernel time) and the forest bytes every workgroup streams per second.  The trees come from scikit-learn's RandomForestRegressor
(the reference's settings) when it is importable -- then the reference-style CPU predict on 20 000 rows is timed for context -- else
from a NumPy builder of bootstrap trees with random splits and min_samples_leaf = 2 (about 1.4 x scikit-learn's node count at N = 200).
Kernel shares: `rocprofv3 --kernel-trace --stats -- python tools/time_forest.py --quick`."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from bogp import _lib, forest  # noqa: E402
from support import forest_engine  # noqa: E402

M, REPS, WARM = 1_000_000, 25, 3
LEVELS = 5


def rows(rng, n):
    X = np.empty((n, 8))
    X[:, :4] = rng.uniform(-5, 5, size=(n, 4))
    X[:, 4] = rng.integers(0, 11, n)
    X[:, 5] = rng.integers(-3, 4, n)
    X[:, 6:] = rng.integers(0, LEVELS, size=(n, 2))
    return X


def encode(X):
    return np.hstack([X[:, :6]] + [(X[:, [c]] == np.arange(LEVELS)[None, :]).astype(float) for c in (6, 7)])


def target(X):
    return np.sum(X[:, :4] ** 2, 1) + 3 * np.abs(X[:, 4] - 5) + 2 * X[:, 5] + 4 * X[:, 6] - 2.5 * (X[:, 7] == 2) + 3 * np.sin(X[:, 0] * (1 + X[:, 7]))


class _T:
    pass


def numpy_tree(E, y, rng, max_features):
    """One bootstrap tree with random (feature, cut) splits that keep two samples a side."""
    idx0 = rng.integers(0, len(E), len(E))
    feat, thr, left, right, val = [], [], [], [], []

    def grow(idx):
        me = len(feat)
        feat.append(-2), thr.append(-2.0), left.append(-1), right.append(-1), val.append(float(y[idx].mean()))
        if len(idx) >= 4 and np.ptp(y[idx]) > 0:
            for f in rng.permutation(E.shape[1])[:max_features]:
                v = np.sort(E[idx, f])
                cuts = np.flatnonzero(v[2:-1] > v[1:-2]) + 2  # v[c - 1] < v[c], two samples a side
                if len(cuts):
                    c = int(rng.choice(cuts))
                    t = 0.5 * (v[c - 1] + v[c])
                    go = E[idx, f] <= t
                    feat[me], thr[me] = int(f), float(t)
                    left[me] = grow(idx[go])
                    right[me] = grow(idx[~go])
                    break
        return me

    sys.setrecursionlimit(10000)
    grow(idx0)
    t = _T()
    t.feature, t.threshold, t.children_left, t.children_right = np.array(feat), np.array(thr), np.array(left), np.array(right)
    t.value = np.array(val).reshape(-1, 1, 1)
    e = _T()
    e.tree_ = t
    return e


def fit(N, T, seed):
    rng = np.random.default_rng(seed)
    X = rows(rng, N)
    E, y = encode(X), target(X)
    try:
        from sklearn.ensemble import RandomForestRegressor

        m = RandomForestRegressor(n_estimators=T, max_features=5 / 6, min_samples_leaf=2, random_state=seed).fit(E, y)
        how = "scikit-learn"
    except ImportError:
        m = _T()
        m.estimators_ = [numpy_tree(E, y, rng, max(1, int(E.shape[1] * 5 / 6))) for _ in range(T)]
        m.n_outputs_, m.n_features_in_ = 1, E.shape[1]
        how = "numpy builder"
    m._cat_idx, m._categories = [6, 7], [list(range(LEVELS))] * 2
    return m, y, how


def stats(ts):
    return "%.3f [%.3f .. %.3f]" % (float(np.median(ts)), float(np.min(ts)), float(np.max(ts)))


def main():
    cases = [(50, 100), (200, 100), (1000, 100), (2048, 100), (200, 500)]
    if "--quick" in sys.argv:
        cases = [(200, 100)]
    eng = _lib.Engine(0)
    kind, lo, hi, nl = [0] * 4 + [1] * 4, [-5.0] * 4 + [0, -3, 0, 0], [5.0] * 4 + [10, 3, LEVELS - 1, LEVELS - 1], [0] * 4 + [11, 7, LEVELS, LEVELS]
    acq = [(_lib.ACQ_MGFI, 2.0), (_lib.ACQ_EI, 0.0)]
    for N, T in cases:
        model, y, how = fit(N, T, 1)
        pk = forest.pack(model)
        f, t, test = pk.raw()
        eng.forest_set(pk.d_raw, pk.tree_offset, f, t, pk.left, pk.right, pk.value, test)
        info = eng.forest_info()
        eng.generate_candidates_mixed(kind, lo, hi, nl, M, seed=7)
        sample = eng.read_candidates(np.arange(2000))
        _, visits = forest_engine.leaves((pk.tree_offset, f, t, pk.left, pk.right, pk.value, test), sample, count_visits=True)
        per_row = visits / len(sample)
        plugin = float(y.min())
        k_pred, k_sweep, wall = [], [], []
        for r in range(WARM + REPS):
            eng.forest_predict()
            a = eng.last_timing()["acquisition_ms"]
            t0 = time.perf_counter()
            eng.forest_sweep_topk(acq, plugin, True, 1)
            w = 1e3 * (time.perf_counter() - t0)
            b = eng.last_timing()["acquisition_ms"]
            if r >= WARM:
                k_pred.append(a), k_sweep.append(b), wall.append(w)
        kp, ks = float(np.median(k_pred)), float(np.median(k_sweep))
        nblk = (M + 255) // 256
        print("N=%d T=%d (%s): nodes %d leaves %d depth %d, d_raw %d d_enc %d, packed %d bytes, LDS %d bytes/workgroup | k_forest moments %s ms, "
              "with 2 criteria %s ms, sweep call (wall) %s ms | %.1f visits/row -> %.3g node visits/s; forest streamed %.3g bytes/s; %.3g candidates/s"
              % (N, T, how, info["nodes"], info["leaves"], info["depth"], pk.d_raw, pk.d_enc, info["bytes"], info["lds_bytes"], stats(k_pred), stats(k_sweep),
                 stats(wall), per_row, M * per_row / (kp * 1e-3), nblk * info["bytes"] / (kp * 1e-3), M / (ks * 1e-3)), flush=True)
        if how == "scikit-learn":
            E = encode(rows(np.random.default_rng(3), 20000)).astype(np.float32)
            t0 = time.perf_counter()
            P = np.stack([e.predict(E) for e in model.estimators_], 1)
            P.mean(1), P.std(1, ddof=1) ** 2
            print("    CPU context (this machine's CPU, scikit-learn per-tree predict + mean / std, 20 000 rows): %.3f s" % (time.perf_counter() - t0), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
