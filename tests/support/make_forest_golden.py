"""Writes tests/golden/G40_forest.npz from the imported reference (run on a machine that has the reference tree and scikit-learn;
never on the GPU machine).  Data only.

Two reference `RandomForest` models (surrogate/random_forest.py:63-155), fitted by scikit-learn:
  "mx_"  a mixed space -- 4 reals, 2 integers, 2 categoricals of 5 levels (16 encoded columns), N = 200, 100 trees;
  "ds_"  an all-discrete space -- 3 integers in 0..3 and one categorical of 3 levels, N = 60, 20 trees -- whose M candidates repeat
         rows, so that exact ties occur.
Per model: the packed arrays (tree_offset, feature, threshold, left, right, value: scikit-learn's `tree_` arrays concatenated), the
column map (d_raw, cat_idx, cat_sizes), y's variance and minimum, M candidates as ENCODED float32 rows (`_check_X`, then the float32
cast of `_validate_X_predict`), the reference's mu / MSE of every row (`predict(eval_MSE=True)`), the per-tree predictions of the
first 256 rows (`estimators_[t].predict`), the reference's own EI / EpsilonPI / UCB / MGFI through its classes for the first rows
(one row per call; `PI` cannot be built in the reference -- its constructor sets epsilon = 0, which the setter's assert rejects -- so
the PI column is EpsilonPI's formula at epsilon = 0 on the reference's moments), and argmax / top 16 per criterion over all M rows from
the reference's moments with the oracle's criterion formulas (oracle/gp_oracle.py), cross-checked against the class values.

Asserted here, so that the reference alone satisfies them (further seeds are tried until they hold):
  * per criterion, consecutive distinct values among the best 17 differ by more than 1e-9 relative (both models);
  * no mixed row has MSE <= 1e-12 var(y);
  * on the all-discrete model at least one criterion's maximum is attained by two or more rows."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), REF, os.path.join(ROOT, "oracle", "shims")]
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

from support import ref_suite_plugin  # noqa: E402

ref_suite_plugin.pytest_configure(None)  # the OneHotEncoder keyword patch

from bayes_optim.acquisition import acquisition_fun as A  # noqa: E402
from bayes_optim.surrogate import RandomForest  # noqa: E402

from oracle import gp_oracle as O  # noqa: E402

CRITERIA = [("EI", O.ACQ_EI, 0.0), ("PI", O.ACQ_EPSILON_PI, 0.0), ("EpsilonPI", O.ACQ_EPSILON_PI, 0.05), ("UCB", O.ACQ_UCB, 0.5),
            ("MGFI", O.ACQ_MGFI, 2.0)]
PAR_NAME = {"EpsilonPI": "epsilon", "UCB": "alpha", "MGFI": "t"}
LEVELS = ["red", "green", "blue", "cyan", "black"]


def rows_mixed(rng, n):
    X = np.empty((n, 8), dtype=object)
    for k in range(4):
        X[:, k] = rng.uniform(-5, 5, n)
    X[:, 4] = rng.integers(0, 11, n)
    X[:, 5] = rng.integers(-3, 4, n)
    X[:, 6] = rng.choice(LEVELS, n)
    X[:, 7] = rng.choice(LEVELS, n)
    return X


def f_mixed(X):
    w = {l: i for i, l in enumerate(LEVELS)}
    return np.array([sum(float(v) ** 2 for v in r[:4]) + 3.0 * abs(r[4] - 5) + 2.0 * r[5] + 4.0 * w[r[6]] - 2.5 * (r[7] == "blue")
                     + 3 * np.sin(float(r[0]) * (1 + w[r[7]])) for r in X])


def rows_discrete(rng, n):
    X = np.empty((n, 4), dtype=object)
    for k in range(3):
        X[:, k] = rng.integers(0, 4, n)
    X[:, 3] = rng.choice(LEVELS[:3], n)
    return X


def f_discrete(X):
    w = {l: i for i, l in enumerate(LEVELS)}
    return np.array([(r[0] - 1) ** 2 + abs(r[1] - 2) + 0.5 * r[2] * w[r[3]] for r in X], dtype=float)


def topk(v, k):
    return np.argsort(-v, kind="stable")[:k]  # ties -> lower index, as np.argmax's first maximum


def gaps_ok(v, k=17):
    best = np.unique(v[topk(v, k)])
    return len(best) < 2 or np.all(np.diff(best) > 1e-9 * np.abs(best[1:]))


def build(prefix, rows, f, levels, N, T, M, n_class, seed):
    rng = np.random.default_rng(seed)
    X = rows(rng, N)
    y = f(X) + rng.normal(0, 0.1, N)
    rf = RandomForest(n_estimators=T, levels=levels, random_state=seed)
    rf.fit(X, y)
    Xc = rows(rng, M)
    enc = np.asarray(rf._check_X(Xc), dtype=np.float64).astype(np.float32)
    mu, mse = rf.predict(Xc, eval_MSE=True)
    per_tree = np.stack([e.predict(enc[:256]) for e in rf.estimators_], axis=1)
    plugin = float(np.min(y))
    out = {}
    cls = np.full((len(CRITERIA), n_class), np.nan)
    for c, (name, aid, par) in enumerate(CRITERIA):
        v = O.acquisition(aid, par, mu, mse, plugin, 1e8, True)  # sigma2 = 1e8: EI's guard sd / 1e4 < 1e-6 is the forest's sd < 1e-10
        if name == "PI":
            cls[c] = v[:n_class]
        else:
            kw = {PAR_NAME[name]: par} if name in PAR_NAME else {}
            crit = getattr(A, name)(model=rf, minimize=True, **kw)
            cls[c] = [float(np.ravel(crit(Xc[i : i + 1]))[0]) for i in range(n_class)]
        np.testing.assert_allclose(v[:n_class], cls[c], rtol=1e-12, atol=1e-300)
        out[prefix + "top16_" + name] = topk(v, 16)
        out[prefix + "acq_" + name] = v
    vals = [out[prefix + "acq_" + n] for n, _, _ in CRITERIA]
    if not all(gaps_ok(v) for v in vals):
        return None
    ties = [int(np.sum(v == v.max())) for v in vals]
    trees = [e.tree_ for e in rf.estimators_]
    off = np.cumsum([0] + [len(t.children_left) for t in trees]).astype(np.int64)
    cat = np.concatenate
    out.update({prefix + k: v for k, v in dict(
        tree_offset=off, feature=cat([t.feature for t in trees]).astype(np.int32), threshold=cat([t.threshold for t in trees]),
        left=cat([t.children_left for t in trees]).astype(np.int32), right=cat([t.children_right for t in trees]).astype(np.int32),
        value=cat([t.value.reshape(-1) for t in trees]), d_raw=X.shape[1], cat_idx=np.array(rf._cat_idx, dtype=np.int64),
        cat_sizes=np.array([len(c) for c in rf._categories], dtype=np.int64), var_y=float(np.var(y)), plugin=plugin,
        Xenc=enc, mu=mu, mse=mse, per_tree=per_tree, class_values=cls, ties=np.array(ties)).items()})
    for n, _, _ in CRITERIA:
        del out[prefix + "acq_" + n]
    return out, ties, float(mse.min()), float(np.var(y)), [float(np.min(np.diff(np.unique(v[topk(v, 17)])), initial=np.inf)) for v in vals]


def main():
    data = {"criteria": np.array([n for n, _, _ in CRITERIA]), "acq_id": np.array([a for _, a, _ in CRITERIA]),
            "acq_par": np.array([p for _, _, p in CRITERIA])}
    lv = {6: LEVELS, 7: LEVELS}
    for seed in range(1, 50):
        r = build("mx_", rows_mixed, f_mixed, lv, 200, 100, 8000, 300, seed)
        if r is not None and r[2] > 1e-12 * r[3]:
            print("mixed: seed %d, min MSE %.4g (var y %.4g), ties %s, smallest gaps among the best 17 %s" % (seed, r[2], r[3], r[1], r[4]))
            data.update(r[0])
            break
    else:
        raise SystemExit("no seed satisfies the mixed conditions")
    for seed in range(1, 200):
        r = build("ds_", rows_discrete, f_discrete, {3: LEVELS[:3]}, 60, 20, 2000, 100, seed)
        if r is not None and max(r[1]) >= 2:
            print("discrete: seed %d, ties at the maximum per criterion %s, smallest gaps %s" % (seed, r[1], r[4]))
            data.update(r[0])
            break
    else:
        raise SystemExit("no seed satisfies the all-discrete conditions")
    path = os.path.join(ROOT, "tests", "golden", "G40_forest.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
