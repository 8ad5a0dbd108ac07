"""Writes tests/golden/G42_forest_ehvi.npz from the imported reference (run on a machine that has the reference tree, scikit-learn and
torch; never on the GPU machine).  Data only.

Three reference `RandomForest` models (surrogate/random_forest.py:63-155) fitted by scikit-learn on y (N, m) as `BaseMOBO.y` forms it
(mobo.py:66-76: the raw objectives MinMax-scaled, then negated), i.e. one tree structure with m values a leaf:
  "mx2_"  m = 2 on a mixed space -- 3 reals, 1 integer in 0..10, 2 categoricals of 5 and 3 levels -- N = 120, 30 trees, M = 4096;
  "mx3_"  the same with m = 3;
  "ds2_"  m = 2 on an all-discrete space -- 3 integers in 0..3 and one categorical of 3 levels -- N = 60, 20 trees, whose M = 4096
          candidates repeat rows, so that exact ties occur.
Per model: the packed arrays (scikit-learn's `tree_` arrays concatenated, `value` (nodes, m)), the column map (d_raw, cat_idx,
cat_sizes), the M candidates as ENCODED float32 rows (`_check_X`, then the float32 cast of `_validate_X_predict`), the reference's
mu / MSE (M, m) (`predict(eval_MSE=True)`), the per-tree, per-output predictions of the first 256 rows (`estimators_[t].predict`),
ref_point = min(y) * 0.8 (mobo.py:63) and the float64 cells of the reference's `NondominatedPartitioning`, the reference's own EHVI of
the first 256 rows exactly as MOBO builds it (float32 tensors, mobo.py:177-186, one row per call), the float64 values of all rows
from tests/support/ehvi_ref64.py on the reference's moments, and argmax / top 16 of those.

Asserted here, so that the reference alone satisfies them (further seeds are tried until they hold):
  * consecutive distinct values among the best 17 differ by more than 1e-9 relative;
  * the reference's float32 values are within 1e-5 of the batch maximum of the float64 ones;
  * no "mx*_" row has an MSE <= 1e-12;
  * on "ds2_" the maximum is attained by two or more rows."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), REF, os.path.join(ROOT, "oracle", "shims")]
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import sklearn  # noqa: E402
import torch  # noqa: E402
from sklearn.preprocessing import MinMaxScaler  # noqa: E402

from support import ehvi_ref64, ref_suite_plugin  # noqa: E402

ref_suite_plugin.pytest_configure(None)  # the OneHotEncoder keyword patch

from bayes_optim.multi_objective import EHVI  # noqa: E402
from bayes_optim.surrogate import RandomForest  # noqa: E402
from bayes_optim.utils.multi_objective.box_decompositions import NondominatedPartitioning  # noqa: E402

L5 = ["red", "green", "blue", "cyan", "black"]
L3 = ["x", "y", "z"]
N_CLASS = 256


def rows_mixed(rng, n):
    X = np.empty((n, 6), dtype=object)
    for k in range(3):
        X[:, k] = np.round(rng.uniform(-5, 5, n), 2)  # (Real variables of precision 2, as the spaces of unittest/test_mobo.py)
    X[:, 3] = rng.integers(0, 11, n)
    X[:, 4] = rng.choice(L5, n)
    X[:, 5] = rng.choice(L3, n)
    return X


def f_mixed(X):
    w5, w3 = {l: i for i, l in enumerate(L5)}, {l: i for i, l in enumerate(L3)}
    f1 = [sum((float(v) - 1.0) ** 2 for v in r[:3]) + 2.0 * abs(r[3] - 5) + 3.0 * w5[r[4]] for r in X]
    f2 = [sum((float(v) + 1.0) ** 2 for v in r[:3]) + 1.5 * r[3] + 4.0 * (r[5] == "y") - 2.0 * w5[r[4]] for r in X]
    f3 = [sum(abs(float(v)) for v in r[:3]) + 3 * np.sin(float(r[0]) * (1 + w3[r[5]])) + 0.5 * (10 - r[3]) for r in X]
    return np.column_stack([f1, f2, f3])


def rows_discrete(rng, n):
    X = np.empty((n, 4), dtype=object)
    for k in range(3):
        X[:, k] = rng.integers(0, 4, n)
    X[:, 3] = rng.choice(L3, n)
    return X


def f_discrete(X):
    w3 = {l: i for i, l in enumerate(L3)}
    f1 = [(r[0] - 1) ** 2 + abs(r[1] - 2) + 0.5 * r[2] * w3[r[3]] for r in X]
    f2 = [(r[0] - 3) ** 2 + r[1] + (2 - w3[r[3]]) * (3 - r[2]) for r in X]
    return np.column_stack([f1, f2]).astype(float)


def topk(v, k):
    return np.argsort(-v, kind="stable")[:k]  # ties -> lower index, as np.argmax's first maximum


def gaps(v, k=17):
    best = np.unique(v[topk(v, k)])
    return np.diff(best) / np.abs(best[1:]) if len(best) > 1 else np.array([np.inf])


def build(prefix, rows, f, levels, m, N, T, M, seed):
    rng = np.random.default_rng(seed)
    X = rows(rng, N)
    y = MinMaxScaler().fit_transform(f(X)[:, :m] + rng.normal(0, 0.05, (N, m))) * (-1) ** True  # mobo.py:72-76 with minimize=True
    rf = RandomForest(n_estimators=T, levels=levels, random_state=seed)
    rf.fit(X, y)
    assert rf.n_outputs_ == m
    Xc = rows(rng, M)
    enc = np.asarray(rf._check_X(Xc), dtype=np.float64).astype(np.float32)
    mu, mse = rf.predict(Xc, eval_MSE=True)
    per_tree = np.stack([e.predict(enc[:N_CLASS]) for e in rf.estimators_], axis=1)  # (256, T, m)
    assert mu.shape == mse.shape == (M, m) and per_tree.shape == (N_CLASS, T, m)
    P = np.stack([e.predict(enc) for e in rf.estimators_], axis=-1)  # (M, m, T)
    assert np.array_equal(mu, P.mean(-1)) and np.array_equal(mse, P.std(-1, ddof=1) ** 2.0)
    ref_point = np.min(y, axis=0) * 0.8  # mobo.py:63
    part64 = NondominatedPartitioning(ref_point=torch.tensor(ref_point, dtype=torch.float64), Y=torch.tensor(y, dtype=torch.float64))
    lo, hi = (np.asarray(b, dtype=float) for b in part64.get_hypercell_bounds())
    part32 = NondominatedPartitioning(ref_point=torch.Tensor(ref_point), Y=torch.Tensor(y))
    crit = EHVI(model=rf, ref_point=ref_point.tolist(), partitioning=part32)
    ehvi32 = np.array([float(np.ravel(crit(Xc[i : i + 1]))[0]) for i in range(N_CLASS)])
    ehvi64 = ehvi_ref64.ehvi(mu, mse, lo, hi)
    err32 = float(np.max(np.abs(ehvi32 - ehvi64[:N_CLASS])) / np.max(np.abs(ehvi64)))
    gap = float(np.min(gaps(ehvi64)))
    ties = int(np.sum(ehvi64 == ehvi64.max()))
    if not (gap > 1e-9 and err32 <= 1e-5):
        return None
    trees = [e.tree_ for e in rf.estimators_]
    off = np.cumsum([0] + [len(t.children_left) for t in trees]).astype(np.int64)
    cat = np.concatenate
    out = {prefix + k: v for k, v in dict(
        tree_offset=off, feature=cat([t.feature for t in trees]).astype(np.int32), threshold=cat([t.threshold for t in trees]),
        left=cat([t.children_left for t in trees]).astype(np.int32), right=cat([t.children_right for t in trees]).astype(np.int32),
        value=cat([t.value[:, :, 0] for t in trees]), d_raw=X.shape[1], cat_idx=np.array(rf._cat_idx, dtype=np.int64),
        cat_sizes=np.array([len(c) for c in rf._categories], dtype=np.int64), Xenc=enc, mu=mu, mse=mse, per_tree=per_tree,
        ref_point=ref_point, lower=lo, upper=hi, ehvi32=ehvi32, ehvi64=ehvi64, argmax=int(np.argmax(ehvi64)),
        top16=topk(ehvi64, 16), ties=ties).items()}
    stats = dict(seed=seed, cells=len(lo), gap=gap, err32=err32, min_mse=float(mse.min()), ties=ties,
                 nodes=max(len(t.children_left) for t in trees), depth=max(t.max_depth for t in trees))
    return out, stats


def main():
    data = {"versions": np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "scikit-learn " + sklearn.__version__])}
    lv = {4: L5, 5: L3}
    jobs = [("mx2_", rows_mixed, f_mixed, lv, 2, 120, 30, lambda s: s["min_mse"] > 1e-12),
            ("mx3_", rows_mixed, f_mixed, lv, 3, 120, 30, lambda s: s["min_mse"] > 1e-12),
            ("ds2_", rows_discrete, f_discrete, {3: L3}, 2, 60, 20, lambda s: s["ties"] >= 2)]
    for prefix, rows, f, levels, m, N, T, ok in jobs:
        for seed in range(1, 200):
            r = build(prefix, rows, f, levels, m, N, T, 4096, seed)
            if r is not None and ok(r[1]):
                print(prefix, r[1])
                data.update(r[0])
                break
        else:
            raise SystemExit("no seed satisfies the conditions of " + prefix)
    path = os.path.join(ROOT, "tests", "golden", "G42_forest_ehvi.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
