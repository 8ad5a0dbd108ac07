"""TEST-ONLY stand-in for the multi-output forest side of `bogp._lib.Engine`: `forest_engine.ForestEngine` plus a NumPy restatement of
csrc/kernels_forest_ehvi.hip.

A forest with m outputs is one tree structure whose leaves hold m values (`value` (nodes, m)): a row reaches one leaf per tree
(`forest_engine.leaves` on the node indices), the per-tree predictions are (M, T, m), mu is their mean over the trees and MSE
`std(ddof=1) ** 2`, per output (random_forest.py:141-155); EHVI on these moments is `ehvi_ref64.ehvi` (analytic.py:176-274 in float64).
It exercises the host logic where there is no GPU; nothing in the product path can reach it."""
import numpy as np

from bogp import _lib
from support import ehvi_ref64
from support import forest_engine as S


def leaves_multi(forest, X):
    """Per-tree, per-output predictions (M, T, m) of float rows X for forest = (tree_offset, feature, threshold, left, right,
    value (nodes, m), test or None)."""
    off, feat, thr, left, right, val, test = forest
    val = np.asarray(val, dtype=float)
    node = S.leaves((off, feat, thr, left, right, np.arange(len(val), dtype=float), test), X).astype(np.int64)  # global node index of the leaf
    return val[node]


def moments_multi(P):
    return np.mean(P, axis=1), np.std(P, axis=1, ddof=1) ** 2.0


def topk(v, k):
    """(values (k,), indices (k,)): first maximum, NaN maximal, ties to the lower index, slots beyond len(v) are (-inf, -1)."""
    key = np.where(np.isnan(v), np.inf, v)
    order = np.argsort(-key, kind="stable")[:k]
    best, idx = np.full(k, -np.inf), np.full(k, -1, dtype=np.int64)
    best[: len(order)], idx[: len(order)] = v[order], order
    return best, idx


class ForestEhviEngine(S.ForestEngine):
    forest_m = 0

    def forest_set(self, d, tree_offset, feature, threshold, left, right, value, test=None):
        super().forest_set(d, tree_offset, feature, threshold, left, right, value, test)
        self.forest_m = 1

    def forest_set_multi(self, d, m, tree_offset, feature, threshold, left, right, value, test=None):
        if not 2 <= int(m) <= _lib.MAX_TARGETS:
            raise _lib.BogpError(_lib.ERR_INVALID, "bogp_forest_set_multi: m = %d outputs outside [2, %d]" % (m, _lib.MAX_TARGETS))
        value = np.asarray(value, dtype=float)
        if value.shape != (len(np.asarray(left)), int(m)):
            raise ValueError("value must have the shape (nodes, m)")
        f = (np.asarray(tree_offset, np.int64), np.asarray(feature, np.int64), np.asarray(threshold, float), np.asarray(left, np.int64),
             np.asarray(right, np.int64), value, None if test is None else np.asarray(test, np.int64))
        S.validate(int(d), *f)
        if int(d) != self.d:
            self.M = 0
        self.forest, self.d, self.forest_T, self.forest_m = f, int(d), len(f[0]) - 1, int(m)
        self.calls.append("forest_set_multi")

    def forest_outputs(self):
        return self.forest_m

    def _one(self, who):
        self._need()
        if self.forest_m > 1:
            raise _lib.BogpError(_lib.ERR_UNSUPPORTED, "%s: the forest has %d outputs" % (who, self.forest_m))

    def _multi(self, who):
        self._need()
        if self.forest_m < 2:
            raise _lib.BogpError(_lib.ERR_UNSUPPORTED, "%s: the forest has one output" % who)

    def forest_leaves(self, first_row, n):
        self._one("bogp_forest_leaves")
        return super().forest_leaves(first_row, n)

    def forest_predict(self, eval_MSE=True):
        self._one("bogp_forest_predict")
        return super().forest_predict(eval_MSE)

    def forest_sweep_topk(self, acq, plugin, minimize=True, k=1, return_values=False):
        self._one("bogp_forest_sweep_topk")
        return super().forest_sweep_topk(acq, plugin, minimize, k, return_values)

    def forest_leaves_multi(self, first_row, n):
        self._multi("bogp_forest_leaves_multi")
        return leaves_multi(self.forest, self.Xs[first_row : first_row + n])

    def forest_predict_multi(self, eval_MSE=True):
        self._multi("bogp_forest_predict_multi")
        mu, mse = moments_multi(leaves_multi(self.forest, self.Xs))
        return mu, (mse if eval_MSE else None)

    def forest_sweep_ehvi(self, lower, upper, k=1, return_values=False, return_moments=False):
        self._multi("bogp_forest_sweep_ehvi")
        lower, upper = np.asarray(lower, float), np.asarray(upper, float)
        if lower.shape != upper.shape or lower.ndim != 2 or lower.shape[1] != self.forest_m:
            raise _lib.BogpError(_lib.ERR_INVALID, "bogp_forest_sweep_ehvi: m = %d but the forest has %d outputs" % (lower.shape[-1], self.forest_m))
        mu, mse = moments_multi(leaves_multi(self.forest, self.Xs))
        vals = ehvi_ref64.ehvi(mu, mse, lower, upper)
        out = topk(vals, int(k))
        self.calls.append("sweep_ehvi")
        if return_values:
            out += (vals,)
        if return_moments:
            out += (mu, mse)
        return out
