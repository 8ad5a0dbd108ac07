"""TEST-ONLY stand-in for the forest side of `bogp._lib.Engine`: a NumPy traversal with the semantics of csrc/kernels_forest.hip.

A row is rounded to float32; at an inner node it goes left iff `float64(x32[feature]) <= threshold` (test 0, scikit-learn's
Tree.predict) or iff `x32[feature] != threshold` (test 1: a one-hot split rewritten onto the raw column of level indices); a leaf is
`left == -1`.  mu is the mean over the trees and MSE `std(ddof=1) ** 2`, as random_forest.py:150-154 forms them; the criteria are the
oracle's (oracle/gp_oracle.py), with EI's guard for a model without sigma2 (sd / 1e4 < 1e-6).  It exercises the host logic where
there is no GPU; nothing in the product path can reach it."""
import numpy as np

from bogp import _lib
from oracle import gp_oracle as O
from oracle import philox
from support import philox_mixed


def leaves(forest, X, count_visits=False):
    """Per-tree predictions (M, T) of float rows X for forest = (tree_offset, feature, threshold, left, right, value, test or None)."""
    off, feat, thr, left, right, val, test = forest
    x32 = np.asarray(X, dtype=np.float64).astype(np.float32)
    M, T = len(x32), len(off) - 1
    out = np.empty((M, T))
    visits = 0
    rows = np.arange(M)
    for t in range(T):
        o = int(off[t])
        node = np.zeros(M, dtype=np.int64)
        for _ in range(int(off[t + 1]) - o + 1):
            g = o + node
            live = left[g] >= 0
            if not live.any():
                break
            visits += int(live.sum())
            xv = x32[rows, np.where(live, feat[g], 0)]
            if test is None:
                go_left = xv.astype(np.float64) <= thr[g]
            else:
                go_left = np.where(test[g] == 1, xv != thr[g].astype(np.float32), xv.astype(np.float64) <= thr[g])
            node = np.where(live, np.where(go_left, left[g], right[g]), node)
        else:
            raise ValueError("tree %d does not end in leaves" % t)
        out[:, t] = val[o + node]
    return (out, visits) if count_visits else out


def moments(P):
    return np.mean(P, axis=-1), np.std(P, axis=-1, ddof=1) ** 2.0


def validate(d, off, feat, thr, left, right, val, test):
    T = len(off) - 1
    if T < 2:
        raise _lib.BogpError(_lib.ERR_INVALID, "bogp_forest_set: T = %d trees; the variance over the trees (ddof = 1) needs T >= 2" % T)
    for t in range(T):
        o, n = int(off[t]), int(off[t + 1] - off[t])
        seen, stack = {0}, [0]
        while stack:
            u = stack.pop()
            l, r = int(left[o + u]), int(right[o + u])
            if l == -1:
                if r != -1:
                    raise _lib.BogpError(_lib.ERR_INVALID, "bogp_forest_set: half a leaf")
                continue
            if not (0 <= l < n and 0 <= r < n):
                raise _lib.BogpError(_lib.ERR_INVALID, "bogp_forest_set: child outside its tree")
            if l == r or l in seen or r in seen:
                raise _lib.BogpError(_lib.ERR_INVALID, "bogp_forest_set: node already reached (cycle or shared subtree)")
            if not 0 <= int(feat[o + u]) < d:
                raise _lib.BogpError(_lib.ERR_INVALID, "bogp_forest_set: feature outside [0, d)")
            seen.update((l, r))
            stack += [l, r]


class ForestEngine:
    def __init__(self, device=0):
        self.N = self.d = self.M = 0
        self.forest = None
        self.comm_rank = self.comm_world = 0
        self.xform = None
        self.calls = []

    def close(self):
        pass

    def forest_set(self, d, tree_offset, feature, threshold, left, right, value, test=None):
        f = (np.asarray(tree_offset, np.int64), np.asarray(feature, np.int64), np.asarray(threshold, float), np.asarray(left, np.int64),
             np.asarray(right, np.int64), np.asarray(value, float), None if test is None else np.asarray(test, np.int64))
        validate(int(d), *f)
        if int(d) != self.d:
            self.M = 0
        self.forest, self.d, self.forest_T = f, int(d), len(f[0]) - 1
        self.calls.append("forest_set")

    def set_candidate_transform(self, scales=None, precisions=None, lo=None, hi=None):
        self.xform = None if scales is None and precisions is None else (scales, precisions, lo, hi)

    def upload_candidates(self, Xs, lazy=False):
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.d:
            raise ValueError("candidates must have shape (M, %d)" % self.d)
        self.Xs, self.M = Xs, len(Xs)
        self.calls.append("upload")

    def generate_candidates_mixed(self, kind, lo, hi, n_levels, M, seed=0, first_row=0):
        kind, nl = np.asarray(kind), np.asarray(n_levels)
        if np.any((kind == _lib.COLUMN_DISCRETE) & (nl <= 0)):
            raise _lib.BogpError(_lib.ERR_INVALID, "bogp_candidates_generate_mixed: n_levels must be > 0")
        X = philox_mixed.mixed_box(lo, hi, np.where(kind == _lib.COLUMN_DISCRETE, nl, 0), int(M), int(seed), int(first_row))
        if self.xform is not None:
            X = philox.transform(X, *self.xform)
        self.Xs, self.M = X, int(M)
        self.calls.append("generate_mixed")

    def read_candidates(self, rows):
        return self.Xs[np.asarray(rows, dtype=np.int64).ravel()].copy()

    def _need(self):
        if self.forest is None:
            raise _lib.BogpError(_lib.ERR_INVALID, "no forest: call bogp_forest_set first")
        if self.M <= 0:
            raise _lib.BogpError(_lib.ERR_INVALID, "no candidates")

    def forest_leaves(self, first_row, n):
        self._need()
        return leaves(self.forest, self.Xs[first_row : first_row + n])

    def forest_predict(self, eval_MSE=True):
        self._need()
        mu, mse = moments(leaves(self.forest, self.Xs))
        return mu, (mse if eval_MSE else None)

    def forest_sweep_topk(self, acq, plugin, minimize=True, k=1, return_values=False):
        self._need()
        mu, mse = moments(leaves(self.forest, self.Xs))
        vals = np.array([O.acquisition(a, p, mu, mse, plugin, 1e8, minimize) for a, p in acq])
        q = len(acq)
        best, idx = np.full((q, k), -np.inf), np.full((q, k), -1, dtype=np.int64)
        for c in range(q):
            order = np.argsort(-vals[c], kind="stable")[:k]  # ties -> lower index
            best[c, : len(order)], idx[c, : len(order)] = vals[c][order], order
        self.calls.append("sweep")
        return (best, idx, vals) if return_values else (best, idx)
