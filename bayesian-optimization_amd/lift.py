"""The linear lift of a reduced search space: PCA-BO's map back to the original box and its box penalty.

`bayes_optim.extension.PCABO` (extension.py:89-208) fits its surrogate on the first r principal components of the (rank
weighted) data and maximises the criterion over a box of that REDUCED space (`_compute_bounds`, :113-119).  Every candidate z
is mapped back, x_ = (z A + mean) + center (`LinearTransform.inverse_transform`, :56-59), and `penalized_acquisition`
(:62-86) returns -sum(violations of the original box) INSTEAD of the criterion whenever x_ leaves the box.  `Lift` holds
(A, mean, center, lo, hi) and restates the map and the penalty in NumPy, operation by operation as `k_lift_penalty`
(csrc/kernels_lift.hip) evaluates them: the sum over the r components in index order, every product and sum rounded on its
own.  The device engine takes the same five arrays (`Engine.set_lift`) for its lifted sweep (`bogp_lift_sweep_topk`)."""
from __future__ import annotations

import numpy as np


class Lift:
    """x_ = (z A + mean) + center and the box [lo, hi] of the original space.  A: (r, D) = `pca.components_`, mean: (D,) =
    `pca.mean_`, center: (D,) = `LinearTransform.center` (None = 0), lo / hi: (D,)."""

    def __init__(self, A, mean, center, lo, hi):
        self.A = np.ascontiguousarray(A, dtype=float)
        if self.A.ndim != 2:
            raise ValueError("A must be an (r, D) array")
        self.r, self.D = self.A.shape
        self.mean = np.asarray(mean, dtype=float).ravel()
        self.center = np.zeros(self.D) if center is None else np.asarray(center, dtype=float).ravel()
        self.lo = np.asarray(lo, dtype=float).ravel()
        self.hi = np.asarray(hi, dtype=float).ravel()
        for name in ("mean", "center", "lo", "hi"):
            if len(getattr(self, name)) != self.D:
                raise ValueError("%s must have D = %d entries" % (name, self.D))
        if not np.all(np.isfinite(self.A)) or not np.all(np.isfinite(self.mean)) or not np.all(np.isfinite(self.center)):
            raise ValueError("A, mean and center must be finite")
        if not np.all(self.lo <= self.hi):  # (NaN bounds fail here too)
            raise ValueError("the box needs lo <= hi in every dimension")

    @classmethod
    def from_pca(cls, pca, bounds) -> "Lift":
        """From a fitted `LinearTransform` / scikit-learn `PCA` and the ORIGINAL box `bounds` (D pairs, or a search space
        with `.bounds`)."""
        if not hasattr(pca, "components_"):
            raise ValueError("the PCA is not fitted (its inverse_transform is the identity, extension.py:57-58): there is nothing to lift")
        b = np.atleast_2d(np.asarray(getattr(bounds, "bounds", bounds), dtype=float))
        return cls(pca.components_, pca.mean_, getattr(pca, "center", None), b[:, 0], b[:, 1])

    def to_original(self, Z) -> np.ndarray:
        """Rows of the reduced space (M, r) -> points of the original space (M, D)."""
        Z = np.atleast_2d(np.asarray(Z, dtype=float))
        if Z.shape[1] != self.r:
            raise ValueError("rows must have r = %d entries" % self.r)
        acc = np.zeros((len(Z), self.D))
        for j in range(self.r):
            acc = acc + Z[:, j : j + 1] * self.A[j]
        return (acc + self.mean) + self.center

    def penalty(self, Z) -> np.ndarray:
        """-(sum_{x_i < lo_i} (lo_i - x_i) + sum_{x_i > hi_i} (x_i - hi_i)) per row: -0.0 for a feasible row (a point ON a
        bound is feasible), negative otherwise (extension.py:66-71)."""
        X = self.to_original(Z)
        s_lo, s_hi = np.zeros(len(X)), np.zeros(len(X))
        with np.errstate(invalid="ignore"):
            for i in range(self.D):
                x = X[:, i]
                s_lo = np.where(x < self.lo[i], s_lo + (self.lo[i] - x), s_lo)
                s_hi = np.where(x > self.hi[i], s_hi + (x - self.hi[i]), s_hi)
        return -1.0 * (s_lo + s_hi)

    def feasible(self, Z) -> np.ndarray:
        """Boolean mask of the rows whose criterion counts (the reference's `penalty == 0`, :73)."""
        return self.penalty(Z) == 0

    def reduced_bounds(self):
        """The box of the reduced space PCA-BO searches: the bounding box of the ball around the original box
        (`PCABO._compute_bounds`, extension.py:113-119), as a list of r (lo, hi) pairs."""
        C = (self.lo + self.hi) / 2
        radius = np.sqrt(np.sum((self.lo - C) ** 2))
        C = C - self.mean - self.center
        C_ = C.dot(self.A.T)
        return [(c - radius, c + radius) for c in C_]
