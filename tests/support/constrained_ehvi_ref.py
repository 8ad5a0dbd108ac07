"""TEST-ONLY: NumPy restatement of the feasibility-weighted EHVI of `bogp_sweep_ehvi_constrained` (include/bogp.h) from given
moments.  Targets 0 .. m - 1 are the objectives, target m + j a constraint feasible in [lo[j], hi[j]]:

    P     = 1; for j = 0 .. c - 1: P *= feasibility(mu, MSE, sigma2 of target m + j, lo_j, hi_j)   (support.constrained_ref, this order)
    E     = support.ehvi_ref64.ehvi of the objective columns over the cells (lower, upper)
    value = 0 where P == 0;  otherwise E P for C >= 1 cells;  otherwise P for C == 0 (the probability of feasibility alone)
"""
import numpy as np

from support.constrained_ref import feasibility, topk  # noqa: F401  (topk: for the stand-in engine)
from support.ehvi_ref64 import ehvi


def values(mu, mse, sigma2, m, lower, upper, lo, hi):
    """(value (M,), P (M,)) from moments mu, mse (M, m + c), sigma2 (m + c,), cells lower, upper (C, m), bounds lo, hi (c,)."""
    mu, mse, sigma2 = np.atleast_2d(np.asarray(mu, float)), np.atleast_2d(np.asarray(mse, float)), np.asarray(sigma2, float).ravel()
    lo, hi = np.asarray(lo, float).ravel(), np.asarray(hi, float).ravel()
    m = int(m)
    c = mu.shape[1] - m
    assert m >= 2 and c >= 1 and len(lo) == len(hi) == c and len(sigma2) == m + c
    if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(hi < lo):
        raise ValueError("bounds must not be NaN, and hi >= lo")
    P = np.ones(len(mu))
    for j in range(c):
        P = P * feasibility(mu[:, m + j], mse[:, m + j], sigma2[m + j], lo[j], hi[j])
    lower, upper = np.asarray(lower, float).reshape(-1, m), np.asarray(upper, float).reshape(-1, m)
    if len(lower) == 0:
        v = P.copy()
    else:
        with np.errstate(all="ignore"):
            v = ehvi(mu[:, :m], mse[:, :m], lower, upper) * P
    return np.where(P == 0.0, 0.0, v), P
