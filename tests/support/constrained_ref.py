"""TEST-ONLY: NumPy restatement of the feasibility-weighted criteria of `bogp_sweep_constrained` (include/bogp.h) from given
moments, with scipy's `ndtr`.  Target 0 is the objective, target k >= 1 a constraint feasible in [lo[k - 1], hi[k - 1]]:

    sd_k  = sqrt(MSE_k)                                   (no floor)
    PoF_k = [lo <= mu_k <= hi]                            if sd_k / sqrt(sigma2_k) < 1e-6   (EI's guard, acquisition_fun.py:153-176)
          = ndtr(-za) - ndtr(-zb) if za > 0 else ndtr(zb) - ndtr(za),   za = (lo - mu_k) / sd_k, zb = (hi - mu_k) / sd_k
    P     = 1; for k = 1 .. m - 1: P *= PoF_k             (this order)
    value = base * P,  base = the oracle's criterion on target 0, or 1 for ACQ_NONE
"""
import numpy as np
from scipy.special import ndtr

from oracle import gp_oracle as O

ACQ_NONE = -1
ALLOWED = (O.ACQ_EI, O.ACQ_EPSILON_PI, O.ACQ_MGFI, ACQ_NONE)


def feasibility(mu, mse, sigma2, lo, hi):
    """PoF of one constraint for every row: mu, mse (M,), sigma2, lo, hi scalars."""
    mu, mse = np.asarray(mu, float), np.asarray(mse, float)
    with np.errstate(all="ignore"):
        sd = np.sqrt(mse)
        guard = sd / np.sqrt(sigma2) < 1e-6
        za, zb = (lo - mu) / sd, (hi - mu) / sd
        tail = ndtr(-za) - ndtr(-zb)
        body = ndtr(zb) - ndtr(za)
    return np.where(guard, ((lo <= mu) & (mu <= hi)).astype(float), np.where(za > 0, tail, body))


def check(acq, lo, hi):
    for a, _ in acq:
        if a == O.ACQ_UCB:
            raise ValueError("UCB changes sign: its product with a probability orders nothing")
        if a not in ALLOWED:
            raise ValueError("unknown acquisition id %r" % (a,))
    lo, hi = np.asarray(lo, float).ravel(), np.asarray(hi, float).ravel()
    if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(hi < lo):
        raise ValueError("bounds must not be NaN, and hi >= lo")
    return lo, hi


def constrained(mu, mse, sigma2, lo, hi, acq, plugin, minimize):
    """(values (q, M), P (M,)) from moments mu, mse (M, m), sigma2 (m,), bounds lo, hi (m - 1,), criteria acq = [(id, par)]."""
    mu, mse, sigma2 = np.atleast_2d(np.asarray(mu, float)), np.atleast_2d(np.asarray(mse, float)), np.asarray(sigma2, float).ravel()
    lo, hi = check(acq, lo, hi)
    m = mu.shape[1]
    assert len(lo) == len(hi) == m - 1 and len(sigma2) == m
    P = np.ones(len(mu))
    for k in range(1, m):
        P = P * feasibility(mu[:, k], mse[:, k], sigma2[k], lo[k - 1], hi[k - 1])
    vals = []
    with np.errstate(all="ignore"):
        for a, par in acq:
            base = np.ones(len(mu)) if a == ACQ_NONE else np.asarray(O.acquisition(a, par, mu[:, 0], mse[:, 0], plugin, sigma2[0], minimize), float).ravel()
            vals.append(base * P)
    return np.array(vals), P


def topk(v, k):
    """(values (k,), indices (k,)) of the k best rows: first maximum, ties to the lower index, NaN maximal; (-inf, -1) beyond M."""
    v = np.asarray(v, float)
    key = np.where(np.isnan(v), np.inf, v)
    order = np.lexsort((np.arange(len(v)), -key))[:k]
    best, idx = np.full(k, -np.inf), np.full(k, -1, dtype=np.int64)
    best[: len(order)], idx[: len(order)] = v[order], order
    return best, idx
