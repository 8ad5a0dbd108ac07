"""TEST-ONLY NumPy float64 restatement of the feasibility-weighted criteria of `bogp_point_eval_constrained` (include/bogp.h) AND
their input gradients for a multi-target Gaussian process.

Posterior and its input gradients: `ehvi_grad_ref.moments` (one gamma column and one sigma2 per target, a shared variance bracket).
Probability of feasibility: `constrained_ref.feasibility`; its derivatives in the mean and the standard deviation,
    dF/dmu = (phi(za) - phi(zb)) / sd,   dF/dsd = (za phi(za) - zb phi(zb)) / sd,   za = (lo - mu) / sd, zb = (hi - mu) / sd,
an infinite side contributing 0 and both being 0 under the small-variance guard (sd / sqrt(sigma2) < 1e-6: F is the indicator).
Criterion on target 0: the value is the oracle's (`O.acquisition`), the slope the reference's `return_dx` chain rule
(acquisition_fun.py:181-188 EI, 220-227 EpsilonPI, 292-309 MGFI) with its guards, which return a zero gradient.  With sd_k = sqrt(MSE_k)
(no floor) and dsd_k/dx = dMSE_k/dx / (2 sd_k):
    P = prod_k F_k,   dP/dx = sum_k (prod_{j != k} F_j) (dF_k/dmu dmu_k/dx + dF_k/dsd dsd_k/dx)
    value = base P,   dvalue/dx = P dbase/dx + base dP/dx
where a factor that is exactly 0 removes its term whatever the other factor is (0 / 0 at sd = 0 included).  It imports nothing from bogp."""
import numpy as np
from scipy.special import ndtr

from oracle import gp_oracle as O
from support import constrained_ref as CR
from support import ehvi_grad_ref as ER

ACQ_NONE = CR.ACQ_NONE
T_MAX = 22.36


def _phi(z):
    with np.errstate(all="ignore"):
        return np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


def _times(c, v):
    """c v with c == 0 -> 0 whatever v is (c a scalar, v an array or a scalar)"""
    return np.zeros_like(np.asarray(v, float)) if c == 0 else c * np.asarray(v, float)


def feasibility_grad(mu, mse, sigma2, lo, hi):
    """(F, dF/dmu, dF/dsd) of one constraint at one posterior (scalars)."""
    F = float(CR.feasibility(mu, mse, sigma2, lo, hi))
    sd = np.sqrt(mse)
    if sd / np.sqrt(sigma2) < 1e-6:
        return F, 0.0, 0.0
    za, zb = (lo - mu) / sd, (hi - mu) / sd
    pa = _phi(za) if np.isfinite(lo) else 0.0
    pb = _phi(zb) if np.isfinite(hi) else 0.0
    ta = za * pa if np.isfinite(lo) else 0.0
    tb = zb * pb if np.isfinite(hi) else 0.0
    return F, float((pa - pb) / sd), float((ta - tb) / sd)


def base_and_slope(acq_id, par, mu0, mse0, dmu0, dmse0, plugin, sigma2_0, minimize):
    """(base, dbase/dx (d,)) of the criterion on target 0; ACQ_NONE: (1, 0)."""
    d = len(dmu0)
    if acq_id == ACQ_NONE:
        return 1.0, np.zeros(d)
    with np.errstate(all="ignore"):
        base = float(np.ravel(O.acquisition(acq_id, par, np.array([mu0]), np.array([mse0]), plugin, sigma2_0, minimize))[0])
        sign = 1.0 if minimize else -1.0
        y, dy, sd = sign * mu0, sign * np.asarray(dmu0, float), np.sqrt(mse0)
        dsd = np.asarray(dmse0, float) / (2.0 * sd)
        if acq_id == O.ACQ_EI:
            if sd / np.sqrt(sigma2_0) < 1e-6:
                return base, np.zeros(d)
            z = (plugin - y) / sd
            return base, -dy * ndtr(z) + dsd * _phi(z)
        if acq_id == O.ACQ_EPSILON_PI:
            coef = 1 - par if y > 0 else 1 + par
            z = (plugin - coef * y) / sd
            return base, -(coef * dy + z * dsd) * _phi(z) / sd
        if acq_id == O.ACQ_MGFI:
            if np.isclose(sd, 0):
                return base, np.zeros(d)
            t = min(par, T_MAX)
            with np.errstate(all="raise"):
                try:
                    z = (plugin - (y - t * sd**2.0)) / sd
                    term = np.exp(t * (plugin + t * sd**2.0 / 2 - y - 1))
                    dz = -((dy - 2.0 * t * sd * dsd) + z * dsd) / sd
                    slope = term * (_phi(z) * dz + ndtr(z) * (t**2 * sd * dsd - t * dy))
                except FloatingPointError:
                    slope = np.zeros(d)
            return base, slope
    raise ValueError("criterion id %r is not one the feasibility-weighted criterion takes" % (acq_id,))


def from_moments(mu, mse, dmu, dmse, sigma2, lo, hi, acq, plugin, minimize):
    """One row from its moments: (values (q,), dvalues (q, d), P, dP (d,))."""
    lo, hi = CR.check(acq, lo, hi)
    m, d = len(mu), dmu.shape[1]
    assert len(lo) == len(hi) == m - 1
    F, dP = np.ones(m), np.zeros(d)
    parts = []
    for k in range(1, m):
        F[k], fm, fs = feasibility_grad(mu[k], mse[k], sigma2[k], lo[k - 1], hi[k - 1])
        with np.errstate(all="ignore"):
            dsd = dmse[k] / (2.0 * np.sqrt(mse[k]))
        parts.append(_times(fm, dmu[k]) + _times(fs, dsd))
    P = 1.0
    for k in range(1, m):
        P = P * F[k]
    for k in range(1, m):
        excl = float(np.prod(np.delete(F, [0, k])))
        dP = dP + _times(excl, parts[k - 1])
    vals, grads = [], []
    for a, par in acq:
        base, slope = base_and_slope(a, par, mu[0], mse[0], dmu[0], dmse[0], plugin, sigma2[0], minimize)
        vals.append(base * P)
        grads.append(_times(P, slope) + _times(base, dP))
    return np.array(vals), np.array(grads), P, dP


def constrained_grad(st, x, lo, hi, acq, plugin, minimize):
    """(values (q,), dvalues (q, d), P, dP (d,), mu (m,), mse (m,), dmu (m, d), dmse (m, d)) at the single row x."""
    mu, mse, dmu, dmse = ER.moments(st, x)
    sigma2 = np.asarray(st.sigma2, float).ravel()
    return from_moments(mu, mse, dmu, dmse, sigma2, lo, hi, acq, plugin, minimize) + (mu, mse, dmu, dmse)


def batch(st, X, lo, hi, acq, plugin, minimize):
    """The outputs of bogp_point_eval_constrained for the rows of X: acq (B, q), dacq (B, q, d), pof (B,), dpof (B, d), mu, mse (B, m),
    dmu, dmse (B, m, d)."""
    out = [[] for _ in range(8)]
    for x in np.atleast_2d(np.asarray(X, float)):
        for o, val in zip(out, constrained_grad(st, x, lo, hi, acq, plugin, minimize)):
            o.append(val)
    return tuple(np.array(o) for o in out)
