"""TEST-ONLY NumPy float64 restatement of `bogp_point_eval_ehvi_constrained` (include/bogp.h): the feasibility-weighted expected
hypervolume improvement of a multi-target Gaussian process AND its input gradient.

Targets 0 .. m - 1 are the objectives (maximised as given), target m + j the constraint feasible in [lo_j, hi_j].  Composed from
    `ehvi_grad_ref.moments`                 mu_k, MSE_k = max(0, sigma2_k s), dmu_k/dx, dMSE_k/dx of all m + c targets
    `ehvi_grad_ref.ehvi_and_coefficients`   E, dE/dmu_k, dE/dsd_k over the cells of the objectives, sd_k = sqrt(max(MSE_k, 1e-9));
                                            dsd_k/dx = dMSE_k/dx / (2 sd_k) where MSE_k > 1e-9, exactly 0 otherwise
    `constrained_grad_ref.feasibility_grad` F_j, dF_j/dmu, dF_j/dsd with sd = sqrt(MSE) (no floor), dsd/dx = dMSE/dx / (2 sd)
    `constrained_grad_ref._times`           a factor that is exactly 0 removes its term whatever the other factor is
and the case rules
    P = prod_j F_j (index order from 1.0),  dP/dx = sum_j (prod_{l != j} F_l) (dF_j/dmu dmu/dx + dF_j/dsd dsd/dx)
    P == 0:     value +0.0, gradient 0          C == 0:  value P, gradient dP          otherwise:  value E P, gradient P dE + E dP
E and dE are reported as 0 where the cells are not read (P == 0 or C == 0).  It imports nothing from bogp."""
import numpy as np

from support import constrained_grad_ref as CG
from support import ehvi_grad_ref as ER


def from_moments(mu, mse, dmu, dmse, sigma2, m, lower, upper, lo, hi):
    """One row from its moments: (value, dvalue (d,), P, dP (d,), E, dE (d,))."""
    mu, mse, sigma2 = np.asarray(mu, float).ravel(), np.asarray(mse, float).ravel(), np.asarray(sigma2, float).ravel()
    lo, hi = np.asarray(lo, float).ravel(), np.asarray(hi, float).ravel()
    m, mt, d = int(m), len(mu), dmu.shape[1]
    c = mt - m
    assert m >= 2 and c >= 1 and len(lo) == len(hi) == c and len(sigma2) == mt
    if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(hi < lo):
        raise ValueError("bounds must not be NaN, and hi >= lo")
    F, parts = np.ones(c), []
    for j in range(c):
        k = m + j
        F[j], fm, fs = CG.feasibility_grad(mu[k], mse[k], sigma2[k], lo[j], hi[j])
        with np.errstate(all="ignore"):
            dsd = dmse[k] / (2.0 * np.sqrt(mse[k]))
        parts.append(CG._times(fm, dmu[k]) + CG._times(fs, dsd))
    P = 1.0
    for j in range(c):
        P = P * F[j]
    dP = np.zeros(d)
    for j in range(c):
        dP = dP + CG._times(float(np.prod(np.delete(F, j))), parts[j])
    lower, upper = np.asarray(lower, float).reshape(-1, m), np.asarray(upper, float).reshape(-1, m)
    if P == 0.0:
        return 0.0, np.zeros(d), P, dP, 0.0, np.zeros(d)
    if len(lower) == 0:
        return P, dP.copy(), P, dP, 0.0, np.zeros(d)
    with np.errstate(all="ignore"):
        E, c_mu, c_sd, sd = ER.ehvi_and_coefficients(mu[:m], mse[:m], lower, upper)
    dE = np.zeros(d)
    for k in range(m):
        dE = dE + CG._times(c_mu[k], dmu[k])
        if mse[k] > 1e-9:
            dE = dE + CG._times(c_sd[k], dmse[k] / (2.0 * sd[k]))
    return E * P, CG._times(P, dE) + CG._times(E, dP), P, dP, E, dE


def at(st, x, m, lower, upper, lo, hi):
    """(value, dvalue, P, dP, E, dE, mu (m + c,), mse (m + c,), dmu (m + c, d), dmse (m + c, d)) at the single row x."""
    mu, mse, dmu, dmse = ER.moments(st, x)
    return from_moments(mu, mse, dmu, dmse, st.sigma2, m, lower, upper, lo, hi) + (mu, mse, dmu, dmse)


def batch(st, X, m, lower, upper, lo, hi):
    """The outputs of bogp_point_eval_ehvi_constrained for the rows of X: val (B,), dval (B, d), pof (B,), dpof (B, d), ehvi (B,),
    dehvi (B, d), mu, mse (B, m + c), dmu, dmse (B, m + c, d)."""
    out = [[] for _ in range(10)]
    for x in np.atleast_2d(np.asarray(X, float)):
        for o, val in zip(out, at(st, x, m, lower, upper, lo, hi)):
            o.append(val)
    return tuple(np.array(o) for o in out)
