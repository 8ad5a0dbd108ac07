"""TEST-ONLY NumPy float64 restatement of the input gradient of EHVI for a multi-target Gaussian process.

Posterior: the arithmetic of `oracle/gp_oracle.predict` and `gradient` at ONE row, with one gamma column (and one
sigma2) per target -- mu_k = beta_k + r . gamma_k, MSE_k = max(0, sigma2_k s) with the shared bracket
s = 1 - |L^-1 r|^2 + u^2, d mu_k / dx = gamma_k^T dr/dx, d MSE_k / dx = 2 sigma2_k (-(L^-1 r)^T L^-1 dr/dx + u^T (Ft^T Ft)^-1 du/dx).
Criterion: per cell c and target k, a = (l - mu) / sd, b = (u - mu) / sd, G(z) = phi(z) - z Phi(-z),
    f = sd (G(a) - G(b)),  df/dmu = Phi(-a) - Phi(-b),  df/dsd = phi(a) - phi(b)      (b terms 0 for u = +inf)
    EHVI = sum_c prod_k f_ck,  dEHVI/dmu_j = sum_c (prod_{k != j} f_ck) df_cj/dmu_j  (product of the others, no division)
with sd_k = sqrt(max(MSE_k, 1e-9)) (analytic.py:233): d sd_k / dx = d MSE_k / dx / (2 sd_k) where MSE_k > 1e-9, else 0.
It imports nothing from bogp."""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import ndtr

from oracle import gp_oracle as O

_SQRT2PI = np.sqrt(2.0 * np.pi)


def _phi(z):
    return np.exp(-0.5 * z * z) / _SQRT2PI


def _G(z):
    return _phi(z) - z * ndtr(-z)


def moments(st, x):
    """(mu (m,), mse (m,), dmu (m, d), dmse (m, d)) of the m targets of the oracle state `st` at the single row x."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    N = st.X.shape[0]
    r = O.corr(st.kernel, st.theta, O.l1_cross_distances(x, st.X)).reshape(1, N)
    r_dx = O.corr_dx(st, x, r).T  # (N, d)
    beta = np.broadcast_to(np.asarray(st.beta, float).reshape(1, -1), (1, st.gamma.shape[1]))
    mu = (beta + r.dot(st.gamma)).ravel()
    dmu = st.gamma.T.dot(r_dx)  # (m, d): the constant basis has a zero Jacobian
    rt = solve_triangular(st.C, r.T, lower=True)
    rt_dx = solve_triangular(st.C, r_dx, lower=True)
    s = 1.0 - float((rt**2.0).sum())
    s_dx = -1.0 * np.dot(rt.T, rt_dx)  # (1, d)
    if st.estimate_trend:
        u = np.dot(st.Ft.T, rt) - 1.0
        u_dx = np.dot(st.Ft.T, rt_dx)
        s += float((solve_triangular(st.G.T, u, lower=True) ** 2.0).sum())
        s_dx = s_dx + u.T.dot(np.linalg.inv(np.dot(st.Ft.T, st.Ft))).dot(u_dx)
    sigma2 = np.asarray(st.sigma2, float).ravel()
    mse = np.maximum(s * sigma2, 0.0)
    dmse = 2.0 * sigma2[:, None] * s_dx
    return mu, mse, dmu, dmse


def ehvi_and_coefficients(mu, mse, lower, upper):
    """EHVI and its partial derivatives in mu_k and sd_k: (value, dE/dmu (m,), dE/dsd (m,), sd (m,))."""
    mu, mse = np.asarray(mu, float).ravel(), np.asarray(mse, float).ravel()
    lower, upper = np.atleast_2d(np.asarray(lower, float)), np.atleast_2d(np.asarray(upper, float))
    m = len(mu)
    sd = np.sqrt(np.maximum(mse, 1e-9))
    a = (lower - mu) / sd
    fin = np.isfinite(upper)
    b = (np.where(fin, upper, 0.0) - mu) / sd
    f = sd * (_G(a) - np.where(fin, _G(b), 0.0))  # (C, m)
    fm = ndtr(-a) - np.where(fin, ndtr(-b), 0.0)
    fs = _phi(a) - np.where(fin, _phi(b), 0.0)
    value = float(np.prod(f, axis=1).sum())
    dE_dmu, dE_dsd = np.empty(m), np.empty(m)
    for j in range(m):
        others = np.prod(np.delete(f, j, axis=1), axis=1)
        dE_dmu[j] = float((others * fm[:, j]).sum())
        dE_dsd[j] = float((others * fs[:, j]).sum())
    return value, dE_dmu, dE_dsd, sd


def ehvi_grad(st, x, lower, upper, parts=False):
    """(EHVI, dEHVI/dx (d,)) at the row x; with `parts` also the mean path and the sd path of the gradient separately."""
    mu, mse, dmu, dmse = moments(st, x)
    value, c_mu, c_sd, sd = ehvi_and_coefficients(mu, mse, lower, upper)
    free = mse > 1e-9
    dsd = np.where(free[:, None], dmse / (2.0 * sd[:, None]), 0.0)
    g_mu = (c_mu[:, None] * dmu).sum(axis=0)
    g_sd = (c_sd[:, None] * dsd).sum(axis=0)
    if parts:
        return value, g_mu + g_sd, g_mu, g_sd
    return value, g_mu + g_sd


def batch(st, X, lower, upper):
    """The outputs of bogp_point_eval_ehvi for the rows of X: ehvi (B,), dehvi (B, d), mu, mse (B, m), dmu, dmse (B, m, d)."""
    X = np.atleast_2d(np.asarray(X, float))
    out = [[] for _ in range(6)]
    for x in X:
        mu, mse, dmu, dmse = moments(st, x)
        v, g = ehvi_grad(st, x, lower, upper)
        for o, val in zip(out, (v, g, mu, mse, dmu, dmse)):
            o.append(val)
    return tuple(np.array(o) for o in out)
