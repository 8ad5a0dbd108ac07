"""Sample paths of the fitted surrogate (Thompson sampling): the host side of `bogp_sweep_thompson`.

The reference declares `GaussianProcess.sampling_prior` / `sampling_posterior` and leaves both as `pass` (gpr.py:312-316).  Here a
path is drawn by pathwise conditioning (Matheron's rule on a random-Fourier-feature prior draw; Wilson et al. 2020).  With the
committed R, r(x) = k(x, X), sigma2, gamma, beta (mu(x) = beta + r(x) . gamma, MSE(x) = sigma2 (1 - r^T R^-1 r + u^2), gpr.py:486-510)
and L features shared by the q paths of a call:

    z_j(x)    = sqrt(2 sigma2 / L) sum_l W[l, j] cos(omega_l . x + b_l)              the prior draw, Var ~ sigma2
    s_j       = z_j(X) + sqrt(sigma2 (diag(R) - 1)) * E[:, j]                         what it "observes" at the training rows
    bt_j      = 1^T R^-1 s_j / (1^T R^-1 1)   (ordinary kriging; 0 under simple kriging)
    gt_j      = R^-1 (s_j - bt_j 1)
    path_j(x) = mu(x) + z_j(x) - r(x) . gt_j - bt_j

The predictor is linear in the data, so the kriging of the draw's own "data" is subtracted: E[path] = mu and Var[path] = MSE, the
u^2 term included, when omega follows the kernel's spectral density.  In the reference's parametrisation (kernel.py: SE =
exp(-sum theta_i d_i^2), Matern on dists = sqrt(sum theta_i d_i^2), absolute-exponential = exp(-sum theta_i |d_i|)), n ~ N(0, I_d):

    SE                       omega = n * sqrt(2 theta)
    Matern nu                omega = n * sqrt(theta) * sqrt(2 nu / g),  g ~ chi2(2 nu)      (nu = 1/2, 3/2, 5/2 or any nu > 0)
    absolute-exponential     omega_i = theta_i * Cauchy(0, 1), independent per dimension

`draw` makes ALL random numbers on the host from `np.random.default_rng(seed)` in ONE order -- n (L x d), then g (L; Matern) or the
Cauchy variates (L x d; absolute-exponential), then b (L), W (L x q), E (N x q) -- and the device consumes the same arrays as
`paths_numpy`, the dense float64 restatement.  The noisy and noise-estimating modes are refused: there the reference pairs an
unscaled r(x) with a rescaled R (gpr.py:949-979), R - K(X, X) is indefinite, and no Gaussian process has that mean / MSE pair as
its conditional law.

The second half of the module is the multi-target form for Thompson batches under modelled constraints
(`bogp_sweep_thompson_constrained`): `state_of_multi`, `draw_multi`, `paths_multi_numpy`, the selection rule `select_numpy` and
`merge_ranks`.  `state_of`, `draw`, `paths_numpy` and `sampling_posterior` serve one target and refuse several, as before."""
from __future__ import annotations

import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import _lib

MAX_PATHS = 16  # BOGP_MAX_PATHS
MAX_FEATURES = 16384  # BOGP_MAX_FEATURES

Draw = namedtuple("Draw", "omega phase weights eps")  # (L, d), (L,), (L, q), (N, q)

_MATERN_NU = {_lib.KERNEL_MATERN12: 0.5, _lib.KERNEL_MATERN32: 1.5, _lib.KERNEL_MATERN52: 2.5}


def dense_state(X, y, theta, kernel, estimate_trend=True, beta=0.0, nugget=0.0, nu=None, sigma2=None):
    """A model for `draw` / `paths_numpy` without an engine: R = K(X, X) + diag(nugget), beta by generalised least squares under
    ordinary kriging (else as given), sigma2 concentrated unless given."""
    X = np.ascontiguousarray(X, dtype=float)
    y = np.asarray(y, dtype=float).reshape(len(X))
    st = SimpleNamespace(X=X, y=y, theta=np.broadcast_to(np.asarray(theta, dtype=float).ravel(), (X.shape[1],)).copy(), kernel=int(kernel),
                         nu=nu, estimate_trend=bool(estimate_trend), nugget=np.broadcast_to(np.asarray(nugget, dtype=float), (len(X),)).copy(),
                         beta=float(beta), sigma2=sigma2)  # fmt: skip
    R = correlation(st, X, X) + np.diag(st.nugget)
    Ri1 = np.linalg.solve(R, np.ones(len(X)))
    if st.estimate_trend:
        st.beta = float(Ri1 @ y / Ri1.sum())
    if sigma2 is None:
        res = y - st.beta
        st.sigma2 = float(res @ np.linalg.solve(R, res) / len(X))
    return st


def _gp_refusals(model):
    """What `state_of` and `state_of_multi` refuse of a model alike, in this order: a forest, no fit, the mode, the trend basis."""
    if type(model).__name__ == "RandomForest" or hasattr(model, "estimators_"):
        raise NotImplementedError("a forest model has no posterior paths to draw (Thompson sampling conditions a Gaussian process)")
    if getattr(model, "_committed_par", None) is None:
        raise Exception("The model is not fitted yet!")
    mode = "noisy" if getattr(model, "_committed_restricted", False) else model.estimation_mode
    if mode != "noiseless":
        raise NotImplementedError("posterior paths in the %s mode: the reference pairs an unscaled r(x) with a rescaled R there "
                                  "(gpr.py:949-979), which is no Gaussian process's conditional law; use nugget=0, noise_estim=False" % mode)  # fmt: skip
    if type(model.mean).__name__ != "constant_trend":
        raise NotImplementedError("posterior paths serve the constant trend basis, not the polynomial trends (%s)" % type(model.mean).__name__)


def state_of(model):
    """What the formulas read, from a fitted `GaussianProcess` (or a `dense_state`, returned as it is).  The refusals live here."""
    if isinstance(model, SimpleNamespace):
        refuse_kernel(model.kernel)
        return model
    _gp_refusals(model)
    if np.ndim(model.y) > 1 and model.y.shape[1] > 1:
        raise NotImplementedError("posterior paths serve one target (EHVI / several targets: the model has %d)" % model.y.shape[1])
    refuse_kernel(model.kernel_id)
    d = model.X.shape[1]
    return SimpleNamespace(X=model.X, y=np.asarray(model.y, dtype=float).reshape(len(model.X)), kernel=model.kernel_id, nu=model._nu,
                           theta=np.broadcast_to(np.asarray(model.theta_, dtype=float).ravel(), (d,)).copy(), nugget=np.zeros(len(model.X)),
                           estimate_trend=bool(model.estimate_trend), beta=float(np.ravel(model.mean.beta)[0]),
                           sigma2=float(np.ravel(model.sigma2)[0]))  # fmt: skip


def refuse_kernel(kernel):
    if kernel == _lib.KERNEL_CUBIC:
        raise NotImplementedError("posterior paths with the cubic kernel: no spectral draw is defined for it")
    if kernel == _lib.KERNEL_GENEXP:
        raise NotImplementedError("posterior paths with the generalized-exponential kernel: no spectral draw is defined for it")


def _nu_of(st):
    return float(st.nu) if st.kernel == _lib.KERNEL_MATERN_NU else _MATERN_NU.get(st.kernel)


def correlation(st, A, B):
    """k(A_i, B_j) in the reference's parametrisation (kernel.py:159-329), (len(A), len(B))."""
    D = np.abs(np.asarray(A, dtype=float)[:, None, :] - np.asarray(B, dtype=float)[None, :, :])
    if st.kernel == _lib.KERNEL_ABSEXP:
        return np.exp(-(D * st.theta).sum(-1))
    s = (D * D * st.theta).sum(-1)
    if st.kernel == _lib.KERNEL_SE:
        return np.exp(-s)
    dists = np.sqrt(s)
    if st.kernel == _lib.KERNEL_MATERN12:
        return np.exp(-dists)
    if st.kernel == _lib.KERNEL_MATERN32:
        K = dists * math.sqrt(3.0)
        return (1.0 + K) * np.exp(-K)
    if st.kernel == _lib.KERNEL_MATERN52:
        K = dists * math.sqrt(5.0)
        return (1.0 + K + K**2 / 3.0) * np.exp(-K)
    if st.kernel == _lib.KERNEL_MATERN_NU:
        from scipy.special import gamma, kv

        nu = float(st.nu)
        t = math.sqrt(2.0 * nu) * np.where(dists == 0.0, np.finfo(float).eps, dists)  # (strict zeros result in nan, kernel.py:203)
        return (2.0 ** (1.0 - nu)) / gamma(nu) * t**nu * kv(nu, t)
    raise NotImplementedError("kernel id %r has no posterior paths" % (st.kernel,))


def draw(model, q, n_features=1024, seed=None):
    """The random numbers of q paths over `n_features` shared features: Draw(omega (L, d), phase (L,), weights (L, q), eps (N, q)),
    from `np.random.default_rng(seed)` in the order n, g or the Cauchy variates, b, W, E.  Reproducible per seed."""
    st = state_of(model)
    q, L = int(q), int(n_features)
    if q < 1:
        raise ValueError("q = %d: at least one path" % q)
    if L < 16 or L > MAX_FEATURES or L % 16:
        raise ValueError("n_features = %d: a multiple of 16 in [16, %d]" % (L, MAX_FEATURES))
    N, d = st.X.shape
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((L, d))
    if st.kernel == _lib.KERNEL_SE:
        omega = n * np.sqrt(2.0 * st.theta)
    elif st.kernel == _lib.KERNEL_ABSEXP:
        omega = st.theta * rng.standard_cauchy((L, d))
    else:
        nu = _nu_of(st)
        g = rng.chisquare(2.0 * nu, size=L)
        omega = n * np.sqrt(st.theta) * np.sqrt(2.0 * nu / g)[:, None]
    phase = rng.uniform(0.0, 2.0 * np.pi, size=L)
    weights = rng.standard_normal((L, q))
    eps = rng.standard_normal((N, q))
    return Draw(np.ascontiguousarray(omega), phase, weights, eps)


def prior_draw(st, dr, X):
    """z(X): (len(X), q)."""
    L = len(dr.phase)
    return math.sqrt(2.0 * st.sigma2 / L) * (np.cos(np.asarray(X, dtype=float) @ dr.omega.T + dr.phase) @ dr.weights)


def paths_numpy(model, dr, X, conditioned=True):
    """The dense float64 restatement of the formulas above: (paths (q, len(X)), (gt (N, q), bt (q,))).  `conditioned=False`: the
    prior paths beta + z_j(x), and zero coefficients."""
    st = state_of(model)
    X = np.atleast_2d(np.asarray(X, dtype=float))
    N, q = len(st.X), dr.weights.shape[1]
    z = prior_draw(st, dr, X)
    if not conditioned:
        return (st.beta + z).T, (np.zeros((N, q)), np.zeros(q))
    R = correlation(st, st.X, st.X) + np.diag(st.nugget)
    s = prior_draw(st, dr, st.X) + np.sqrt(st.sigma2 * st.nugget)[:, None] * dr.eps
    Ri1 = np.linalg.solve(R, np.ones(N))
    Ris = np.linalg.solve(R, s)
    bt = (Ri1 @ s) / Ri1.sum() if st.estimate_trend else np.zeros(q)
    gt = Ris - np.outer(Ri1, bt)
    r = correlation(st, X, st.X)
    mu = st.beta + r @ np.linalg.solve(R, st.y - st.beta)
    return (mu[:, None] + z - r @ gt - bt).T, (gt, bt)


def moments_numpy(model, X):
    """mu (M,) and MSE (M,) of the predictor the paths are conditioned on (gpr.py:486-510, unclipped), densely."""
    st = state_of(model)
    X = np.atleast_2d(np.asarray(X, dtype=float))
    R = correlation(st, st.X, st.X) + np.diag(st.nugget)
    r = correlation(st, X, st.X)
    Rir = np.linalg.solve(R, r.T)
    Ri1 = np.linalg.solve(R, np.ones(len(st.X)))
    u2 = (Ri1 @ r.T - 1.0) ** 2 / Ri1.sum() if st.estimate_trend else 0.0
    mu = st.beta + r @ np.linalg.solve(R, st.y - st.beta)
    return mu, st.sigma2 * (1.0 - np.einsum("mn,nm->m", r, Rir) + u2)


def batch_seeds(seed, n):
    """Seeds of n calls derived from one: the seed itself for one call, children of `np.random.SeedSequence(seed)` otherwise."""
    return [seed] if n == 1 else list(np.random.SeedSequence(seed).spawn(n))


def sample(model, X, n_samples=1, n_features=1024, seed=None, conditioned=True):
    """`GaussianProcess.sampling_posterior` / `sampling_prior`: (len(X), n_samples) path values on the device, 16 paths per call."""
    state_of(model)
    X = model._check_X(X)
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError("n_samples = %d: at least one path" % n_samples)
    eng = model.engine
    eng.upload_candidates(X)
    sizes = [min(MAX_PATHS, n_samples - a) for a in range(0, n_samples, MAX_PATHS)]
    cols = []
    for qb, sd in zip(sizes, batch_seeds(seed, len(sizes))):
        out = eng.sweep_thompson(draw(model, qb, n_features, sd), conditioned=conditioned, return_values=True)
        cols.append(np.asarray(out["paths"]).T)
    return np.concatenate(cols, axis=1)


# ----------------------------------------------------------------------------------------------------------------------
# joint paths of a multi-target model: Thompson batches under modelled constraints (`bogp_sweep_thompson_constrained`)
# ----------------------------------------------------------------------------------------------------------------------
# The targets of a multi-target model share R (and so theta and r(x)) and are a priori independent; its trend is a FIXED constant, so the
# conditional law is the simple-kriging one.  A call carries q batch members of m targets over shared features; column j m + t of the
# weights and of eps is member j's path of target t:
#
#     z_{j,t}(x)    = sqrt(2 sigma2_t / L) sum_l W[l, j m + t] cos(omega_l . x + b_l)
#     s_{j,t}       = z_{j,t}(X) + sqrt(sigma2_t (diag(R) - 1)) * E[:, j m + t]
#     gt_{j,t}      = R^-1 s_{j,t}
#     path_{j,t}(x) = beta + r(x) . (gamma_t - gt_{j,t}) + z_{j,t}(x),      gamma_t = R^-1 (y_t - beta)
#
# Independent weights over shared features give independent targets.  The selection rule is Eriksson & Poloczek's (2021): the best
# objective value among the rows whose drawn constraints hold, the least violating row when there is none (`select_numpy`).


def dense_state_multi(X, Y, theta, kernel, beta=0.0, nu=None, sigma2=None):
    """A multi-target model for `draw_multi` / `paths_multi_numpy` without an engine: Y (N, m), a fixed constant trend `beta`, sigma2
    (m,) concentrated per target unless given."""
    X = np.ascontiguousarray(X, dtype=float)
    Y = np.asarray(Y, dtype=float).reshape(len(X), -1)
    st = SimpleNamespace(X=X, y=Y, theta=np.broadcast_to(np.asarray(theta, dtype=float).ravel(), (X.shape[1],)).copy(), kernel=int(kernel),
                         nu=nu, estimate_trend=False, nugget=np.zeros(len(X)), beta=float(beta), sigma2=sigma2, multi=True)  # fmt: skip
    res = Y - st.beta
    st.gamma = np.linalg.solve(correlation(st, X, X), res)  # (N, m)
    if sigma2 is None:
        st.sigma2 = np.einsum("nt,nt->t", res, st.gamma) / len(X)
    st.sigma2 = np.asarray(st.sigma2, dtype=float).ravel()
    return st


def state_of_multi(model):
    """What the joint formulas read, from a `GaussianProcess` fitted on y (N, m), m >= 2 (or a `dense_state_multi`, returned as it
    is): X, y (N, m), theta, kernel, beta, and per target sigma2 (m,) and gamma (N, m).  The refusals live here."""
    if isinstance(model, SimpleNamespace):
        refuse_kernel(model.kernel)
        if not getattr(model, "multi", False):
            raise ValueError("joint paths need a multi-target state (thompson.dense_state_multi)")
        return model
    _gp_refusals(model)
    if np.ndim(model.y) < 2 or model.y.shape[1] < 2:
        raise ValueError("joint paths need a model fitted on y (N, m) with m >= 2 columns (objective, constraints): one target goes to "
                         "thompson.state_of")  # fmt: skip
    if model.estimate_trend:
        raise NotImplementedError("a multi-target model has a fixed constant trend (gpr.py:787): joint paths with an estimated one")
    refuse_kernel(model.kernel_id)
    d, m = model.X.shape[1], model.y.shape[1]
    return SimpleNamespace(X=model.X, y=np.asarray(model.y, dtype=float), kernel=model.kernel_id, nu=model._nu,
                           theta=np.broadcast_to(np.asarray(model.theta_, dtype=float).ravel(), (d,)).copy(), nugget=np.zeros(len(model.X)),
                           estimate_trend=False, beta=float(np.ravel(model.mean.beta)[0]),
                           sigma2=np.broadcast_to(np.asarray(model.sigma2, dtype=float).ravel(), (m,)).copy(),
                           gamma=np.asarray(model.gamma, dtype=float).reshape(len(model.X), m), multi=True)  # fmt: skip


def draw_multi(model, q, n_features=1024, seed=None):
    """The random numbers of q members' joint paths of the m targets: `draw`'s arrays in `draw`'s RNG order with q m columns, column
    j m + t member j's path of target t.  q m <= 16."""
    st = state_of_multi(model)
    q, m = int(q), st.y.shape[1]
    if q < 1:
        raise ValueError("q = %d: at least one member" % q)
    if q * m > MAX_PATHS:
        raise ValueError("q = %d members of %d targets: at most %d columns in one call" % (q, m, MAX_PATHS))
    return draw(SimpleNamespace(X=st.X, kernel=st.kernel, theta=st.theta, nu=st.nu), q * m, n_features, seed)


def paths_multi_numpy(model, dr, X):
    """The dense float64 restatement of the joint formulas: (paths (q, m, len(X)), gt (N, q m))."""
    st = state_of_multi(model)
    X = np.atleast_2d(np.asarray(X, dtype=float))
    N, m = st.y.shape
    qm = dr.weights.shape[1]
    if qm % m:
        raise ValueError("the draw has %d columns, no multiple of the %d targets" % (qm, m))
    L = len(dr.phase)
    scale = np.tile(np.sqrt(2.0 * st.sigma2 / L), qm // m)  # column j m + t: target t's
    R = correlation(st, st.X, st.X) + np.diag(st.nugget)
    z = (np.cos(X @ dr.omega.T + dr.phase) @ dr.weights) * scale
    s = (np.cos(st.X @ dr.omega.T + dr.phase) @ dr.weights) * scale
    if dr.eps is not None:
        s = s + np.sqrt(np.outer(st.nugget, np.tile(st.sigma2, qm // m))) * dr.eps
    gt = np.linalg.solve(R, s)
    gamma = np.tile(np.linalg.solve(R, st.y - st.beta), (1, qm // m))
    r = correlation(st, X, st.X)
    paths = st.beta + r @ (gamma - gt) + z
    return paths.T.reshape(qm // m, m, len(X)), gt


def objective_path_at(model, dr, gt, j, x):
    """path_{j,0}(x) at ONE point from the coefficients `gt` (N, q m) a call returned and the model's own gamma_0:
    beta + r(x) . (gamma_0 - gt_{j,0}) + z_{j,0}(x).  O(N d + L d), no solve."""
    st = state_of_multi(model)
    m = st.y.shape[1]
    x = np.asarray(x, dtype=float).reshape(1, -1)
    gamma0 = st.gamma[:, 0]
    z = math.sqrt(2.0 * st.sigma2[0] / len(dr.phase)) * (np.cos(x @ dr.omega.T + dr.phase) @ dr.weights[:, j * m])
    return float(st.beta + correlation(st, x, st.X)[0] @ (gamma0 - np.asarray(gt)[:, j * m]) + z[0])


def moments_multi_numpy(model, X):
    """mu (M, m) and MSE (M, m) of the multi-target predictor the joint paths are conditioned on, densely."""
    st = state_of_multi(model)
    X = np.atleast_2d(np.asarray(X, dtype=float))
    R = correlation(st, st.X, st.X) + np.diag(st.nugget)
    r = correlation(st, X, st.X)
    mu = st.beta + r @ np.linalg.solve(R, st.y - st.beta)
    return mu, np.outer(1.0 - np.einsum("mn,nm->m", r, np.linalg.solve(R, r.T)), st.sigma2)


def rank_numpy(crit, k):
    """`bogp_sweep_topk`'s ranking of every row of `crit` (n, M): first maximum, ties to the lower index, NaN maximal; slots beyond
    M are (-inf, -1).  (values (n, k), indices (n, k))."""
    n, M = crit.shape
    val, idx = np.full((n, k), -np.inf), np.full((n, k), -1, dtype=np.int64)
    for j in range(n):
        order = np.argsort(-np.where(np.isnan(crit[j]), np.inf, crit[j]), kind="stable")[:k]
        val[j, : len(order)], idx[j, : len(order)] = crit[j][order], order
    return val, idx


def select_numpy(paths, lo, hi, sigma2, minimize=True, k=1):
    """The selection of `bogp_sweep_thompson_constrained` on path values (q, m, M), in the device's own operations -- comparisons,
    differences and single products, no sum -- so that it reproduces the device's scores from the device's paths exactly:

        e_t = max(lo_t - c_t, c_t - hi_t, 0),  viol = max_{t >= 1} e_t / sqrt(sigma2_t),  feas = every lo_t <= c_t <= hi_t
        A = feas ? (-c_0 if minimize else c_0) : -inf,   B = 0.0 - viol,   a NaN among the m values: A = B = -inf

    Returns a dict: A, B (q, M), feas (q, M), best_val / best_idx (q, 2, k): per member the ranking of A, then of B."""
    paths = np.asarray(paths, dtype=float)
    q, m, M = paths.shape
    lo, hi = np.asarray(lo, dtype=float).ravel(), np.asarray(hi, dtype=float).ravel()
    inv_sd = 1.0 / np.sqrt(np.asarray(sigma2, dtype=float).ravel()[1:])
    if len(lo) != m - 1 or len(hi) != m - 1 or len(inv_sd) != m - 1:
        raise ValueError("lo, hi hold one bound per constraint, sigma2 one value per target (%d targets)" % m)
    feas = np.ones((q, M), dtype=bool)
    viol = np.zeros((q, M))
    with np.errstate(invalid="ignore"):
        for t in range(1, m):
            c = paths[:, t]
            d1, d2 = lo[t - 1] - c, c - hi[t - 1]
            e = np.where(d1 > 0.0, d1, 0.0)
            e = np.where(d2 > e, d2, e)
            p = e * inv_sd[t - 1]
            viol = np.where(p > viol, p, viol)
            feas &= (lo[t - 1] <= c) & (c <= hi[t - 1])
    bad = np.isnan(paths).any(axis=1)
    A = np.where(feas, -1 * paths[:, 0] if minimize else paths[:, 0], -np.inf)
    B = 0.0 - viol
    A[bad], B[bad] = -np.inf, -np.inf
    k = int(k)
    va, ia = rank_numpy(A, k)
    vb, ib = rank_numpy(B, k)
    return dict(A=A, B=B, feas=feas & ~bad, best_val=np.stack([va, vb], axis=1), best_idx=np.stack([ia, ib], axis=1))


def merge_ranks(best_val, best_idx, k=None):
    """A member's proposal list from its rankings (2, k'): the A ranks whose value is above -inf (rows whose drawn constraints
    hold, best objective first), then the B ranks (least violating first) whose row is not already listed; unfilled slots (-1) are
    dropped and the list is cut to `k` (default k').  Returns a list of (row, which, rank): which = 0 for an A rank, 1 for a B rank."""
    best_val, best_idx = np.asarray(best_val), np.asarray(best_idx)
    k = best_val.shape[-1] if k is None else int(k)
    out, seen = [], set()
    for r in range(best_val.shape[-1]):
        gi = int(best_idx[0, r])
        if gi >= 0 and best_val[0, r] > -np.inf and gi not in seen:
            out.append((gi, 0, r))
            seen.add(gi)
    for r in range(best_val.shape[-1]):
        gi = int(best_idx[1, r])
        if gi >= 0 and best_val[1, r] > -np.inf and gi not in seen:
            out.append((gi, 1, r))
            seen.add(gi)
    return out[:k]
