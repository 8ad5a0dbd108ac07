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
`merge_ranks`; `hvi_select_numpy` is the selection rule of `bogp_sweep_thompson_ehvi`, which draws the same joint paths for the
objectives of a multi-objective run.  `state_of`, `draw`, `paths_numpy` and `sampling_posterior` serve one target and refuse several, as before."""
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


def correlation_dx(st, A, B):
    """d k(A_i, B_j) / d A_ik in the reference's expressions (corr_dx, gpr.py:600-661, the D = 0 conventions included), (len(A),
    len(B), d); the five kernels that have one."""
    diff = np.asarray(A, dtype=float)[:, None, :] - np.asarray(B, dtype=float)[None, :, :]
    r = correlation(st, A, B)[:, :, None]
    if st.kernel == _lib.KERNEL_ABSEXP:
        return -r * st.theta * np.sign(diff)
    if st.kernel == _lib.KERNEL_SE:
        return -2.0 * r * (st.theta * diff)
    D = np.sqrt((diff * diff * st.theta).sum(-1))[:, :, None]
    if st.kernel == _lib.KERNEL_MATERN32:
        return -3.0 * np.exp(-math.sqrt(3.0) * D) * (st.theta * diff)
    if st.kernel == _lib.KERNEL_MATERN52:
        return -(5.0 / 3.0) * (1.0 + math.sqrt(5.0) * D) * np.exp(-math.sqrt(5.0) * D) * (st.theta * diff)
    if st.kernel == _lib.KERNEL_MATERN12:
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(D > 0.0, -(st.theta * diff) / D * r, 0.0)
    raise NotImplementedError("the correlation of kernel id %r has no input-derivative (corr_dx leaves it undefined in the reference, "
                              "gpr.py:655-658)" % (st.kernel,))  # fmt: skip


def path_grad_numpy(model, dr, X, members, conditioned=True, parts=False):
    """The dense float64 restatement of `bogp_point_eval_path`: value (B,) and input gradient (B, d) of path members[b] at row b of
    X, with `paths_numpy`'s own gt, bt:

        v   = beta - bt_j + sum_n c_j[n] r_n(x) + sum_l Wt[l, j] cos(omega_l . x + phi_l),      c_j = gamma - gt_j, Wt = sqrt(2 sigma2 / L) W
        g_k = sum_n c_j[n] d r_n / d x_k - sum_l Wt[l, j] sin(omega_l . x + phi_l) omega_lk

    `parts=True` adds a dict of the sums of the ABSOLUTE terms: A_v (B,) of the value, A_g (B, d) of every gradient component, and the
    conditioning and feature shares of each (cond_v, feat_v, cond_g, feat_g)."""
    st = state_of(model)
    X = np.atleast_2d(np.asarray(X, dtype=float))
    members = np.asarray(members, dtype=int).ravel()
    N, L = len(st.X), len(dr.phase)
    Wt = math.sqrt(2.0 * st.sigma2 / L) * dr.weights[:, members]  # (L, B)
    ph = X @ dr.omega.T + dr.phase  # (B, L)
    if conditioned:
        _, (gt, bt) = paths_numpy(st, dr, st.X[:1], True)
        R = correlation(st, st.X, st.X) + np.diag(st.nugget)
        c = (np.linalg.solve(R, st.y - st.beta)[:, None] - gt)[:, members]  # (N, B)
        r, rdx = correlation(st, X, st.X), correlation_dx(st, X, st.X)
        bt = bt[members]
    else:
        c, r, rdx, bt = np.zeros((N, len(X))), np.zeros((len(X), N)), np.zeros((len(X), N, X.shape[1])), np.zeros(len(X))
    val = st.beta - bt + np.einsum("bn,nb->b", r, c) + np.einsum("bl,lb->b", np.cos(ph), Wt)
    u = -np.sin(ph) * Wt.T  # (B, L)
    grad = np.einsum("nb,bnk->bk", c, rdx) + u @ dr.omega
    if not parts:
        return val, grad
    cond_v, feat_v = np.einsum("bn,nb->b", np.abs(r), np.abs(c)), np.abs(Wt).sum(axis=0)
    cond_g, feat_g = np.einsum("nb,bnk->bk", np.abs(c), np.abs(rdx)), np.abs(Wt).T @ np.abs(dr.omega)
    return val, grad, dict(A_v=abs(st.beta) + np.abs(bt) + cond_v + feat_v, A_g=cond_g + feat_g, cond_v=cond_v, feat_v=feat_v, cond_g=cond_g,
                           feat_g=feat_g)  # fmt: skip


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


def hvi_select_numpy(paths, lower, upper, sigma2, k=1):
    """The selection of `bogp_sweep_thompson_ehvi` on path values (q, m, M) over the cells (lower, upper) (C x m; targets
    maximised), in the device's own operations and order -- so that it reproduces the device's scores from the device's paths
    exactly.  With y_k = paths[j, k, row]:

        per cell c in order:  t_k = max(min(y_k, u_ck) - l_ck, 0);  p = t_0, p = p t_1, ...;  acc = acc + p              (acc from 0.0)
                              cm = max_k (max(l_ck - y_k, y_k - u_ck, 0) / sqrt(sigma2_k)) (from 0.0);  dist = min(dist, cm) (from +inf)
        A = acc > 0 ? acc : -inf,   B = 0.0 - dist,   a NaN among the m values: A = B = -inf

    A is the hypervolume the drawn vector would add to the front whose non-dominated region the cells partition; B ranks the rows
    whose draw adds none by their scaled Chebyshev distance to that region.  Returns a dict: A, B (q, M), best_val / best_idx
    (q, 2, k): per member the ranking of A, then of B (`select_numpy`'s shapes, for `merge_ranks`)."""
    paths = np.asarray(paths, dtype=float)
    q, m, M = paths.shape
    lower, upper = np.atleast_2d(np.asarray(lower, dtype=float)), np.atleast_2d(np.asarray(upper, dtype=float))
    inv_sd = 1.0 / np.sqrt(np.asarray(sigma2, dtype=float).ravel())
    if lower.shape != upper.shape or lower.shape[1] != m or len(inv_sd) != m:
        raise ValueError("lower, upper hold C x %d cell bounds, sigma2 one value per target" % m)
    acc, dist = np.zeros((q, M)), np.full((q, M), np.inf)
    with np.errstate(invalid="ignore"):
        for c in range(len(lower)):
            p, cm = None, np.zeros((q, M))
            for t in range(m):
                y, lb, ub = paths[:, t], lower[c, t], upper[c, t]
                s = np.fmax(np.fmin(y, ub) - lb, 0.0)
                p = s if t == 0 else p * s
                e = np.fmax(np.fmax(lb - y, y - ub), 0.0)
                cm = np.fmax(cm, e * inv_sd[t])
            acc = acc + p
            dist = np.fmin(dist, cm)
        A = np.where(acc > 0.0, acc, -np.inf)
    B = 0.0 - dist
    bad = np.isnan(paths).any(axis=1)
    A[bad], B[bad] = -np.inf, -np.inf
    k = int(k)
    va, ia = rank_numpy(A, k)
    vb, ib = rank_numpy(B, k)
    return dict(A=A, B=B, best_val=np.stack([va, vb], axis=1), best_idx=np.stack([ia, ib], axis=1))


def hvi_constrained_select_numpy(paths, n_obj, lower, upper, lo, hi, sigma2, k=1):
    """The selection of `bogp_sweep_thompson_ehvi_constrained` on path values (q, m, M) -- targets 0 .. n_obj - 1 the objectives
    (maximised) over the cells (lower, upper) (C x n_obj), targets n_obj .. m - 1 constraints feasible in [lo, hi] -- in the device's
    own operations and order, from the pieces of `select_numpy` (the violation and the feasibility of the constraint columns) and
    `hvi_select_numpy` (HVI and dist of the objective columns):

        A = feas and HVI > 0 ? HVI : -inf,   B = feas ? 0.0 - dist : -inf,   V = 0.0 - viol,   a NaN among the m values: A = B = V = -inf

    Returns a dict: A, B, V (q, M), feas (q, M), best_val / best_idx (q, 3, k): per member the ranking of A, then of B, then of V."""
    paths = np.asarray(paths, dtype=float)
    q, m, M = paths.shape
    n_obj = int(n_obj)
    sigma2 = np.asarray(sigma2, dtype=float).ravel()
    if not 2 <= n_obj < m or len(sigma2) != m:
        raise ValueError("n_obj = %d objectives among %d targets (at least two, and at least one constraint); sigma2 one value per target" % (n_obj, m))
    # `select_numpy` reads its column 0 as an objective and the rest as constraints: the last objective stands in, its A is not used
    con = select_numpy(paths[:, n_obj - 1 :], lo, hi, sigma2[n_obj - 1 :], minimize=False, k=1)
    obj = hvi_select_numpy(paths[:, :n_obj], lower, upper, sigma2[:n_obj], k=1)
    bad = np.isnan(paths).any(axis=1)
    feas = con["feas"] & ~bad
    A, B = np.where(feas, obj["A"], -np.inf), np.where(feas, obj["B"], -np.inf)
    V = np.where(bad, -np.inf, con["B"])
    ranks = [rank_numpy(s, int(k)) for s in (A, B, V)]
    return dict(A=A, B=B, V=V, feas=feas, best_val=np.stack([r[0] for r in ranks], axis=1), best_idx=np.stack([r[1] for r in ranks], axis=1))


def _sum_16x16(part):
    """The 256 thread partials (..., 256) added as the point kernels add them: 16 runs of 16 in order, then the 16 sums in order."""
    runs = part.reshape(part.shape[:-1] + (16, 16))
    for _ in range(2):
        s = runs[..., 0]
        for u in range(1, 16):
            s = s + runs[..., u]
        runs = s
    return runs


def hvi_scalarise_numpy(y, jac, lower, upper):
    """Phase B of `k_point_path_hvi` (kernels_point_path_hvi.hip) in its own operations and order, from path values y (B, m) and their
    Jacobians jac (B, m, d): the C cells dealt over 256 threads (thread t: cells t, t + 256, ... ascending), per cell

        t_k = max(min(y_k, u_ck) - l_ck, 0);  pre_0 = 1, pre_{k+1} = pre_k t_k;  acc = acc + pre_m
        suf_{m-1} = 1, suf_{k-1} = suf_k t_k;  w_k = w_k + pre_k suf_k  where l_ck < y_k < u_ck (both strict)

    the thread partials added as `_sum_16x16` adds them, grad = w_0 J_0, then + w_t J_t with t ascending; a NaN among the m values:
    HVI = -inf and a zero gradient.  Returns (hvi (B,), grad (B, d), w (B, m))."""
    y, jac = np.atleast_2d(np.asarray(y, dtype=float)), np.asarray(jac, dtype=float)
    lower, upper = np.atleast_2d(np.asarray(lower, dtype=float)), np.atleast_2d(np.asarray(upper, dtype=float))
    B, m = y.shape
    rounds = -(-len(lower) // 256)
    pad = np.zeros((rounds * 256 - len(lower), m))  # a cell [0, 0]^m adds +0.0 to acc and nothing to w: the thread has no such cell
    lo, up = np.vstack([lower, pad]).reshape(rounds, 256, m), np.vstack([upper, pad]).reshape(rounds, 256, m)
    acc, w = np.zeros((B, 256)), np.zeros((B, m, 256))
    with np.errstate(invalid="ignore"):
        for r in range(rounds):
            t = [np.fmax(np.fmin(y[:, k, None], up[r, :, k]) - lo[r, :, k], 0.0) for k in range(m)]
            pre = [np.ones((B, 256))]
            for k in range(m):
                pre.append(pre[k] * t[k])
            acc = acc + pre[m]
            suf = np.ones((B, 256))
            for k in range(m - 1, -1, -1):
                inside = (lo[r, :, k] < y[:, k, None]) & (y[:, k, None] < up[r, :, k])
                w[:, k] = np.where(inside, w[:, k] + pre[k] * suf, w[:, k])
                suf = suf * t[k]
        hvi, w = _sum_16x16(acc), _sum_16x16(w)
        grad = w[:, 0, None] * jac[:, 0]
        for k in range(1, m):
            grad = grad + w[:, k, None] * jac[:, k]
    bad = np.isnan(y).any(axis=1)
    hvi[bad], grad[bad] = -np.inf, 0.0
    return hvi, grad, w


def hvi_grad_numpy(model, dr, X, members, lower, upper, parts=False, from_device=None):
    """The dense float64 restatement of `bogp_point_eval_path_hvi`: the hypervolume improvement (B,) of member members[b]'s joint draw
    at row b of X over the cells (lower, upper), and its input gradient (B, d).  With `paths_multi_numpy`'s own gt:

        y_t   = beta + sum_n c_{j,t}[n] r_n(x) + sum_l Wt[l, j m + t] cos(omega_l . x + phi_l),   c_{j,t} = gamma_t - gt_{j,t}, Wt = sqrt(2 sigma2_t / L) W
        J_tk  = sum_n c_{j,t}[n] d r_n / d x_k - sum_l Wt[l, j m + t] sin(omega_l . x + phi_l) omega_lk        (`path_grad_numpy`'s derivative)
        HVI   = sum_c prod_k max(0, min(y_k, u_ck) - l_ck),   grad = sum_t w_t J_t,   w_t = sum_c [l_ct < y_t < u_ct] prod_{i != t} t_i

    the scalarisation by `hvi_scalarise_numpy`.  `parts=True` adds a dict: y (B, m), jac (B, m, d), w (B, m) and the sums of the ABSOLUTE
    terms A_v (B, m) of every value and A_g (B, m, d) of every Jacobian entry.  `from_device=(y, jac)`: the scalarisation alone, on
    values the device returned -- it then reproduces the device's HVI and gradient byte for byte."""
    if from_device is not None:
        hvi, grad, w = hvi_scalarise_numpy(from_device[0], from_device[1], lower, upper)
        return (hvi, grad, dict(y=from_device[0], jac=from_device[1], w=w)) if parts else (hvi, grad)
    st = state_of_multi(model)
    X = np.atleast_2d(np.asarray(X, dtype=float))
    members = np.asarray(members, dtype=int).ravel()
    m, L = st.y.shape[1], len(dr.phase)
    cols = members[:, None] * m + np.arange(m)  # (B, m)
    Wt = (np.sqrt(2.0 * st.sigma2 / L) * dr.weights[:, cols])  # (L, B, m)
    _, gt = paths_multi_numpy(st, dr, st.X[:1])
    R = correlation(st, st.X, st.X) + np.diag(st.nugget)
    c = np.linalg.solve(R, st.y - st.beta)[:, None, :] - gt[:, cols]  # (N, B, m)
    ph = X @ dr.omega.T + dr.phase  # (B, L)
    r, rdx = correlation(st, X, st.X), correlation_dx(st, X, st.X)
    y = st.beta + np.einsum("bn,nbt->bt", r, c) + np.einsum("bl,lbt->bt", np.cos(ph), Wt)
    u = -np.sin(ph)[:, :, None] * Wt.transpose(1, 0, 2)  # (B, L, m)
    jac = np.einsum("nbt,bnk->btk", c, rdx) + np.einsum("blt,lk->btk", u, dr.omega)
    hvi, grad, w = hvi_scalarise_numpy(y, jac, lower, upper)
    if not parts:
        return hvi, grad
    A_v = abs(st.beta) + np.einsum("bn,nbt->bt", np.abs(r), np.abs(c)) + np.abs(Wt).sum(axis=0)
    A_g = np.einsum("nbt,bnk->btk", np.abs(c), np.abs(rdx)) + np.einsum("lbt,lk->btk", np.abs(Wt), np.abs(dr.omega))
    return hvi, grad, dict(y=y, jac=jac, w=w, A_v=A_v, A_g=A_g)


def tighten(lo, hi, sd, tau):
    """The POLISH bounds of `feasible_merit_numpy` from the true intervals [lo, hi] (n_con,): plo = lo + tau sd, phi = hi - tau sd with sd
    the constraints' prior standard deviations -- a quadratic penalty converges from outside the feasible set, so it is set against an
    interval `tau` standard deviations inside the true one.  An interval narrower than 2 tau sd becomes its midpoint; infinite bounds
    stay infinite.  Returns (plo, phi)."""
    lo, hi, sd = np.asarray(lo, dtype=float).ravel(), np.asarray(hi, dtype=float).ravel(), np.asarray(sd, dtype=float).ravel()
    plo, phi = lo + tau * sd, hi - tau * sd
    with np.errstate(invalid="ignore"):
        narrow = plo > phi
        mid = 0.5 * lo + 0.5 * hi
    return np.where(narrow, mid, plo), np.where(narrow, mid, phi)


def feasible_scalarise_numpy(y, jac, n_obj, lower, upper, plo, phi, sigma2, minimize=True, rho=100.0):
    """Phase B of `k_point_path_feasible` (kernels_point_path_feasible.hip) in its own operations and order, from path values y (B, m)
    and their Jacobians jac (B, m, d); columns 0 .. n_obj - 1 the objectives, the rest constraints with polish bounds [plo, phi]:

        i ascending:  d1 = plo_i - c_i, d2 = c_i - phi_i;  e = d1 > 0 ? d1 : 0;  up = d2 > e;  e = up ? d2 : e;  v = e inv_sd_i
                      P = P + v v;  g = (2 v) inv_sd_i;  u_i = up ? g : 0 - g
        n_obj = 1:    F = (s y_0) inv_sd_0, W_0 = s inv_sd_0                          (s = -1 when minimising)
        n_obj >= 2:   (HVI, w) by `hvi_scalarise_numpy` over the objective columns;  F = HVI f_scale, W_t = w_t f_scale, f_scale = prod inv_sd_k
        merit = F - rho P;   grad = W_0 J_0, + W_t J_t (t ascending), then - (rho u_i) J_{n_obj+i} (i ascending)

    inv_sd = 1 / sqrt(sigma2) (m,); a NaN among the m values: merit = -inf and a zero gradient.  Returns (merit (B,), grad (B, d), a dict:
    F, P (B,), W (B, n_obj), u (B, n_con))."""
    y, jac = np.atleast_2d(np.asarray(y, dtype=float)), np.asarray(jac, dtype=float)
    B, m = y.shape
    n_obj = int(n_obj)
    plo, phi = np.asarray(plo, dtype=float).ravel(), np.asarray(phi, dtype=float).ravel()
    inv_sd = 1.0 / np.sqrt(np.asarray(sigma2, dtype=float).ravel())
    if not 1 <= n_obj < m or len(plo) != m - n_obj or len(phi) != m - n_obj or len(inv_sd) != m:
        raise ValueError("n_obj = %d objectives among %d targets; plo, phi one bound per constraint, sigma2 one value per target" % (n_obj, m))
    P, u = np.zeros(B), np.zeros((B, m - n_obj))
    with np.errstate(invalid="ignore"):
        for i in range(m - n_obj):
            c, isd = y[:, n_obj + i], inv_sd[n_obj + i]
            d1, d2 = plo[i] - c, c - phi[i]
            e = np.where(d1 > 0.0, d1, 0.0)
            up = d2 > e
            e = np.where(up, d2, e)
            v = e * isd
            P = P + v * v
            g = (2.0 * v) * isd
            u[:, i] = np.where(up, g, 0.0 - g)
        if n_obj == 1:
            s = -1.0 if minimize else 1.0
            F, W = (s * y[:, 0]) * inv_sd[0], np.full((B, 1), s * inv_sd[0])
        else:
            f_scale = 1.0
            for k in range(n_obj):
                f_scale = f_scale * inv_sd[k]
            hvi, _, w = hvi_scalarise_numpy(np.where(np.isnan(y[:, :n_obj]), 0.0, y[:, :n_obj]), jac[:, :n_obj], lower, upper)
            F, W = hvi * f_scale, w * f_scale
        merit = F - rho * P
        grad = W[:, 0, None] * jac[:, 0]
        for t in range(1, n_obj):
            grad = grad + W[:, t, None] * jac[:, t]
        for i in range(m - n_obj):
            grad = grad - (rho * u[:, i])[:, None] * jac[:, n_obj + i]
    bad = np.isnan(y).any(axis=1)
    merit[bad], grad[bad] = -np.inf, 0.0
    return merit, grad, dict(F=F, P=P, W=W, u=u)


def feasible_merit_numpy(model, dr, X, members, n_obj, lower, upper, plo, phi, minimize=True, rho=100.0, parts=False, from_device=None,
                         sigma2=None):
    """The dense float64 restatement of `bogp_point_eval_path_feasible`: the merit (B,) of member members[b]'s joint draw of n_obj
    objectives and the constraints at row b of X, and its input gradient (B, d):

        merit = F - rho sum_i (e_i / sd_i)^2,   e_i = max(plo_i - c_i, c_i - phi_i, 0)       against the POLISH bounds (`tighten`)
        F     = +-y_0 / sd_0  (n_obj = 1; lower = upper = None)   or   HVI(y_0 .. y_{n_obj-1}) / prod_k sd_k  over the cells (lower, upper)

    y and J as `hvi_grad_numpy` restates them, the scalarisation by `feasible_scalarise_numpy`.  `parts=True` adds a dict: y (B, m), jac
    (B, m, d), A_v, A_g (the sums of the absolute terms, `hvi_grad_numpy`'s) and F, P, W, u.  `from_device=(y, jac)` with `sigma2` (m,):
    the scalarisation alone, on values the device returned -- it then reproduces the device's merit and gradient byte for byte."""
    if from_device is not None:
        merit, grad, p = feasible_scalarise_numpy(from_device[0], from_device[1], n_obj, lower, upper, plo, phi, sigma2, minimize, rho)
        return (merit, grad, dict(p, y=from_device[0], jac=from_device[1])) if parts else (merit, grad)
    st = state_of_multi(model)
    m = st.y.shape[1]
    _, _, p = hvi_grad_numpy(st, dr, X, members, np.zeros((1, m)), np.full((1, m), np.inf), parts=True)  # y, J and their absolute sums
    merit, grad, ps = feasible_scalarise_numpy(p["y"], p["jac"], n_obj, lower, upper, plo, phi, st.sigma2 if sigma2 is None else sigma2, minimize, rho)
    return (merit, grad, dict(ps, y=p["y"], jac=p["jac"], A_v=p["A_v"], A_g=p["A_g"])) if parts else (merit, grad)


def merge_ranks(best_val, best_idx, k=None):
    """A member's proposal list from its rankings (n_tiers, k'), tier after tier: the A ranks whose value is above -inf (rows whose
    drawn constraints hold, best objective first), then the B ranks (least violating first) whose row is not already listed, then
    those of every further tier (`hvi_constrained_select_numpy`'s V); unfilled slots (-1) are dropped and the list is cut to `k`
    (default k').  Returns a list of (row, which, rank): which = 0 for an A rank, 1 for a B rank, ..."""
    best_val, best_idx = np.asarray(best_val), np.asarray(best_idx)
    k = best_val.shape[-1] if k is None else int(k)
    out, seen = [], set()
    for which in range(best_val.shape[0]):
        for r in range(best_val.shape[-1]):
            gi = int(best_idx[which, r])
            if gi >= 0 and best_val[which, r] > -np.inf and gi not in seen:
                out.append((gi, which, r))
                seen.add(gi)
    return out[:k]
