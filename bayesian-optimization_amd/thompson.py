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
its conditional law."""
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


def state_of(model):
    """What the formulas read, from a fitted `GaussianProcess` (or a `dense_state`, returned as it is).  The refusals live here."""
    if isinstance(model, SimpleNamespace):
        refuse_kernel(model.kernel)
        return model
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
