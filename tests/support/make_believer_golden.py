"""Writes tests/golden/G43_believer.npz from the imported reference (run on a machine that has the reference tree; sklearn must
be importable).  Two noiseless states (nugget 0), N = 70, d = 3, M = 1500 candidates: Matern-3/2 under ordinary kriging (prefix
"m32ok_") and the squared exponential under simple kriging ("sesk_"), pinned at given theta through
`log_likelihood_concentrated(par, env)`.  Four believed rows per state -- two pending points off the candidate set, then two
candidate rows -- and, for each prefix j = 1 .. 4 of them, the reference's OWN `predict(Xs, eval_MSE=True)` of a reference model
REBUILT on X + {p_1 .. p_j} with y = mu(p) at the same theta: its mean, its MSE and its sigma2 (concentrated, so it changes with
N: a test compares MSE_j / sigma2_j).  Stored per state: X, y, par, kernel, mode, estimate_trend, beta, Xs, the committed
model's mu / mse / sigma2, believed (4, d), believed_rows (the candidate indices of the last two), mu_j, mse_j (4, M), sigma2_j (4)."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "shims"))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

from bayes_optim.surrogate import GaussianProcess, trend  # noqa: E402

KERNEL_SE, KERNEL_MATERN32, MODE_NOISELESS = 0, 2, 0  # include/bogp.h


def pinned(X, y, corr, par, ordinary, beta):
    d = X.shape[1]
    gp = GaussianProcess(mean=trend.constant_trend(d, beta=None if ordinary else beta), corr=corr, thetaL=[1e-4] * d, thetaU=[1e2] * d,
                         nugget=0)  # fmt: skip
    assert gp.estimation_mode == "noiseless" and bool(gp.estimate_trend) == ordinary
    gp._check_data(X, y)
    env = {}
    llf = gp.log_likelihood_concentrated(par, env)
    assert np.isfinite(llf), llf
    gp.theta_ = par
    gp.noise_var = env["noise_var"]
    gp.sigma2 = np.atleast_1d(env["sigma2"]).astype(float)
    gp.rho, gp.Yt, gp.C = env["rho"], env["Yt"], env["C"]
    if ordinary:
        gp.Ft, gp.G, gp.Q = env["Ft"], env["G"], env["Q"]
    gp.compute_beta_gamma()
    gp.is_fitted = True
    return gp


def state(prefix, corr, kernel, par, ordinary, seed):
    rng = np.random.default_rng(seed)
    N, d, M = 70, 3, 1500
    X = rng.uniform(-2, 2, size=(N, d))
    y = np.sin(X @ np.array([0.9, -0.6, 0.4])) + 0.25 * np.sum(X**2, axis=1) + 0.05 * rng.normal(size=N)
    beta = 0.5
    gp = pinned(X, y, corr, par, ordinary, beta)
    Xs = rng.uniform(-2.2, 2.2, size=(M, d))
    mu, mse = gp.predict(Xs, eval_MSE=True)
    rows = np.argsort(-mse[:, 0])[[0, 7]]  # two candidate rows the model knows little about
    believed = np.vstack([rng.uniform(-2, 2, size=(2, d)), Xs[rows]])
    mu_j, mse_j, s2_j = [], [], []
    for j in range(1, 5):
        P = believed[:j]
        gp_j = pinned(np.vstack([X, P]), np.r_[y, gp.predict(P).ravel()], corr, par, ordinary, beta)
        m, s = gp_j.predict(Xs, eval_MSE=True)
        mu_j.append(m[:, 0])
        mse_j.append(s[:, 0])
        s2_j.append(float(gp_j.sigma2[0]))
    cond = np.linalg.cond(gp.C @ gp.C.T)
    print("%s cond(R) %.3g  sigma2 %.4g -> %s" % (prefix, cond, gp.sigma2[0], np.round(s2_j, 4)))
    out = dict(X=X, y=y.reshape(-1, 1), par=par, kernel=np.array(kernel), mode=np.array(MODE_NOISELESS), estimate_trend=np.array(ordinary),
               beta=np.array(beta), Xs=Xs, mu=mu[:, 0], mse=mse[:, 0], sigma2=gp.sigma2, believed=believed, believed_rows=rows,
               mu_j=np.array(mu_j), mse_j=np.array(mse_j), sigma2_j=np.array(s2_j))  # fmt: skip
    return {prefix + k: v for k, v in out.items()}


def main():
    out = {}
    out.update(state("m32ok_", "matern", KERNEL_MATERN32, np.array([1.5, 1.0, 2.0]), True, 4301))
    out.update(state("sesk_", "squared_exponential", KERNEL_SE, np.array([2.0, 1.5, 2.5]), False, 4302))
    path = os.path.join(ROOT, "tests", "golden", "G43_believer.npz")
    np.savez_compressed(path, **out)
    print("G43_believer %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
