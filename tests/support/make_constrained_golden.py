"""Writes tests/golden/G45_constrained.npz from the imported reference (run on a machine that has the reference tree).  One state:
a reference `GaussianProcess` with a fixed constant trend (the only one several targets take, gpr.py:787), Matern-3/2, d = 4,
N = 200, pinned at given hyper-parameters in noise_estim mode (so that sigma2 differs per target) on y with three columns -- one
objective, standardised as BaseBO.update_model standardises the fitness (base.py:433-437), and two constraints, each divided by its
standard deviation and not shifted, as `install(expensive_constraints=True)` scales them.  Stored: X, y, par, kernel, mode,
noise_var, the reference's sigma2 and its `predict` moments (mu, mse: M x 3) on 2048 candidates Xs.  Data only."""
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

KERNEL_MATERN32, MODE_NOISE_ESTIM = 2, 2  # include/bogp.h


def main():
    rng = np.random.default_rng(4500)
    N, d, M = 200, 4, 2048
    X = rng.uniform(-2, 2, size=(N, d))

    def columns(Z):
        f = np.sum((Z - 0.5) ** 2, 1)
        g1 = 1.0 - Z[:, 0] - Z[:, 1] + 0.5 * np.sin(3 * Z[:, 2])  # g1 <= 0 feasible
        g2 = np.sum(Z**2, 1) - 6.0 + Z[:, 3]  # an interval on g2
        return f, g1, g2

    f, g1, g2 = columns(X)
    y = np.column_stack([(f - f.mean()) / f.std(), g1 / g1.std(), g2 / g2.std()])
    gp = GaussianProcess(mean=trend.constant_trend(d, beta=0.0), corr="matern", thetaL=[1e-4] * d, thetaU=[1e2] * d, nugget=1e-6,
                         noise_estim=True)  # fmt: skip
    gp._check_data(X, y)
    par = np.r_[np.full(d, 0.8), 0.97]
    env = {}
    llf = gp.log_likelihood_concentrated(par, env)
    assert np.isfinite(llf), llf
    gp.theta_ = par[:d]
    gp.noise_var = env["noise_var"]
    gp.sigma2 = np.atleast_1d(env["sigma2"]).astype(float)
    gp.rho, gp.Yt, gp.C = env["rho"], env["Yt"], env["C"]
    gp.compute_beta_gamma()
    gp.is_fitted = True
    Xs = rng.uniform(-2.2, 2.2, size=(M, d))
    mu, mse = gp.predict(Xs, eval_MSE=True)
    out = dict(X=X, y=y, par=par, kernel=np.array(KERNEL_MATERN32), mode=np.array(MODE_NOISE_ESTIM), noise_var=np.array(0.0),
               sigma2=gp.sigma2, Xs=Xs, mu=np.asarray(mu, dtype=float), mse=np.asarray(mse, dtype=float))  # fmt: skip
    path = os.path.join(ROOT, "tests", "golden", "G45_constrained.npz")
    np.savez_compressed(path, **out)
    print("G45_constrained %.1f KB; sigma2 %s; mse range %.3g .. %.3g" % (os.path.getsize(path) / 1024, gp.sigma2, mse.min(), mse.max()))


if __name__ == "__main__":
    main()
