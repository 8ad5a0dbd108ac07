"""Writes tests/golden/G48_constrained_ehvi.npz from the imported reference (run on a machine that has the reference tree; torch and
sklearn must be importable).  One state: a reference `GaussianProcess` with a fixed constant trend (the only one several targets
take, gpr.py:787), Matern-3/2, d = 4, N = 200, pinned at given hyper-parameters in noise_estim mode (so that sigma2 differs per
target) on y with four columns -- two MOBO-style objectives (the raw objectives MinMax-scaled and negated, as mobo.py:66-76 forms
`self.y` for minimisation) and two constraints, each divided by its standard deviation and not shifted, as
`install(expensive_constraints=True, constrained_mobo=True)` scales them.  Stored: X, y, par, kernel, mode, noise_var, the reference's
sigma2 and its `predict` moments (mu, mse: M x 4) on 2048 candidates Xs, the constraint bounds lo / hi, ref_point (min(y) * 0.8 of the
objective columns, mobo.py:63), the reference's float64 `NondominatedPartitioning` cells of the FEASIBLE front, and the reference's
own per-row float32 EHVI of the two objective columns over those cells (its criterion on a wrapper that slices the model's moments,
one row per call).  Data only."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "shims"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.preprocessing import MinMaxScaler  # noqa: E402

from bayes_optim.multi_objective import EHVI  # noqa: E402
from bayes_optim.surrogate import GaussianProcess, trend  # noqa: E402
from bayes_optim.utils.multi_objective.box_decompositions import NondominatedPartitioning  # noqa: E402

from support.constrained_ref import feasibility  # noqa: E402

KERNEL_MATERN32, MODE_NOISE_ESTIM = 2, 2  # include/bogp.h
M_OBJ = 2


class ObjectiveColumns:
    """the reference's criterion asks its model for `predict(X, eval_MSE=True)`: the first M_OBJ columns of the four-target model's"""

    def __init__(self, gp):
        self.gp = gp

    def predict(self, X, eval_MSE=True):
        mu, mse = self.gp.predict(X, eval_MSE=True)
        return mu[:, :M_OBJ], mse[:, :M_OBJ]


def main():
    rng = np.random.default_rng(4800)
    N, d, M = 200, 4, 2048
    X = rng.uniform(-2, 2, size=(N, d))
    F = np.column_stack([np.sum((X - 1.0) ** 2, 1), np.sum((X + 1.0) ** 2, 1)])
    g1 = 0.5 - X[:, 0] - X[:, 1] + 0.5 * np.sin(3 * X[:, 2])  # g1 <= 0 feasible
    g2 = np.sum(X**2, 1) - 4.0  # an interval on g2
    y = np.column_stack([MinMaxScaler().fit_transform(F) * (-1) ** True, g1 / g1.std(), g2 / g2.std()])  # mobo.py:72-76 with minimize=True
    lo, hi = np.array([-np.inf, -1.5]), np.array([0.0, 1.0])
    gp = GaussianProcess(mean=trend.constant_trend(d, beta=0.0), corr="matern", thetaL=[1e-4] * d, thetaU=[1e2] * d, nugget=1e-6,
                         noise_estim=True)  # fmt: skip
    gp._check_data(X, y)
    par = np.r_[np.full(d, 4.0), 0.97]  # (shorter length scales than G45: the log-likelihood of the min-max scaled columns must stay <= 0, gpr.py:981)
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
    mu, mse = (np.asarray(a, dtype=float) for a in gp.predict(Xs, eval_MSE=True))
    feasible = np.all((y[:, M_OBJ:] >= lo) & (y[:, M_OBJ:] <= hi), axis=1)
    yo = y[feasible, :M_OBJ]
    ref_point = np.min(y[:, :M_OBJ], axis=0) * 0.8  # mobo.py:63
    part64 = NondominatedPartitioning(ref_point=torch.tensor(ref_point, dtype=torch.float64), Y=torch.tensor(yo, dtype=torch.float64))
    assert len(part64.pareto_Y) >= 3, "at least 3 feasible front points above the reference point"
    lower, upper = (np.asarray(b, dtype=float) for b in part64.get_hypercell_bounds())
    P = np.ones(M)
    for j in range(2):
        P = P * feasibility(mu[:, M_OBJ + j], mse[:, M_OBJ + j], gp.sigma2[M_OBJ + j], lo[j], hi[j])
    assert 0 < P.min() and P.max() > 0.5, (P.min(), P.max())
    # the reference's own criterion on the objective columns: float32 tensors (mobo.py:180-181), one row per call
    part32 = NondominatedPartitioning(ref_point=torch.Tensor(ref_point), Y=torch.Tensor(yo))
    crit = EHVI(model=ObjectiveColumns(gp), ref_point=ref_point.tolist(), partitioning=part32)
    ehvi32 = np.array([float(np.ravel(crit(x.reshape(1, -1)))[0]) for x in Xs])
    out = dict(X=X, y=y, par=par, kernel=np.array(KERNEL_MATERN32), mode=np.array(MODE_NOISE_ESTIM), noise_var=np.array(0.0),
               sigma2=gp.sigma2, Xs=Xs, mu=mu, mse=mse, lo=lo, hi=hi, ref_point=ref_point, lower=lower, upper=upper, ehvi32=ehvi32)  # fmt: skip
    path = os.path.join(ROOT, "tests", "golden", "G48_constrained_ehvi.npz")
    np.savez_compressed(path, **out)
    print("G48_constrained_ehvi %.1f KB; feasible %d of %d, front %d, cells %d; P %.3g .. %.3g; sigma2 %s"
          % (os.path.getsize(path) / 1024, feasible.sum(), N, len(part64.pareto_Y), len(lower), P.min(), P.max(), gp.sigma2))  # fmt: skip


if __name__ == "__main__":
    main()
