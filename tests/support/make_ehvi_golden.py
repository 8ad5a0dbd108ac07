"""Writes tests/golden/G39_ehvi.npz from the imported reference (run on a machine that has the reference tree; torch and sklearn
must be importable).  Two states, m = 2 (Matern-3/2) and m = 3 (squared exponential), d = 3: a reference `GaussianProcess` with a
fixed constant trend (the only one several targets take, gpr.py:787) pinned at given hyper-parameters (noise_estim mode, so
that sigma2 differs per target) on MOBO-style y -- the raw objectives MinMax-scaled and negated, as mobo.py:66-76 forms
`self.y` for minimisation.  Stored per state (prefix "m2_" / "m3_"): X, y, par, kernel, mode, noise_var, the reference's
predict on 2048 candidates Xs (mu, mse: M x m), ref_point (min(y) * 0.8, mobo.py:63), the reference's float64 cell bounds
(NondominatedPartitioning on float64 tensors), and the reference's own per-row EHVI exactly as MOBO builds it
(float32 tensors, mobo.py:177-186, one row per call)."""
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
import torch  # noqa: E402
from sklearn.preprocessing import MinMaxScaler  # noqa: E402

from bayes_optim.multi_objective import EHVI  # noqa: E402
from bayes_optim.surrogate import GaussianProcess, trend  # noqa: E402
from bayes_optim.utils.multi_objective.box_decompositions import NondominatedPartitioning  # noqa: E402

KERNEL_SE, KERNEL_MATERN32, MODE_NOISE_ESTIM = 0, 2, 2  # include/bogp.h


def objectives(X, m):
    f = [np.sum((X - 1.0) ** 2, 1), np.sum((X + 1.0) ** 2, 1), np.sum(np.abs(X), 1) + np.sin(3 * X[:, 0])]
    return np.column_stack(f[:m])


def state(m, N, corr, kernel, seed):
    rng = np.random.default_rng(seed)
    d = 3
    X = rng.uniform(-2, 2, size=(N, d))
    y = MinMaxScaler().fit_transform(objectives(X, m)) * (-1) ** True  # mobo.py:72-76 with minimize=True
    gp = GaussianProcess(mean=trend.constant_trend(d, beta=0.0), corr=corr, thetaL=[1e-4] * d, thetaU=[1e2] * d, nugget=1e-6,
                         noise_estim=True)  # fmt: skip
    gp._check_data(X, y)
    par = np.r_[np.full(d, 10.0), 0.95]
    env = {}
    llf = gp.log_likelihood_concentrated(par, env)
    assert np.isfinite(llf), llf
    gp.theta_ = par[:d]
    gp.noise_var = env["noise_var"]
    gp.sigma2 = np.atleast_1d(env["sigma2"]).astype(float)
    gp.rho, gp.Yt, gp.C = env["rho"], env["Yt"], env["C"]
    gp.compute_beta_gamma()
    gp.is_fitted = True
    Xs = rng.uniform(-2.2, 2.2, size=(2048, d))
    mu, mse = gp.predict(Xs, eval_MSE=True)
    ref_point = np.min(y, axis=0) * 0.8  # mobo.py:63
    part64 = NondominatedPartitioning(ref_point=torch.tensor(ref_point, dtype=torch.float64), Y=torch.tensor(y, dtype=torch.float64))
    lo, hi = (np.asarray(b, dtype=float) for b in part64.get_hypercell_bounds())
    # the driver's own criterion: float32 tensors (mobo.py:180-181), one row per call (the inner optimiser's usage)
    part32 = NondominatedPartitioning(ref_point=torch.Tensor(ref_point), Y=torch.Tensor(y))
    crit = EHVI(model=gp, ref_point=ref_point.tolist(), partitioning=part32)
    ehvi32 = np.array([float(np.ravel(crit(x.reshape(1, -1)))[0]) for x in Xs])
    p = "m%d_" % m
    return {p + "X": X, p + "y": y, p + "par": par, p + "kernel": np.array(kernel), p + "mode": np.array(MODE_NOISE_ESTIM),
            p + "noise_var": np.array(0.0), p + "sigma2": gp.sigma2, p + "Xs": Xs, p + "mu": mu, p + "mse": mse,
            p + "ref_point": ref_point, p + "lower": lo, p + "upper": hi, p + "ehvi32": ehvi32}  # fmt: skip


def main():
    out = {}
    out.update(state(2, 60, "matern", KERNEL_MATERN32, 3902))
    out.update(state(3, 90, "squared_exponential", KERNEL_SE, 3903))
    path = os.path.join(ROOT, "tests", "golden", "G39_ehvi.npz")
    np.savez_compressed(path, **out)
    print("G39_ehvi %.1f KB; cells m2 %d, m3 %d" % (os.path.getsize(path) / 1024, len(out["m2_lower"]), len(out["m3_lower"])))


if __name__ == "__main__":
    main()
