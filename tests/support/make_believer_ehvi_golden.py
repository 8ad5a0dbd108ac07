"""Writes tests/golden/G44_believer_ehvi.npz from the imported reference (run on a machine that has the reference tree; torch and
sklearn must be importable).  Two noiseless states (nugget 0) with a fixed constant trend (the only one several targets take,
gpr.py:787), d = 3, M = 1500 candidates: m = 2 (Matern-3/2, N = 60, prefix "m2_") and m = 3 (squared exponential, N = 90, "m3_"),
pinned at given theta through `log_likelihood_concentrated(par, env)` on MOBO-style y (the objectives of make_ehvi_golden.py,
MinMax-scaled and negated, mobo.py:66-76).  Four believed rows per state -- two pending points off the candidate set, then two
candidate rows -- and, for each prefix j = 1 .. 4 of them, a reference model REBUILT on X + {p_1 .. p_j} with y = mu(p) at the
same theta.  "Fixed hyper-parameters" includes sigma2: the rebuilt model's is pinned to the committed model's (its own
concentrated value is sigma2 N / (N + j), because a believed mean adds no residual -- printed, and asserted, here).  Stored per
state: X, y, par, kernel, mode, beta, Xs, the committed model's sigma2, ref_point (min(y) * 0.8, mobo.py:63), believed (4, d),
believed_rows, and per prefix the rebuilt model's own predict (mu_j, mse_j: (4, M, m); sigma2_j (4, m)), the float64 cells of the
reference's NondominatedPartitioning on y u mu(p_1 .. p_j) (lower_j, upper_j) and the reference's own per-row EHVI on the rebuilt
model exactly as MOBO builds it (float32 tensors, mobo.py:177-186, one row per call): ehvi32_j (4, M)."""
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

KERNEL_SE, KERNEL_MATERN32, MODE_NOISELESS = 0, 2, 0  # include/bogp.h
BETA = 0.0


def objectives(X, m):
    f = [np.sum((X - 1.0) ** 2, 1), np.sum((X + 1.0) ** 2, 1), np.sum(np.abs(X), 1) + np.sin(3 * X[:, 0])]
    return np.column_stack(f[:m])


def pinned(X, y, corr, par):
    d = X.shape[1]
    gp = GaussianProcess(mean=trend.constant_trend(d, beta=BETA), corr=corr, thetaL=[1e-4] * d, thetaU=[1e2] * d, nugget=0)
    assert gp.estimation_mode == "noiseless" and not gp.estimate_trend
    gp._check_data(X, y)
    env = {}
    llf = gp.log_likelihood_concentrated(par, env)
    assert np.isfinite(llf), llf
    gp.theta_ = par
    gp.noise_var = env["noise_var"]
    gp.sigma2 = np.atleast_1d(env["sigma2"]).astype(float)
    gp.rho, gp.Yt, gp.C = env["rho"], env["Yt"], env["C"]
    gp.compute_beta_gamma()
    gp.is_fitted = True
    return gp


def state(m, N, corr, kernel, par, seed):
    rng = np.random.default_rng(seed)
    d, M = 3, 1500
    X = rng.uniform(-2, 2, size=(N, d))
    y = MinMaxScaler().fit_transform(objectives(X, m)) * (-1) ** True  # mobo.py:72-76 with minimize=True
    gp = pinned(X, y, corr, par)
    Xs = rng.uniform(-2.2, 2.2, size=(M, d))
    mu, mse = gp.predict(Xs, eval_MSE=True)
    rows = np.argsort(-mse[:, 0])[[0, 7]]  # two candidate rows the model knows little about
    believed = np.vstack([rng.uniform(-2, 2, size=(2, d)), Xs[rows]])
    ref_point = np.min(y, axis=0) * 0.8  # mobo.py:63
    out = dict(X=X, y=y, par=par, kernel=np.array(kernel), mode=np.array(MODE_NOISELESS), beta=np.array(BETA), Xs=Xs, sigma2=gp.sigma2,
               ref_point=ref_point, believed=believed, believed_rows=rows)  # fmt: skip
    mu_j, mse_j, s2_j, e32_j = [], [], [], []
    for j in range(1, 5):
        P = believed[:j]
        y_j = np.vstack([y, gp.predict(P).reshape(j, m)])
        gp_j = pinned(np.vstack([X, P]), y_j, corr, par)
        np.testing.assert_allclose(gp_j.sigma2, gp.sigma2 * N / (N + j), rtol=1e-6)  # a believed mean adds no residual
        gp_j.sigma2 = gp.sigma2.copy()  # fixed hyper-parameters include sigma2
        a, s = gp_j.predict(Xs, eval_MSE=True)
        mu_j.append(a)
        mse_j.append(s)
        s2_j.append(gp_j.sigma2.copy())
        part64 = NondominatedPartitioning(ref_point=torch.tensor(ref_point, dtype=torch.float64), Y=torch.tensor(y_j, dtype=torch.float64))
        lo, hi = (np.asarray(b, dtype=float) for b in part64.get_hypercell_bounds())
        out["lower_%d" % j], out["upper_%d" % j] = lo, hi
        part32 = NondominatedPartitioning(ref_point=torch.Tensor(ref_point), Y=torch.Tensor(y_j))
        crit = EHVI(model=gp_j, ref_point=ref_point.tolist(), partitioning=part32)
        e32_j.append(np.array([float(np.ravel(crit(x.reshape(1, -1)))[0]) for x in Xs]))
        print("m%d prefix %d: cells %d, max EHVI %.4g" % (m, j, len(lo), e32_j[-1].max()))
    print("m%d cond(R) %.3g  sigma2 %s" % (m, np.linalg.cond(gp.C @ gp.C.T), np.round(gp.sigma2, 4)))
    out.update(mu_j=np.array(mu_j), mse_j=np.array(mse_j), sigma2_j=np.array(s2_j), ehvi32_j=np.array(e32_j))
    return {"m%d_" % m + k: v for k, v in out.items()}


def main():
    out = {}
    out.update(state(2, 60, "matern", KERNEL_MATERN32, np.array([4.5, 3.0, 6.0]), 4402))
    out.update(state(3, 90, "squared_exponential", KERNEL_SE, np.array([3.0, 2.25, 3.75]), 4403))
    path = os.path.join(ROOT, "tests", "golden", "G44_believer_ehvi.npz")
    np.savez_compressed(path, **out)
    print("G44_believer_ehvi %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
