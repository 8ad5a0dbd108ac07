"""MOBO ask() at a realistic state (N = 100, d = 3, m = 3; MOBO-style y: MinMax-scaled, negated).
`device` (the default): what `ask()` does under `bogp.install()` with optimizer="sweep-device", max_FEs = 1e5 -- build
`bogp.EHVI` from y (Pareto front + cells on the host) and sweep 1e5 device-generated candidates -- on a `bogp.GaussianProcess`
fitted on the device.  `reference`: the reference's own MOBO.ask() with its default inner optimiser (OnePlusOne_Cholesky_CMA
maximising the torch EHVI, one row per call) on the reference's CPU GaussianProcess (needs the reference tree).
Prints the median of 5 asks in ms (`profiles/ehvi_mobo_ask.txt`)."""
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
N, d, m, M = 100, 3, 3, 100_000


def data():
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 10, size=(N, d))
    F = np.column_stack([X[:, 0] ** 2 + X[:, 1] + X[:, 2] ** 2, X[:, 0] + X[:, 1] ** 2 + X[:, 2] ** 2, X[:, 0] ** 2 + X[:, 1] + X[:, 2]])
    y = -(F - F.min(0)) / (F.max(0) - F.min(0))
    return X, F, y


def device():
    import bogp
    from bogp import optim

    X, _, y = data()
    gp = bogp.GaussianProcess(mean=bogp.trend.constant_trend(d, beta=0.0), corr="matern", thetaL=[1e-3] * d, thetaU=[1e2] * d, nugget=1e-6,
                              random_start=3, wait_iter=3, eval_budget=200)  # fmt: skip
    np.random.seed(0)
    gp.fit(X, y)
    box = optim.Box([(0.0, 10.0)] * d)
    ts = []
    for rep in range(6):  # the first pays the initialisation of the candidate generator
        t0 = time.perf_counter()
        crit = bogp.EHVI(model=gp, ref_point=np.min(y, axis=0) * 0.8, Y=y)
        x, f = optim.argmax_restart(crit, box, eval_budget=M, optimizer="sweep-device")
        ts.append(time.perf_counter() - t0)
    print("device: ask (EHVI criterion + sweep of %d device-generated candidates, %d cells) median %.2f ms (first %.2f ms)"
          % (M, len(crit.cell_lower_bounds), 1e3 * np.median(ts[1:]), 1e3 * ts[0]))  # fmt: skip


def reference():
    sys.path.insert(0, os.environ.get("BOGP_REFERENCE", "/root/reference"))
    sys.path.insert(0, os.path.join(ROOT, "oracle", "shims"))
    from bayes_optim import MOBO
    from bayes_optim.search_space import RealSpace
    from bayes_optim.surrogate import GaussianProcess

    X, F, _ = data()
    space = RealSpace([0, 10]) * d
    model = GaussianProcess(thetaL=np.full(d, 1e-3), thetaU=np.full(d, 1e2), nugget=1e-6, noise_estim=False, likelihood="concentrated")
    opt = MOBO(search_space=space, obj_fun=[lambda x, k=k: 0.0 for k in range(m)], n_obj=m, model=model, max_FEs=10_000, DoE_size=N,
               eval_type="list", n_job=1, verbose=False, minimize=True, acquisition_optimization={"optimizer": "OnePlusOne_Cholesky_CMA"})  # fmt: skip
    opt.tell([list(x) for x in X], [tuple(f) for f in F])
    ts = []
    for rep in range(5):
        t0 = time.perf_counter()
        opt.ask(1)
        ts.append(time.perf_counter() - t0)
    print("reference: MOBO.ask(1), %s + torch EHVI on the CPU GaussianProcess: median %.1f ms" % (opt._optimizer, 1e3 * np.median(ts)))


if __name__ == "__main__":
    (reference if sys.argv[1:] == ["reference"] else device)()
