"""Writes tests/golden/G41_pcabo.npz from the imported reference (run on a machine that has the reference tree; sklearn must be
importable).  Two states after a short run of the reference's own `PCABO` (extension.py:89-208, its CPU GaussianProcess, the
default "BFGS" inner optimiser) on the weighted sphere of example/example_PCABO.py in [-5, 5]^D: (D = 5, n_components = 0.95)
and (D = 20, n_components = 3).  Stored per state (prefix "d5_" / "d20_"):
  X, y          the reduced training set (pca.transform of the data) and the standardised y the last update_model fitted on
  par, kernel, mode, noise_var, estimate_trend   the fitted hyper-parameters [theta, sigma2] of that model: Matern-3/2,
                ordinary kriging, noisy mode with the nugget 1e-6 -- what a device engine commits to hold the same model
  A, mean, center, bounds, reduced_bounds   pca.components_, pca.mean_, LinearTransform.center, the original box (D x 2),
                `PCABO._compute_bounds` (r x 2)
  Z             4096 uniform candidates of the reduced box
  value         per row what the reference's OWN wrapper from `PCABO._create_acquisition` (EI) returns for it
  penalty       per row the penalty of `penalized_acquisition` (recomputed with its expressions; 0 for a feasible row)
  x_orig        pca.inverse_transform(z) of the first 256 rows
  argmax, top16 np.argmax of `value` and its 16 best rows (ties -> lower index)
  plugin        the EI plugin (min of the standardised y)
The generator asserts that at least 100 rows are feasible and that no mapped coordinate lies within 1e-9 (hi - lo) of a bound.
The driver's run is not bit-reproducible from one invocation to the next (the reference fits with threaded BLAS and its restarts
end in slightly different optima), so a second run writes a different, equally valid pair of states: the committed file is the record."""
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

from bayes_optim.extension import PCABO, RealSpace  # noqa: E402

KERNEL_MATERN32, MODE_NOISY = 2, 1  # include/bogp.h
M = 4096


def state(D, n_components, n_iter, seed):
    np.random.seed(seed)
    w = np.arange(1, D + 1)
    fitness = lambda x: float(np.sum((w * np.asarray(x)) ** 2))  # noqa: E731
    opt = PCABO(search_space=RealSpace([-5, 5]) * D, obj_fun=fitness, DoE_size=2 * D,
                max_FEs=2 * D + n_iter, verbose=False, n_point=1, n_components=n_components,
                acquisition_optimization={"optimizer": "BFGS"})  # fmt: skip
    for _ in range(n_iter + 1):  # the DoE, then n_iter model-based steps
        X = opt.ask()
        opt.tell(X, [fitness(x) for x in X])
    gp, pca = opt.model, opt._pca
    assert gp.estimation_mode == "noisy" and gp.estimate_trend and float(np.ravel(gp.noise_var)[0]) == 1e-6
    bounds = np.array([[-5.0, 5.0]] * D)
    rb = np.array(opt._search_space.bounds, dtype=float)
    r = len(rb)
    Z = np.random.default_rng(seed).uniform(rb[:, 0], rb[:, 1], size=(M, r))
    wrapper = opt._create_acquisition(fun="EI", par={}, return_dx=False)  # functools.partial(penalized_acquisition, ...)
    value = np.array([float(np.ravel(wrapper(z))[0]) for z in Z])
    x_orig = np.array([np.asarray(pca.inverse_transform(z), dtype=float) for z in Z], dtype=float)
    penalty = np.empty(M)
    for i, x_ in enumerate(x_orig):  # extension.py:66-71
        lower, upper = np.nonzero(x_ < bounds[:, 0])[0], np.nonzero(x_ > bounds[:, 1])[0]
        penalty[i] = -1 * (np.sum([bounds[j, 0] - x_[j] for j in lower]) + np.sum([x_[j] - bounds[j, 1] for j in upper]))
    feas = penalty == 0
    assert np.array_equal(value[~feas], penalty[~feas])
    near = np.min(np.minimum(np.abs(x_orig - bounds[:, 0]), np.abs(x_orig - bounds[:, 1])) / (bounds[:, 1] - bounds[:, 0]))
    assert feas.sum() >= 100, feas.sum()
    assert near > 1e-9, near
    order = np.lexsort((np.arange(M), -value))
    Xr = pca.transform(np.array(opt.data))
    y = np.asarray(opt.data.fitness, dtype=float)
    y_ = (y - np.mean(y)) / np.std(y)
    assert np.allclose(gp.X, Xr, rtol=0, atol=1e-12) and np.allclose(gp.y.ravel(), y_, rtol=0, atol=1e-12)
    p = "d%d_" % D
    print("D = %d, r = %d: N = %d, feasible %d of %d, feasible argmax %s, nearest approach to a bound %.2e (hi - lo), "
          "value[top16] - value[top17] = %.3e" % (D, r, len(y_), feas.sum(), M, bool(feas[order[0]]), near, value[order[15]] - value[order[16]]))  # fmt: skip
    return {p + "X": np.asarray(gp.X, dtype=float), p + "y": np.asarray(gp.y, dtype=float).reshape(-1, 1),
            p + "par": np.r_[np.ravel(gp.par["theta"]), np.ravel(gp.par["sigma2"])], p + "kernel": np.array(KERNEL_MATERN32),
            p + "mode": np.array(MODE_NOISY), p + "noise_var": np.array(1e-6), p + "estimate_trend": np.array(True),
            p + "A": np.asarray(pca.components_, dtype=float), p + "mean": np.asarray(pca.mean_, dtype=float),
            p + "center": np.asarray(pca.center, dtype=float), p + "bounds": bounds, p + "reduced_bounds": rb, p + "Z": Z,
            p + "value": value, p + "penalty": penalty, p + "x_orig": x_orig[:256], p + "argmax": np.array(int(np.argmax(value))),
            p + "top16": order[:16].astype(np.int64), p + "plugin": np.array(float(np.min(gp.y)))}  # fmt: skip


def main():
    out = {}
    out.update(state(5, 0.95, 8, 4105))
    out.update(state(20, 3, 6, 4120))
    path = os.path.join(ROOT, "tests", "golden", "G41_pcabo.npz")
    np.savez_compressed(path, **out)
    print("G41_pcabo %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
