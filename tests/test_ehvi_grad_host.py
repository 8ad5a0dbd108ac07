"""Input gradient of EHVI, the parts that need no GPU: the NumPy restatement (tests/support/ehvi_grad_ref.py) against central
differences of the float64 EHVI restatement over the same posterior, the clamp at a training point, `EHVI(input_gradient=True)`
and the routing of `optim.argmax_restart` / `polish_topk` on the oracle-backed stand-in (tests/support/ehvi_grad_engine.py), and
the reference's `MOBO` under `install(ehvi_gradient=True)`."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle import gp_oracle as O

import bogp
from bogp import _lib, optim, pareto
from support import ehvi_grad_ref as R
from support.ehvi_grad_engine import EhviGradOracleEngine
from support.ehvi_ref64 import ehvi as ehvi_ref

REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
BOX = (-2.0, 2.0)


def _state(m, d, kernel, noisy=True, N=30, seed=0):
    """An m-target oracle state at fixed hyper-parameters (fixed constant trend, as several targets require) and the cells of a
    small front of its observations."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(*BOX, size=(N, d))
    Y = np.sin(X @ rng.normal(size=(d, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    if noisy:
        st = O.make_state(np.r_[np.full(d, 0.6 / d), 0.9], X, Y, kernel, O.MODE_NOISE_ESTIM, 0.0, beta=0.0)
    else:  # (short length scales keep the noiseless R well conditioned)
        st = O.make_state(np.full(d, 200.0 / d), X, Y, kernel, O.MODE_NOISELESS, 0.0, beta=0.0)
    ref = Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
    lo, hi = pareto.hypercell_bounds(Y[: (8 if m < 5 else 4)], ref)
    return st, X, Y, lo, hi, rng


@pytest.mark.parametrize("d", [2, 6])
@pytest.mark.parametrize("kernel", [O.KERNEL_SE, O.KERNEL_MATERN52])
@pytest.mark.parametrize("m", [2, 3, 5])
def test_restatement_against_central_differences(m, kernel, d):
    """Tolerance (ledger T15): the difference quotient's own error, estimated per case as max |FD(h) - FD(h / 2)| with h = 1e-5 of
    the box width, times 10 -- both sides relative to max |grad EHVI| of the case.  Measured: the restatement sits at 1.0 .. 1.4
    times that estimate (1e-10 .. 2e-7 relative), i.e. at the O(h^2) truncation error of FD(h) itself."""
    st, X, Y, lo, hi, rng = _state(m, d, kernel, seed=100 * m + 10 * kernel + d)
    h = 1e-5 * (BOX[1] - BOX[0])

    def value(z):
        mu, mse = O.predict(st, z[None, :])
        return ehvi_ref(mu, mse, lo, hi)[0]

    def fd(x, step):
        return np.array([(value(x + step * e) - value(x - step * e)) / (2 * step) for e in np.eye(d)])

    err = own = scale = 0.0
    n = 0
    while n < 4:
        x = rng.uniform(BOX[0] + 0.1, BOX[1] - 0.1, size=d)  # away from the training set (a continuous draw)
        v, g = R.ehvi_grad(st, x, lo, hi)
        if not v > 1e-8:  # (targets of O(1): below this the 2^m expansion of the value restatement has lost its digits to
            continue      #  cancellation, and its difference quotient says nothing)
        n += 1
        np.testing.assert_allclose(v, value(x), rtol=1e-9, atol=0)  # (product form against the 2^m expansion)
        a, b = fd(x, h), fd(x, h / 2)
        err, own, scale = max(err, np.abs(g - a).max()), max(own, np.abs(a - b).max()), max(scale, np.abs(g).max())
    print("m=%d kernel=%d d=%d: |grad - FD| / max|grad| = %.3g, FD's own error estimate %.3g" % (m, kernel, d, err / scale, own / scale))
    assert err / scale <= 10.0 * own / scale


def test_clamp_at_a_training_point_of_a_noiseless_model():
    st, X, Y, lo, hi, _ = _state(2, 2, O.KERNEL_MATERN52, noisy=False, seed=5)
    mu, mse, dmu, dmse = R.moments(st, X[3])
    assert np.all(mse <= 1e-9)  # the clamp of analytic.py:233 is active for every target
    v, g, g_mu, g_sd = R.ehvi_grad(st, X[3], lo, hi, parts=True)
    assert np.all(g_sd == 0.0) and np.all(np.isfinite(g)) and np.array_equal(g, g_mu)
    # next to it the sd path is alive again
    _, _, _, g_sd2 = R.ehvi_grad(st, X[3] + 0.05, lo, hi, parts=True)
    assert np.abs(g_sd2).max() > 0


# ----------------------------------------------------------------------------------------------------------------------
# EHVI(input_gradient=True) on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
def _gp(d=2, m=2, N=30, seed=9):
    rng = np.random.default_rng(seed)
    X = rng.uniform(*BOX, size=(N, d))
    Y = np.sin(X @ rng.normal(size=(d, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(d, beta=0.0), corr="matern", thetaL=[1e-3] * d, thetaU=[1e2] * d, nugget=1e-6)
    model._engine = EhviGradOracleEngine()
    model.set_state(np.r_[np.full(d, 0.6 / d), 0.9], X, Y)
    ref = Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
    return model, Y, ref


def _box(d=2, seed=None):
    return optim.Box([BOX] * d, random_seed=seed)


def test_return_shapes_and_values():
    model, Y, ref = _gp()
    crit = bogp.EHVI(model=model, ref_point=ref, Y=Y, input_gradient=True)
    plain = bogp.EHVI(model=model, ref_point=ref, Y=Y)
    assert crit.input_gradient and not plain.input_gradient
    X = np.random.default_rng(0).uniform(*BOX, size=(5, 2))
    v1, g1 = crit(X[:1], return_dx=True)
    assert v1.shape == (1,) and g1.shape == (1, 2)  # the single-objective criteria's one-row shapes
    v5, g5 = crit(X, return_dx=True)
    assert v5.shape == (5, 1) and g5.shape == (5, 2)  # ... and their M-row shapes
    assert v5[0, 0] == v1[0] and np.array_equal(g5[0], g1[0])
    eng = model.engine
    eng.calls.clear()
    vals = crit(X)  # at most 64 rows: the same call
    assert vals.shape == (5,) and eng.calls == [("point_eval_ehvi", 5)]
    ref_vals = plain(X)  # (the sweep path: the 2^m expansion instead of the product -- T12's absolute term covers its cancellation)
    np.testing.assert_allclose(vals, ref_vals, rtol=1e-10, atol=1e-12 * np.abs(ref_vals).max())
    eng.calls.clear()
    big = np.random.default_rng(1).uniform(*BOX, size=(65, 2))
    assert crit(big).shape == (65,) and eng.calls[0][0] == "sweep_ehvi"
    vr, gr = R.ehvi_grad(eng.st, X[0], crit.cell_lower_bounds, crit.cell_upper_bounds)
    assert v1[0] == vr and np.array_equal(g1[0], gr)


@pytest.mark.parametrize("optimizer", ["BFGS", "sweep-BFGS", "sweep-device-BFGS"])
def test_polish_optimisers_reach_at_least_the_sweep_winner(optimizer):
    """The hybrids polish the sweep's own top rows (same candidates under the same seed), so their result is >= the sweep's winner
    by construction.  "BFGS" (10 restarts of L-BFGS-B from uniform starts) is compared with the best of as many uniform rows."""
    model, Y, ref = _gp()
    crit = bogp.EHVI(model=model, ref_point=ref, Y=Y, input_gradient=True)
    eng = model.engine
    sweep_of = {"BFGS": "sweep", "sweep-BFGS": "sweep", "sweep-device-BFGS": "sweep-device"}[optimizer]
    budget = 10 if optimizer == "BFGS" else 200
    np.random.seed(4)
    xs, fs = optim.argmax_restart(crit, _box(seed=7), eval_budget=budget, optimizer=sweep_of)
    eng.calls.clear()
    np.random.seed(4)
    xp, fp = optim.argmax_restart(crit, _box(seed=7), eval_budget=200, n_restart=10, optimizer=optimizer)
    print("%s: sweep winner %.6g, result %.6g" % (optimizer, fs, fp))
    assert fp >= fs
    assert all(BOX[0] <= v <= BOX[1] for v in xp) and len(xp) == 2
    np.testing.assert_allclose(fp, crit(np.array([xp]))[0], rtol=1e-12)
    if optimizer != "BFGS":
        assert eng.calls[0] == ("sweep_ehvi", 200, 10)  # ehvi.sweep(k), then the polish (sequential fall-back: no polish_ehvi here)
    assert any(c == ("point_eval_ehvi", 1) for c in eng.calls)


def test_polish_topk_dispatches_to_the_engine_polish():
    model, Y, ref = _gp()
    crit = bogp.EHVI(model=model, ref_point=ref, Y=Y, input_gradient=True)
    seen = {}

    def polish_ehvi(starts, lo, hi, lower, upper, max_evals=50):
        seen.update(starts=np.array(starts), lo=np.array(lo), hi=np.array(hi), lower=lower, upper=upper, max_evals=max_evals)
        return np.array(starts) + 0.0, np.arange(len(starts), dtype=float), np.ones(len(starts), dtype=np.int32)

    model.engine.polish_ehvi = polish_ehvi
    starts = np.array([[0.1, 0.2], [0.3, 0.4], [9.0, 9.0]])
    xs, fs = optim.polish_topk(crit, starts, np.array([BOX, BOX]), max_iter=17)
    assert np.array_equal(xs, starts) and fs.tolist() == [0.0, 1.0, 2.0]
    assert seen["max_evals"] == 17 and seen["lo"].tolist() == [-2.0, -2.0] and seen["hi"].tolist() == [2.0, 2.0]
    assert seen["lower"] is crit.cell_lower_bounds and seen["upper"] is crit.cell_upper_bounds


def test_default_criterion_still_refuses_and_forest_is_refused(monkeypatch):
    model, Y, ref = _gp()
    plain = bogp.EHVI(model=model, ref_point=ref, Y=Y)
    with pytest.raises(NotImplementedError, match="no input gradient"):
        plain(np.zeros((1, 2)), return_dx=True)
    for name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="input gradient"):
            optim.argmax_restart(plain, _box(), eval_budget=10, optimizer=name)
    monkeypatch.setattr(bogp.acquisition._forest, "is_forest_model", lambda mdl: True)
    with pytest.raises(NotImplementedError, match="input gradient"):
        bogp.EHVI(model=model, ref_point=ref, Y=Y, input_gradient=True)


def test_refusals_by_name(monkeypatch):
    model, Y, ref = _gp()
    crit = bogp.EHVI(model=model, ref_point=ref, Y=Y, input_gradient=True)
    masks, values = np.array([False, True, False]), [0.5]

    @functools.wraps(functools.partial(crit))
    def fixed(X):  # the shape of the reference's partial_argument wrapper (utils.py:184-213): `masks` / `values` in its closure
        full = np.empty((1, len(masks)))
        full[:, ~masks], full[:, masks] = X, values
        return crit(full)

    fixed.__wrapped__ = functools.partial(crit)
    assert optim.unwrap_criterion(fixed)[0] is crit and optim.unwrap_criterion(fixed)[1] is not None
    for name in ("sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="fixed variables"):
            optim.argmax_restart(fixed, _box(), eval_budget=20, optimizer=name)
        with pytest.raises(NotImplementedError, match="unconstrained"):
            optim.argmax_restart(crit, _box(), g=lambda x: -1.0, eval_budget=20, optimizer=name)
        lifted = functools.partial(lambda x, **kw: 0.0, acquisition_func=functools.partial(crit), bounds=np.array([BOX, BOX]), pca=object())
        with pytest.raises(NotImplementedError, match="lift"):
            optim.argmax_restart(lifted, _box(), eval_budget=20, optimizer=name)
    monkeypatch.setattr(EhviGradOracleEngine, "comm_world", 2, raising=False)
    monkeypatch.setattr(EhviGradOracleEngine, "comm_rank", 0, raising=False)
    with pytest.raises(NotImplementedError, match="one rank"):
        optim.argmax_restart(crit, _box(), eval_budget=20, optimizer="sweep-BFGS")


# ----------------------------------------------------------------------------------------------------------------------
# the reference's MOBO under install(ehvi_gradient=True)
# ----------------------------------------------------------------------------------------------------------------------
has_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")


def _mobo(bayes_optim, optimizer):
    from bayes_optim import MOBO
    from bayes_optim.search_space import RealSpace

    np.random.seed(3)
    space = RealSpace([0, 10], var_name="a", precision=2) + RealSpace([0, 10], var_name="b", precision=2) + RealSpace([0, 10], var_name="c", precision=2)
    fs = (lambda x: x[0] ** 2 + x[1] + x[2] ** 2, lambda x: x[0] + x[1] ** 2 + x[2] ** 2)
    model = bayes_optim.GaussianProcess(theta0=np.full(3, 0.5), thetaL=np.full(3, 1e-3), thetaU=np.full(3, 1e2), nugget=1e-6,
                                        noise_estim=False, likelihood="concentrated")  # fmt: skip
    opt = MOBO(search_space=space, obj_fun=fs, model=model, max_FEs=100, DoE_size=6, eval_type="list", n_job=1, verbose=False,
               minimize=True, acquisition_optimization={"optimizer": optimizer, "max_FEs": 200, "n_restart": 4})  # fmt: skip
    return opt, fs, model


@has_ref
@pytest.mark.timeout(900)
def test_mobo_under_install_with_the_gradient_switch(monkeypatch):
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim

    monkeypatch.setattr(_lib, "Engine", EhviGradOracleEngine)
    undo = bogp.install(bayes_optim, ehvi_gradient=True)
    try:
        opt, fs, model = _mobo(bayes_optim, "sweep-BFGS")
        assert type(model).__module__.startswith("bogp")
        X = opt.ask()  # the design of experiments
        opt.tell(X, [tuple(f(x) for f in fs) for x in X])
        for _ in range(3):
            eng = model.engine
            eng.calls.clear()
            X = opt.ask(1)
            eng = model.engine
            sweeps = [c for c in eng.calls if c[0] == "sweep_ehvi"]
            assert sweeps == [("sweep_ehvi", 200, 4)] and ("point_eval_ehvi", 1) in eng.calls
            assert len(X) == 1 and all(0.0 <= v <= 10.0 for v in X[0])
            opt.tell(X, [tuple(f(x) for f in fs) for x in X])
        w = bayes_optim.mobo.MOBO._create_acquisition(opt)
        crit = optim.unwrap_criterion(w)[0]
        assert isinstance(crit, bogp.EHVI) and crit.input_gradient
        # "BFGS": return_dx bound as BO._create_acquisition binds it, so the wrapper hands the reference's loop (value, gradient)
        opt._optimizer = "BFGS"
        wb = bayes_optim.mobo.MOBO._create_acquisition(opt)
        out = wb(np.array([1.0, 2.0, 3.0]))
        assert isinstance(out, tuple) and len(out) == 2 and np.asarray(out[1]).size == 3
    finally:
        undo()
    assert bayes_optim.mobo.MOBO._create_acquisition.__module__.startswith("bayes_optim")  # uninstall() restored

    # plain install(): the same configuration behaves as before -- MOBO keeps the reference's EHVI, which "sweep-BFGS" cannot serve
    undo = bogp.install(bayes_optim)
    try:
        opt, fs, model = _mobo(bayes_optim, "sweep-BFGS")
        X = opt.ask()
        opt.tell(X, [tuple(f(x) for f in fs) for x in X])
        assert optim.unwrap_criterion(bayes_optim.mobo.MOBO._create_acquisition(opt))[0] is None
        with pytest.raises(TypeError, match="needs one of this package's criteria"):
            opt.ask(1)
    finally:
        undo()
