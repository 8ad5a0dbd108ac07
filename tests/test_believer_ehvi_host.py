"""Kriging-believer batches under EHVI, the parts that need no GPU: the library's grid decomposition (`bogp_ehvi_grid_cells`,
host code of libbogp) against `pareto.hypercell_bounds` bit for bit; the dense restatement (tests/support/believer_ehvi_ref.py)
against a dense refit per target and against the reference's rebuilt models of golden G44; the routing and the refusals of
`optim.ehvi_believer_batch` and of `install(batch_strategy="believer")` for the reference's MOBO on the oracle-backed stand-in."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import gp_oracle as O

import bogp
from bogp import _lib, optim, pareto
from support.believer_ehvi_engine import BelieverEhviOracleEngine
from support.believer_ehvi_ref import BelieverEhviRef

REF = os.environ.get("BOGP_REFERENCE", "/root/reference")


# ----------------------------------------------------------------------------------------------------------------------
# bogp_ehvi_grid_cells
# ----------------------------------------------------------------------------------------------------------------------
def _same_cells(Y, r):
    m = len(r)
    lo, hi = _lib.grid_cells(Y, r)
    plo, phi = pareto.hypercell_bounds(np.asarray(Y, float).reshape(-1, m), r)
    assert lo.shape == plo.shape == hi.shape == phi.shape and lo.shape[1] == m
    assert np.array_equal(lo, plo) and np.array_equal(hi, phi)
    return len(lo)


@pytest.mark.parametrize("m", [2, 3, 4])
def test_grid_cells_equal_the_python_decomposition(m):
    """Random rows rounded to one decimal (coordinates shared between front points, dominated rows, rows at or below the reference
    point), duplicates of front rows, a single row, no row at all: both arrays of `pareto.hypercell_bounds`, `np.array_equal`."""
    rng = np.random.default_rng(m)
    r = np.full(m, -0.5)
    counts = []
    for n in (0, 1, 2, 7, 16, 30):
        for trial in range(4):
            Y = np.round(rng.normal(size=(n, m)), 1)
            if n > 2:
                Y[2] = Y[0]  # a duplicate
                Y[1, 0] = r[0]  # exactly at the reference point in one objective
                Y[n - 1] = r - 0.25  # below it in every one
            counts.append(_same_cells(Y, r))
    assert max(counts) > (4 if m == 2 else 20) and min(counts) == 1
    assert _same_cells(np.empty((0, m)), r) == 1  # an empty front: one cell [ref, +inf)
    lo, hi = _lib.grid_cells(np.empty((0, m)), r)
    assert np.array_equal(lo, r[None, :]) and np.all(np.isinf(hi))
    assert _same_cells(np.tile(r - 1.0, (3, 1)), r) == 1  # no row above the reference point
    # a continuous front: every coordinate distinct, (P + 1)^(m - 1) cells
    t = np.linspace(0.1, 0.9, 5)
    Y = np.column_stack([t] * (m - 1) + [1.0 - t])
    assert _same_cells(Y, np.zeros(m)) == 6 ** (m - 1)


def test_grid_cells_count_limits_and_refusals():
    lib = _lib.load()
    dp = C.POINTER(C.c_double)

    def raw(m, Y, r, lower=None, upper=None, cap=0):
        Y = None if Y is None else np.ascontiguousarray(Y, dtype=float)
        r = np.ascontiguousarray(r, dtype=float)
        return lib.bogp_ehvi_grid_cells(m, 0 if Y is None else len(Y), _lib._ptr(Y), r.ctypes.data_as(dp), _lib._ptr(lower), _lib._ptr(upper), cap)

    t = np.linspace(0.1, 0.9, 5)
    Y = np.column_stack([t, t, 1.0 - t])
    assert raw(3, Y, np.zeros(3)) == 36  # count only: no arrays, the capacity is not looked at
    lo, hi = np.full((36, 3), -7.0), np.full((36, 3), -7.0)
    assert raw(3, Y, np.zeros(3), lo, hi, 35) == _lib.ERR_INVALID  # the capacity is too small ...
    assert np.all(lo == -7.0) and np.all(hi == -7.0)  # ... and nothing was written
    assert raw(3, Y, np.zeros(3), lo, hi, 36) == 36 and np.array_equal(lo, pareto.hypercell_bounds(Y, np.zeros(3))[0])
    assert raw(3, Y, np.zeros(3), lo, None, 36) == _lib.ERR_INVALID  # one array without the other
    assert raw(3, None, np.zeros(3)) == 1  # n = 0
    assert raw(1, Y[:, :1], np.zeros(1)) == _lib.ERR_INVALID and raw(9, np.ones((2, 9)), np.zeros(9)) == _lib.ERR_INVALID
    bad = Y.copy()
    bad[3, 1] = np.nan
    assert raw(3, bad, np.zeros(3)) == _lib.ERR_INVALID
    bad[3, 1] = np.inf
    assert raw(3, bad, np.zeros(3)) == _lib.ERR_INVALID
    assert raw(3, Y, np.array([0.0, -np.inf, 0.0])) == _lib.ERR_INVALID
    # a front whose grid passes BOGP_MAX_EHVI_CELLS: 41 mutually non-dominated points in four objectives, 42^3 = 74 088 cells;
    # 40 of them give 41^3 = 68 921, 39 give 64 000 -- the first count the library serves
    t = np.arange(1, 42, dtype=float)
    big = np.column_stack([t, t, t, 42 - t])
    assert raw(4, big, np.zeros(4)) == _lib.ERR_INVALID and raw(4, big[:40], np.zeros(4)) == _lib.ERR_INVALID
    assert raw(4, big[:39], np.zeros(4)) == 64000 <= _lib.MAX_EHVI_CELLS
    with pytest.raises(ValueError, match="more than 65536"):
        _lib.grid_cells(big, np.zeros(4))
    with pytest.raises(ValueError):
        pareto.hypercell_bounds(big, np.zeros(4))
    # many objectives and many points: the count is formed in 64 bits and checked factor by factor
    t = np.arange(1, 3001, dtype=float)
    assert raw(8, np.column_stack([t] * 7 + [3001 - t]), np.zeros(8)) == _lib.ERR_INVALID


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _problem(seed, m=3, N=30, d=3, M=200):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, size=(N, d))
    Y = np.sin(X @ rng.normal(size=(d, m))) * (1.0 + np.arange(m)) + 0.1 * rng.normal(size=(N, m))
    return X, Y, rng.uniform(-2.2, 2.2, size=(M, d)), rng.uniform(-2, 2, size=(3, d))


def _ref_of(st):
    state = dict(C=st.C, gamma=st.gamma, beta=float(st.beta[0, 0]), sigma2=st.sigma2)
    return BelieverEhviRef(st.X, st.theta, st.kernel, state)


def test_per_target_mse_equals_a_dense_refit():
    """Matern-3/2, noiseless, three targets: after each of four believed points (two pending rows off the candidates, then two
    winners) the restatement's MSE_k / sigma2_k and means are the bracket and the means of the model REBUILT on X + {p_1..p_B} with
    y = mu(p) at the same theta, to 1e-10 per target (the rebuilt sigma2 is concentrated, so the brackets are compared); the front
    the steps saw is the front of `front` and the believed means."""
    X, Y, Xs, pend = _problem(7)
    theta = np.array([0.8, 0.5, 1.1])
    st = O.make_state(theta, X, Y, O.KERNEL_MATERN32, O.MODE_NOISELESS, 0.0, estimate_trend=False, beta=0.2)
    ref = _ref_of(st)
    rp = Y.min(axis=0) - 0.2
    out = ref.run(Xs, Y[:8], rp, 3, pending=pend[:2])
    pts = np.vstack([pend[:2], out["best_x"]])
    mu0 = O.predict(st, Xs)[0]
    np.testing.assert_allclose(out["mu"], mu0, rtol=0, atol=1e-12)
    for B in range(1, 5):
        Xb = np.vstack([X, pts[:B]])
        Yb = np.vstack([Y, O.predict(st, pts[:B], eval_MSE=False)])
        st_b = O.make_state(theta, Xb, Yb, O.KERNEL_MATERN32, O.MODE_NOISELESS, 0.0, estimate_trend=False, beta=0.2)
        mu_b, mse_b = O.predict(st_b, Xs)
        for t in range(3):
            np.testing.assert_allclose(np.maximum(0.0, out["s"][B]), mse_b[:, t] / st_b.sigma2[t], rtol=0, atol=1e-10)
            if 2 <= B <= 4:  # what step B - 2 saw
                np.testing.assert_allclose(out["mse"][B - 2][:, t] / st.sigma2[t], mse_b[:, t] / st_b.sigma2[t], rtol=0, atol=1e-10)
        np.testing.assert_allclose(mu_b, mu0, rtol=0, atol=1e-10)
        np.testing.assert_allclose(st_b.sigma2, st.sigma2 * len(X) / (len(X) + B), rtol=1e-8)  # a believed mean adds no residual
    assert np.all(out["pivots"] > 1e-3) and len(set(out["best_idx"].tolist())) == 3
    assert np.all(out["mse"][2][out["best_idx"][:2]] == 0.0)  # a believed candidate row is determined
    F = np.vstack([Y[:8], ref.mean(pend[:2])])
    for j in range(3):
        lo, hi = pareto.hypercell_bounds(F, rp)
        assert np.array_equal(out["cells"][j][0], lo) and np.array_equal(out["cells"][j][1], hi) and out["n_cells"][j] == len(lo)
        F = np.vstack([F, out["best_mu"][j]])
    fixed = ref.run(Xs, Y[:8], rp, 3, pending=pend[:2], believe_front=False)
    assert len(set(fixed["n_cells"].tolist())) == 1 and np.array_equal(fixed["cells"][2][0], pareto.hypercell_bounds(Y[:8], rp)[0])
    np.testing.assert_array_equal(fixed["mse"][0], out["mse"][0])  # the variance is conditioned either way


@pytest.mark.parametrize("state", ["m2", "m3"])
def test_restatement_against_the_references_rebuilt_models(state):
    """G44: the restatement's MSE_j / sigma2 per target against the reference's own predict of the models rebuilt on X + the believed
    points (T2: rtol 1e-6, atol 1e-12), and the mean, which must not move (T1); the grid cells of y u mu(p_1 .. p_j) give the EHVI of
    the reference's own cells (T12)."""
    from support.ehvi_ref64 import ehvi as ehvi_ref

    g = {k[len(state) + 1 :]: v for k, v in load_golden("G44_believer_ehvi").items() if k.startswith(state + "_")}
    m = g["y"].shape[1]
    st = O.make_state(g["par"], g["X"], g["y"], int(g["kernel"]), int(g["mode"]), 0.0, estimate_trend=False, beta=float(g["beta"]))
    np.testing.assert_allclose(st.sigma2, g["sigma2"], rtol=1e-9)
    ref = _ref_of(st)
    for j in range(1, 5):
        out = ref.run(g["Xs"], g["y"], g["ref_point"], 1, pending=g["believed"][:j])
        for t in range(m):
            np.testing.assert_allclose(out["mse"][0][:, t] / st.sigma2[t], g["mse_j"][j - 1][:, t] / g["sigma2_j"][j - 1][t], rtol=1e-6, atol=1e-12)
            np.testing.assert_allclose(out["mu"][:, t], g["mu_j"][j - 1][:, t], rtol=1e-6, atol=1e-9)
        mine = ehvi_ref(g["mu_j"][j - 1], g["mse_j"][j - 1], *out["cells"][0])
        theirs = ehvi_ref(g["mu_j"][j - 1], g["mse_j"][j - 1], g["lower_%d" % j], g["upper_%d" % j])
        assert np.all(np.abs(mine - theirs) <= 1e-6 * np.abs(theirs) + 1e-12 * np.abs(theirs).max())
        assert np.abs(mine - g["ehvi32_j"][j - 1]).max() <= 1e-5 * np.abs(g["ehvi32_j"][j - 1]).max()
    assert np.all(out["mse"][0][g["believed_rows"]] <= 1e-12 * st.sigma2)


# ----------------------------------------------------------------------------------------------------------------------
# the Python routing on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def gp():
    X, Y, _, _ = _problem(9, m=2, N=40)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=1e-6)
    model._engine = BelieverEhviOracleEngine()
    model.set_state(np.r_[0.6, 0.6, 0.6, 0.9], X, Y)
    return model, Y


def _box(seed=3):
    return optim.Box([(-2.2, 2.2)] * 3, random_seed=seed)


def test_ehvi_believer_batch_routes(gp):
    model, Y = gp
    eng = model.engine
    Xs = _problem(9, m=2, N=40, M=300)[2]
    rp = Y.min(axis=0) - 0.1
    crit = bogp.EHVI(model=model, ref_point=rp, Y=Y)
    eng.calls.clear()
    xs, fs = bogp.ehvi_believer_batch(crit, _box(), 300, 3, Xs=Xs)
    assert eng.calls == [("upload", 300), ("sweep_believer_ehvi", 3, 0, True)]
    assert len(xs) == len(fs) == 3 and all(isinstance(x, list) and len(x) == 3 for x in xs) and all(isinstance(f, float) for f in fs)
    assert len({tuple(x) for x in xs}) == 3
    vals = crit(Xs)
    assert fs[0] == float(np.max(vals)) and xs[0] == Xs[int(np.argmax(vals))].tolist()  # step 0 is the plain EHVI sweep
    # pending rows and the front switch reach the engine; the front that travels is the criterion's
    eng.calls.clear()
    xs2, fs2 = bogp.ehvi_believer_batch(crit, _box(), 300, 2, Xs=Xs, pending=Xs[:2] + 0.01, believe_front=False)
    assert eng.calls[-1] == ("sweep_believer_ehvi", 2, 2, False)
    want = BelieverEhviOracleEngine.sweep_believer_ehvi(eng, crit.pareto_Y, rp, 2, pending=Xs[:2] + 0.01, believe_front=False)
    assert [list(x) for x in want["best_x"]] == list(xs2) and tuple(want["best_val"]) == fs2

    class Part:  # a partitioning object carries its front as well
        pareto_Y, num_outcomes = pareto.pareto_front(Y, rp), 2

        def get_hypercell_bounds(self):
            return pareto.hypercell_bounds(Y, rp)

    xs3, fs3 = bogp.ehvi_believer_batch(bogp.EHVI(model=model, ref_point=rp, partitioning=Part()), _box(), 300, 3, Xs=Xs)
    assert xs3 == xs and fs3 == fs
    # host-sampled and device-drawn candidates
    eng.calls.clear()
    bogp.ehvi_believer_batch(crit, _box(5), 250, 2)
    assert eng.calls[0] == ("upload", 250)
    eng.calls.clear()
    bogp.ehvi_believer_batch(crit, _box(5), 250, 2, design="LHS", seed=4)
    assert eng.calls[0] == ("generate", 250, "LHS") and eng.calls[1][0] == "sweep_believer_ehvi"


def test_what_the_ehvi_believer_refuses(gp, monkeypatch):
    model, Y = gp
    Xs = _problem(9, m=2, N=40, M=100)[2]
    rp = Y.min(axis=0) - 0.1
    crit = bogp.EHVI(model=model, ref_point=rp, Y=Y)
    with pytest.raises(ValueError, match="no front to extend"):
        bogp.ehvi_believer_batch(bogp.EHVI(model=model, ref_point=rp, cells=pareto.hypercell_bounds(Y, rp)), _box(), 100, 2, Xs=Xs)
    with pytest.raises(TypeError, match="believer_batch"):
        bogp.ehvi_believer_batch(bogp.EI(model=model), _box(), 100, 2, Xs=Xs)
    with pytest.raises(ValueError, match="at most 32"):
        bogp.ehvi_believer_batch(crit, _box(), 100, 33, Xs=Xs)
    with pytest.raises(ValueError, match="at least one"):
        bogp.ehvi_believer_batch(crit, _box(), 100, 0, Xs=Xs)
    with pytest.raises(NotImplementedError, match="lift"):
        bogp.ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, lift=object())
    with pytest.raises(NotImplementedError, match="fixed variables"):
        bogp.ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, masks=np.array([True, False, False]), values=[0.0])
    with pytest.raises(NotImplementedError, match="constraints"):
        bogp.ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, h=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="constraints"):
        bogp.ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, g=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, rank=0, world=2)
    monkeypatch.setattr(optim._forest, "is_forest_model", lambda m: True)
    with pytest.raises(NotImplementedError, match="forest"):
        bogp.ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs)
    monkeypatch.undo()
    # believer_batch keeps refusing EHVI, and says where it went
    with pytest.raises(NotImplementedError, match="ehvi_believer_batch"):
        bogp.believer_batch(crit, _box(), 100, q=2, Xs=Xs)


# ----------------------------------------------------------------------------------------------------------------------
# the reference's MOBO under install(batch_strategy="believer")
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
def test_mobo_proposes_q_points_under_the_believer_strategy(monkeypatch):
    """`MOBO(n_point=3).ask()` after a first `tell()`: three distinct points from ONE `sweep_believer_ehvi` call under
    install(batch_strategy="believer"); NotImplementedError (the inherited BaseBO method, base.py:496-497) under the default
    install(), and the method is gone from the class again after uninstall()."""
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim
    from bayes_optim import MOBO
    from bayes_optim.search_space import RealSpace

    created = []

    def engine(device=0):
        created.append(BelieverEhviOracleEngine(device))
        return created[-1]

    monkeypatch.setattr(_lib, "Engine", engine)
    fs = (lambda x: x[0] ** 2 + x[1] + x[2] ** 2, lambda x: x[0] + x[1] ** 2 + x[2] ** 2)

    def driver(optimizer="sweep"):
        np.random.seed(3)
        space = RealSpace([0, 10], var_name="a", precision=2) + RealSpace([0, 10], var_name="b", precision=2) + RealSpace([0, 10], var_name="c", precision=2)
        model = bayes_optim.GaussianProcess(theta0=np.full(3, 0.5), thetaL=np.full(3, 1e-3), thetaU=np.full(3, 1e2), nugget=1e-6,
                                            noise_estim=False, likelihood="concentrated")  # fmt: skip
        opt = MOBO(search_space=space, obj_fun=fs, model=model, max_FEs=100, DoE_size=6, n_point=3, eval_type="list", n_job=1,
                   verbose=False, minimize=True, acquisition_optimization={"optimizer": optimizer, "max_FEs": 300})  # fmt: skip
        X = opt.ask()  # the design of experiments
        opt.tell(X, [tuple(f(x) for f in fs) for x in X])
        return opt, model

    assert "_batch_arg_max_acquisition" not in MOBO.__dict__
    undo = bogp.install(bayes_optim, batch_strategy="believer")
    try:
        opt, model = driver()
        assert type(model).__module__.startswith("bogp")
        model.engine.calls.clear()
        X = opt.ask()
        assert len(X) == 3 and len({tuple(np.round(x, 12)) for x in X}) == 3
        calls = [c for c in model.engine.calls if c[0].startswith("sweep")]
        assert calls == [("sweep_believer_ehvi", 3, 0, True)], calls
        assert ("upload", 300) in model.engine.calls
        opt.tell(X, [tuple(f(x) for f in fs) for x in X])
        assert len(opt.ask(2)) == 2 and model.engine.calls[-1] == ("sweep_believer_ehvi", 2, 0, True)
        with pytest.raises(NotImplementedError):  # a fixed variable: the inherited method
            opt.ask(3, fixed={"a": 1.0})
        opt_cma, _ = driver("OnePlusOne_Cholesky_CMA")  # not an optimiser of the sweep family: the inherited method
        with pytest.raises(NotImplementedError):
            opt_cma.ask(3)
    finally:
        undo()
    assert "_batch_arg_max_acquisition" not in MOBO.__dict__  # inherited again
    undo = bogp.install(bayes_optim)
    try:
        opt, model = driver()
        with pytest.raises(NotImplementedError):
            opt.ask(3)
        assert len(opt.ask(1)) == 1
    finally:
        undo()
