"""Modelled constraints of a multi-objective run on the host side (no GPU): exact cases of the NumPy restatement
(tests/support/constrained_ehvi_ref.py), `bogp.ConstrainedEHVI` and the sweep routing on the oracle-backed stand-in engine
(tests/support/constrained_ehvi_engine.py), a toy problem on which the feasibility weight changes the winner, and the reference's
unmodified `MOBO` under `install(expensive_constraints=True, constrained_mobo=True)`."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle import gp_oracle as O
from support import constrained_ehvi_ref as R
from support.constrained_ehvi_engine import ConstrainedEhviOracleEngine
from support.ehvi_ref64 import ehvi as ehvi_ref

import bogp
from bogp import optim, pareto

REF = "/root/reference"
INF = float("inf")


# ----------------------------------------------------------------------------------------------------------------------
# 1. exact cases of the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _moments(M=200, mt=4, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(M, mt)), rng.uniform(1e-3, 2.0, size=(M, mt)), rng.uniform(0.5, 2.0, size=mt)


def _cells(m, seed=1):
    Y = np.random.default_rng(seed).normal(size=(12, m))
    return pareto.hypercell_bounds(Y, np.full(m, -2.5))


def test_every_constraint_bound_infinite_is_exactly_ehvi():
    mu, mse, s2 = _moments()
    for m in (2, 3):
        lower, upper = _cells(m)
        v, P = R.values(mu, mse, s2, m, lower, upper, np.full(4 - m, -INF), np.full(4 - m, INF))
        assert np.all(P == 1.0)
        assert np.array_equal(v, ehvi_ref(mu[:, :m], mse[:, :m], lower, upper)) and np.all(v > 0)


def test_lo_equal_hi_is_plus_zero_everywhere_and_the_winner_is_row_zero():
    mu, mse, s2 = _moments()
    lower, upper = _cells(2)
    v, P = R.values(mu, mse, s2, 2, lower, upper, [0.25, -INF], [0.25, INF])
    assert np.all(P == 0.0) and np.all(v == 0.0) and not np.any(np.signbit(v))
    best, idx = R.topk(v, 3)
    assert list(idx) == [0, 1, 2] and np.all(best == 0.0)
    # the rule is part of the definition: an infinite E (or a NaN one) does not reach a row whose P is 0
    mu2 = mu.copy()
    mu2[:5, 0] = INF
    v2, _ = R.values(mu2, mse, s2, 2, lower, upper, [0.25, -INF], [0.25, INF])
    assert np.all(v2 == 0.0)


def test_no_cells_is_the_probability_of_feasibility_and_nan_propagates():
    mu, mse, s2 = _moments()
    v, P = R.values(mu, mse, s2, 2, np.zeros((0, 2)), np.zeros((0, 2)), [-INF, -0.5], [0.0, 0.5])
    assert np.array_equal(v, P) and 0 < P.min() and P.max() < 1
    mu2 = mu.copy()
    mu2[7, 2] = np.nan
    lower, upper = _cells(2)
    v2, P2 = R.values(mu2, mse, s2, 2, lower, upper, [-INF, -0.5], [0.0, 0.5])
    assert np.isnan(P2[7]) and np.isnan(v2[7]) and R.topk(v2, 1)[1][0] == 7  # a NaN P is not == 0; NaN is maximal
    with pytest.raises(ValueError, match="hi >= lo"):
        R.values(mu, mse, s2, 2, lower, upper, [0.5, -INF], [0.0, 0.0])


# ----------------------------------------------------------------------------------------------------------------------
# 2. bogp.ConstrainedEHVI on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
def _g_true(X):
    return 0.8 - X[:, 0] - X[:, 1] + 0.3 * np.sin(6 * X[:, 0])


def _objectives(X):
    """two objectives, maximised as given: both pull towards small x0 + x1, where the constraint fails"""
    return np.c_[-(X[:, 0] ** 2) - 0.5 * X[:, 1], -(X[:, 1] ** 2) - 0.5 * X[:, 0]]


def _toy(seed, N=24, M=3000):
    """maximise both objectives on [0, 1]^2 subject to 0.8 - x0 - x1 + 0.3 sin(6 x0) <= 0; columns scaled as the drop-in scales them
    (objectives min-max scaled, the constraint divided by its standard deviation and never shifted)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, 2))
    F, g = _objectives(X), _g_true(X)
    Y = np.c_[(F - F.min(0)) / (F.max(0) - F.min(0)), g / g.std()]
    Xs = rng.uniform(0, 1, (M, 2))
    return X, Y, Xs


def _gp(X, Y):
    d = X.shape[1]
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(d, beta=0.0), corr="matern52", thetaL=[1e-3] * d, thetaU=[1e3] * d, nugget=0)
    model._engine = ConstrainedEhviOracleEngine()
    model.set_state(np.full(d, 60.0), X, Y)
    return model


def test_the_cells_come_from_the_feasible_front_only():
    X, Y, _ = _toy(0)
    model = _gp(X, Y)
    ref = Y[:, :2].min(0) - 0.1
    crit = bogp.ConstrainedEHVI(model=model, ref_point=ref)
    feas = Y[:, 2] <= 0
    assert 0 < feas.sum() < len(Y) and crit.n_feasible == feas.sum() and not crit.feasibility_only
    assert np.array_equal(crit.lo, [-INF]) and np.array_equal(crit.hi, [0.0]) and crit.n_obj == 2
    lower, upper = pareto.hypercell_bounds(Y[feas, :2], ref)
    assert np.array_equal(crit.cell_lower_bounds, lower) and np.array_equal(crit.cell_upper_bounds, upper)
    assert np.array_equal(crit.pareto_Y, pareto.pareto_front(Y[feas, :2], ref))
    # the front of ALL rows holds an infeasible row: the unconstrained cells differ
    all_lower, _ = pareto.hypercell_bounds(Y[:, :2], ref)
    front_all = pareto.pareto_front(Y[:, :2], ref)
    assert any(not np.any(np.all(crit.pareto_Y == p, axis=1)) for p in front_all)
    assert all_lower.shape != lower.shape or not np.array_equal(all_lower, lower)
    # moving one dominating feasible row into infeasibility changes the cells
    j = int(np.flatnonzero(feas)[np.argmax(Y[feas, 0])])  # on the feasible front: the best feasible row of objective 0
    Y2 = Y.copy()
    Y2[j, 2] = 1.0
    crit2 = bogp.ConstrainedEHVI(model=_gp(X, Y2), ref_point=ref)
    assert crit2.n_feasible == crit.n_feasible - 1
    assert not np.any(np.all(crit2.pareto_Y == Y[j, :2], axis=1)) and np.any(np.all(crit.pareto_Y == Y[j, :2], axis=1))
    assert crit2.cell_lower_bounds.shape != lower.shape or not np.array_equal(crit2.cell_lower_bounds, lower)
    # an explicit Y, explicit cells, explicit bounds
    c3 = bogp.ConstrainedEHVI(model=model, ref_point=ref, Y=Y[:, :2] * 1.0, lo=[-1.0], hi=[INF])
    assert c3.n_feasible == int((Y[:, 2] >= -1.0).sum())
    c4 = bogp.ConstrainedEHVI(model=model, ref_point=ref, cells=(np.zeros((1, 2)), np.full((1, 2), INF)))
    assert c4.cell_lower_bounds.shape == (1, 2) and c4.pareto_Y is None


def test_a_single_cell_and_no_feasible_row():
    X, Y, Xs = _toy(0)
    model = _gp(X, Y)
    eng = model.engine
    feas = Y[:, 2] <= 0
    high = Y[feas, :2].max(0) + 0.5  # no feasible row above this reference point: hypercell_bounds' own answer, the cell [ref, +inf)
    one = bogp.ConstrainedEHVI(model=model, ref_point=high)
    assert one.n_feasible == feas.sum() and not one.feasibility_only and len(one.pareto_Y) == 0
    assert np.array_equal(one.cell_lower_bounds, high[None, :]) and np.all(np.isinf(one.cell_upper_bounds))
    one(Xs[:40])
    assert eng.calls[-1] == ("sweep_ehvi_constrained", 2, 1, 1)
    none = bogp.ConstrainedEHVI(model=model, ref_point=Y[:, :2].min(0) - 0.1, lo=[-INF], hi=[Y[:, 2].min() - 1.0])
    assert none.n_feasible == 0 and none.feasibility_only and none.cell_lower_bounds.shape == (0, 2)
    v = none(Xs[:40])
    assert eng.calls[-1] == ("sweep_ehvi_constrained", 2, 0, 1) and np.all((v >= 0) & (v <= 1))
    mu, mse = O.predict_chunked(eng.st, Xs[:40], 1024)
    assert np.array_equal(v, R.values(mu, mse, eng.st.sigma2, 2, none.cell_lower_bounds, none.cell_upper_bounds, none.lo, none.hi)[1])
    assert not any(c[0] in ("sweep", "sweep_topk", "sweep_ehvi", "sweep_constrained") for c in eng.calls)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_feasibility_weight_moves_the_winner_into_the_feasible_region(seed):
    X, Y, Xs = _toy(seed)
    model = _gp(X, Y)
    eng = model.engine
    crit = bogp.ConstrainedEHVI(model=model, ref_point=Y[:, :2].min(0) - 0.1)
    assert crit.n_feasible > 0
    eng.upload_candidates(Xs)
    best, idx, vals, pof, mu, mse = eng.sweep_ehvi_constrained(crit.cell_lower_bounds, crit.cell_upper_bounds, crit.lo, crit.hi,
                                                               return_values=True, return_pof=True, return_moments=True)  # fmt: skip
    plain = ehvi_ref(mu[:, :2], mse[:, :2], crit.cell_lower_bounds, crit.cell_upper_bounds)
    i, j = int(np.argmax(plain)), int(idx[0])
    g = _g_true(Xs)
    print("seed %d: EHVI winner PoF %.3g, g %.3f | constrained winner PoF %.3g, g %.3f" % (seed, pof[i], g[i], pof[j], g[j]))
    assert pof[i] < 1e-2 and g[i] > 0  # the plain EHVI winner over the same cells: almost surely infeasible, and truly so
    assert pof[j] > 0.3 and g[j] <= 0  # the constrained winner: probably feasible, and truly so
    assert np.array_equal(crit(Xs), vals) and crit(Xs).shape == (len(Xs),)
    b1, i1 = crit.sweep(k=3)
    assert b1.shape == (3,) and i1[0] == j


def test_argmax_restart_and_the_sweep_helpers_return_the_stand_ins_winner():
    X, Y, Xs = _toy(1)
    model = _gp(X, Y)
    eng = model.engine
    crit = bogp.ConstrainedEHVI(model=model, ref_point=Y[:, :2].min(0) - 0.1)
    C = len(crit.cell_lower_bounds)
    assert optim.is_ehvi(crit) and optim.is_constrained_ehvi(crit) and not optim.is_constrained(crit)
    assert not optim.is_constrained_ehvi(bogp.EHVI(model=model, ref_point=[0, 0, 0], Y=Y))
    box = optim.Box([(0, 1), (0, 1)], random_seed=5)
    x, f = optim.argmax_restart(crit, box, eval_budget=500, optimizer="sweep")
    assert eng.calls[-1] == ("sweep_ehvi_constrained", 2, C, 1) and np.allclose(x, eng.winners[-1]) and f > 0
    for name, method in (("sweep-device", "uniform"), ("sweep-device-lhs", "LHS"), ("sweep-device-sobol", "sobol")):
        np.random.seed(3)
        x, f = optim.argmax_restart(crit, box, eval_budget=400, optimizer=name)
        assert eng.calls[-2] == ("generate", 400, method) and eng.calls[-1] == ("sweep_ehvi_constrained", 2, C, 1)
        assert np.allclose(x, eng.winners[-1])
    # the reference's wrapper around the criterion (functools.partial, as MOBO._create_acquisition wraps it)
    x2, _ = optim.argmax_restart(functools.partial(crit), box, eval_budget=300, optimizer="sweep")
    assert np.allclose(x2, eng.winners[-1])
    best, idx, xb = optim.sweep_argmax([crit], Xs[:700])
    assert eng.calls[-1] == ("sweep_ehvi_constrained", 2, C, 1) and best.shape == (1,) and xb.shape == (1, 2)
    mu, mse = O.predict_chunked(eng.st, Xs[:700], 1024)
    want, _ = R.values(mu, mse, eng.st.sigma2, 2, crit.cell_lower_bounds, crit.cell_upper_bounds, crit.lo, crit.hi)
    assert idx[0] == np.argmax(want) and best[0] == want.max() and np.array_equal(xb[0], Xs[idx[0]])
    tv, ti, tx = optim.sweep_topk([crit], Xs[:700], 4)
    assert eng.calls[-1] == ("sweep_ehvi_constrained", 2, C, 4) and tv.shape == (1, 4) and ti[0, 0] == idx[0] and tx.shape == (1, 4, 2)
    gv, gi, gx = optim.sweep_generated([crit], box, 300, 11)
    assert gv.shape == (1,) and gx.shape == (1, 2) and eng.calls[-1] == ("sweep_ehvi_constrained", 2, C, 1)
    assert np.allclose(gx[0], eng.winners[-1])
    kv, ki, kx = optim.sweep_topk_generated([crit], box, 300, 3, 11)
    assert kv.shape == (1, 3) and kv[0, 0] == gv[0] and eng.calls[-1] == ("sweep_ehvi_constrained", 2, C, 3)
    assert not any(c[0] in ("sweep", "sweep_topk", "sweep_ehvi", "sweep_constrained") for c in eng.calls)


def test_refusals_by_name(monkeypatch):
    X, Y, Xs = _toy(2)
    model = _gp(X, Y)
    ref = Y[:, :2].min(0) - 0.1
    crit = bogp.ConstrainedEHVI(model=model, ref_point=ref)
    box = optim.Box([(0, 1), (0, 1)], random_seed=5)
    name = "ConstrainedEHVI"
    with pytest.raises(ValueError, match=r"ref_point \(3,\) and model.y \(24, 3\)"):
        bogp.ConstrainedEHVI(model=model, ref_point=[0, 0, 0])  # no constraint column left
    with pytest.raises(ValueError, match="model.y"):
        bogp.ConstrainedEHVI(model=model, ref_point=[0.0])
    with pytest.raises(ValueError, match="one bound"):
        bogp.ConstrainedEHVI(model=model, ref_point=ref, lo=[0, 0], hi=[1, 1])
    with pytest.raises(ValueError, match="hi >= lo"):
        bogp.ConstrainedEHVI(model=model, ref_point=ref, lo=[1.0], hi=[0.0])
    with pytest.raises(ValueError, match="at most one"):
        bogp.ConstrainedEHVI(model=model, ref_point=ref, Y=Y[:, :2], cells=(np.zeros((1, 2)), np.ones((1, 2))))
    with pytest.raises(NotImplementedError, match=name):
        crit(Xs[:1], return_dx=True)
    for opt_name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match=name):
            optim.argmax_restart(crit, box, eval_budget=50, optimizer=opt_name)
    with pytest.raises(NotImplementedError, match=name):
        optim.believer_batch([crit, crit], box, 100)
    with pytest.raises(NotImplementedError, match=name):
        optim.batch_argmax([crit, crit], box, 100, strategy="believer")
    with pytest.raises(NotImplementedError, match=name):
        optim.ehvi_believer_batch(crit, box, 100, 2)
    with pytest.raises(NotImplementedError, match=name):
        optim.constrained_believer_batch(crit, box, 100, q=2)
    with pytest.raises(NotImplementedError, match=name):
        optim.batch_argmax([crit, crit], box, 100, strategy="thompson")
    with pytest.raises(NotImplementedError, match=name):
        optim.thompson_batch(model, box, 100, 2, criteria=[crit])
    with pytest.raises(NotImplementedError, match=name):
        optim.polish_topk(crit, Xs[:3], np.array([[0.0, 1.0], [0.0, 1.0]]))
    lift = bogp.Lift(np.eye(2), np.zeros(2), np.zeros(2), np.zeros(2), np.ones(2))
    with pytest.raises(NotImplementedError, match=name):
        optim.sweep_argmax([crit], Xs[:50], lift=lift)
    # fixed variables (the reference's partial_argument closure: `masks` / `values`) and cheap callables
    masks, values = np.array([False, True]), [0.5]

    @functools.wraps(crit)
    def fixed(x):
        return crit(x) if masks is None else values

    with pytest.raises(NotImplementedError, match="fixed variables"):
        optim.argmax_restart(fixed, optim.Box([(0, 1)], random_seed=5), eval_budget=50, optimizer="sweep")
    for opt_name in ("sweep", "sweep-device"):
        with pytest.raises(NotImplementedError, match="h / g"):
            optim.argmax_restart(crit, box, g=lambda x: 0.5 - x[0], eval_budget=50, optimizer=opt_name)
        with pytest.raises(NotImplementedError, match="h / g"):
            optim.argmax_restart(crit, box, h=lambda x: 0.5 - x[0], eval_budget=50, optimizer=opt_name)
    with pytest.raises(ValueError, match="sweeps alone"):
        optim.sweep_argmax([crit, crit], Xs[:50])
    monkeypatch.setattr(optim._forest, "is_forest_model", lambda m: True)
    with pytest.raises(NotImplementedError, match="forest"):
        bogp.ConstrainedEHVI(model=model, ref_point=ref)
    monkeypatch.undo()
    monkeypatch.setattr(ConstrainedEhviOracleEngine, "comm_world", 2, raising=False)
    with pytest.raises(NotImplementedError, match="one rank"):
        optim.sweep_argmax([crit], Xs[:50])
    with pytest.raises(NotImplementedError, match=name):
        optim.argmax_restart(crit, box, eval_budget=50, optimizer="sweep")
    assert not any(c[0] in ("sweep", "sweep_topk", "sweep_ehvi", "sweep_constrained") for c in model.engine.calls)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the reference's MOBO under install(expensive_constraints=True, constrained_mobo=True)
# ----------------------------------------------------------------------------------------------------------------------
def _ref_modules():
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim

    return bayes_optim


@pytest.fixture()
def reference(monkeypatch):
    if not os.path.isdir(os.path.join(REF, "bayes_optim")):
        pytest.skip("reference tree not present")
    bayes_optim = _ref_modules()
    created = []

    def engine(device=0):
        created.append(ConstrainedEhviOracleEngine(device))
        return created[-1]

    monkeypatch.setattr(bogp._lib, "Engine", engine)
    yield bayes_optim, created
    bogp.uninstall()


_F = (lambda x: x[0] ** 2 + 0.5 * x[1], lambda x: x[1] ** 2 + 0.5 * x[0])  # minimised: both pull towards the origin, where g > 0


def _mobo(bayes_optim, optimizer="sweep", **kw):
    from bayes_optim import MOBO
    from bayes_optim.search_space import RealSpace

    space = RealSpace([0, 1], var_name="a") + RealSpace([0, 1], var_name="b")
    model = bayes_optim.GaussianProcess(theta0=np.full(2, 1.0), thetaL=np.full(2, 1e-2), thetaU=np.full(2, 1e2), nugget=1e-6,
                                        noise_estim=False, likelihood="concentrated")  # fmt: skip
    opt = MOBO(search_space=space, obj_fun=_F, model=model, max_FEs=100, DoE_size=8, eval_type="list", n_job=1, verbose=False,
               minimize=True, acquisition_optimization={"optimizer": optimizer, "max_FEs": 300}, **kw)  # fmt: skip
    return opt, model


def _evaluate(X):
    A = np.asarray(X, dtype=float)
    return [tuple(f(x) for f in _F) for x in A], _g_true(A).tolist()


def test_install_keyword_rules():
    with pytest.raises(ValueError, match="constrained_mobo=True needs expensive_constraints=True"):
        bogp.install(object(), constrained_mobo=True)


@pytest.mark.timeout(900)
def test_the_reference_mobo_models_its_g_vals(reference):
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True, constrained_mobo=True)
    np.random.seed(4)
    opt, model = _mobo(bayes_optim)
    assert type(model).__module__.startswith("bogp")
    X = opt.ask()  # the DoE
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    assert model.y.shape == (8, 3)
    eng = model.engine
    for it in range(6):
        n_before = len(eng.__dict__.get("winners", []))
        X = opt.ask(1)
        assert model.engine is eng and len(eng.winners) == n_before + 1  # every ask goes through the new call ...
        assert eng.calls[-1][0] == "sweep_ehvi_constrained" and eng.calls[-1][1] == 2
        np.testing.assert_allclose(X[0], eng.winners[-1], rtol=0, atol=1e-12)  # ... and proposes its winner
        f, g = _evaluate(X)
        opt.tell(X, f, g_vals=g)
    assert model.y.shape == (len(opt.data), 3) and eng.n_t == 3 and len(opt.data) == 14
    assert not any(c[0] in ("sweep", "sweep_topk", "sweep_ehvi", "sweep_constrained") for c in eng.calls)
    C = opt._bogp_constraints
    assert C.shape == (14, 1) and np.allclose(C[:, 0], _g_true(np.asarray(opt.data, dtype=float)[:, :2]))
    np.testing.assert_allclose(model.y[:, 2], C[:, 0] / C[:, 0].std())  # scaled, never shifted
    np.testing.assert_allclose(model.y[:, :2], opt.y)  # the objectives as the reference transforms them
    crit = optim.unwrap_criterion(opt._create_acquisition())[0]
    assert isinstance(crit, bogp.ConstrainedEHVI) and np.array_equal(crit.lo, [-INF]) and np.array_equal(crit.hi, [0.0])
    np.testing.assert_allclose(crit.ref_point, opt.ref_point)
    ok = C[:, 0] <= 0
    assert crit.n_feasible == ok.sum()
    # feasible_front: feasible rows only, none dominated by another feasible row, and every other feasible row is dominated
    front = bogp.feasible_front(opt)
    rows = np.asarray(front, dtype=float)[:, :2].reshape(-1, 2)
    assert len(rows) == (pareto.is_non_dominated(opt.y[ok]).sum() if ok.any() else 0)
    assert np.all(_g_true(rows) <= 0)
    data = np.asarray(opt.data, dtype=float)[:, :2]
    yfront = np.array([opt.y[np.flatnonzero(np.all(np.isclose(data, r), axis=1))[0]] for r in rows]).reshape(-1, 2)
    for yr in opt.y[ok]:
        on_front = np.any(np.all(yfront == yr, axis=1))
        dominated = np.any(np.all(yfront >= yr, axis=1) & np.any(yfront > yr, axis=1))
        assert on_front != dominated
    # n_point = q is refused by name, as are the errors of the tell wrapper
    with pytest.raises(NotImplementedError, match="ConstrainedEHVI"):
        opt.ask(3)
    X = opt.ask(1)
    f, g = _evaluate(X)
    with pytest.raises(ValueError, match="carries no h_vals"):
        opt.tell(X, f)
    with pytest.raises(ValueError, match="g and"):
        opt.tell(X, f, g_vals=[[g[0], g[0]]])
    with pytest.raises(ValueError, match="non-finite"):
        opt.tell(X, f, g_vals=[np.nan])
    n = len(opt.data)
    assert len(opt._bogp_constraints) == n
    opt.tell(X, f, g_vals=g, h_vals=None)
    assert len(opt.data) == n + 1 == len(opt._bogp_constraints)


@pytest.mark.timeout(900)
def test_mixed_tells_equalities_and_refused_configurations(reference):
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True, constrained_mobo=True, equality_tol=0.2)
    np.random.seed(5)
    opt, model = _mobo(bayes_optim)
    X = opt.ask()
    f, g = _evaluate(X)
    opt.tell(X, f)  # no constraint values: the reference's behaviour ...
    assert getattr(opt, "_bogp_constraints", None) is None and model.y.shape[1] == 2 and bogp.feasible_front(opt) is None
    X2 = opt.ask(1)
    assert model.engine.calls[-1][0] == "sweep_ehvi"
    f2, g2 = _evaluate(X2)
    with pytest.raises(ValueError, match="were told without them"):  # ... and then values cannot start
        opt.tell(X2, f2, g_vals=g2)
    # one g and one h column: bounds (-inf, 0] and [-tol, tol] / std
    np.random.seed(6)
    opt, model = _mobo(bayes_optim)
    X = opt.ask()
    f, g = _evaluate(X)
    h = (np.asarray(X)[:, 0] - 0.5).tolist()
    opt.tell(X, f, g_vals=g, h_vals=[[v] for v in h])
    assert model.y.shape == (8, 4) and opt._bogp_constraint_counts == (1, 1)
    crit = optim.unwrap_criterion(opt._create_acquisition())[0]
    assert isinstance(crit, bogp.ConstrainedEHVI)
    np.testing.assert_allclose(crit.lo, [-INF, -0.2 / np.std(h)])
    np.testing.assert_allclose(crit.hi, [0.0, 0.2 / np.std(h)])
    opt.ask(1)
    assert model.engine.calls[-1][0] == "sweep_ehvi_constrained"
    # an inner optimiser outside the sweep family is refused instead of dropping the constraints
    for name in ("OnePlusOne_Cholesky_CMA", "BFGS"):
        np.random.seed(7)
        o, _ = _mobo(bayes_optim, optimizer=name)
        Xd = o.ask()
        fd, gd = _evaluate(Xd)
        o.tell(Xd, fd, g_vals=gd)
        with pytest.raises(NotImplementedError, match="sweep family"):
            o.ask(1)


@pytest.mark.timeout(900)
def test_default_installs_are_unchanged(reference):
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True)  # without constrained_mobo: refused by name, exactly as before
    np.random.seed(4)
    opt, model = _mobo(bayes_optim)
    X = opt.ask()
    f, g = _evaluate(X)
    with pytest.raises(NotImplementedError, match="not for the multi-objective MOBO"):
        opt.tell(X, f, g_vals=g)
    opt.tell(X, f)
    assert model.y.shape[1] == 2
    bogp.uninstall()
    bogp.install(bayes_optim)  # the default: the values are ignored, as in the reference
    np.random.seed(4)
    opt, model = _mobo(bayes_optim)
    X = opt.ask()
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    X = opt.ask(1)
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    eng = model.engine
    assert model.y.shape[1] == 2 and getattr(opt, "_bogp_constraints", None) is None and bogp.feasible_front(opt) is None
    assert any(c[0] == "sweep_ehvi" for c in eng.calls) and not any(c[0] == "sweep_ehvi_constrained" for c in eng.calls)
