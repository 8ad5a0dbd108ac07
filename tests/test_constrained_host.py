"""Modelled constraints on the host side (no GPU): the library's host function `bogp_feasibility` against mpmath, exact cases of it
and of the NumPy restatement (tests/support/constrained_ref.py), `bogp.Constrained` and the sweep routing on the oracle-backed
stand-in engine (tests/support/constrained_engine.py), a toy problem on which the feasibility weight changes the winner, and the
reference's unmodified `BO` under `install(expensive_constraints=True)`."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle import gp_oracle as O
from support import constrained_ref as R
from support.constrained_engine import ConstrainedOracleEngine

import bogp
from bogp import _lib, optim

REF = "/root/reference"
INF = float("inf")


# ----------------------------------------------------------------------------------------------------------------------
# 1. bogp_feasibility against mpmath (ledger T18)
# ----------------------------------------------------------------------------------------------------------------------
# Measured over this draw: the library's host function stays within 0.905 x the allowance below (scipy's ndtr in the same
# two-branch form: 2.14; a one-branch Phi(zb) - Phi(za): over 100).  F = 4 x that, rounded up: the margin is for another libm.
T18_F = 4


def _draw(n_trials=30000, seed=1):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_trials):
        mu = rng.normal() * 10 ** rng.uniform(-2, 1.2)
        sd = 10 ** rng.uniform(-3, 1)
        kind = rng.integers(3)
        if kind == 0:
            lo, hi = -INF, 0.0
        elif kind == 1:
            t = 10 ** rng.uniform(-4, 0)
            lo, hi = -t, t
        else:
            lo, hi = np.sort(rng.normal(size=2) * 3)
        mse = sd * sd
        s = np.sqrt(mse)
        za, zb = (lo - mu) / s, (hi - mu) / s
        if max(abs(za) if np.isfinite(za) else 0.0, abs(zb)) > 37:
            continue
        rows.append((mu, mse, float(lo), float(hi), za, zb))
    return rows


def test_feasibility_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    eps = np.finfo(float).eps
    rows = _draw()
    assert len(rows) >= 10000
    assert sum(1 for r in rows if r[4] > 0) >= 500  # a condition, not a tolerance: the upper-tail branch must be exercised
    worst = 0.0
    for mu, mse, lo, hi, za, zb in rows:
        v = _lib.feasibility(mu, mse, 1.0, lo, hi)  # (sigma2 = 1, sd >= 1e-3: the guard stays off)
        if za > 0:
            A, B = mp.ncdf(-mp.mpf(float(za))), mp.ncdf(-mp.mpf(float(zb)))
            exact = A - B
        else:
            B = mp.ncdf(mp.mpf(float(zb)))
            A = mp.ncdf(mp.mpf(float(za))) if np.isfinite(za) else mp.mpf(0)
            exact = B - A
        za2 = za * za if np.isfinite(za) else 0.0
        allow = eps * ((1 + za2) * A + (1 + zb * zb) * B)
        worst = max(worst, float(abs(mp.mpf(float(v)) - exact) / allow))
    print("T18: worst |bogp_feasibility - exact| / allowance = %.4g over %d rows (F = %d)" % (worst, len(rows), T18_F))
    assert worst <= T18_F


def test_restatement_equals_the_host_function_on_the_draw():
    rows = _draw(4000, seed=2)
    a = np.array(rows)
    ref = np.array([R.feasibility(np.array([r[0]]), np.array([r[1]]), 1.0, r[2], r[3])[0] for r in rows])
    lib = np.array([_lib.feasibility(r[0], r[1], 1.0, r[2], r[3]) for r in rows])
    # scipy's ndtr and the library's (cephes' branches on libm's erf / erfc) differ by rounding only: T18's allowance, both at 2.14 + 0.905
    eps = np.finfo(float).eps
    from scipy.special import ndtr

    za, zb = a[:, 4], a[:, 5]
    up = za > 0
    A = np.where(up, ndtr(-za), ndtr(za))
    B = np.where(up, ndtr(-zb), ndtr(zb))
    allow = eps * ((1 + np.where(np.isfinite(za), za * za, 0.0)) * A + (1 + zb * zb) * B)
    assert np.all(np.abs(ref - lib) <= (T18_F + 3) * allow)


# ----------------------------------------------------------------------------------------------------------------------
# 2. exact cases
# ----------------------------------------------------------------------------------------------------------------------
def _moments(M=200, m=3, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(M, m)), rng.uniform(1e-3, 2.0, size=(M, m)), rng.uniform(0.5, 2.0, size=m)


def test_every_bound_infinite_is_exactly_the_base():
    mu, mse, s2 = _moments()
    assert _lib.feasibility(0.3, 0.7, 1.0, -INF, INF) == 1.0
    acq = [(O.ACQ_EI, 0.0), (O.ACQ_EPSILON_PI, 0.05), (O.ACQ_MGFI, 2.0)]
    for minimize in (True, False):
        vals, P = R.constrained(mu, mse, s2, [-INF, -INF], [INF, INF], acq, -0.2, minimize)
        assert np.all(P == 1.0)
        for (a, p), v in zip(acq, vals):
            assert np.array_equal(v, np.ravel(O.acquisition(a, p, mu[:, 0], mse[:, 0], -0.2, s2[0], minimize)))


def test_lo_equal_hi_is_zero_and_zero_variance_is_the_indicator():
    mu, mse, s2 = _moments()
    vals, P = R.constrained(mu, mse, s2, [0.25, -INF], [0.25, INF], [(O.ACQ_EI, 0.0)], 0.0, True)
    assert np.all(P == 0.0) and np.all(vals == 0.0)
    assert _lib.feasibility(0.1, 0.5, 1.0, 0.25, 0.25) == 0.0
    for x, want in ((-1.5, 0.0), (-1.0, 1.0), (0.0, 1.0), (1.0, 1.0), (1.5, 0.0)):  # both sides of both bounds, and the bounds themselves
        assert _lib.feasibility(x, 0.0, 1.0, -1.0, 1.0) == want
        assert R.feasibility(np.array([x]), np.array([0.0]), 1.0, -1.0, 1.0)[0] == want
        assert _lib.feasibility(x, 1e-14, 1.0, -1.0, 1.0) == want  # sd / sqrt(sigma2) = 1e-7: under the guard
    assert _lib.feasibility(-2.0, 0.0, 1.0, -INF, 0.0) == 1.0 and _lib.feasibility(2.0, 0.0, 1.0, -INF, 0.0) == 0.0
    assert _lib.feasibility(2.0, 0.0, 1.0, 0.0, INF) == 1.0 and _lib.feasibility(-2.0, 0.0, 1.0, 0.0, INF) == 0.0


def test_acq_none_is_the_probability_and_refusals():
    mu, mse, s2 = _moments()
    vals, P = R.constrained(mu, mse, s2, [-INF, -0.5], [0.0, 0.5], [(R.ACQ_NONE, 0.0)], 123.0, True)
    assert np.array_equal(vals[0], P) and 0 < P.min() and P.max() < 1
    p1 = np.array([_lib.feasibility(mu[i, 1], mse[i, 1], s2[1], -INF, 0.0) for i in range(len(mu))])
    p2 = np.array([_lib.feasibility(mu[i, 2], mse[i, 2], s2[2], -0.5, 0.5) for i in range(len(mu))])
    np.testing.assert_allclose(P, p1 * p2, rtol=1e-12)
    assert _lib.ACQ_NONE == R.ACQ_NONE == -1
    with pytest.raises(ValueError, match="UCB"):
        R.constrained(mu, mse, s2, [-INF, -INF], [0, 0], [(O.ACQ_UCB, 0.5)], 0.0, True)
    with pytest.raises(ValueError, match="hi >= lo"):
        R.constrained(mu, mse, s2, [0.5, -INF], [0.0, 0], [(O.ACQ_EI, 0.0)], 0.0, True)


# ----------------------------------------------------------------------------------------------------------------------
# 3. bogp.Constrained on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
def _g_true(X):
    return 0.8 - X[:, 0] - X[:, 1] + 0.3 * np.sin(6 * X[:, 0])


def _toy(seed, N=16, M=3000):
    """minimise x0 + x1 on [0, 1]^2 subject to 0.8 - x0 - x1 + 0.3 sin(6 x0) <= 0; columns scaled as the drop-in scales them"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, 2))
    f, g = X.sum(1), _g_true(X)
    Y = np.c_[(f - f.mean()) / f.std(), g / g.std()]
    Xs = rng.uniform(0, 1, (M, 2))
    return X, Y, Xs


def _gp(X, Y):
    d = X.shape[1]
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(d, beta=0.0), corr="matern52", thetaL=[1e-3] * d, thetaU=[1e3] * d, nugget=0)
    model._engine = ConstrainedOracleEngine()
    model.set_state(np.full(d, 30.0), X, Y)
    return model


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_feasibility_weight_moves_the_winner_into_the_feasible_region(seed):
    X, Y, Xs = _toy(seed)
    model = _gp(X, Y)
    eng = model.engine
    crit = bogp.Constrained(model=model, fun="EI", minimize=True)
    assert crit.n_feasible > 0 and crit.plugin == Y[Y[:, 1] <= 0, 0].min()
    eng.upload_candidates(Xs)
    best, idx, vals, pof, mu, mse = eng.sweep_constrained([(crit.acq_id, crit.acq_par())], crit.effective_plugin(), True, crit.lo, crit.hi,
                                                         return_values=True, return_pof=True, return_moments=True)  # fmt: skip
    ei = np.ravel(O.acquisition(O.ACQ_EI, 0.0, mu[:, 0], mse[:, 0], crit.plugin, eng.st.sigma2[0], True))
    i, j = int(np.argmax(ei)), int(idx[0, 0])
    g = _g_true(Xs)
    print("seed %d: EI winner PoF %.3g, g %.3f | constrained winner PoF %.3g, g %.3f" % (seed, pof[i], g[i], pof[j], g[j]))
    assert pof[i] < 1e-2 and g[i] > 0  # the plain EI winner: almost surely infeasible, and truly so
    assert pof[j] > 0.3 and g[j] <= 0  # the constrained winner: probably feasible, and truly so
    assert np.array_equal(crit(Xs), vals[0]) and crit(Xs).shape == (len(Xs),)
    b1, i1 = crit.sweep(k=3)
    assert b1.shape == (3,) and i1[0] == j


def test_plugin_is_the_best_feasible_value_both_ways():
    X, Y, _ = _toy(0)
    model = _gp(X, Y)
    feas = Y[:, 1] <= 0
    assert 0 < feas.sum() < len(Y) and Y[:, 0].min() < Y[feas, 0].min()  # (the best row overall is infeasible: the plugins differ)
    assert bogp.Constrained(model=model, fun="EI", minimize=True).plugin == Y[feas, 0].min()
    assert bogp.Constrained(model=model, fun="MGFI", minimize=False, t=2).plugin == -Y[feas, 0].max()
    wide = bogp.Constrained(model=model, fun="EI", lo=[-INF], hi=[INF])
    assert wide.plugin == Y[:, 0].min()
    given = bogp.Constrained(model=model, fun="EI", minimize=False, plugin=0.7)
    assert given.plugin == -0.7 and given.acq_id == _lib.ACQ_EI
    c = bogp.Constrained(model=model, fun="EpsilonPI", epsilon=0.05)
    assert (c.acq_id, c.acq_par()) == (_lib.ACQ_EPSILON_PI, 0.05)
    c = bogp.Constrained(model=model, fun="PI")
    assert (c.acq_id, c.acq_par()) == (_lib.ACQ_EPSILON_PI, 0.0)
    c = bogp.Constrained(model=model, fun="MGFI", t=50)
    assert (c.acq_id, c.acq_par()) == (_lib.ACQ_MGFI, 22.36)
    assert c.is_constrained and optim.is_constrained(c) and not optim.is_constrained(bogp.EI(model=model))


def test_without_a_feasible_row_the_calls_are_feasibility_only():
    X, Y, Xs = _toy(0)
    model = _gp(X, Y)
    eng = model.engine
    none = bogp.Constrained(model=model, fun="EI", lo=[-INF], hi=[Y[:, 1].min() - 1.0])
    assert none.n_feasible == 0 and none.plugin is None and none.feasibility_only
    none(Xs[:50])
    assert eng.calls[-1] == ("sweep_constrained", (_lib.ACQ_NONE,), 1)
    only = bogp.Constrained(model=model, fun=None)
    assert only.feasibility_only
    v = only(Xs[:50])
    assert eng.calls[-1] == ("sweep_constrained", (_lib.ACQ_NONE,), 1) and np.all((v >= 0) & (v <= 1))
    ei = bogp.Constrained(model=model, fun="EI")
    ei(Xs[:50])
    assert eng.calls[-1] == ("sweep_constrained", (_lib.ACQ_EI,), 1)
    assert not any(c[0] in ("sweep", "sweep_topk") for c in eng.calls)  # never a single-target criterion on the multi-target model


def test_argmax_restart_and_the_sweep_helpers_return_the_stand_ins_winner():
    X, Y, Xs = _toy(1)
    model = _gp(X, Y)
    eng = model.engine
    crit = bogp.Constrained(model=model, fun="EI")
    box = optim.Box([(0, 1), (0, 1)], random_seed=5)
    x, f = optim.argmax_restart(crit, box, eval_budget=500, optimizer="sweep")
    assert eng.calls[-1][0] == "sweep_constrained" and np.allclose(x, eng.winners[-1]) and f > 0
    np.random.seed(3)
    x, f = optim.argmax_restart(crit, box, eval_budget=400, optimizer="sweep-device")
    assert eng.calls[-2] == ("generate", 400, "uniform") and eng.calls[-1][0] == "sweep_constrained" and np.allclose(x, eng.winners[-1])
    # the reference's wrapper around the criterion (functools.partial, as BaseBO._create_acquisition binds return_dx)
    import functools

    x2, _ = optim.argmax_restart(functools.partial(crit, return_dx=False), box, eval_budget=300, optimizer="sweep")
    assert np.allclose(x2, eng.winners[-1])
    # q criteria in one call, top-k, generated designs, batch_argmax
    crits = [crit, bogp.Constrained(model=model, fun="MGFI", t=2), bogp.Constrained(model=model, fun="EpsilonPI", epsilon=0.05)]
    best, idx, xb = optim.sweep_argmax(crits, Xs[:700])
    assert eng.calls[-1] == ("sweep_constrained", (_lib.ACQ_EI, _lib.ACQ_MGFI, _lib.ACQ_EPSILON_PI), 1) and best.shape == (3,) and xb.shape == (3, 2)
    mu, mse = O.predict_chunked(eng.st, Xs[:700], 1024)
    want, _ = R.constrained(mu, mse, eng.st.sigma2, crit.lo, crit.hi, [(c.acq_id, c.acq_par()) for c in crits], crit.plugin, True)
    assert np.array_equal(idx, np.argmax(want, axis=1)) and np.array_equal(best, want.max(axis=1))
    tv, ti, tx = optim.sweep_topk(crits, Xs[:700], 4)
    assert tv.shape == (3, 4) and np.array_equal(ti[:, 0], idx) and tx.shape == (3, 4, 2)
    gv, gi, gx = optim.sweep_generated(crits, box, 300, 11)
    assert gv.shape == (3,) and gx.shape == (3, 2) and eng.calls[-1][0] == "sweep_constrained"
    kv, ki, kx = optim.sweep_topk_generated(crits, box, 300, 3, 11)
    assert kv.shape == (3, 3) and np.array_equal(kv[:, 0], gv)
    xs, fs = optim.batch_argmax(crits, box, 300, k=4, strategy="topk")
    assert len(xs) == 3 and len({tuple(x) for x in xs}) == 3 and eng.calls[-1] == ("sweep_constrained", (_lib.ACQ_EI, _lib.ACQ_MGFI, _lib.ACQ_EPSILON_PI), 4)
    # cheap callables and fixed variables keep today's rules: the host-sampled sweep serves them, device designs refuse them
    x3, _ = optim.argmax_restart(crit, box, g=lambda x: 0.5 - x[0], eval_budget=300, optimizer="sweep")
    assert x3[0] >= 0.5
    with pytest.raises(NotImplementedError, match="unconstrained"):
        optim.argmax_restart(crit, box, g=lambda x: 0.5 - x[0], eval_budget=300, optimizer="sweep-device")


def test_refusals_by_name(monkeypatch):
    X, Y, Xs = _toy(2)
    model = _gp(X, Y)
    crit = bogp.Constrained(model=model, fun="EI")
    box = optim.Box([(0, 1), (0, 1)], random_seed=5)
    with pytest.raises(ValueError, match="UCB"):
        bogp.Constrained(model=model, fun="UCB")
    with pytest.raises(ValueError, match="fun must be"):
        bogp.Constrained(model=model, fun="EHVI")
    with pytest.raises(TypeError, match="takes no parameter"):
        bogp.Constrained(model=model, fun="EI", t=2)
    with pytest.raises(ValueError, match="one bound"):
        bogp.Constrained(model=model, fun="EI", lo=[0, 0], hi=[1, 1])
    with pytest.raises(ValueError, match="hi >= lo"):
        bogp.Constrained(model=model, fun="EI", lo=[1.0], hi=[0.0])
    single = _gp(X, Y[:, :1])
    with pytest.raises(ValueError, match="m >= 2"):
        bogp.Constrained(model=single, fun="EI")
    with pytest.raises(NotImplementedError, match="input gradient"):
        crit(Xs[:1], return_dx=True)
    for name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="input gradient"):
            optim.argmax_restart(crit, box, eval_budget=50, optimizer=name)
    with pytest.raises(NotImplementedError, match="believer"):
        optim.believer_batch([crit, crit], box, 100)
    with pytest.raises(NotImplementedError, match="believer"):
        optim.batch_argmax([crit, crit], box, 100, strategy="believer")
    with pytest.raises(NotImplementedError, match="Thompson"):
        optim.batch_argmax([crit, crit], box, 100, strategy="thompson")
    lift = bogp.Lift(np.eye(2), np.zeros(2), np.zeros(2), np.zeros(2), np.ones(2))
    with pytest.raises(NotImplementedError, match="lifted sweep"):
        optim.sweep_argmax([crit], Xs[:50], lift=lift)
    with pytest.raises(ValueError, match="cannot share a sweep"):
        optim.sweep_argmax([crit, bogp.EI(model=single)], Xs[:50])
    other = bogp.Constrained(model=model, fun="EI", lo=[-INF], hi=[0.5])
    with pytest.raises(ValueError, match="share model, bounds"):
        optim.sweep_topk([crit, other], Xs[:50], 2)
    monkeypatch.setattr(optim._forest, "is_forest_model", lambda m: True)
    with pytest.raises(NotImplementedError, match="forest"):
        bogp.Constrained(model=model, fun="EI")
    monkeypatch.undo()
    monkeypatch.setattr(ConstrainedOracleEngine, "comm_world", 2)
    with pytest.raises(NotImplementedError, match="one rank"):
        optim.sweep_argmax([crit], Xs[:50])


# ----------------------------------------------------------------------------------------------------------------------
# 4. the reference's BO under install(expensive_constraints=True)
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
        created.append(ConstrainedOracleEngine(device))
        return created[-1]

    monkeypatch.setattr(bogp._lib, "Engine", engine)
    yield bayes_optim, created
    bogp.uninstall()


def _bo(bayes_optim, optimizer="sweep", fun="EI", cls="BO", **kw):
    from bayes_optim.search_space import RealSpace

    space = RealSpace([0, 1], var_name="a") + RealSpace([0, 1], var_name="b")
    model = bayes_optim.GaussianProcess(theta0=np.full(2, 1.0), thetaL=np.full(2, 1e-2), thetaU=np.full(2, 1e2), nugget=1e-6,
                                        noise_estim=False, likelihood="concentrated")  # fmt: skip
    opt = getattr(bayes_optim, cls)(search_space=space, obj_fun=lambda x: x[0] + x[1], model=model, max_FEs=100, DoE_size=6, eval_type="list",
                                    n_job=1, verbose=False, minimize=True, acquisition_fun=fun,
                                    acquisition_optimization={"optimizer": optimizer, "max_FEs": 300}, **kw)  # fmt: skip
    return opt, model


def _evaluate(X):
    A = np.asarray(X, dtype=float)
    return A.sum(1).tolist(), _g_true(A).tolist()


@pytest.mark.timeout(900)
def test_the_reference_bo_models_its_g_vals(reference):
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True)
    np.random.seed(4)
    opt, model = _bo(bayes_optim)
    assert type(model).__module__.startswith("bogp")
    X = opt.ask()  # the DoE
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    eng = model.engine
    for it in range(10):
        n_before = len(eng.__dict__.get("winners", []))
        X = opt.ask(1)
        assert all(0 <= v <= 1 for x in X for v in x)
        assert model.engine is eng and len(eng.winners) == n_before + 1  # every ask goes through the constrained sweep ...
        np.testing.assert_allclose(X[0], eng.winners[-1], rtol=0, atol=1e-12)  # ... and proposes its winner
        f, g = _evaluate(X)
        opt.tell(X, f, g_vals=g)
    eng = model.engine
    assert model.y.shape == (len(opt.data), 2) and eng.n_t == 2
    assert len(opt.data) == 16
    assert not any(c[0] in ("sweep", "sweep_topk") for c in eng.calls) and any(c[0] == "sweep_constrained" for c in eng.calls)
    C = opt._bogp_constraints
    assert C.shape == (len(opt.data), 1) and np.allclose(C[:, 0], _g_true(np.asarray(opt.data, dtype=float)[:, :2]))
    np.testing.assert_allclose(model.y[:, 1], C[:, 0] / C[:, 0].std())  # scaled, never shifted
    fit = np.asarray(opt.data.fitness, dtype=float)
    np.testing.assert_allclose(model.y[:, 0], (fit - fit.mean()) / fit.std())
    best = bogp.feasible_xopt(opt)
    ok = C[:, 0] <= 0
    if ok.any():
        assert float(best.fitness) == fit[ok].min() and _g_true(np.asarray([best.tolist()], dtype=float))[0] <= 0
    else:
        assert best is None
    # the errors of the tell wrapper
    X = opt.ask(1)
    f, g = _evaluate(X)
    with pytest.raises(ValueError, match="carries no h_vals"):
        opt.tell(X, f)
    with pytest.raises(ValueError, match="g and"):
        opt.tell(X, f, g_vals=[[g[0], g[0]]])
    with pytest.raises(ValueError, match="non-finite"):
        opt.tell(X, f, g_vals=[np.nan])
    n = len(opt.data)
    opt.tell(X, [np.nan], g_vals=[np.nan])  # a failed evaluation: the row is dropped by post_eval_check, and so are its values
    assert len(opt.data) == n == len(opt._bogp_constraints)
    opt.tell(X, f, g_vals=g, h_vals=None)
    assert len(opt.data) == n + 1 == len(opt._bogp_constraints)


@pytest.mark.timeout(900)
def test_mixed_tells_equalities_and_refused_configurations(reference):
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True, equality_tol=0.2)
    np.random.seed(5)
    opt, model = _bo(bayes_optim, fun="MGFI")
    X = opt.ask()
    f, g = _evaluate(X)
    opt.tell(X, f)  # no constraint values: the reference's behaviour ...
    assert getattr(opt, "_bogp_constraints", None) is None and model.y.shape[1] == 1
    X2 = opt.ask(1)
    f2, g2 = _evaluate(X2)
    with pytest.raises(ValueError, match="were told without them"):  # ... and then values cannot start
        opt.tell(X2, f2, g_vals=g2)
    # one g and one h column: bounds (-inf, 0] and [-tol, tol] / std
    np.random.seed(6)
    opt, model = _bo(bayes_optim, fun="MGFI")
    X = opt.ask()
    f, g = _evaluate(X)
    h = (np.asarray(X)[:, 0] - 0.5).tolist()
    opt.tell(X, f, g_vals=g, h_vals=[[v] for v in h])
    assert model.y.shape == (6, 3) and opt._bogp_constraint_counts == (1, 1)
    from bogp.optim import unwrap_criterion

    crit = unwrap_criterion(opt._create_acquisition(par={}, return_dx=False))[0]
    assert isinstance(crit, bogp.Constrained) and crit.fun == "MGFI" and crit.acq_par() == opt._acquisition_par.get("t", 1)
    np.testing.assert_allclose(crit.lo, [-INF, -0.2 / np.std(h)])
    np.testing.assert_allclose(crit.hi, [0.0, 0.2 / np.std(h)])
    X = opt.ask(1)
    assert any(c[0] == "sweep_constrained" for c in model.engine.calls)
    # UCB, and an inner optimiser outside the sweep family, are refused instead of dropping the constraints
    for kw, err, match in ((dict(fun="UCB"), ValueError, "UCB"), (dict(optimizer="OnePlusOne_Cholesky_CMA"), NotImplementedError, "sweep")):
        np.random.seed(7)
        o, _ = _bo(bayes_optim, **kw)
        Xd = o.ask()
        fd, gd = _evaluate(Xd)
        o.tell(Xd, fd, g_vals=gd)
        with pytest.raises(err, match=match):
            o.ask(1)


@pytest.mark.timeout(900)
def test_parallel_bo_stays_on_topk(reference):
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True, batch_strategy="believer")
    np.random.seed(8)
    opt, model = _bo(bayes_optim, cls="ParallelBO", fun="MGFI", n_point=3)
    X = opt.ask(6)
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    X = opt.ask()
    assert len(X) == 3 and len({tuple(x) for x in X}) == 3
    calls = [c for c in model.engine.calls if c[0] == "sweep_constrained"]
    assert calls and calls[-1][1] == (_lib.ACQ_MGFI,) * 3 and calls[-1][2] > 1  # one call, q criteria, top-k fall-backs
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    assert model.y.shape == (9, 2)


@pytest.mark.timeout(900)
def test_default_install_ignores_g_vals(reference):
    bayes_optim, created = reference
    bogp.install(bayes_optim)
    np.random.seed(4)
    opt, model = _bo(bayes_optim)
    for _ in range(4):
        X = opt.ask(1)
        f, g = _evaluate(X)
        opt.tell(X, f, g_vals=g)
    eng = model.engine
    assert model.y.shape[1] == 1 and getattr(opt, "_bogp_constraints", None) is None
    assert not any(c[0] == "sweep_constrained" for c in eng.calls) and any(c[0] == "sweep" for c in eng.calls)
    assert bogp.feasible_xopt(opt) is None
