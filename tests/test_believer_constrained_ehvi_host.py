"""Kriging-believer batches for constrained EHVI, the parts that need no GPU: (a) the conditions every shared case
(tests/believer_constrained_ehvi_cases.py) must meet, asserted on the dense restatement
(tests/support/believer_constrained_ehvi_ref.py) alone, and the restatement against a dense refit; (b) the routing and the refusals of
`optim.constrained_ehvi_believer_batch`, the untouched refusals of the other batch entries, the validation of
`install(constrained_mobo_batches=...)` and the reference's MOBO(n_point=3) on the oracle-backed stand-in."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle import gp_oracle as O

import bogp
from bogp import _lib, optim, pareto
from bogp.optim import constrained_ehvi_believer_batch  # noqa: F401  (what this module is about: without it nothing here can run)
from believer_constrained_ehvi_cases import CASES, IDS, Q, constraint_bounds, feasible_rows, low_ref, problem
from support import constrained_ehvi_ref as R
from support.believer_constrained_ehvi_engine import BelieverConstrainedEhviOracleEngine
from support.believer_constrained_ehvi_ref import BelieverConstrainedEhviRef, cells_of

REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
INF = float("inf")


def _ref_of(st):
    return BelieverConstrainedEhviRef(st.X, st.theta, st.kernel, dict(C=st.C, gamma=st.gamma, beta=float(st.beta[0, 0]), sigma2=st.sigma2))


def _state(X, Y, args):
    return O.make_state(args[2], X, Y, args[0], args[1], args[3], estimate_trend=args[4], beta=args[5])


# ----------------------------------------------------------------------------------------------------------------------
# (a) the conditions on the shared cases
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    """every shared case on the restatement, computed once"""
    runs = []
    for c in CASES:
        X, Y, args, Xs, pend, lo, hi, ref_point, front = c.build()
        ref = _ref_of(_state(X, Y, args))
        out = ref.run(Xs, front, ref_point, Q, lo, hi, pending=pend, believe_front=c.believe_front, feasibility_only=c.feasibility_only)
        runs.append((c, ref, lo, hi, ref_point, out))
    return runs


def test_the_case_list_is_the_one_specified():
    cells = [c for c in CASES if not c.feasibility_only and not c.one_cell and c.m < 8]
    assert len(cells) == 24 and {(c.m_obj, c.c, c.N, c.noisy, c.n_pend) for c in cells} == {
        (mo, cc, N, noisy, p) for mo, cc in ((2, 1), (2, 2), (3, 1)) for N in (70, 530) for noisy in (False, True) for p in (0, 2)}  # fmt: skip
    assert all((c.kernel == _lib.KERNEL_SE) == c.noisy for c in CASES)
    assert sorted((c.m_obj, c.c, c.rows) for c in CASES if c.m == 8) == [(2, 6, 599), (7, 1, 599)]
    assert [c.id for c in CASES if c.one_cell] == ["N70-o2-c1-m52-noiseless-p2-onecell"]
    assert sum(c.feasibility_only for c in CASES) == 10 and all(c.believe_front or c.m_obj == 7 for c in CASES)
    assert len(set(IDS)) == len(IDS)
    assert bogp.constrained_ehvi_believer_batch is constrained_ehvi_believer_batch  # exported under the package's name


def test_no_step_of_a_case_is_a_tie(restated):
    """every step's winner beats the runner-up by >= 1e-9 relative; no NaN anywhere"""
    for c, ref, lo, hi, rp, out in restated:
        gap = (out["best_val"] - out["second"]) / np.abs(out["best_val"])
        assert np.all(gap >= 1e-9), (c.id, gap)
        assert len(set(out["best_idx"].tolist())) == Q
        assert not np.any(np.isnan(out["val"])) and not np.any(np.isnan(out["pof"])), c.id


def test_no_row_of_a_case_stands_at_the_variance_guard(restated):
    """no row has sd / sqrt(sigma2) within 1e-3 of the 1e-6 guard of bogp_feasibility, at any step and for any target"""
    for c, ref, lo, hi, rp, out in restated:
        ratio = np.sqrt(out["mse"]) / np.sqrt(ref.sigma2)
        assert not np.any((ratio > 1e-6 * (1 - 1e-3)) & (ratio < 1e-6 * (1 + 1e-3))), c.id


def test_no_believed_mean_decides_by_rounding(restated):
    """no believed constraint mean lies within 1e-6 (1 + |bound|) of a bound, and no believed objective mean within 1e-6 (1 + |value|) of
    ref_point or of a front point's coordinate: feasibility by belief and dominance are decided by no rounding"""
    for c, ref, lo, hi, rp, out in restated:
        m = c.m_obj
        bm = out["believed_mu"]
        for b in (lo, hi):
            fin = np.isfinite(b)
            assert np.all(np.abs(bm[:, m:][:, fin] - b[fin]) > 1e-6 * (1 + np.abs(b[fin]))), c.id
        if c.feasibility_only:
            continue
        for i, y in enumerate(bm[:, :m]):
            coords = np.vstack([rp[None, :], out["fronts"][i]])  # ref_point and the front as it stood when this mean was believed
            assert np.all(np.abs(coords - y) > 1e-6 * (1 + np.abs(coords))), (c.id, i)


def test_the_probability_of_feasibility_is_not_constant_and_values_are_positive(restated):
    for c, ref, lo, hi, rp, out in restated:
        assert out["pof"][0].max() > out["pof"][0].min(), c.id
        if not c.feasibility_only:
            assert np.all(out["n_cells"] >= 1) and np.mean(out["val"][0] > 0) >= 0.25, (c.id, np.mean(out["val"][0] > 0))
        else:
            assert np.all(out["n_cells"] == 0), c.id
            np.testing.assert_array_equal(out["val"], out["pof"])


def test_every_front_situation_occurs(restated):
    """across the list: a believed point, feasible by belief, that changes n_cells; one, infeasible by belief, that would have joined
    the front and leaves it; a feasible one that is dominated; a feasibility-only call; the one-cell case"""
    grew, left, dominated = [], [], []
    for c, ref, lo, hi, rp, out in restated:
        if c.feasibility_only or not c.believe_front:
            continue
        n_before = c.n_pend + np.arange(Q)  # believed points in front of step j
        counts = [len(cells_of(F, rp)[0]) for F in out["fronts"]]
        assert [counts[b] for b in n_before] == out["n_cells"].tolist(), c.id
        for b in range(len(out["feasible"])):
            same = out["fronts"][b].shape == out["fronts"][b + 1].shape and np.array_equal(out["fronts"][b], out["fronts"][b + 1])
            if out["feasible"][b] and counts[b + 1] != counts[b]:
                grew.append(c.id)
            if not out["feasible"][b] and out["nondominated"][b]:
                assert same, (c.id, b)  # infeasible by belief: the front stays
                left.append(c.id)
            if out["feasible"][b] and not out["nondominated"][b]:
                assert same, (c.id, b)
                dominated.append(c.id)
            if not out["feasible"][b]:
                assert same, (c.id, b)
    assert grew and left and dominated, (grew, left, dominated)
    assert any(c.feasibility_only for c in CASES)
    one = [out for c, ref, lo, hi, rp, out in restated if c.one_cell]
    assert len(one) == 1 and one[0]["n_cells"].tolist() == [1] * Q and len(one[0]["fronts"][0]) == 0


def test_per_target_mse_equals_a_dense_refit():
    """Matern-3/2, noiseless, two objectives and one constraint: after each believed point (two pending rows, then the winners) the
    restatement's MSE_k / sigma2_k is the bracket of the model REBUILT on X + {p_1..p_B} with y = mu(p), to 1e-10; the values of step j
    are `constrained_ehvi_ref.values` on those moments over the cells of the front the rule gives; believe_front=False keeps the cells."""
    rng = np.random.default_rng(7)
    X = rng.uniform(-2, 2, size=(30, 3))
    Y = np.sin(X @ rng.normal(size=(3, 3))) * (1.0 + np.arange(3)) + 0.1 * rng.normal(size=(30, 3))
    Xs, pend = rng.uniform(-2.2, 2.2, size=(200, 3)), rng.uniform(-2, 2, size=(2, 3))
    theta = np.array([0.8, 0.5, 1.1])
    st = O.make_state(theta, X, Y, O.KERNEL_MATERN32, O.MODE_NOISELESS, 0.0, estimate_trend=False, beta=0.2)
    ref = _ref_of(st)
    lo, hi = constraint_bounds(Y, 2)
    rp = low_ref(Y, 2)
    front = Y[feasible_rows(Y, 2, lo, hi), :2]
    out = ref.run(Xs, front, rp, 3, lo, hi, pending=pend)
    pts = np.vstack([pend, out["best_x"]])
    for j in range(3):
        B = 2 + j
        Xb = np.vstack([X, pts[:B]])
        Yb = np.vstack([Y, O.predict(st, pts[:B], eval_MSE=False)])
        st_b = O.make_state(theta, Xb, Yb, O.KERNEL_MATERN32, O.MODE_NOISELESS, 0.0, estimate_trend=False, beta=0.2)
        mu_b, mse_b = O.predict(st_b, Xs)
        np.testing.assert_allclose(mu_b, out["mu"], rtol=0, atol=1e-10)
        for t in range(3):
            np.testing.assert_allclose(out["mse"][j][:, t] / st.sigma2[t], mse_b[:, t] / st_b.sigma2[t], rtol=0, atol=1e-10)
        # the front rule, restated from the believed means alone
        F = front
        for mu_p in out["believed_mu"][:B]:
            if np.all((lo <= mu_p[2:]) & (mu_p[2:] <= hi)):
                F = np.vstack([F, mu_p[None, :2]])
        lower, upper = cells_of(pareto.pareto_front(F, rp), rp)
        assert out["n_cells"][j] == len(lower)
        v, P = R.values(out["mu"], out["mse"][j], st.sigma2, 2, lower, upper, lo, hi)
        np.testing.assert_array_equal(v, out["val"][j])
        np.testing.assert_array_equal(P, out["pof"][j])
    assert np.all(out["mse"][2][out["best_idx"][:2]] == 0.0)  # a believed candidate row is determined
    fixed = ref.run(Xs, front, rp, 3, lo, hi, pending=pend, believe_front=False)
    assert len(set(fixed["n_cells"].tolist())) == 1
    np.testing.assert_array_equal(fixed["mse"][0], out["mse"][0])  # the variance is conditioned either way
    only = ref.run(Xs, np.zeros((0, 2)), rp, 3, lo, hi, pending=pend, feasibility_only=True)
    assert only["n_cells"].tolist() == [0, 0, 0]
    np.testing.assert_array_equal(only["val"], only["pof"])
    np.testing.assert_array_equal(only["pof"][0], out["pof"][0])


def test_the_grid_decomposition_is_untouched():
    """`bogp_ehvi_grid_cells` (host only) still is `pareto.hypercell_bounds`, the empty front included"""
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for m, n in ((2, 0), (2, 9), (3, 7)):
        Y = np.ascontiguousarray(rng.normal(size=(n, m)))
        r = np.full(m, -3.0)
        lower, upper = cells_of(pareto.pareto_front(Y, r), r)
        count = lib.bogp_ehvi_grid_cells(m, n, _lib._ptr(Y) if n else None, _lib._ptr(r), None, None, 0)
        assert count == len(lower)
        lo_c, up_c = np.empty((count, m)), np.empty((count, m))
        assert lib.bogp_ehvi_grid_cells(m, n, _lib._ptr(Y) if n else None, _lib._ptr(r), _lib._ptr(lo_c), _lib._ptr(up_c), count) == count
        np.testing.assert_array_equal(lo_c, lower)
        np.testing.assert_array_equal(up_c, upper)


# ----------------------------------------------------------------------------------------------------------------------
# (b) the Python routing on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def gp():
    X, Y, _, Xs, pend = problem(40, 3, _lib.KERNEL_MATERN52, False, seed=9, rows=300)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=1e-6)
    model._engine = BelieverConstrainedEhviOracleEngine()
    model.set_state(np.r_[0.6, 0.6, 0.6, 0.9], X, Y)
    return model, Y, Xs, pend


def _box(seed=3):
    return optim.Box([(-2.2, 2.2)] * 3, random_seed=seed)


def test_constrained_ehvi_believer_batch_routes(gp):
    model, Y, Xs, pend = gp
    eng = model.engine
    rp = low_ref(Y, 2)
    hi = [float(np.quantile(Y[:, 2], 0.6))]
    crit = bogp.ConstrainedEHVI(model=model, ref_point=rp, lo=[-INF], hi=hi)
    assert not crit.feasibility_only and not crit.from_cells and crit.n_feasible > 0
    nf = len(crit.pareto_Y)
    eng.calls.clear()
    xs, fs = bogp.constrained_ehvi_believer_batch(crit, _box(), 300, 3, Xs=Xs)
    assert eng.calls == [("upload", 300), ("sweep_believer_ehvi_constrained", 2, 3, nf, 0, True, False)]
    assert len(xs) == len(fs) == 3 and all(isinstance(x, list) and len(x) == 3 for x in xs) and all(isinstance(f, float) for f in fs)
    assert len({tuple(x) for x in xs}) == 3  # q distinct rows
    vals = crit(Xs)
    assert fs[0] == float(np.max(vals)) and xs[0] == Xs[int(np.argmax(vals))].tolist()  # step 0 is the plain constrained EHVI sweep
    # pending rows and the front switch reach the engine
    eng.calls.clear()
    xs2, fs2 = bogp.constrained_ehvi_believer_batch(crit, _box(), 300, 2, Xs=Xs, pending=pend, believe_front=False)
    assert eng.calls[-1] == ("sweep_believer_ehvi_constrained", 2, 2, nf, 2, False, False)
    want = eng.sweep_believer_ehvi_constrained(crit.pareto_Y, rp, 2, [-INF], hi, pending=pend, believe_front=False)
    assert [list(x) for x in want["best_x"]] == list(xs2) and tuple(want["best_val"]) == fs2
    # no feasible observation: feasibility-only, with an empty front, and it stays so
    none = bogp.ConstrainedEHVI(model=model, ref_point=rp, lo=[float(Y[:, 2].max()) + 1.0], hi=[INF])
    assert none.feasibility_only and none.n_feasible == 0 and none.pareto_Y is None and not none.from_cells
    eng.calls.clear()
    bogp.constrained_ehvi_believer_batch(none, _box(), 300, 2, Xs=Xs)
    assert eng.calls[-1] == ("sweep_believer_ehvi_constrained", 2, 2, 0, 0, True, True)
    # feasible rows, none above the reference point: the one cell, not feasibility-only
    ok = Y[:, 2] <= hi[0]
    one = bogp.ConstrainedEHVI(model=model, ref_point=Y[ok, :2].max(0) + 0.5, lo=[-INF], hi=hi)
    assert not one.feasibility_only and len(one.pareto_Y) == 0
    eng.calls.clear()
    bogp.constrained_ehvi_believer_batch(one, _box(), 300, 2, Xs=Xs)
    assert eng.calls[-1] == ("sweep_believer_ehvi_constrained", 2, 2, 0, 0, True, False)
    # host-sampled and device-drawn candidates
    eng.calls.clear()
    bogp.constrained_ehvi_believer_batch(crit, _box(5), 250, 2)
    assert eng.calls[0] == ("upload", 250)
    eng.calls.clear()
    bogp.constrained_ehvi_believer_batch(crit, _box(5), 250, 2, design="LHS", seed=4)
    assert eng.calls[0] == ("generate", 250, "LHS") and eng.calls[1][0] == "sweep_believer_ehvi_constrained"


def test_what_the_constrained_ehvi_believer_refuses(gp, monkeypatch):
    model, Y, Xs, pend = gp
    Xs = Xs[:100]
    rp = low_ref(Y, 2)
    crit = bogp.ConstrainedEHVI(model=model, ref_point=rp, lo=[-INF], hi=[0.0])
    name = "ConstrainedEHVI"
    with pytest.raises(TypeError, match=name):
        bogp.constrained_ehvi_believer_batch(bogp.EHVI(model=model, ref_point=[0, 0, 0], Y=Y), _box(), 100, 2, Xs=Xs)
    with pytest.raises(TypeError, match=name):
        bogp.constrained_ehvi_believer_batch(bogp.Constrained(model=model, fun="EI", lo=[-INF, -INF], hi=[0.0, 0.0]), _box(), 100, 2, Xs=Xs)
    cells = bogp.ConstrainedEHVI(model=model, ref_point=rp, lo=[-INF], hi=[0.0], cells=(rp[None, :], np.full((1, 2), INF)))
    assert cells.from_cells and cells.pareto_Y is None
    with pytest.raises(ValueError, match="cells= has no front"):
        bogp.constrained_ehvi_believer_batch(cells, _box(), 100, 2, Xs=Xs)
    with pytest.raises(ValueError, match="at least one"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 0, Xs=Xs)
    with pytest.raises(ValueError, match="at most 32"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 33, Xs=Xs)
    with pytest.raises(ValueError, match="at most 32"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 31, Xs=Xs, pending=pend)
    with pytest.raises(NotImplementedError, match="lift"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, lift=object())
    with pytest.raises(NotImplementedError, match="fixed variables"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, masks=np.array([True, False, False]), values=[0.0])
    with pytest.raises(NotImplementedError, match="h / g"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, h=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="h / g"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, g=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs, rank=0, world=2)
    monkeypatch.setattr(optim._forest, "is_forest_model", lambda m: True)
    with pytest.raises(NotImplementedError, match="forest"):
        bogp.constrained_ehvi_believer_batch(crit, _box(), 100, 2, Xs=Xs)
    monkeypatch.undo()
    # the existing entries keep refusing the criterion by name, exactly as before
    with pytest.raises(NotImplementedError, match=name):
        bogp.believer_batch([crit, crit], _box(), 100)
    with pytest.raises(NotImplementedError, match=name):
        bogp.ehvi_believer_batch(crit, _box(), 100, 2)
    with pytest.raises(NotImplementedError, match=name):
        bogp.constrained_believer_batch(crit, _box(), 100, q=2)
    with pytest.raises(NotImplementedError, match=name):
        optim.batch_argmax([crit, crit], _box(), 100, strategy="believer")
    with pytest.raises(NotImplementedError, match=name):
        optim.batch_argmax([crit, crit], _box(), 100, strategy="thompson")
    with pytest.raises(NotImplementedError, match=name):
        bogp.thompson_batch(model, _box(), 100, 2, criteria=[crit])
    assert not any(c[0].startswith("sweep") for c in model.engine.calls)


def test_install_validates_constrained_mobo_batches():
    with pytest.raises(ValueError, match="needs constrained_mobo=True"):
        bogp.install(object(), constrained_mobo_batches="believer")
    with pytest.raises(ValueError, match="needs constrained_mobo=True"):
        bogp.install(object(), expensive_constraints=True, constrained_mobo_batches="believer")
    with pytest.raises(ValueError, match="'topk' or 'believer'"):
        bogp.install(object(), expensive_constraints=True, constrained_mobo=True, constrained_mobo_batches="thompson")
    from bogp import integration

    assert not integration._ORIGINAL and "mobo_batches" not in integration._CONSTRAINTS


# ----------------------------------------------------------------------------------------------------------------------
# the reference's MOBO under install(expensive_constraints=True, constrained_mobo=True, constrained_mobo_batches="believer")
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def reference(monkeypatch):
    if not os.path.isdir(os.path.join(REF, "bayes_optim")):
        pytest.skip("reference tree not present")
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim

    created = []

    def engine(device=0):
        created.append(BelieverConstrainedEhviOracleEngine(device))
        return created[-1]

    monkeypatch.setattr(bogp._lib, "Engine", engine)
    yield bayes_optim, created
    bogp.uninstall()


_F = (lambda x: x[0] ** 2 + 0.5 * x[1], lambda x: x[1] ** 2 + 0.5 * x[0])  # minimised: both pull towards the origin, where g > 0


def _g_true(X):
    return 0.8 - X[:, 0] - X[:, 1] + 0.3 * np.sin(6 * X[:, 0])


def _mobo(bayes_optim, optimizer="sweep", **kw):
    from bayes_optim import MOBO
    from bayes_optim.search_space import RealSpace

    space = RealSpace([0, 1], var_name="a") + RealSpace([0, 1], var_name="b")
    model = bayes_optim.GaussianProcess(theta0=np.full(2, 1.0), thetaL=np.full(2, 1e-2), thetaU=np.full(2, 1e2), nugget=1e-6,
                                        noise_estim=False, likelihood="concentrated")  # fmt: skip
    opt = MOBO(search_space=space, obj_fun=_F, model=model, max_FEs=100, DoE_size=8, eval_type="list", n_job=1, verbose=False,
               minimize=True, n_point=3, acquisition_optimization={"optimizer": optimizer, "max_FEs": 300}, **kw)  # fmt: skip
    return opt, model


def _evaluate(X):
    A = np.asarray(X, dtype=float)
    return [tuple(f(x) for f in _F) for x in A], _g_true(A).tolist()


@pytest.mark.timeout(900)
def test_the_reference_mobo_asks_for_three_points(reference):
    """The reference's unmodified MOBO(n_point=3) with g_vals: ONE `sweep_believer_ehvi_constrained` call per ask, three distinct rows;
    tell; ask again.  A fixed variable and an inner optimiser outside the sweep family keep today's NotImplementedError."""
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True, constrained_mobo=True, constrained_mobo_batches="believer")
    np.random.seed(4)
    opt, model = _mobo(bayes_optim)
    X = opt.ask(8)  # the DoE
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    assert model.y.shape == (8, 3)
    eng = model.engine
    for it in range(2):
        eng.calls.clear()
        X = opt.ask()
        assert len(X) == 3 and len({tuple(x) for x in X}) == 3
        calls = [c for c in eng.calls if c[0].startswith("sweep")]
        assert len(calls) == 1 and calls[0][0] == "sweep_believer_ehvi_constrained" and calls[0][1:3] == (2, 3) and calls[0][4:6] == (0, True), calls
        crit = optim.unwrap_criterion(opt._create_acquisition())[0]
        assert isinstance(crit, bogp.ConstrainedEHVI) and calls[0][6] == (crit.n_feasible == 0)
        assert calls[0][3] == (0 if crit.pareto_Y is None else len(crit.pareto_Y))
        f, g = _evaluate(X)
        opt.tell(X, f, g_vals=g)
    assert model.y.shape == (14, 3) and len(opt._bogp_constraints) == 14
    assert len(opt.ask(1)) == 1 and eng.calls[-1][0] == "sweep_ehvi_constrained"  # one point: the route it took before
    with pytest.raises(NotImplementedError, match="ConstrainedEHVI"):
        opt.ask(3, fixed={"a": 0.5})
    np.random.seed(5)
    other, _ = _mobo(bayes_optim, optimizer="OnePlusOne_Cholesky_CMA")
    Xd = other.ask(8)
    fd, gd = _evaluate(Xd)
    other.tell(Xd, fd, g_vals=gd)
    with pytest.raises(NotImplementedError, match="ConstrainedEHVI"):
        other.ask()


@pytest.mark.timeout(900)
def test_without_the_switch_the_same_mobo_raises_as_before(reference):
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True, constrained_mobo=True, batch_strategy="believer")
    np.random.seed(4)
    opt, model = _mobo(bayes_optim)
    X = opt.ask(8)
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    with pytest.raises(NotImplementedError, match="ConstrainedEHVI"):
        opt.ask()
    assert not any(c[0] == "sweep_believer_ehvi_constrained" for c in model.engine.calls)
    bogp.uninstall()
    from bogp import integration

    assert not integration._CONSTRAINTS and not integration._ORIGINAL
