"""Thompson batches under modelled constraints, on the host: the moments of the joint paths (`thompson.paths_multi_numpy` against
the multi-target predictor, the independence of the targets), the selection rule on hand-made path arrays (`select_numpy`,
`merge_ranks`), the Python routing of `constrained_thompson_batch` on a stand-in engine served by the restatement, the reference's
own `ParallelBO` under `install(expensive_constraints=True, constraint_thompson=True)`, and -- on the restatement alone -- the
conditions that keep tests/test_gpu_thompson_constrained.py from hiding a failure, for every case of
tests/thompson_constrained_cases.py."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT

import bogp
import thompson_constrained_cases as TC
from bogp import _lib, optim, thompson
from support.thompson_constrained_engine import ThompsonConstrainedOracleEngine

REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
INF = float("inf")


# ----------------------------------------------------------------------------------------------------------------------
# moments
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("kernel", [_lib.KERNEL_SE, _lib.KERNEL_MATERN52])
def test_joint_paths_have_the_predictors_moments_and_independent_targets(kernel, m):
    """400 draws (16 // m members a call): per target the mean and variance of the paths match mu_t / MSE_t within 6 standard errors,
    and the sample correlation between two targets' paths at a point is within 6 standard errors of 0."""
    X, Y, theta, Xs = TC.problem(12, 3, 30, kernel, m)
    st = TC.state(X, Y, theta, kernel)
    mu, mse = thompson.moments_multi_numpy(st, Xs)  # (M, m)
    q = 16 // m
    n_calls = -(-400 // q)
    P = np.concatenate([thompson.paths_multi_numpy(st, thompson.draw_multi(st, q, 512, seed=1000 + s), Xs)[0] for s in range(n_calls)])[:400]
    n = len(P)
    assert n == 400
    far = mse.min(axis=1) > 1e-3 * st.sigma2.min()  # rows that are no training point's neighbour: a variance to speak of
    assert far.sum() >= 3
    mean, var = P.mean(axis=0).T, P.var(axis=0, ddof=1).T  # (M, m)
    assert np.all(np.abs(mean - mu)[far] <= 6 * np.sqrt(mse[far] / n))
    assert np.all(np.abs(var - mse)[far] <= 6 * mse[far] * np.sqrt(2.0 / (n - 1)))
    Z = (P - P.mean(axis=0)) / P.std(axis=0, ddof=1)
    for a in range(m):
        for b in range(a + 1, m):
            corr = (Z[:, a] * Z[:, b]).sum(axis=0) / (n - 1)
            assert np.all(np.abs(corr[far]) <= 6 / np.sqrt(n)), (a, b)


def test_joint_paths_interpolate_and_the_draw_keeps_draws_order():
    X, Y, theta, _ = TC.problem(5, 3, 30, _lib.KERNEL_MATERN52, 3)
    st = TC.state(X, Y, theta, _lib.KERNEL_MATERN52)
    dr = thompson.draw_multi(st, 5, 64, seed=7)
    assert dr.weights.shape == (64, 15) and dr.eps.shape == (30, 15)
    one = thompson.draw(thompson.dense_state(X, Y[:, 0], theta, _lib.KERNEL_MATERN52), 15, 64, seed=7)  # the same stream, 15 columns
    for a, b in zip(dr, one):
        np.testing.assert_array_equal(a, b)
    paths, gt = thompson.paths_multi_numpy(st, dr, X)
    assert paths.shape == (5, 3, 30) and gt.shape == (30, 15)
    assert np.max(np.abs(paths - Y.T[None])) <= 1e-9  # noiseless: every member's every path passes through the data
    assert abs(thompson.objective_path_at(st, dr, gt, 2, X[4]) - Y[4, 0]) <= 1e-9
    with pytest.raises(ValueError, match="at most 16 columns"):
        thompson.draw_multi(st, 6, 64)
    with pytest.raises(ValueError, match="at least one"):
        thompson.draw_multi(st, 0, 64)
    with pytest.raises(ValueError, match="multi-target"):
        thompson.draw_multi(thompson.dense_state(X, Y[:, 0], theta, _lib.KERNEL_SE), 2, 64)


# ----------------------------------------------------------------------------------------------------------------------
# selection on hand-made paths
# ----------------------------------------------------------------------------------------------------------------------
def _paths(obj, *cons):
    return np.array([[obj] + list(cons)], dtype=float)  # one member: (1, m, M)


def test_selection_on_mixed_rows():
    #            row:  0     1     2     3     4     5
    p = _paths([3.0, 1.0, 2.0, 0.5, 4.0, 0.0], [-1.0, 0.5, -0.1, 2.0, 0.0, -3.0], [0.0, 0.0, 5.0, 0.0, 0.0, 0.0])
    lo, hi, s2 = [-INF, -1.0], [0.0, 1.0], [1.0, 4.0, 0.25]
    sel = thompson.select_numpy(p, lo, hi, s2, minimize=True, k=4)
    np.testing.assert_array_equal(sel["feas"][0], [True, False, False, False, True, True])  # c == hi is feasible (row 4)
    np.testing.assert_array_equal(sel["A"][0], [-3.0, -INF, -INF, -INF, -4.0, -0.0])
    # viol: row 1: 0.5 / 2; row 2: (5 - 1) / 0.5 = 8 beats 0; row 3: 2 / 2 -- the largest scaled excess, not a sum
    np.testing.assert_array_equal(sel["B"][0], [0.0, -0.25, -8.0, -1.0, 0.0, 0.0])
    assert np.all(np.signbit(sel["B"][0]) == [False, True, True, True, False, False])  # 0.0 - 0.0 is +0.0
    np.testing.assert_array_equal(sel["best_idx"][0, 0], [5, 0, 4, 1])  # A: best first, then the -inf rows by index
    np.testing.assert_array_equal(sel["best_val"][0, 0], [-0.0, -3.0, -4.0, -INF])
    np.testing.assert_array_equal(sel["best_idx"][0, 1], [0, 4, 5, 1])  # B: the feasible rows tie at 0.0, lower index first
    assert thompson.merge_ranks(sel["best_val"][0], sel["best_idx"][0]) == [(5, 0, 0), (0, 0, 1), (4, 0, 2), (1, 1, 3)]
    assert thompson.merge_ranks(sel["best_val"][0], sel["best_idx"][0], 2) == [(5, 0, 0), (0, 0, 1)]
    up = thompson.select_numpy(p, lo, hi, s2, minimize=False, k=1)
    assert up["best_idx"][0, 0, 0] == 4 and up["best_val"][0, 0, 0] == 4.0


def test_selection_without_a_feasible_row_takes_the_least_violating():
    p = _paths([3.0, 1.0, 2.0], [1.0, 0.2, 0.6])
    sel = thompson.select_numpy(p, [-INF], [0.0], [1.0, 0.01], minimize=True, k=3)
    assert not sel["feas"].any() and np.all(sel["A"] == -INF)
    np.testing.assert_array_equal(sel["best_idx"][0, 1], [1, 2, 0])
    np.testing.assert_allclose(sel["best_val"][0, 1], [-2.0, -6.0, -10.0], rtol=1e-15)
    assert [r[:2] for r in thompson.merge_ranks(sel["best_val"][0], sel["best_idx"][0])] == [(1, 1), (2, 1), (0, 1)]


def test_selection_with_every_row_feasible_and_with_equal_bounds():
    p = _paths([3.0, 1.0, 2.0], [1.0, 0.2, 0.6])
    sel = thompson.select_numpy(p, [-INF], [INF], [1.0, 1.0], minimize=False, k=2)
    assert sel["feas"].all() and np.all(sel["B"].view(np.int64) == 0)  # B == +0.0 in every row
    np.testing.assert_array_equal(sel["A"], p[:, 0])
    np.testing.assert_array_equal(sel["best_idx"][0], [[0, 2], [0, 1]])
    # lo == hi: only the exact value is feasible
    eq = thompson.select_numpy(p, [0.2], [0.2], [1.0, 1.0], minimize=True, k=3)
    np.testing.assert_array_equal(eq["feas"][0], [False, True, False])
    np.testing.assert_allclose(eq["B"][0], [-0.8, 0.0, -0.4], rtol=1e-15)
    # an equality band |h| <= 0.5: both sides of the band are measured
    band = thompson.select_numpy(_paths([0.0, 0.0, 0.0, 0.0], [-2.0, -0.5, 0.25, 1.5]), [-0.5], [0.5], [1.0, 1.0], k=4)
    np.testing.assert_array_equal(band["feas"][0], [False, True, True, False])
    np.testing.assert_array_equal(band["B"][0], [-1.5, 0.0, 0.0, -1.0])


def test_selection_never_lists_a_nan_row_and_pads_short_rankings():
    p = _paths([3.0, np.nan, 2.0, 1.0], [-1.0, -1.0, np.nan, 1.0])
    sel = thompson.select_numpy(p, [-INF], [0.0], [1.0, 1.0], minimize=True, k=6)  # M = 4 < k
    np.testing.assert_array_equal(sel["A"][0], [-3.0, -INF, -INF, -INF])
    np.testing.assert_array_equal(sel["B"][0], [0.0, -INF, -INF, -1.0])
    np.testing.assert_array_equal(sel["feas"][0], [True, False, False, False])
    np.testing.assert_array_equal(sel["best_idx"][0, 0], [0, 1, 2, 3, -1, -1])
    np.testing.assert_array_equal(sel["best_idx"][0, 1], [0, 3, 1, 2, -1, -1])
    assert np.all(sel["best_val"][0, :, 4:] == -INF)
    assert thompson.merge_ranks(sel["best_val"][0], sel["best_idx"][0]) == [(0, 0, 0), (3, 1, 1)]  # rows 1 and 2 never
    allnan = thompson.select_numpy(np.full((1, 2, 3), np.nan), [-INF], [0.0], [1.0, 1.0], k=2)
    assert thompson.merge_ranks(allnan["best_val"][0], allnan["best_idx"][0]) == []
    with pytest.raises(ValueError, match="one bound per constraint"):
        thompson.select_numpy(p, [-INF, 0.0], [0.0, 1.0], [1.0, 1.0])


# ----------------------------------------------------------------------------------------------------------------------
# the Python routing on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
def _model(m=3, nugget=0, N=40):
    X, Y, _, _ = TC.problem(10, 3, N, _lib.KERNEL_MATERN52, m, seed=9)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=nugget)
    model._engine = ThompsonConstrainedOracleEngine()
    model.set_state(np.r_[0.6, 0.6, 0.6] if not nugget else np.r_[0.6, 0.6, 0.6, 0.9], X, Y[:, 0] if m == 1 else Y)
    return model


@pytest.fixture()
def gp():
    return _model()


def _box(seed=3):
    return optim.Box([(-2.2, 2.2)] * 3, random_seed=seed)


def _cands(M=300):
    return np.random.default_rng(21).uniform(-2.2, 2.2, size=(M, 3))


def _crit(model, frac=0.6, **kw):
    Y = model.y
    return bogp.Constrained(model=model, fun="EI", lo=[-INF] * (Y.shape[1] - 1), hi=np.quantile(Y[:, 1:], frac, axis=0), **kw)


def test_constrained_thompson_batch_routes_and_returns_distinct_rows(gp):
    eng, Xs = gp.engine, _cands()
    crit = _crit(gp)
    eng.calls.clear()
    xs, fs = bogp.constrained_thompson_batch(crit, _box(), 300, q=3, n_features=64, seed=4, Xs=Xs)
    assert eng.calls == [("upload", 300), ("sweep_thompson_constrained", 3, 8, True)]
    assert isinstance(xs, tuple) and isinstance(fs, tuple) and len(xs) == len(fs) == 3
    assert all(isinstance(x, list) and len(x) == 3 for x in xs) and all(isinstance(f, float) for f in fs)  # batch_argmax's format
    assert len({tuple(x) for x in xs}) == 3
    st = thompson.state_of_multi(gp)
    assert st.y.shape == (40, 3) and st.sigma2.shape == (3,) and not st.estimate_trend
    dr = thompson.draw_multi(gp, 3, 64, seed=4)
    paths, _ = thompson.paths_multi_numpy(gp, dr, Xs)
    sel = thompson.select_numpy(paths, crit.lo, crit.hi, st.sigma2, True, 1)
    for j in range(3):  # each member's best drawn objective among the rows whose drawn constraints hold, and the path's value there
        assert sel["feas"][j].any()
        best = int(np.argmin(np.where(sel["feas"][j], paths[j, 0], INF)))
        assert xs[j] == Xs[best].tolist() and fs[j] == float(paths[j, 0, best])
    # maximising, reproducible per seed, another seed another batch
    mx = _crit(gp, minimize=False)
    xs2, fs2 = bogp.constrained_thompson_batch(mx, _box(), 300, q=3, n_features=64, seed=4, Xs=Xs)
    sel2 = thompson.select_numpy(paths, mx.lo, mx.hi, st.sigma2, False, 1)
    assert fs2[0] == float(np.max(np.where(sel2["feas"][0], paths[0, 0], -INF)))
    for j in range(3):  # (a later member may find its best row taken: it proposes a feasible row of its own and reports its value)
        row = int(np.flatnonzero(np.all(Xs == np.asarray(xs2[j]), axis=1))[0])
        assert sel2["feas"][j, row] and fs2[j] == float(paths[j, 0, row])
    assert bogp.constrained_thompson_batch(crit, _box(), 300, q=3, n_features=64, seed=4, Xs=Xs) == (xs, fs)
    assert bogp.constrained_thompson_batch(crit, _box(), 300, q=3, n_features=64, seed=5, Xs=Xs)[0] != xs
    # history: a proposal np.isclose to an evaluated point gives way to the member's next listed row
    xs3, _ = bogp.constrained_thompson_batch(crit, _box(), 300, q=3, n_features=64, seed=4, Xs=Xs, history=np.array([xs[0]]))
    second = int(np.argsort(np.where(sel["feas"][0], paths[0, 0], INF), kind="stable")[1])
    assert xs3[0] == Xs[second].tolist() and xs3[1:] == xs[1:]
    # a feasibility-only criterion and one with another fun are served alike: fun is not used
    none = bogp.Constrained(model=gp, fun=None, lo=crit.lo, hi=crit.hi)
    assert bogp.constrained_thompson_batch(none, _box(), 300, q=3, n_features=64, seed=4, Xs=Xs) == (xs, fs)
    # host-sampled and device-drawn candidates
    eng.calls.clear()
    bogp.constrained_thompson_batch(crit, _box(5), 250, q=2, n_features=64, seed=1)
    assert eng.calls[0] == ("upload", 250)
    eng.calls.clear()
    bogp.constrained_thompson_batch(crit, _box(5), 250, q=2, n_features=64, design="LHS", seed=4)
    assert eng.calls[0] == ("generate", 250, "LHS") and eng.calls[1][0] == "sweep_thompson_constrained"


def test_more_members_than_a_call_holds_run_in_several_calls(gp):
    """m = 3: five members a call.  q = 12 runs calls of 5, 5 and 2 with derived seeds; a later call steps over the rows taken."""
    eng, Xs = gp.engine, _cands()
    crit = _crit(gp)
    eng.calls.clear()
    xs, fs = bogp.constrained_thompson_batch(crit, _box(), 300, q=12, n_features=64, seed=2, Xs=Xs)
    sweeps = [c for c in eng.calls if c[0] == "sweep_thompson_constrained"]
    assert [c[1] for c in sweeps] == [5, 5, 2] and [c[2] for c in sweeps] == [8, 13, 18]
    assert len(xs) == 12 and len({tuple(x) for x in xs}) == 12
    seeds = thompson.batch_seeds(2, 3)
    st = thompson.state_of_multi(gp)
    paths, _ = thompson.paths_multi_numpy(gp, thompson.draw_multi(gp, 5, 64, seed=seeds[0]), Xs)
    sel = thompson.select_numpy(paths, crit.lo, crit.hi, st.sigma2, True, 1)
    assert xs[0] == Xs[int(sel["best_idx"][0, 0, 0])].tolist()


def test_a_member_without_a_feasible_row_proposes_its_least_violating_row(gp):
    eng, Xs = gp.engine, _cands()
    far = bogp.Constrained(model=gp, fun="EI", lo=[40.0, 40.0], hi=[INF, INF])
    assert far.feasibility_only
    xs, fs = bogp.constrained_thompson_batch(far, _box(), 300, q=2, n_features=64, seed=4, Xs=Xs)
    st = thompson.state_of_multi(gp)
    paths, _ = thompson.paths_multi_numpy(gp, thompson.draw_multi(gp, 2, 64, seed=4), Xs)
    sel = thompson.select_numpy(paths, far.lo, far.hi, st.sigma2, True, 1)
    assert not sel["feas"].any()
    for j in range(2):
        row = int(np.argmax(sel["B"][j]))
        assert xs[j] == Xs[row].tolist() and abs(fs[j] - paths[j, 0, row]) <= 1e-9 * (1 + abs(paths[j, 0, row]))


def test_what_the_constrained_thompson_batch_refuses(gp, monkeypatch):
    Xs = _cands(100)
    crit = _crit(gp)
    single = _model(m=1)
    with pytest.raises(TypeError, match="bogp.Constrained"):
        bogp.constrained_thompson_batch(bogp.EI(model=single), _box(), 100, q=2, Xs=Xs)
    with pytest.raises(TypeError, match="bogp.Constrained"):
        bogp.constrained_thompson_batch(gp, _box(), 100, q=2, Xs=Xs)
    cehvi = type("C", (), dict(is_constrained_ehvi=True, is_ehvi=True, model=gp))()
    with pytest.raises(NotImplementedError, match="ConstrainedEHVI"):
        bogp.constrained_thompson_batch(cehvi, _box(), 100, q=2, Xs=Xs)
    with pytest.raises(NotImplementedError, match="lift"):
        bogp.constrained_thompson_batch(crit, _box(), 100, q=2, Xs=Xs, lift=object())
    with pytest.raises(NotImplementedError, match="fixed variables"):
        bogp.constrained_thompson_batch(crit, _box(), 100, q=2, Xs=Xs, masks=np.array([True, False, False]), values=[0.0])
    with pytest.raises(NotImplementedError, match="h / g"):
        bogp.constrained_thompson_batch(crit, _box(), 100, q=2, Xs=Xs, h=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="h / g"):
        bogp.constrained_thompson_batch(crit, _box(), 100, q=2, Xs=Xs, g=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.constrained_thompson_batch(crit, _box(), 100, q=2, Xs=Xs, rank=0, world=2)
    with pytest.raises(ValueError, match="at least one point"):
        bogp.constrained_thompson_batch(crit, _box(), 100, q=0, Xs=Xs)
    noisy = _model(nugget=1e-6)
    with pytest.raises(NotImplementedError, match="noisy mode"):
        bogp.constrained_thompson_batch(_crit(noisy), _box(), 100, q=2, Xs=Xs)
    for kid, name in ((_lib.KERNEL_CUBIC, "cubic"), (_lib.KERNEL_GENEXP, "generalized-exponential")):
        mdl = _model()
        c = _crit(mdl)
        mdl.kernel_id = kid  # (the refusal reads the committed kernel)
        with pytest.raises(NotImplementedError, match=name):
            bogp.constrained_thompson_batch(c, _box(), 100, q=2, Xs=Xs)
    monkeypatch.setattr(optim._forest, "is_forest_model", lambda m: True)
    with pytest.raises(NotImplementedError, match="forest"):
        bogp.constrained_thompson_batch(crit, _box(), 100, q=2, Xs=Xs)
    monkeypatch.undo()
    # everything existing keeps refusing exactly as it did
    with pytest.raises(NotImplementedError, match="have no Thompson batches: strategy='topk' serves them"):
        optim.batch_argmax([crit, crit], _box(), 100, strategy="thompson")
    with pytest.raises(NotImplementedError, match="have no Thompson batches"):
        bogp.thompson_batch(gp, _box(), 100, 2, Xs=Xs, criteria=[crit, crit])
    with pytest.raises(NotImplementedError, match="several targets"):
        thompson.state_of(gp)
    with pytest.raises(NotImplementedError, match="several targets"):
        gp.sampling_posterior(Xs[:3])
    with pytest.raises(ValueError, match="m >= 2"):
        thompson.state_of_multi(single)


def test_install_validates_constraint_thompson():
    from bogp import integration

    with pytest.raises(ValueError, match="needs expensive_constraints=True"):
        bogp.install(object(), constraint_thompson=True)
    with pytest.raises(ValueError, match="two batch strategies"):
        bogp.install(object(), expensive_constraints=True, constraint_thompson=True, constraint_batches="believer")
    with pytest.raises(ValueError, match="'topk' or 'believer'"):  # (asserted by the believer's test too: unchanged)
        bogp.install(object(), expensive_constraints=True, constraint_batches="thompson")
    assert not integration._ORIGINAL and "batches" not in integration._CONSTRAINTS


@pytest.mark.timeout(900)
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
def test_parallel_bo_reaches_the_constrained_thompson_batch(monkeypatch):
    """The reference's unmodified ParallelBO(n_point=3) with g_vals and a noiseless device model (seeded: a fit whose likelihood is
    invalid would raise the nugget and leave the noiseless mode, which Thompson sampling refuses) on the stand-in engine: ONE
    `sweep_thompson_constrained` call per ask, three distinct points; a fixed variable keeps the route it had."""
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim
    from bayes_optim.search_space import RealSpace

    monkeypatch.setattr(bogp._lib, "Engine", lambda device=0: ThompsonConstrainedOracleEngine(device))
    undo = bogp.install(bayes_optim, expensive_constraints=True, constraint_thompson=True)
    try:
        np.random.seed(8)
        space = RealSpace([-5, 5], var_name="a") + RealSpace([-5, 5], var_name="b")
        model = bogp.GaussianProcess(corr="matern", thetaL=1e-2 * np.ones(2), thetaU=10 * np.ones(2), nugget=0, random_start=2)
        opt = bayes_optim.ParallelBO(search_space=space, obj_fun=lambda x: x[0] ** 2 + x[1] ** 2, model=model, max_FEs=100, DoE_size=6,
                                     eval_type="list", n_job=1, verbose=False, minimize=True, acquisition_fun="MGFI", n_point=3,
                                     acquisition_optimization={"optimizer": "sweep", "max_FEs": 300}, random_seed=11)  # fmt: skip

        def evaluate(X):
            A = np.asarray(X, dtype=float)
            return (A**2).sum(1).tolist(), (9.0 - (A[:, 0] - 1.0) ** 2 - (A[:, 1] + 1.0) ** 2).tolist()  # g <= 0: outside a disc

        X = opt.ask(6)
        f, g = evaluate(X)
        opt.tell(X, f, g_vals=g)
        for _ in range(2):
            model.engine.calls.clear()
            X = opt.ask()
            assert len(X) == 3 and len({tuple(x) for x in X}) == 3
            calls = [c for c in model.engine.calls if c[0].startswith("sweep")]
            assert len(calls) == 1 and calls[0][:2] == ("sweep_thompson_constrained", 3) and calls[0][3] is True, calls
            f, g = evaluate(X)
            opt.tell(X, f, g_vals=g)
        assert model.y.shape == (12, 2)
        model.engine.calls.clear()
        assert len(opt.ask(3, fixed={"a": 0.5})) == 3  # a fixed variable: today's route
        assert not any(c[0] == "sweep_thompson_constrained" for c in model.engine.calls)
    finally:
        undo()
        bogp.uninstall()


# ----------------------------------------------------------------------------------------------------------------------
# the conditions on the device cases, on the restatement alone
# ----------------------------------------------------------------------------------------------------------------------
def test_the_case_lists_are_the_ones_specified():
    assert len(TC.SHAPES) == 28
    cols = list(zip(*TC.SHAPES))
    assert set(cols[0]) == set(TC.MS) and set(cols[1]) == set(TC.DS) and set(cols[2]) == set(TC.NS) and set(cols[3]) == set(TC.LS)
    assert set(zip(cols[4], cols[5])) == set(TC.MQ) and set(cols[6]) == set(TC.KERNELS) and set(cols[7]) == {True, False}
    assert {q * m for m, q in TC.MQ} >= {16, 15, 2} and all(q * m <= 16 for m, q in TC.MQ)
    assert [TC.CASES[n][:3] for n in TC.MIXED] == [(2, 67, 3), (3, 5, 1), (4, 300, 20), (5, 300, 3), (8, 64, 4)]
    assert {TC.CASES[n][5] for n in TC.CASES} == {"median", "none", "open"} and {TC.CASES[n][4] for n in TC.CASES} == {True, False}


@pytest.mark.parametrize("cfg", range(len(TC.SHAPES)))
def test_every_shape_is_well_conditioned_and_reads_the_conditioning_term(cfg):
    M, d, N, L, m, q, kernel, _ = TC.SHAPES[cfg]
    X, Y, theta, Xs = TC.problem(M, d, N, kernel, m)
    st = TC.state(X, Y, theta, kernel)
    ref = TC.restate(st, thompson.draw_multi(st, q, L, seed=cfg), Xs)
    assert ref.cond <= 1e8 and ref.phase <= 1e6 and ref.share >= 1e-2, (ref.cond, ref.phase, ref.share)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_every_selection_case_is_decided_on_the_restatement(name):
    c = TC.case(name)
    ref = TC.restate(c.st, c.dr, c.Xs)
    assert ref.cond <= 1e8 and ref.phase <= 1e6
    sel = thompson.select_numpy(ref.paths, c.lo, c.hi, c.st.sigma2, c.minimize, 17)
    share = sel["feas"].mean(axis=1)
    kind = TC.CASES[name][5]
    if kind == "median":
        assert share.min() >= 0.005 and share.max() <= 0.95, share
    elif kind == "none":
        assert share.max() == 0.0 and np.all(sel["B"] < -1.0)  # far from every bound
    else:
        assert share.min() == 1.0
    assert TC.conditions(c, ref) == []
