"""Kriging-believer batches under modelled constraints, the parts that need no GPU: (a) the conditions every shared case
(tests/believer_constrained_cases.py) must meet, asserted on the dense restatement (tests/support/believer_constrained_ref.py) alone; the
restatement against a dense refit; (b) the routing and the refusals of `optim.constrained_believer_batch`, the untouched refusals of
`believer_batch` / `batch_argmax`, the validation of `install(constraint_batches=...)` and the reference's ParallelBO on the
oracle-backed stand-in."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle import gp_oracle as O

import bogp
from bogp import _lib, optim
from believer_constrained_cases import ACQ_FEASIBILITY, ACQ_MIXED, CASES, IDS, problem, quantile_bounds
from support.believer_constrained_engine import BelieverConstrainedOracleEngine
from support.believer_constrained_ref import BelieverConstrainedRef

REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
INF = float("inf")


def _ref_of(st):
    return BelieverConstrainedRef(st.X, st.theta, st.kernel, dict(C=st.C, gamma=st.gamma, beta=float(st.beta[0, 0]), sigma2=st.sigma2))


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
        X, Y, args, Xs, pend, lo, hi, plugin = c.build()
        ref = _ref_of(_state(X, Y, args))
        runs.append((c, ref, lo, hi, ref.run(Xs, c.acq, plugin, c.minimize, lo, hi, pending=pend)))
    return runs


def test_the_case_list_is_the_one_specified():
    mixed = [c for c in CASES if c.acq is ACQ_MIXED and c.m < 8]
    assert len(mixed) == 32 and {(c.N, c.m, c.noisy, c.n_pend, c.minimize) for c in mixed} == {
        (N, m, noisy, p, mn) for N in (70, 530) for m in (2, 3) for noisy in (False, True) for p in (0, 2) for mn in (True, False)}  # fmt: skip
    assert all((c.kernel == _lib.KERNEL_SE) == c.noisy for c in CASES)
    assert [(c.N, c.rows) for c in CASES if c.m == 8] == [(70, 599)]
    pof = {(c.N, c.m, c.noisy) for c in CASES if c.acq is ACQ_FEASIBILITY}
    assert pof == {(70, 2, False), (70, 2, True), (70, 3, False), (70, 3, True), (530, 3, False)}
    assert len(set(IDS)) == len(IDS)
    assert [a for a, _ in ACQ_MIXED] == [_lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_MGFI, _lib.ACQ_EI] and ACQ_MIXED[2][1] == 2.0


def test_no_step_of_a_case_is_a_tie(restated):
    """1. every step's winner / runner-up gap exceeds 1e-9 relative"""
    for c, ref, lo, hi, out in restated:
        gap = (out["best_val"] - out["second"]) / np.abs(out["best_val"])
        assert np.all(gap > 1e-9), (c.id, gap)
        assert len(set(out["best_idx"].tolist())) == len(c.acq)
        for j in range(len(c.acq)):  # a NaN (PI at sd = 0 on the row whose mean is the believed plugin) stands on a winner's row only
            assert set(np.flatnonzero(np.isnan(out["acq"][j])).tolist()) <= set(out["best_idx"][:j].tolist()), (c.id, j)


def test_no_row_of_a_case_stands_at_the_variance_guard(restated):
    """2. no row has sd / sqrt(sigma2) within 1e-3 of the 1e-6 guard, at any step and for any target"""
    for c, ref, lo, hi, out in restated:
        ratio = np.sqrt(out["mse"]) / np.sqrt(ref.sigma2)
        assert not np.any((ratio > 1e-6 * (1 - 1e-3)) & (ratio < 1e-6 * (1 + 1e-3))), c.id


def test_no_believed_mean_of_a_case_stands_at_a_bound(restated):
    """3. no believed mean lies within 1e-6 (1 + |bound|) of a bound: feasibility by belief is decided by no rounding"""
    for c, ref, lo, hi, out in restated:
        bm = out["believed_mu"][:, 1:]
        for b in (lo, hi):
            fin = np.isfinite(b)
            assert np.all(np.abs(bm[:, fin] - b[fin]) > 1e-6 * (1 + np.abs(b[fin]))), c.id


def test_both_plugin_situations_occur(restated):
    """4. across the list: a feasible believed point lowers the plugin of a later step, and an infeasible believed point that would
    have lowered it does not"""
    lowered = [c.id for c, ref, lo, hi, out in restated if c.acq is ACQ_MIXED and np.any(np.diff(out["plugins"]) < 0)]
    blocked = [c.id for c, ref, lo, hi, out in restated if c.acq is ACQ_MIXED and out["blocked"].any()]
    assert lowered and blocked, (lowered, blocked)
    for c, ref, lo, hi, out in restated:
        assert np.all(np.diff(out["plugins"]) <= 0)
        n_before = c.n_pend + np.arange(len(c.acq))  # believed points in front of step j
        plugin = c.build()[7]
        for j in range(len(c.acq)):
            bm = out["believed_mu"][: n_before[j]]
            ok = np.all((bm[:, 1:] >= lo) & (bm[:, 1:] <= hi), axis=1)
            y_hat = bm[ok, 0] if c.minimize else -bm[ok, 0]
            assert out["plugins"][j] == min([plugin] + y_hat.tolist()), (c.id, j)


def test_per_target_mse_equals_a_dense_refit():
    """Matern-3/2, noiseless, three targets: after each believed point (two pending rows, then the winners) the restatement's
    MSE_k / sigma2_k is the bracket of the model REBUILT on X + {p_1..p_B} with y = mu(p), to 1e-10; the values of step j are
    `constrained_ref.constrained` on those moments with the plugin the rule gives; believe_plugin=False keeps the plugin."""
    from support import constrained_ref as R

    rng = np.random.default_rng(7)
    X = rng.uniform(-2, 2, size=(30, 3))
    Y = np.sin(X @ rng.normal(size=(3, 3))) * (1.0 + np.arange(3)) + 0.1 * rng.normal(size=(30, 3))
    Xs, pend = rng.uniform(-2.2, 2.2, size=(200, 3)), rng.uniform(-2, 2, size=(2, 3))
    theta = np.array([0.8, 0.5, 1.1])
    st = O.make_state(theta, X, Y, O.KERNEL_MATERN32, O.MODE_NOISELESS, 0.0, estimate_trend=False, beta=0.2)
    ref = _ref_of(st)
    lo, hi = quantile_bounds(Y)
    acq = ACQ_MIXED[:3]
    out = ref.run(Xs, acq, float(Y[:, 0].max()), True, lo, hi, pending=pend)
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
        vals, pof = R.constrained(out["mu"], out["mse"][j], st.sigma2, lo, hi, [acq[j]], out["plugins"][j], True)
        np.testing.assert_array_equal(vals[0], out["acq"][j])
        np.testing.assert_array_equal(pof, out["pof"][j])
    assert np.all(out["mse"][2][out["best_idx"][:2]] == 0.0)  # a believed candidate row is determined
    fixed = ref.run(Xs, acq, float(Y[:, 0].max()), True, lo, hi, pending=pend, believe_plugin=False)
    assert np.all(fixed["plugins"] == float(Y[:, 0].max())) and np.any(out["plugins"] < fixed["plugins"])
    np.testing.assert_array_equal(fixed["mse"][0], out["mse"][0])  # the variance is conditioned either way


# ----------------------------------------------------------------------------------------------------------------------
# (b) the Python routing on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def gp():
    X, Y, _, Xs, pend = problem(40, 2, _lib.KERNEL_MATERN52, False, seed=9, rows=300)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=1e-6)
    model._engine = BelieverConstrainedOracleEngine()
    model.set_state(np.r_[0.6, 0.6, 0.6, 0.9], X, Y)
    return model, Y, Xs, pend


def _box(seed=3):
    return optim.Box([(-2.2, 2.2)] * 3, random_seed=seed)


def test_constrained_believer_batch_routes(gp):
    model, Y, Xs, pend = gp
    eng = model.engine
    lo, hi = [-INF], [float(np.quantile(Y[:, 1], 0.6))]
    crit = bogp.Constrained(model=model, fun="EI", lo=lo, hi=hi)
    assert not crit.feasibility_only
    eng.calls.clear()
    xs, fs = bogp.constrained_believer_batch(crit, _box(), 300, q=3, Xs=Xs)
    assert eng.calls == [("upload", 300), ("sweep_believer_constrained", (_lib.ACQ_EI,) * 3, 0, True)]
    assert len(xs) == len(fs) == 3 and all(isinstance(x, list) and len(x) == 3 for x in xs) and all(isinstance(f, float) for f in fs)
    assert len({tuple(x) for x in xs}) == 3  # q distinct rows
    vals = crit(Xs)
    assert fs[0] == float(np.max(vals)) and xs[0] == Xs[int(np.argmax(vals))].tolist()  # step 0 is the plain constrained sweep
    # a sequence of criteria in order, pending rows and the plugin switch reach the engine
    mg = bogp.Constrained(model=model, fun="MGFI", lo=lo, hi=hi, t=2)
    pi = bogp.Constrained(model=model, fun="PI", lo=lo, hi=hi)
    eng.calls.clear()
    xs2, fs2 = bogp.constrained_believer_batch([crit, pi, mg], _box(), 300, Xs=Xs, pending=pend, believe_plugin=False)
    assert eng.calls[-1] == ("sweep_believer_constrained", (_lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_MGFI), 2, False)
    want = eng.sweep_believer_constrained([(c.acq_id, c.acq_par()) for c in (crit, pi, mg)], crit.effective_plugin(), True, lo, hi, pending=pend,
                                          believe_plugin=False)  # fmt: skip
    assert [list(x) for x in want["best_x"]] == list(xs2) and tuple(want["best_val"]) == fs2
    with pytest.raises(ValueError, match="3 criteria"):
        bogp.constrained_believer_batch([crit, pi, mg], _box(), 300, q=2, Xs=Xs)
    # a model without a feasible observation: every step is feasibility-only and stays so
    none = bogp.Constrained(model=model, fun="EI", lo=[float(Y[:, 1].max()) + 1.0], hi=[INF])
    assert none.feasibility_only
    eng.calls.clear()
    bogp.constrained_believer_batch(none, _box(), 300, q=2, Xs=Xs)
    assert eng.calls[-1] == ("sweep_believer_constrained", (_lib.ACQ_NONE,) * 2, 0, True)
    # host-sampled and device-drawn candidates
    eng.calls.clear()
    bogp.constrained_believer_batch(crit, _box(5), 250, q=2)
    assert eng.calls[0] == ("upload", 250)
    eng.calls.clear()
    bogp.constrained_believer_batch(crit, _box(5), 250, q=2, design="LHS", seed=4)
    assert eng.calls[0] == ("generate", 250, "LHS") and eng.calls[1][0] == "sweep_believer_constrained"


def test_what_the_constrained_believer_refuses(gp, monkeypatch):
    model, Y, Xs, pend = gp
    Xs = Xs[:100]
    crit = bogp.Constrained(model=model, fun="EI", lo=[-INF], hi=[0.0])
    single = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=1e-6)
    single._engine = BelieverConstrainedOracleEngine()
    single.set_state(np.r_[0.6, 0.6, 0.6, 0.9], model.X, Y[:, 0])
    with pytest.raises(TypeError, match="bogp.Constrained"):
        bogp.constrained_believer_batch(bogp.EI(model=single), _box(), 100, q=2, Xs=Xs)
    with pytest.raises(TypeError, match="bogp.Constrained"):
        bogp.constrained_believer_batch([crit, bogp.EI(model=single)], _box(), 100, Xs=Xs)
    with pytest.raises(ValueError, match="share model, bounds"):
        bogp.constrained_believer_batch([crit, bogp.Constrained(model=model, fun="EI", lo=[-INF], hi=[0.5])], _box(), 100, Xs=Xs)
    with pytest.raises(ValueError, match="at most 32"):
        bogp.constrained_believer_batch(crit, _box(), 100, q=33, Xs=Xs)
    with pytest.raises(ValueError, match="at most 32"):
        bogp.constrained_believer_batch(crit, _box(), 100, q=31, Xs=Xs, pending=pend)
    with pytest.raises(ValueError, match="at least one"):
        bogp.constrained_believer_batch([], _box(), 100, Xs=Xs)
    with pytest.raises(NotImplementedError, match="lift"):
        bogp.constrained_believer_batch(crit, _box(), 100, q=2, Xs=Xs, lift=object())
    with pytest.raises(NotImplementedError, match="fixed variables"):
        bogp.constrained_believer_batch(crit, _box(), 100, q=2, Xs=Xs, masks=np.array([True, False, False]), values=[0.0])
    with pytest.raises(NotImplementedError, match="h / g"):
        bogp.constrained_believer_batch(crit, _box(), 100, q=2, Xs=Xs, h=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="h / g"):
        bogp.constrained_believer_batch(crit, _box(), 100, q=2, Xs=Xs, g=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.constrained_believer_batch(crit, _box(), 100, q=2, Xs=Xs, rank=0, world=2)
    monkeypatch.setattr(optim._forest, "is_forest_model", lambda m: True)
    with pytest.raises(NotImplementedError, match="forest"):
        bogp.constrained_believer_batch(crit, _box(), 100, q=2, Xs=Xs)
    monkeypatch.undo()
    # the single-objective and Thompson entries keep refusing the criterion exactly as before
    with pytest.raises(NotImplementedError, match="have no believer batches: strategy='topk' serves them"):
        bogp.believer_batch(crit, _box(), 100, q=2, Xs=Xs)
    with pytest.raises(NotImplementedError, match="have no believer batches: strategy='topk' serves them"):
        optim.batch_argmax([crit, crit], _box(), 100, strategy="believer")
    with pytest.raises(NotImplementedError, match="have no Thompson batches: strategy='topk' serves them"):
        optim.batch_argmax([crit, crit], _box(), 100, strategy="thompson")
    with pytest.raises(NotImplementedError, match="have no Thompson batches"):
        bogp.thompson_batch(model, _box(), 100, 2, Xs=Xs, criteria=[crit, crit])


def test_install_validates_constraint_batches():
    with pytest.raises(ValueError, match="needs expensive_constraints=True"):
        bogp.install(object(), constraint_batches="believer")
    with pytest.raises(ValueError, match="'topk' or 'believer'"):
        bogp.install(object(), expensive_constraints=True, constraint_batches="thompson")
    from bogp import integration

    assert not integration._ORIGINAL and "batches" not in integration._CONSTRAINTS


# ----------------------------------------------------------------------------------------------------------------------
# the reference's ParallelBO under install(expensive_constraints=True, constraint_batches="believer")
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
        created.append(BelieverConstrainedOracleEngine(device))
        return created[-1]

    monkeypatch.setattr(bogp._lib, "Engine", engine)
    yield bayes_optim, created
    bogp.uninstall()


def _parallel_bo(bayes_optim, optimizer="sweep"):
    from bayes_optim.search_space import RealSpace

    space = RealSpace([0, 1], var_name="a") + RealSpace([0, 1], var_name="b")
    model = bayes_optim.GaussianProcess(theta0=np.full(2, 1.0), thetaL=np.full(2, 1e-2), thetaU=np.full(2, 1e2), nugget=1e-6,
                                        noise_estim=False, likelihood="concentrated")  # fmt: skip
    opt = bayes_optim.ParallelBO(search_space=space, obj_fun=lambda x: x[0] + x[1], model=model, max_FEs=100, DoE_size=6, eval_type="list",
                                 n_job=1, verbose=False, minimize=True, acquisition_fun="MGFI", n_point=3,
                                 acquisition_optimization={"optimizer": optimizer, "max_FEs": 300})  # fmt: skip
    return opt, model


def _evaluate(X):
    A = np.asarray(X, dtype=float)
    return A.sum(1).tolist(), (0.25 - (A[:, 0] - 0.5) ** 2 - (A[:, 1] - 0.5) ** 2).tolist()  # g <= 0: outside a disc


@pytest.mark.timeout(900)
def test_parallel_bo_reaches_the_constrained_believer(reference):
    """ParallelBO(n_point=3, MGFI) with g_vals: ONE `sweep_believer_constrained` call per ask with the three criteria, three distinct
    points; a step with a fixed variable keeps the top-k route; without the keyword the same run reaches `sweep_constrained`."""
    bayes_optim, created = reference
    bogp.install(bayes_optim, expensive_constraints=True, constraint_batches="believer")
    np.random.seed(8)
    opt, model = _parallel_bo(bayes_optim)
    X = opt.ask(6)
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    for _ in range(2):
        model.engine.calls.clear()
        X = opt.ask()
        assert len(X) == 3 and len({tuple(x) for x in X}) == 3
        calls = [c for c in model.engine.calls if c[0].startswith("sweep")]
        assert len(calls) == 1 and calls[0][0] == "sweep_believer_constrained" and len(calls[0][1]) == 3 and calls[0][2:] == (0, True), calls
        assert set(calls[0][1]) <= {_lib.ACQ_MGFI, _lib.ACQ_NONE}
        f, g = _evaluate(X)
        opt.tell(X, f, g_vals=g)
    assert model.y.shape == (12, 2)
    model.engine.calls.clear()
    assert len(opt.ask(3, fixed={"a": 0.5})) == 3  # a fixed variable: today's route
    assert not any(c[0] == "sweep_believer_constrained" for c in model.engine.calls)
    bogp.uninstall()
    bogp.install(bayes_optim, expensive_constraints=True, batch_strategy="believer")  # without the keyword: top-k, as before
    np.random.seed(8)
    opt, model = _parallel_bo(bayes_optim)
    X = opt.ask(6)
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    X = opt.ask()
    assert len(X) == 3
    calls = [c for c in model.engine.calls if c[0].startswith("sweep")]
    assert calls and all(c[0] == "sweep_constrained" for c in calls) and calls[-1][2] > 1
