"""Kriging-believer batches on the host side (no GPU): the NumPy restatement of the recursion (tests/support/believer_ref.py)
against a brute-force dense refit on X + the believed points, the Python routing (`bogp.believer_batch`,
`batch_argmax(strategy=...)`) on the oracle-backed stand-in engine of tests/support/believer_engine.py, the refusals, and the
reference's own `ParallelBO` under `install(batch_strategy="believer")`."""
import os
import sys
import types
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle import gp_oracle as O

import bogp
from bogp import _lib, optim
from support.believer_engine import BelieverOracleEngine
from support.believer_ref import BelieverRef

REF = os.environ.get("BOGP_REFERENCE", "/root/reference")


def _problem(seed, N=30, d=3, M=200):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, size=(N, d))
    y = np.sin(X @ rng.normal(size=d)) + 0.1 * rng.normal(size=N)
    return X, y.reshape(-1, 1), rng.uniform(-2.2, 2.2, size=(M, d)), rng.uniform(-2, 2, size=(3, d))


def _ref_of(st):
    state = dict(C=st.C, gamma=st.gamma.ravel(), Ft=None if st.Ft is None else st.Ft.ravel(), G=0.0 if st.G is None else float(st.G[0, 0]),
                 beta=float(st.beta[0, 0]), sigma2=float(st.sigma2[0]))  # fmt: skip
    return BelieverRef(st.X, st.theta, st.kernel, state, st.estimate_trend)


@pytest.mark.parametrize("estimate_trend", [False, True], ids=["simple", "ordinary"])
def test_recursion_equals_a_dense_refit(estimate_trend):
    """Matern-3/2, noiseless: after each of three believed points (two pending rows off the candidates, then a winner) the
    restatement's s_B and mean are the bracket 1 - |L'^-1 r'|^2 + u'^2 and the mean of the model REBUILT on X + {p_1..p_B} with
    y = mu(p) at the same theta, to 1e-10 (the rebuilt sigma2 differs -- it is concentrated -- so the brackets are compared)."""
    X, y, Xs, pend = _problem(7)
    theta = np.array([0.8, 0.5, 1.1])
    st = O.make_state(theta, X, y, O.KERNEL_MATERN32, O.MODE_NOISELESS, 0.0, estimate_trend=estimate_trend, beta=0.2)
    ref = _ref_of(st)
    out = ref.run(Xs, [(O.ACQ_EI, 0.0), (O.ACQ_UCB, 2.0)], float(y.min()), True, pending=pend[:2])
    pts = np.vstack([pend[:2], out["best_x"]])
    mu0 = O.predict(st, Xs)[0][:, 0]
    np.testing.assert_allclose(out["mu"], mu0, rtol=0, atol=1e-12)
    for B in range(1, 4):
        Xb = np.vstack([X, pts[:B]])
        yb = np.vstack([y, O.predict(st, pts[:B], eval_MSE=False)])
        st_b = O.make_state(theta, Xb, yb, O.KERNEL_MATERN32, O.MODE_NOISELESS, 0.0, estimate_trend=estimate_trend, beta=0.2)
        mu_b, mse_b = O.predict(st_b, Xs)
        np.testing.assert_allclose(np.maximum(0.0, out["s"][B]), mse_b[:, 0] / st_b.sigma2[0], rtol=0, atol=1e-10)
        np.testing.assert_allclose(mu_b[:, 0], mu0, rtol=0, atol=1e-10)
    assert np.all(out["pivots"][:3] > 1e-3)  # the three points were informative
    assert len(set(out["best_idx"].tolist())) == 2
    assert out["s"][3][out["best_idx"][0]] <= 1e-10  # a believed candidate row is determined


def test_pivot_guard_and_plugin_rule():
    X, y, Xs, pend = _problem(8)
    st = O.make_state(np.array([0.8, 0.5, 1.1]), X, y, O.KERNEL_MATERN52, O.MODE_NOISELESS, 0.0, estimate_trend=True)
    ref = _ref_of(st)
    acq = [(O.ACQ_EI, 0.0), (O.ACQ_EI, 0.0), (O.ACQ_MGFI, 2.0)]
    plain = ref.run(Xs, acq, float(y.min()), True, pending=pend[:1])
    # a training point and a repeated point are absorbed: pivots at the floor, every output unchanged
    dup = ref.run(Xs, acq, float(y.min()), True, pending=np.vstack([X[4], pend[:1], pend[:1]]), believe_plugin=True)
    assert dup["pivots"][0] <= 1e-12 and dup["pivots"][2] <= 1e-12 and dup["pivots"][1] > 1e-6
    np.testing.assert_array_equal(dup["best_idx"], plain["best_idx"])
    np.testing.assert_allclose(dup["mse"], plain["mse"], rtol=1e-9, atol=1e-12 * ref.sigma2)
    # the plugin follows the believed means only when asked to
    low = Xs[int(np.argmin(plain["mu"]))]
    on = ref.run(Xs, acq[:1], 10.0, True, pending=low[None, :], believe_plugin=True)
    off = ref.run(Xs, acq[:1], 10.0, True, pending=low[None, :], believe_plugin=False)
    np.testing.assert_array_equal(on["mse"], off["mse"])
    assert np.all(on["acq"][0] <= off["acq"][0]) and on["acq"][0].max() < off["acq"][0].max()
    # maximising: y_hat = -mu, the plugin arrives negated
    mx = ref.run(Xs, acq[:2], -float(y.max()), False)
    assert len(set(mx["best_idx"].tolist())) == 2


# ----------------------------------------------------------------------------------------------------------------------
# the Python routing on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def gp():
    X, y, _, _ = _problem(9, N=40)
    model = bogp.GaussianProcess(corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=1e-6)
    model._engine = BelieverOracleEngine()
    model.set_state(np.r_[0.6, 0.6, 0.6, 0.9], X, y)
    return model


def _box(seed=3):
    return optim.Box([(-2.2, 2.2)] * 3, random_seed=seed)


def test_believer_batch_routes_and_replicates(gp):
    eng = gp.engine
    Xs = _problem(9, N=40, M=300)[2]
    crit = bogp.EI(model=gp)
    eng.calls.clear()
    xs, fs = bogp.believer_batch(crit, _box(), 300, q=3, Xs=Xs)
    assert eng.calls == [("upload", 300), ("sweep_believer", 3, 0, True)]
    assert len(xs) == len(fs) == 3 and all(isinstance(x, list) and len(x) == 3 for x in xs) and all(isinstance(f, float) for f in fs)
    assert len({tuple(x) for x in xs}) == 3  # one criterion three times: the believer alone keeps the points apart
    assert fs[0] == float(np.max(crit(Xs))) and xs[0] == Xs[int(np.argmax(crit(Xs).ravel()))].tolist()  # step 0 is the plain sweep
    # a list is used in order; pending rows and the plugin switch reach the engine
    crits = [bogp.UCB(model=gp, alpha=1.0), bogp.EpsilonPI(model=gp, epsilon=0.01), bogp.MGFI(model=gp, t=2.0)]
    eng.calls.clear()
    xs2, fs2 = bogp.believer_batch(crits, _box(), 300, Xs=Xs, pending=Xs[:2] + 0.01, believe_plugin=False)
    assert eng.calls[-1] == ("sweep_believer", 3, 2, False) and len(xs2) == 3
    want = BelieverOracleEngine.sweep_believer(eng, [(c.acq_id, c.acq_par()) for c in crits], crits[1].effective_plugin(), True,
                                               pending=Xs[:2] + 0.01, believe_plugin=False)  # fmt: skip
    assert [list(x) for x in want["best_x"]] == list(xs2) and tuple(want["best_val"]) == fs2
    # host-sampled and device-drawn candidates
    eng.calls.clear()
    bogp.believer_batch(crit, _box(5), 250, q=2)
    assert eng.calls[0] == ("upload", 250)
    eng.calls.clear()
    bogp.believer_batch(crit, _box(5), 250, q=2, design="LHS", seed=4)
    assert eng.calls[0] == ("generate", 250, "LHS") and eng.calls[1][0] == "sweep_believer"
    with pytest.raises(ValueError, match="q = 2 but 3"):
        bogp.believer_batch(crits, _box(), 300, q=2, Xs=Xs)
    with pytest.raises(ValueError, match="at most 32"):
        bogp.believer_batch(crit, _box(), 300, q=33, Xs=Xs)


@pytest.mark.parametrize("make", [lambda m: bogp.EpsilonPI(model=m, epsilon=0.05), lambda m: bogp.MGFI(model=m, t=2.0),
                                  lambda m: bogp.UCB(model=m, alpha=2.0), lambda m: bogp.EI(model=m)], ids=["epsilonpi", "mgfi", "ucb", "ei"])
def test_one_criterion_q_times_proposes_q_rows(gp, make):
    """A row that is a winner has zero variance afterwards, where EpsilonPI is exactly 1 once its mean is the plugin and UCB is
    its bare mean: it keeps that value but does not compete again, so every criterion replicated q times proposes q rows."""
    Xs = _problem(9, N=40, M=300)[2]
    for believe_plugin in (True, False):
        xs, fs = bogp.believer_batch(make(gp), _box(), 300, q=4, Xs=Xs, believe_plugin=believe_plugin)
        assert len({tuple(x) for x in xs}) == 4


def test_fused_step_keeps_topk_for_what_the_believer_does_not_serve():
    from bogp import integration

    integration._BATCH["strategy"] = "believer"
    try:
        assert integration._strategy_of(None, {}) == {"strategy": "believer"}
        assert integration._strategy_of(np.array([True, False]), {}) == {}  # fixed variables
        assert integration._strategy_of(None, {"h": lambda x: 0.0}) == {} and integration._strategy_of(None, {"g": lambda x: 0.0}) == {}
    finally:
        integration._BATCH.clear()
    assert integration._strategy_of(None, {}) == {}


def test_what_the_believer_refuses(gp):
    crit = bogp.EI(model=gp)
    box = _box()

    class RandomForest:
        pass

    forest_crit = types.SimpleNamespace(acq_id=0, acq_par=lambda: 0.0, model=RandomForest(), minimize=True)
    ehvi = types.SimpleNamespace(is_ehvi=True, model=gp, minimize=True)
    with pytest.raises(NotImplementedError, match="forest"):
        bogp.believer_batch(forest_crit, box, 100, q=2)
    with pytest.raises(NotImplementedError, match="EHVI"):
        bogp.believer_batch(ehvi, box, 100, q=2)
    with pytest.raises(NotImplementedError, match="lift"):
        bogp.believer_batch(crit, box, 100, q=2, lift=bogp.Lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3)))
    with pytest.raises(NotImplementedError, match="fixed variables"):
        bogp.believer_batch(crit, box, 100, q=2, masks=np.array([True, False, False]), values=[0.0])
    with pytest.raises(NotImplementedError, match="constraints"):
        bogp.believer_batch(crit, box, 100, q=2, g=lambda x: -1.0)
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.believer_batch(crit, box, 100, q=2, rank=0, world=2)
    with pytest.raises(NotImplementedError, match="constraints"):
        bogp.batch_argmax([crit, crit], box, 100, h=lambda x: 0.0, strategy="believer")
    with pytest.raises(ValueError, match="strategy"):
        bogp.batch_argmax([crit], box, 100, strategy="greedy")


def test_batch_argmax_strategy_keyword(gp):
    eng = gp.engine
    Xs = _problem(9, N=40, M=300)[2]
    crits = [bogp.MGFI(model=gp, t=t) for t in (0.5, 1.0, 2.0)]
    eng.calls.clear()
    plain = bogp.batch_argmax(crits, _box(), 300, k=4, Xs=Xs)
    calls_plain = list(eng.calls)
    eng.calls.clear()
    topk = bogp.batch_argmax(crits, _box(), 300, k=4, Xs=Xs, strategy="topk")
    assert eng.calls == calls_plain == [("upload", 300), ("sweep_topk", 3, 4)] and topk == plain  # today's path, untouched
    eng.calls.clear()
    bel = bogp.batch_argmax(crits, _box(), 300, k=4, Xs=Xs, history=Xs[:5], strategy="believer")
    assert eng.calls == [("upload", 300), ("sweep_believer", 3, 0, True)]
    assert bel == bogp.believer_batch(crits, _box(), 300, Xs=Xs) and len({tuple(x) for x in bel[0]}) == 3


# ----------------------------------------------------------------------------------------------------------------------
# the reference's ParallelBO under install(batch_strategy="believer")
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
def test_parallel_bo_under_the_believer_strategy(monkeypatch):
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim
    from bayes_optim import ParallelBO, RealSpace

    created = []

    def engine(device=0):
        created.append(BelieverOracleEngine(device))
        return created[-1]

    monkeypatch.setattr(_lib, "Engine", engine)
    # every SearchSpace the reference builds on the way re-seeds the global stream from the operating system (`random_seed=None`,
    # search_space.py:130-134): pinned here, so that the two runs below can be compared at all
    seed = np.random.seed
    monkeypatch.setattr(np.random, "seed", lambda s=None: seed(77 if s is None else s))
    dim = 2
    f = lambda x: float(np.sum(np.asarray(x) ** 2))  # noqa: E731

    def one_ask(strategy):
        undo = bogp.install(bayes_optim, batch_strategy=strategy)
        try:
            np.random.seed(5)  # (the design of experiments and the restarts of the fit draw from the global stream)
            model = bogp.GaussianProcess(corr="squared_exponential", thetaL=1e-3 * np.ones(dim), thetaU=10 * np.ones(dim), nugget=1e-6,
                                         random_start=2)  # fmt: skip
            opt = ParallelBO(search_space=RealSpace([-5, 5]) * dim, obj_fun=f, model=model, max_FEs=30, DoE_size=6, n_point=4,
                             acquisition_fun="MGFI", acquisition_par={"t": 2}, acquisition_optimization={"optimizer": "sweep", "max_FEs": 400},
                             verbose=False, random_seed=11)  # fmt: skip
            X = opt.ask()
            opt.tell(X, [f(x) for x in X])
            np.random.seed(123)
            X = opt.ask()
            return X, np.random.get_state()[1].copy(), np.random.get_state()[2], model.engine.calls
        finally:
            undo()

    X_b, key_b, pos_b, calls_b = one_ask("believer")
    X_t, key_t, pos_t, calls_t = one_ask("topk")
    assert len(X_b) == 4 and len({tuple(np.round(x, 12)) for x in X_b}) == 4
    assert ("sweep_believer", 4, 0, True) in calls_b and not any(c[0] == "sweep_believer" for c in calls_t)
    assert any(c[0] == "sweep_topk" for c in calls_t) and not any(c[0] == "sweep_topk" for c in calls_b)
    assert pos_b == pos_t and np.array_equal(key_b, key_t)  # np.random stands where the plain fused path leaves it
    with pytest.raises(ValueError, match="batch_strategy"):
        bogp.install(bayes_optim, batch_strategy="greedy")
    bogp.uninstall()


@pytest.mark.parametrize("prefix", ["m32ok", "sesk"])
def test_restatement_against_the_references_rebuilt_models(prefix):
    """G43 (tests/support/make_believer_golden.py) without a device: the restatement's s_B after each prefix of the four believed
    rows against the reference's own predict of the model rebuilt on X + {p_1 .. p_B}, MSE / sigma2 under T2, the mean under T1."""
    from conftest import load_golden

    g = {k[len(prefix) + 1 :]: v for k, v in load_golden("G43_believer").items() if k.startswith(prefix + "_")}
    st = O.make_state(g["par"], g["X"], g["y"], int(g["kernel"]), int(g["mode"]), 0.0, estimate_trend=bool(g["estimate_trend"]),
                      beta=float(g["beta"]))  # fmt: skip
    out = _ref_of(st).run(g["Xs"], [(O.ACQ_EI, 0.0)], float(g["y"].min()), True, pending=g["believed"])
    for B in range(1, 5):
        np.testing.assert_allclose(np.maximum(0.0, out["s"][B]), g["mse_j"][B - 1] / g["sigma2_j"][B - 1], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(out["mu"], g["mu_j"][B - 1], rtol=1e-6, atol=1e-9)
    assert np.all(out["s"][4][g["believed_rows"]] <= 1e-12)
