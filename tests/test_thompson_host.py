"""Thompson-sampling batches on the host side (no GPU): the law of the paths of `bogp.thompson.paths_numpy` (mean and variance
against the kriging predictor, over the spectral draws of five kernels and both kriging flavours), interpolation, the draw's
reproducibility, the Python routing (`bogp.thompson_batch`, `batch_argmax(strategy="thompson")`,
`GaussianProcess.sampling_posterior`) on the oracle-backed stand-in engine of tests/support/thompson_engine.py, the refusals, and
the reference's own `ParallelBO` under `install(batch_strategy="thompson")`."""
import os
import sys
import types
import warnings

import numpy as np
import pytest

from conftest import ROOT

import bogp
from bogp import _lib, optim, thompson
from support.thompson_engine import ThompsonOracleEngine

REF = os.environ.get("BOGP_REFERENCE", "/root/reference")

KERNELS = {"se": _lib.KERNEL_SE, "matern32": _lib.KERNEL_MATERN32, "matern52": _lib.KERNEL_MATERN52, "matern12": _lib.KERNEL_MATERN12,
           "absexp": _lib.KERNEL_ABSEXP}  # fmt: skip


def _data(seed, N=30, d=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, size=(N, d))
    y = np.sin(X @ rng.normal(size=d)) + 0.1 * rng.normal(size=N)
    return rng, X, y


@pytest.mark.parametrize("estimate_trend", [True, False], ids=["ordinary", "simple"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_paths_have_the_predictors_mean_and_mse(kernel, estimate_trend):
    """d = 3, N = 30, L = 512, nugget 1e-4; S = 400 independent draws of (omega, b, W, E) with 16 paths each; 5 points, one of them
    0.01 from a training row.  Per draw i: m_i = the mean of its 16 paths, v_i = the mean of (path - mu)^2 -- 400 independent values
    each, with E[m_i] = mu and E[v_i] = MSE when the spectral draw is the kernel's.  Both sample means must sit within 6 of their
    own standard errors std / sqrt(S): a central-limit bound, not a tuned number."""
    rng, X, y = _data(11)
    st = thompson.dense_state(X, y, [0.7, 0.4, 1.0], KERNELS[kernel], estimate_trend, beta=0.2, nugget=1e-4)
    Xt = np.vstack([rng.uniform(-2, 2, size=(4, 3)), X[7] + np.array([0.01, 0.0, 0.0])])
    mu, mse = thompson.moments_numpy(st, Xt)
    assert np.all(mse > 0) and mse[4] < 0.05 * mse[:4].max()  # the near point is nearly determined, the others are not
    S = 400
    m, v = np.empty((S, 5)), np.empty((S, 5))
    for i in range(S):
        paths, _ = thompson.paths_numpy(st, thompson.draw(st, 16, 512, seed=[5, i]), Xt)
        m[i] = paths.mean(axis=0)
        v[i] = ((paths - mu) ** 2).mean(axis=0)
    z_mean = np.abs(m.mean(axis=0) - mu) / (m.std(axis=0, ddof=1) / np.sqrt(S))
    z_var = np.abs(v.mean(axis=0) - mse) / (v.std(axis=0, ddof=1) / np.sqrt(S))
    print("%s %s: |mean - mu| / se = %s, |var - MSE| / se = %s" % (kernel, estimate_trend, np.round(z_mean, 2), np.round(z_var, 2)))
    assert np.all(z_mean <= 6.0), z_mean
    assert np.all(z_var <= 6.0), z_var


def test_general_nu_draw_is_the_matern_draw_at_its_order():
    """nu = 1.5 through the general-nu kernel: the same correlation and, per seed, the same draw as Matern-3/2."""
    _, X, y = _data(12)
    a = thompson.dense_state(X, y, [0.7, 0.4, 1.0], _lib.KERNEL_MATERN32, nugget=1e-6)
    b = thompson.dense_state(X, y, [0.7, 0.4, 1.0], _lib.KERNEL_MATERN_NU, nugget=1e-6, nu=1.5)
    np.testing.assert_allclose(thompson.correlation(b, X[:5], X), thompson.correlation(a, X[:5], X), rtol=1e-12, atol=1e-15)
    da, db = thompson.draw(a, 3, 64, seed=1), thompson.draw(b, 3, 64, seed=1)
    for u, w in zip(da, db):
        np.testing.assert_array_equal(u, w)


@pytest.mark.parametrize("estimate_trend", [True, False], ids=["ordinary", "simple"])
def test_paths_interpolate_the_training_data(estimate_trend):
    """nugget 1e-10: |path_j(X_i) - y_i| <= 6 sqrt(MSE(X_i)) + the mean's own allowance (T1: atol 1e-9 beside rtol 1e-6), every i, j."""
    _, X, y = _data(13)
    st = thompson.dense_state(X, y, [2.0, 1.5, 2.5], _lib.KERNEL_MATERN52, estimate_trend, beta=0.1, nugget=1e-10)
    _, mse = thompson.moments_numpy(st, X)
    paths, (gt, bt) = thompson.paths_numpy(st, thompson.draw(st, 16, 512, seed=3), X)
    assert paths.shape == (16, 30) and gt.shape == (30, 16) and bt.shape == (16,)
    bound = 6.0 * np.sqrt(np.maximum(mse, 0.0)) + 1e-9 + 1e-6 * np.abs(y)
    assert np.all(np.abs(paths - y) <= bound), np.max(np.abs(paths - y) - bound)
    prior, (g0, b0) = thompson.paths_numpy(st, thompson.draw(st, 16, 512, seed=3), X, conditioned=False)
    assert np.max(np.abs(prior - y)) > 0.1 and not g0.any() and not b0.any()  # the prior paths do not


def test_draw_is_reproducible_per_seed_and_ordered():
    _, X, y = _data(14)
    for kernel in (_lib.KERNEL_SE, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP):
        st = thompson.dense_state(X, y, [0.7], kernel, nugget=1e-6)  # an isotropic theta is broadcast
        a, b, c = thompson.draw(st, 4, 64, seed=9), thompson.draw(st, 4, 64, seed=9), thompson.draw(st, 4, 64, seed=10)
        assert a.omega.shape == (64, 3) and a.phase.shape == (64,) and a.weights.shape == (64, 4) and a.eps.shape == (30, 4)
        assert all(np.array_equal(u, w) for u, w in zip(a, b)) and not np.array_equal(a.omega, c.omega)
        assert np.all((a.phase >= 0) & (a.phase < 2 * np.pi))
    # the documented order: n first, whatever the kernel, so the SE draw is n * sqrt(2 theta) of the generator's first L x d normals
    st = thompson.dense_state(X, y, [0.7, 0.4, 1.0], _lib.KERNEL_SE, nugget=1e-6)
    n = np.random.default_rng(9).standard_normal((64, 3))
    np.testing.assert_array_equal(thompson.draw(st, 4, 64, seed=9).omega, n * np.sqrt(2.0 * st.theta))
    for bad in (0, 8, 24, thompson.MAX_FEATURES + 16):
        with pytest.raises(ValueError, match="multiple of 16"):
            thompson.draw(st, 2, bad)
    with pytest.raises(ValueError, match="at least one"):
        thompson.draw(st, 0, 64)


# ----------------------------------------------------------------------------------------------------------------------
# the Python routing on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
def _model(corr="matern", nugget=0, **kw):
    _, X, y = _data(15, N=40)
    model = bogp.GaussianProcess(corr=corr, thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=nugget, **kw)
    model._engine = ThompsonOracleEngine()
    model.set_state(np.r_[0.9, 0.6, 1.2] if not nugget else np.r_[0.9, 0.6, 1.2, 0.9], X, y)
    return model


@pytest.fixture()
def gp():
    return _model()


def _box(seed=3):
    return optim.Box([(-2.2, 2.2)] * 3, random_seed=seed)


def _cands(M=300):
    return np.random.default_rng(21).uniform(-2.2, 2.2, size=(M, 3))


def test_thompson_batch_routes_and_returns_distinct_rows(gp):
    eng, Xs = gp.engine, _cands()
    eng.calls.clear()
    xs, fs = bogp.thompson_batch(gp, _box(), 300, q=3, n_features=64, seed=4, Xs=Xs)
    assert eng.calls == [("upload", 300), ("sweep_thompson", 3, 8, True)]
    assert isinstance(xs, tuple) and isinstance(fs, tuple) and len(xs) == len(fs) == 3
    assert all(isinstance(x, list) and len(x) == 3 for x in xs) and all(isinstance(f, float) for f in fs)  # batch_argmax's format
    paths, _ = thompson.paths_numpy(gp, thompson.draw(gp, 3, 64, seed=4), Xs)
    for j in range(3):  # each path's own minimiser and its value there (the three happen to differ)
        assert xs[j] == Xs[int(np.argmin(paths[j]))].tolist() and fs[j] == float(paths[j].min())
    xs2, fs2 = bogp.thompson_batch(gp, _box(), 300, q=3, n_features=64, seed=4, Xs=Xs, minimize=False)
    assert [fs2[j] == float(paths[j].max()) for j in range(3)] == [True] * 3
    # the same format as batch_argmax's
    plain = bogp.batch_argmax([bogp.MGFI(model=gp, t=t) for t in (0.5, 1.0, 2.0)], _box(), 300, Xs=Xs)
    assert [type(a) for a in plain] == [type(xs), type(fs)] and [type(a[0]) for a in plain] == [type(xs[0]), type(fs[0])]
    # history: a proposal np.isclose to an evaluated point gives way to the path's next rank
    xs3, _ = bogp.thompson_batch(gp, _box(), 300, q=3, n_features=64, seed=4, Xs=Xs, history=np.array([xs[0]]))
    assert xs3[0] == Xs[int(np.argsort(paths[0], kind="stable")[1])].tolist() and xs3[1:] == xs[1:]
    # host-sampled and device-drawn candidates
    eng.calls.clear()
    bogp.thompson_batch(gp, _box(5), 250, q=2, n_features=64, seed=1)
    assert eng.calls[0] == ("upload", 250)
    eng.calls.clear()
    bogp.thompson_batch(gp, _box(5), 250, q=2, n_features=64, design="LHS", seed=4)
    assert eng.calls[0] == ("generate", 250, "LHS") and eng.calls[1][0] == "sweep_thompson"


def test_paths_sharing_one_minimiser_still_propose_q_rows(gp, monkeypatch):
    """Equal columns of W make the q paths one and the same function: the fall-back through the k ranks keeps the rows apart."""
    real = thompson.draw

    def same(model, q, n_features=1024, seed=None):
        dr = real(model, q, n_features, seed)
        return dr._replace(weights=np.repeat(dr.weights[:, :1], q, axis=1), eps=np.repeat(dr.eps[:, :1], q, axis=1))

    monkeypatch.setattr(thompson, "draw", same)
    Xs = _cands()
    xs, fs = bogp.thompson_batch(gp, _box(), 300, q=5, n_features=64, seed=4, Xs=Xs)
    path = thompson.paths_numpy(gp, same(gp, 5, 64, 4), Xs)[0][0]
    order = np.argsort(path, kind="stable")[:5]
    assert [list(x) for x in xs] == Xs[order].tolist() and fs == tuple(float(v) for v in path[order])
    # more than 16 paths: calls of 16 with derived seeds, rows taken by an earlier call stay taken
    gp.engine.calls.clear()
    xs, fs = bogp.thompson_batch(gp, _box(), 300, q=19, n_features=64, seed=4, Xs=Xs, k=24)
    assert [c[:2] for c in gp.engine.calls if c[0] == "sweep_thompson"] == [("sweep_thompson", 16), ("sweep_thompson", 3)]
    assert len({tuple(x) for x in xs}) == 19


def test_sampling_posterior_and_prior_shapes(gp):
    Xs = _cands(50)
    assert gp.sampling_posterior(Xs[0]).shape == (1, 1)  # the one-argument call of the reference's stub: one path
    for n in (1, 16, 17):
        s = gp.sampling_posterior(Xs, n_samples=n, n_features=64, seed=2)
        assert s.shape == (50, n) and np.all(np.isfinite(s))
    p = gp.sampling_prior(Xs, n_samples=17, n_features=64, seed=2)
    assert p.shape == (50, 17)
    one = gp.sampling_posterior(Xs, n_samples=3, n_features=64, seed=2)
    np.testing.assert_array_equal(one, thompson.paths_numpy(gp, thompson.draw(gp, 3, 64, seed=2), Xs)[0].T)
    np.testing.assert_array_equal(one, gp.sampling_posterior(Xs, n_samples=3, n_features=64, seed=2))
    # the posterior paths pass through the data of a noiseless model, the prior paths do not
    at_X = gp.sampling_posterior(gp.X, n_samples=4, n_features=256, seed=5)
    np.testing.assert_allclose(at_X, np.repeat(gp.y.reshape(-1, 1), 4, axis=1), rtol=1e-6, atol=1e-6)
    assert np.max(np.abs(gp.sampling_prior(gp.X, n_samples=4, n_features=256, seed=5) - gp.y.reshape(-1, 1))) > 0.1


def test_batch_argmax_strategy_keyword(gp):
    eng, Xs = gp.engine, _cands()
    crits = [bogp.MGFI(model=gp, t=t) for t in (0.5, 1.0, 2.0)]
    eng.calls.clear()
    plain = bogp.batch_argmax(crits, _box(), 300, k=4, Xs=Xs)
    assert eng.calls == [("upload", 300), ("sweep_topk", 3, 4)]  # the default is today's path
    eng.calls.clear()
    th = bogp.batch_argmax(crits, _box(), 300, k=4, Xs=Xs, seed=6, strategy="thompson")
    assert eng.calls == [("upload", 300), ("sweep_thompson", 3, 4, True)]
    assert len({tuple(x) for x in th[0]}) == 3 and th != plain
    assert th == bogp.thompson_batch(gp, _box(), 300, q=3, seed=6, Xs=Xs, k=4)
    mx = bogp.batch_argmax([bogp.UCB(model=gp, alpha=1.0, minimize=False)] * 2, _box(), 300, Xs=Xs, seed=6, strategy="thompson")
    assert mx == bogp.thompson_batch(gp, _box(), 300, q=2, seed=6, Xs=Xs, minimize=False)
    with pytest.raises(ValueError, match="'topk', 'believer' or 'thompson'"):
        bogp.batch_argmax(crits, _box(), 300, strategy="greedy")


def test_what_thompson_sampling_refuses(gp):
    box = _box()

    class RandomForest:
        pass

    with pytest.raises(NotImplementedError, match="forest"):
        bogp.thompson_batch(RandomForest(), box, 100, q=2)
    ehvi = types.SimpleNamespace(is_ehvi=True, model=gp, minimize=True)
    with pytest.raises(NotImplementedError, match="EHVI"):
        bogp.batch_argmax([ehvi, ehvi], box, 100, strategy="thompson")
    with pytest.raises(NotImplementedError, match="lift"):
        bogp.thompson_batch(gp, box, 100, q=2, lift=bogp.Lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3)))
    with pytest.raises(NotImplementedError, match="fixed variables"):
        bogp.thompson_batch(gp, box, 100, q=2, masks=np.array([True, False, False]), values=[0.0])
    with pytest.raises(NotImplementedError, match="constraints"):
        bogp.thompson_batch(gp, box, 100, q=2, g=lambda x: -1.0)
    with pytest.raises(NotImplementedError, match="constraints"):
        bogp.batch_argmax([bogp.EI(model=gp)] * 2, box, 100, h=lambda x: 0.0, strategy="thompson")
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.thompson_batch(gp, box, 100, q=2, rank=0, world=2)
    with pytest.raises(NotImplementedError, match="noisy mode"):
        bogp.thompson_batch(_model(nugget=1e-6), box, 100, q=2)
    with pytest.raises(NotImplementedError, match="noisy mode"):
        _model(nugget=1e-6).sampling_posterior(_cands(5))
    noise_estim = _model(nugget=1e-6, noise_estim=True)
    with pytest.raises(NotImplementedError, match="noise_estim mode"):
        bogp.thompson_batch(noise_estim, box, 100, q=2)
    linear = _model()
    linear.mean = bogp.trend.linear_trend(3, beta=np.zeros(4))
    with pytest.raises(NotImplementedError, match="polynomial trend"):
        bogp.thompson_batch(linear, box, 100, q=2)
    for kid, name in ((_lib.KERNEL_CUBIC, "cubic"), (_lib.KERNEL_GENEXP, "generalized-exponential")):
        m = _model()
        m.kernel_id = kid  # (the refusal reads the committed kernel; neither kernel needs a model of its own for that)
        with pytest.raises(NotImplementedError, match=name):
            bogp.thompson_batch(m, box, 100, q=2)
    two = _model()
    two.y = np.c_[two.y, two.y]
    with pytest.raises(NotImplementedError, match="several targets"):
        bogp.thompson_batch(two, box, 100, q=2)
    unfitted = bogp.GaussianProcess(corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=0)
    with pytest.raises(Exception, match="not fitted"):
        bogp.thompson_batch(unfitted, box, 100, q=2)


def test_fused_step_strategy_and_the_unchanged_default():
    from bogp import integration

    assert integration._strategy_of(None, {}) == {}  # nothing installed: the default
    integration._BATCH["strategy"] = "thompson"
    try:
        assert integration._strategy_of(None, {}) == {"strategy": "thompson"}
        assert integration._strategy_of(np.array([True, False]), {}) == {}  # fixed variables keep top-k, as under the believer
        assert integration._strategy_of(None, {"h": lambda x: 0.0}) == {} and integration._strategy_of(None, {"g": lambda x: 0.0}) == {}
    finally:
        integration._BATCH.clear()


@pytest.mark.timeout(600)
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
def test_parallel_bo_under_the_thompson_strategy(monkeypatch):
    """Two ask() / tell() rounds of the reference's unmodified ParallelBO with a noiseless device model on the stand-in engine."""
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim
    from bayes_optim import ParallelBO, RealSpace

    monkeypatch.setattr(_lib, "Engine", lambda device=0: ThompsonOracleEngine(device))
    dim = 2
    f = lambda x: float(np.sum(np.asarray(x) ** 2))  # noqa: E731

    def run(strategy):
        undo = bogp.install(bayes_optim, **({} if strategy is None else {"batch_strategy": strategy}))
        try:
            np.random.seed(5)
            model = bogp.GaussianProcess(corr="matern", thetaL=1e-2 * np.ones(dim), thetaU=10 * np.ones(dim), nugget=0, random_start=2)
            opt = ParallelBO(search_space=RealSpace([-5, 5]) * dim, obj_fun=f, model=model, max_FEs=30, DoE_size=6, n_point=4,
                             acquisition_fun="MGFI", acquisition_par={"t": 2}, acquisition_optimization={"optimizer": "sweep", "max_FEs": 400},
                             verbose=False, random_seed=11)  # fmt: skip
            rounds = []
            for _ in range(3):  # the design of experiments, then two model-based rounds
                X = opt.ask()
                opt.tell(X, [f(x) for x in X])
                rounds.append(X)
            return rounds, [c[0] for c in model.engine.calls]
        finally:
            undo()

    rounds, calls = run("thompson")
    for X in rounds[1:]:
        assert len(X) == 4 and len({tuple(np.round(x, 12)) for x in X}) == 4
    assert calls.count("sweep_thompson") == 2 and "sweep_topk" not in calls and "sweep_believer" not in calls
    _, calls_default = run(None)
    assert "sweep_topk" in calls_default and "sweep_thompson" not in calls_default  # the default install() is unchanged
    with pytest.raises(ValueError, match="'topk', 'believer' or 'thompson'"):
        bogp.install(bayes_optim, batch_strategy="greedy")
    bogp.uninstall()
