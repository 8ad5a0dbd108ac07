"""Host side of the random-forest surrogate (bogp/forest.py, the routing in optim.py / integration.py) without a GPU: the engine is the
NumPy traversal of tests/support/forest_engine.py, injected by monkeypatching `bogp._lib.Engine`.  Packing and the column map are held
against scikit-learn's own `estimators_[t].predict` and the reference's `RandomForest` (where the reference tree is present), the
stand-in's moments against the recorded reference values of tests/golden/G40_forest.npz; the device twin is tests/test_gpu_forest.py."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT, load_golden

import bogp
from bogp import _lib
from bogp import forest as F
from support import forest_engine as S
from support import philox_mixed

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
LABELS = ["red", "green", "blue", "cyan", "black"]


@pytest.fixture()
def engines(monkeypatch):
    created = []

    def engine(device=0):
        created.append(S.ForestEngine(device))
        return created[-1]

    monkeypatch.setattr(bogp._lib, "Engine", engine)
    return created


@pytest.fixture()
def reference():
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    from support import ref_suite_plugin

    ref_suite_plugin.pytest_configure(None)  # OneHotEncoder(sparse=...) of the reference on current scikit-learn
    import bayes_optim

    return bayes_optim


def _rows(rng, n):
    X = np.empty((n, 5), dtype=object)
    X[:, 0] = rng.uniform(-5, 5, n)
    X[:, 1] = rng.choice(LABELS, n)
    X[:, 2] = rng.integers(0, 11, n)
    X[:, 3] = rng.uniform(0, 1, n)
    X[:, 4] = rng.choice(["x", "y", "z"], n)
    return X


def _f(X):
    w = {l: i for i, l in enumerate(LABELS)}
    return np.array([float(r[0]) ** 2 + 3 * w[r[1]] + abs(r[2] - 4) + 5 * float(r[3]) * (r[4] == "y") for r in X])


LEVELS = {1: LABELS, 4: ["x", "y", "z"]}


def _forest_tuple(pk, raw):
    if raw:
        f, t, test = pk.raw()
        return (pk.tree_offset, f, t, pk.left, pk.right, pk.value, test)
    return (pk.tree_offset, pk.feature, pk.threshold, pk.left, pk.right, pk.value, None)


def _check_pack(model, X, enc):
    pk = F.pack(model)
    want = np.stack([e.predict(np.asarray(enc, dtype=np.float32)) for e in model.estimators_], axis=1)
    assert np.any(pk.threshold[pk.left >= 0] != pk.threshold[pk.left >= 0].astype(np.float32))  # midpoints float32 cannot hold
    assert np.array_equal(S.leaves(_forest_tuple(pk, False), enc), want)
    assert np.array_equal(S.leaves(_forest_tuple(pk, True), pk.to_index(X)), want)
    assert np.array_equal(pk.encode(X), np.asarray(enc, dtype=float))
    assert np.array_equal(pk.encode_index(pk.to_index(X)), np.asarray(enc, dtype=float))
    return pk


def test_package_imports_without_scikit_learn():
    code = ("import sys; sys.modules['sklearn'] = None; import bogp; from bogp import forest, optim, acquisition; "
            "assert 'RandomForest' not in vars(bogp)\n"
            "try:\n    bogp.RandomForest\nexcept ImportError:\n    print('lazy')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "lazy", out.stderr


def test_pack_of_bogp_random_forest_reproduces_every_tree(engines):
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(0)
    X = _rows(rng, 150)
    rf = bogp.RandomForest(levels=LEVELS, random_state=2)
    assert rf.n_estimators == 100 and rf.max_features == 5 / 6 and rf.min_samples_leaf == 2
    rf.fit(X, _f(X).reshape(-1, 1))
    Xt = _rows(rng, 400)
    pk = _check_pack(rf, Xt, rf._check_X(Xt))
    assert pk.d_raw == 5 and pk.d_enc == 3 + 5 + 3 and pk.noncat == [0, 2, 3] and pk.cat_idx == [1, 4]
    # predict runs on the engine: mean and std(ddof = 1)^2 over the trees
    mu, mse = rf.predict(Xt, eval_MSE=True)
    P = np.stack([e.predict(rf._check_X(Xt).astype(np.float32)) for e in rf.estimators_], axis=1)
    assert np.array_equal(mu, P.mean(axis=1)) and np.array_equal(mse, P.std(axis=1, ddof=1) ** 2.0)
    assert np.array_equal(rf.predict(Xt[:3]), mu[:3])
    assert len(engines) == 1 and engines[0].calls.count("forest_set") == 1
    rf.fit(X[:100], _f(X[:100]))  # a new fit is packed again
    rf.predict(Xt[:3])
    assert engines[0].calls.count("forest_set") == 2
    with pytest.raises(ValueError, match="unknown level"):
        rf.predict([[0.0, "purple", 3, 0.5, "x"]])


def test_multi_output_forests_are_refused():
    sk = pytest.importorskip("sklearn.ensemble")
    rng = np.random.default_rng(0)
    m = sk.RandomForestRegressor(n_estimators=3).fit(rng.normal(size=(30, 2)), rng.normal(size=(30, 2)))
    with pytest.raises(NotImplementedError, match="several outputs"):
        F.pack(m)
    with pytest.raises(ValueError, match="not fitted"):
        F.pack(sk.RandomForestRegressor())


@needs_reference
def test_pack_of_the_reference_forest_and_its_column_map(reference, engines):
    from bayes_optim.surrogate import RandomForest

    rng = np.random.default_rng(1)
    X = _rows(rng, 150)
    y = _f(X)
    ref = RandomForest(levels=LEVELS, random_state=3)
    ref.fit(X, y)
    Xt = _rows(rng, 300)
    enc = np.asarray(ref._check_X(Xt), dtype=float)
    pk = _check_pack(ref, Xt, enc)
    # mu / MSE of the stand-in against the reference's own predict
    rmu, rmse = ref.predict(Xt, eval_MSE=True)
    mu, mse = S.moments(S.leaves(_forest_tuple(pk, True), pk.to_index(Xt)))
    assert np.array_equal(mu, rmu) and np.array_equal(mse, rmse)
    # ours encodes as the reference does, and the same seed grows the same forest
    ours = bogp.RandomForest(levels=LEVELS, random_state=3)
    assert np.array_equal(ours._check_X(Xt), enc)
    ours.fit(X, y)
    omu, omse = ours.predict(Xt, eval_MSE=True)
    assert np.array_equal(omu, rmu) and np.array_equal(omse, rmse)
    # the reference's model through bogp.forest.predict
    dmu, dmse = F.predict(ref, Xt, eval_MSE=True)
    assert np.array_equal(dmu, rmu) and np.array_equal(dmse, rmse)


def test_stand_in_matches_the_recorded_reference_moments():
    g = load_golden("G40_forest")
    for p in ("mx_", "ds_"):
        forest = tuple(g[p + k] for k in ("tree_offset", "feature", "threshold", "left", "right", "value")) + (None,)
        P = S.leaves(forest, g[p + "Xenc"])
        assert np.array_equal(P[:256], g[p + "per_tree"])
        mu, mse = S.moments(P)
        assert np.array_equal(mu, g[p + "mu"]) and np.array_equal(mse, g[p + "mse"])
        # a plain sequential sum in tree order stays within a few ulp of NumPy's pairwise mean / std
        seq_mu = np.zeros(len(P))
        for t in range(P.shape[1]):
            seq_mu += P[:, t]
        seq_mu /= P.shape[1]
        np.testing.assert_allclose(seq_mu, mu, rtol=2e-15)


def test_mixed_generator_restatement():
    lo, hi, nl = [-1.0, 0.0, 3.0, 0.0], [1.0, 4.0, 9.0, 0.0], [0, 5, 4, 1]
    X = philox_mixed.mixed_box(lo, hi, nl, 5000, 9, first_row=17)
    assert np.all((X[:, 0] >= -1) & (X[:, 0] < 1)) and set(np.unique(X[:, 1])) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert set(np.unique(X[:, 2])) == {3.0, 5.0, 7.0, 9.0} and np.all(X[:, 3] == 0.0)
    assert np.array_equal(philox_mixed.mixed_box(lo, hi, nl, 100, 9, first_row=1017), X[1000:1100])
    from oracle import philox

    assert np.array_equal(X[:, 0], philox.uniform_box(lo, hi, 5000, 9, first_row=17)[:, 0])  # the uniform generator's stream


# ---- routing: synthetic space classes with the reference's names (the reference itself is not needed) ---------------------------
class _Var:
    def __init__(self, bounds, name):
        self.bounds, self.name = bounds, name


class Real(_Var):
    scale, precision = "linear", None


class Integer(_Var):
    step = 1


class Discrete(_Var):
    pass


class Ordinal(_Var):
    pass


class Bool(_Var):
    pass


class Permutation(_Var):
    pass


class _Space:
    def __init__(self, data, seed=0):
        self.data, self.var_name, self.rng = data, [v.name for v in data], np.random.default_rng(seed)

    def sample(self, N=1, method="uniform"):
        X = np.empty((N, len(self.data)), dtype=object)
        for k, v in enumerate(self.data):
            if isinstance(v, Real):
                X[:, k] = self.rng.uniform(v.bounds[0], v.bounds[1], N)
            elif isinstance(v, Integer):
                X[:, k] = self.rng.integers(v.bounds[0], v.bounds[1] + 1, N)
            else:
                X[:, k] = [v.bounds[i] for i in self.rng.integers(0, len(v.bounds), N)]
        return X


def _space():
    return _Space([Real((-5.0, 5.0), "r0"), Discrete(LABELS, "c0"), Integer((0, 10), "i0"), Real((0.0, 1.0), "r1"), Discrete(["x", "y", "z"], "c1")])


@pytest.fixture()
def fitted(engines):
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(4)
    X = _rows(rng, 120)
    rf = bogp.RandomForest(n_estimators=30, levels=LEVELS, random_state=5)
    rf.fit(X, _f(X))
    return rf


def _member(space, x):
    assert len(x) == len(space.data)
    for v, e in zip(space.data, x):
        if isinstance(v, Real):
            assert isinstance(e, float) and v.bounds[0] <= e <= v.bounds[1]
        elif isinstance(v, Integer):
            assert isinstance(e, (int, np.integer)) and v.bounds[0] <= e <= v.bounds[1]
        else:
            assert e in v.bounds


@pytest.mark.parametrize("optimizer", ["sweep", "sweep-device"])
def test_argmax_restart_serves_a_forest_on_a_mixed_space(fitted, engines, optimizer):
    space = _space()
    for crit in (bogp.EI(model=fitted, minimize=True), bogp.MGFI(model=fitted, minimize=True, t=2.0), bogp.UCB(model=fitted, minimize=False, alpha=1.0),
                 bogp.PI(model=fitted, minimize=True), bogp.EpsilonPI(model=fitted, minimize=True, epsilon=0.01)):
        np.random.seed(3)
        x, f = bogp.argmax_restart(crit, space, eval_budget=3000, optimizer=optimizer)
        _member(space, x)
        swept = engines[0].Xs.copy()  # the rows of that sweep (level indices), decoded and evaluated again: the winner is their maximum
        assert len(swept) == 3000
        vals = crit(F.decode_rows(F.space_columns(space, F.device_of(fitted).packed), swept)).ravel()
        v = crit([x])
        assert v.shape == crit._single_row_shape and float(np.ravel(v)[0]) == f
        assert f == vals.max() and x == F.decode_rows(F.space_columns(space, F.device_of(fitted).packed), swept[[int(np.argmax(vals))]])[0]
    assert engines[0].calls.count("generate_mixed" if optimizer == "sweep-device" else "upload") >= 5
    # several rows: (M, 1), row i the one-row value
    Xs = space.sample(7)
    vals = crit(Xs)
    assert vals.shape == (7, 1) and all(float(np.ravel(crit([r.tolist()]))[0]) == vals[i, 0] for i, r in enumerate(Xs))


def test_batch_and_topk_on_a_forest(fitted, engines):
    space = _space()
    crits = [bogp.MGFI(model=fitted, minimize=True, t=t) for t in (0.5, 1.0, 2.0)]
    hist = space.sample(4)
    for design in (None, "uniform"):
        xs, fs = bogp.batch_argmax(crits, space, 2000, history=hist, k=8, design=design, seed=5)
        assert len(xs) == len(fs) == 3 and len({tuple(x) for x in xs}) == 3
        for x, f, c in zip(xs, fs, crits):
            _member(space, x)
            assert float(np.ravel(c([x]))[0]) == f
    vals, idx, rows = bogp.sweep_topk_generated(crits, space, 2000, 4, seed=6)
    assert vals.shape == idx.shape == (3, 4) and np.all(np.diff(vals, axis=1) <= 0)
    again = bogp.sweep_topk_generated(crits, space, 2000, 4, seed=6)
    assert np.array_equal(again[1], idx) and again[2] == rows
    Xs = space.sample(500)
    v2, i2, r2 = bogp.sweep_topk(crits, Xs, 4)
    assert r2[1][0] == Xs[int(i2[1, 0])].tolist() and v2[1, 0] == float(np.max(crits[1](Xs)))
    # a history row is stepped over
    v3, i3, r3 = bogp.sweep_topk([crits[0]], Xs, 2)
    xs, fs = bogp.batch_argmax([crits[0]], space, len(Xs), history=[r3[0][0]], k=2, Xs=Xs)
    assert xs[0] == r3[0][1] and fs[0] == v3[0, 1]


def test_what_a_forest_sweep_refuses(fitted, engines):
    space = _space()
    crit = bogp.EI(model=fitted, minimize=True)
    with pytest.raises(NotImplementedError, match="no input gradient"):
        crit(space.sample(1), return_dx=True)
    for opt, msg in (("sweep-device-lhs", "Latin hypercube"), ("sweep-device-sobol", "Sobol"), ("BFGS", "input gradient"),
                     ("sweep-BFGS", "input gradient"), ("sweep-device-BFGS", "input gradient")):
        with pytest.raises(NotImplementedError, match=msg):
            bogp.argmax_restart(crit, space, eval_budget=100, optimizer=opt)
    with pytest.raises(NotImplementedError, match="no constraints"):
        bogp.argmax_restart(crit, space, g=lambda x: -1.0, eval_budget=100, optimizer="sweep")
    with pytest.raises(NotImplementedError, match="no constraints"):
        bogp.batch_argmax([crit], space, 100, h=lambda x: 0.0)
    with pytest.raises(NotImplementedError, match="no fixed variables"):
        bogp.batch_argmax([crit], space, 100, masks=np.array([True, False, False, False, False]), values=[0.0])
    with pytest.raises(NotImplementedError, match="no fixed variables"):
        F.argmax_restart(crit, space, 100, "sweep", masks=np.array([True, False, False, False, False]))
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.sweep_topk_generated([crit], space, 100, 2, seed=1, rank=0, world=2)
    with pytest.raises(NotImplementedError, match="uniform design only"):
        bogp.sweep_topk_generated([crit], space, 100, 2, seed=1, method="LHS")
    F.device_of(fitted)  # (everything above is refused before an engine exists)
    assert len(engines) == 1
    engines[0].comm_world = 2
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.argmax_restart(crit, space, eval_budget=100, optimizer="sweep")
    engines[0].comm_world = 0
    ehvi = bogp.EHVI(model=fitted, ref_point=np.zeros(2), Y=np.zeros((3, 2)))
    with pytest.raises(NotImplementedError, match="EHVI"):
        bogp.argmax_restart(ehvi, space, eval_budget=100, optimizer="sweep")
    bad = _Space(space.data[:4] + [Permutation([0, 1, 2], "p")])
    with pytest.raises(NotImplementedError, match="Permutation"):
        bogp.argmax_restart(crit, bad, eval_budget=100, optimizer="sweep-device")
    uneven = _Space(space.data[:2] + [Ordinal([1, 2, 4, 8], "o")] + space.data[3:])
    with pytest.raises(NotImplementedError, match="equally spaced"):
        bogp.argmax_restart(crit, uneven, eval_budget=100, optimizer="sweep-device")
    with pytest.raises(_lib.BogpError, match="T >= 2"):
        S.ForestEngine().forest_set(1, [0, 1], [-2], [-2.0], [-1], [-1], [1.0])


def test_numeric_levels_outside_the_model_are_drawn_as_numbers(engines):
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(7)
    X = np.column_stack([rng.uniform(0, 1, 80), rng.choice([2, 4, 6], 80), rng.integers(0, 2, 80)]).astype(object)
    rf = bogp.RandomForest(n_estimators=10, levels={}, random_state=1).fit(X, np.array([float(a) + b + 3 * c for a, b, c in X]))
    space = _Space([Real((0.0, 1.0), "r"), Ordinal([2, 4, 6], "o"), Bool([False, True], "b")])
    np.random.seed(0)
    x, f = bogp.argmax_restart(bogp.UCB(model=rf, minimize=False, alpha=0.1), space, eval_budget=500, optimizer="sweep-device")
    assert x[1] in (2, 4, 6) and x[2] in (False, True) and isinstance(x[2], bool)
    drawn = engines[0].Xs
    assert set(np.unique(drawn[:, 1])) == {2.0, 4.0, 6.0} and set(np.unique(drawn[:, 2])) == {0.0, 1.0}


# ---- the reference's driver under install() ----------------------------------------------------------------------------------------
def _criterion_behind(w):
    import functools

    for _ in range(8):
        if isinstance(w, functools.partial):
            w = w.func
        elif hasattr(w, "__wrapped__"):
            w = w.__wrapped__
        else:
            break
    return w


@needs_reference
@pytest.mark.parametrize("which", ["reference", "bogp"])
def test_reference_bo_with_a_forest_under_install(reference, engines, which):
    from bayes_optim import BO, DiscreteSpace, IntegerSpace, RealSpace
    from bayes_optim.acquisition import acquisition_fun as ref_acq

    undo = bogp.install(reference)
    try:
        def space():
            return RealSpace([-5, 5], var_name="r") * 2 + IntegerSpace([0, 10], var_name="i") + DiscreteSpace(LABELS, var_name="c")

        def f(x):
            return float(x[0] ** 2 + x[1] ** 2 + abs(x[2] - 4) + 3 * LABELS.index(x[3]))

        def model(sp):
            from bayes_optim.surrogate import RandomForest

            return RandomForest(levels=sp.levels) if which == "reference" else bogp.RandomForest(levels=sp.levels)

        for optimizer in ("sweep", "sweep-device"):
            sp = space()
            opt = BO(search_space=sp, obj_fun=f, model=model(sp), max_FEs=12, DoE_size=6, acquisition_fun="EI", verbose=False, random_seed=1,
                     acquisition_optimization={"optimizer": optimizer, "max_FEs": 2000})  # fmt: skip
            n0 = len(engines)
            xopt, fopt, _ = opt.run()
            assert opt.eval_count >= 12 and np.isfinite(fopt)
            for row in np.asarray(opt.data)[:, : opt.dim]:
                assert row.tolist() in sp
            crit = _criterion_behind(opt._create_acquisition(return_dx=False))
            assert isinstance(crit, bogp.acquisition.EI) and crit.model is opt.model
            mine = [e for e in engines[n0:] if "sweep" in e.calls]
            assert mine and ("generate_mixed" in mine[0].calls) == (optimizer == "sweep-device")
        # MIES, the reference's default on a mixed space: nothing changes
        sp = space()
        opt = BO(search_space=sp, obj_fun=f, model=model(sp), max_FEs=8, DoE_size=6, acquisition_fun="EI", verbose=False, random_seed=1,
                 acquisition_optimization={"max_FEs": 50})  # fmt: skip
        assert opt._optimizer == "MIES"
        n0 = len(engines)
        X = opt.ask()
        opt.tell(X, [f(x) for x in X])
        crit = _criterion_behind(opt._create_acquisition(return_dx=False))
        assert type(crit) is ref_acq.EI
        if which == "reference":
            opt.ask()
            assert not any("sweep" in e.calls for e in engines[n0:])
    finally:
        undo()
    from bayes_optim import base

    assert base.BaseBO._create_acquisition.__name__ == "_create_acquisition"
