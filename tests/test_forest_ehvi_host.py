"""Host side of EHVI over forests with several outputs (bogp/forest.py, acquisition.EHVI, the routing in optim.py / integration.py)
without a GPU: the engine is the NumPy restatement of tests/support/forest_ehvi_engine.py, injected by monkeypatching
`bogp._lib.Engine`.  Packing is held against scikit-learn's own `estimators_[t].predict`, the stand-in against the recorded reference
values of tests/golden/G42_forest_ehvi.npz, and the reference's `MOBO` runs under `install()` on the mixed space of its own
unittest/test_mobo.py::test_recommend; the device twin is tests/test_gpu_forest_ehvi.py."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT, load_golden

import bogp
from bogp import _lib
from bogp import forest as F
from support import ehvi_ref64
from support import forest_ehvi_engine as S

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
LABELS = ["red", "green", "blue", "cyan", "black"]
LEVELS = {1: LABELS, 4: ["x", "y", "z"]}


@pytest.fixture()
def engines(monkeypatch):
    created = []

    def engine(device=0):
        created.append(S.ForestEhviEngine(device))
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


def _f(X, m):
    w = {l: i for i, l in enumerate(LABELS)}
    f = [[float(r[0]) ** 2 + 3 * w[r[1]] + abs(r[2] - 4) for r in X], [(float(r[0]) - 2) ** 2 + 5 * float(r[3]) * (r[4] == "y") - w[r[1]] for r in X],
         [abs(float(r[0])) + r[2] * float(r[3]) for r in X]]
    y = np.column_stack(f[:m]).astype(float)
    return -(y - y.min(0)) / (y.max(0) - y.min(0))  # MinMax-scaled and negated, as BaseMOBO.y


def _tuple(pk, raw):
    if raw:
        f, t, test = pk.raw()
        return (pk.tree_offset, f, t, pk.left, pk.right, pk.value, test)
    return (pk.tree_offset, pk.feature, pk.threshold, pk.left, pk.right, pk.value, None)


@pytest.fixture()
def fitted(engines):
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(4)
    X = _rows(rng, 120)
    rf = bogp.RandomForest(n_estimators=30, levels=LEVELS, random_state=5)
    rf.fit(X, _f(X, 2))
    return rf


@pytest.mark.parametrize("m", [2, 3])
def test_pack_multi_output_and_the_surrogate_against_scikit_learn(engines, m):
    """`pack(multi_output=True)`: (nodes, m) values and the column map; `bogp.RandomForest` fitted on y (N, m) predicts (M, m) moments
    that equal the mean and std(ddof=1)^2 of scikit-learn's own per-tree predictions bit for bit; the default `pack` still refuses."""
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(m)
    X = _rows(rng, 150)
    rf = bogp.RandomForest(n_estimators=12, levels=LEVELS, random_state=2)
    rf.fit(X, _f(X, m))
    with pytest.raises(NotImplementedError, match="several outputs"):
        F.pack(rf)
    pk = F.pack(rf, multi_output=True)
    assert pk.m == m and pk.value.shape == (pk.n_nodes, m) and pk.T == 12
    assert pk.d_raw == 5 and pk.d_enc == 11 and pk.cat_idx == [1, 4] and pk.noncat == [0, 2, 3]
    Xt = _rows(rng, 300)
    enc = rf._check_X(Xt)
    want = np.stack([e.predict(np.asarray(enc, dtype=np.float32)) for e in rf.estimators_], axis=1)  # (M, T, m)
    assert np.array_equal(S.leaves_multi(_tuple(pk, False), enc), want)
    assert np.array_equal(S.leaves_multi(_tuple(pk, True), pk.to_index(Xt)), want)
    mu, mse = rf.predict(Xt, eval_MSE=True)
    assert mu.shape == mse.shape == (300, m)
    assert np.array_equal(mu, want.mean(axis=1)) and np.array_equal(mse, want.std(axis=1, ddof=1) ** 2.0)
    assert np.array_equal(rf.predict(Xt[:3]), mu[:3])
    assert len(engines) == 1 and engines[0].calls.count("forest_set_multi") == 1 and engines[0].forest_outputs() == m
    one = bogp.RandomForest(n_estimators=3, levels=LEVELS, random_state=2).fit(X, _f(X, 1))
    assert F.pack(one, multi_output=True).m == 1 and F.pack(one, multi_output=True).value.ndim == 1  # the opt-in changes nothing for one output
    assert one.predict(Xt[:4]).shape == (4,) and engines[1].calls.count("forest_set") == 1


def test_stand_in_matches_the_recorded_reference_values():
    """The NumPy restatement on the packed arrays of G42: per-tree, per-output predictions bit for bit, mu / MSE, EHVI and the winners of
    the reference -- what the device is held against in tests/test_gpu_forest_ehvi.py."""
    g = load_golden("G42_forest_ehvi")
    for p in ("mx2_", "mx3_", "ds2_"):
        forest = tuple(g[p + k] for k in ("tree_offset", "feature", "threshold", "left", "right", "value")) + (None,)
        m = g[p + "value"].shape[1]
        P = S.leaves_multi(forest, g[p + "Xenc"])
        assert np.array_equal(P[:256], g[p + "per_tree"]) and P.shape[2] == m == len(g[p + "ref_point"])
        mu, mse = S.moments_multi(P)
        np.testing.assert_allclose(mu, g[p + "mu"], rtol=1e-13)
        np.testing.assert_allclose(mse, g[p + "mse"], rtol=1e-10, atol=1e-18)
        vals = ehvi_ref64.ehvi(mu, mse, g[p + "lower"], g[p + "upper"])
        np.testing.assert_allclose(vals, g[p + "ehvi64"], rtol=1e-9)
        assert np.array_equal(S.topk(vals, 16)[1], g[p + "top16"]) and int(np.argmax(vals)) == int(g[p + "argmax"])
        assert np.max(np.abs(g[p + "ehvi32"] - g[p + "ehvi64"][:256])) <= 1e-5 * np.max(np.abs(g[p + "ehvi64"]))
        if p != "ds2_":
            assert g[p + "mse"].min() > 1e-12
    assert int(g["ds2_ties"]) >= 2 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "G42_forest_ehvi.npz")) < 2**20


def test_ehvi_on_a_forest_argument_checks_and_refusals(fitted, engines):
    space = _space()
    y = fitted.y
    ehvi = bogp.EHVI(model=fitted, ref_point=y.min(0) * 0.8 - 0.1, Y=y)
    rows = space.sample(50)
    vals = ehvi(rows)  # rows in the reference's format, level labels included
    assert vals.shape == (50,) and vals.max() > 0
    assert ehvi([rows[3].tolist()]).shape == (1,) and ehvi([rows[3].tolist()])[0] == vals[3]
    mu, mse = fitted.predict(rows, eval_MSE=True)
    np.testing.assert_allclose(vals, ehvi_ref64.ehvi(mu, mse, ehvi.cell_lower_bounds, ehvi.cell_upper_bounds), rtol=1e-12)
    best, idx = ehvi.sweep(k=3)  # over the engine's current candidates
    assert np.array_equal(idx, np.argsort(-vals, kind="stable")[:3]) and np.array_equal(best, vals[idx])
    with pytest.raises(NotImplementedError, match="input gradient"):
        ehvi(rows, return_dx=True)
    with pytest.raises(ValueError, match="unknown level"):
        ehvi([[0.0, "purple", 3, 0.5, "x"]])
    # n_obj against the forest's outputs: both numbers and the criterion's name
    three = bogp.EHVI(model=fitted, ref_point=np.full(3, -1.0), cells=(np.full((1, 3), -1.0), np.full((1, 3), np.inf)))
    with pytest.raises(NotImplementedError, match=r"EHVI over 3 objectives on a forest with 2 outputs"):
        three(rows)
    with pytest.raises(NotImplementedError, match=r"EHVI over 3 objectives on a forest with 2 outputs"):
        bogp.argmax_restart(three, space, eval_budget=100, optimizer="sweep")
    # the single-target criteria on a forest with several outputs, by name
    for name, kw in (("EI", {"plugin": 0.0}), ("PI", {"plugin": 0.0}), ("EpsilonPI", {"plugin": 0.0}), ("UCB", {}), ("MGFI", {"plugin": 0.0})):
        crit = getattr(bogp, name)(model=fitted, minimize=True, **kw)
        with pytest.raises(NotImplementedError, match=name + " on a forest with 2 outputs"):
            crit(rows)
        with pytest.raises(NotImplementedError, match=name + " on a forest with 2 outputs"):
            bogp.argmax_restart(crit, space, eval_budget=100, optimizer="sweep-device")
    with pytest.raises(ValueError, match="sweeps alone"):
        bogp.optim.sweep_topk([ehvi, ehvi], rows, 2)
    # what a forest sweep does not take, each by name
    for optimizer, what in (("sweep-device-lhs", "Latin hypercube"), ("sweep-device-sobol", "Sobol"), ("BFGS", "input gradient"),
                            ("sweep-BFGS", "input gradient"), ("sweep-device-BFGS", "input gradient")):
        with pytest.raises(NotImplementedError, match=what):
            bogp.argmax_restart(ehvi, space, eval_budget=100, optimizer=optimizer)
    with pytest.raises(NotImplementedError, match="no constraints"):
        bogp.argmax_restart(ehvi, space, h=lambda x: 0.0, eval_budget=100, optimizer="sweep")
    with pytest.raises(NotImplementedError, match="no fixed variables"):
        F.argmax_restart(ehvi, space, 100, "sweep", masks=np.array([True, False, False, False, False]))
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.sweep_topk_generated([ehvi], space, 100, 2, seed=1, rank=0, world=2)
    engines[0].comm_world = 2
    with pytest.raises(NotImplementedError, match="one rank"):
        bogp.argmax_restart(ehvi, space, eval_budget=100, optimizer="sweep")
    engines[0].comm_world = 0
    with pytest.raises(NotImplementedError, match="Gaussian process model, not a forest"):
        bogp.optim.sweep_topk([ehvi], rows, 2, lift=object())
    # the one-output entry points of the engine refuse the handle
    with pytest.raises(_lib.BogpError, match="2 outputs"):
        engines[0].forest_predict()


class _Var:
    def __init__(self, bounds, name):
        self.bounds, self.name = bounds, name


class Real(_Var):
    scale, precision = "linear", None


class Integer(_Var):
    step = 1


class Discrete(_Var):
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


@pytest.mark.parametrize("optimizer", ["sweep", "sweep-device"])
def test_argmax_restart_and_topk_route_an_ehvi_on_a_forest(fitted, engines, optimizer):
    """The winner is the maximum of `criterion(X)` over the swept rows, decoded to the reference's row format; host-sampled candidates
    under "sweep", `generate_candidates_mixed` under "sweep-device"."""
    space = _space()
    y = fitted.y
    ehvi = bogp.EHVI(model=fitted, ref_point=y.min(0) * 0.8 - 0.1, Y=y)
    np.random.seed(3)
    x, f = bogp.argmax_restart(ehvi, space, eval_budget=1500, optimizer=optimizer)
    cols = F.space_columns(space, F.device_of(fitted).packed)
    swept = engines[0].Xs.copy()
    assert len(swept) == 1500 and engines[0].calls.count("generate_mixed" if optimizer == "sweep-device" else "upload") == 1
    vals = ehvi(F.decode_rows(cols, swept))
    assert f == vals.max() and x == F.decode_rows(cols, swept[[int(np.argmax(vals))]])[0] and ehvi([x])[0] == f
    assert isinstance(x[0], float) and x[1] in LABELS and isinstance(x[2], (int, np.integer)) and x[4] in ("x", "y", "z")
    if optimizer == "sweep":
        rows = space.sample(200)
        tv, ti, pts = bogp.optim.sweep_topk([ehvi], rows, 4)
        assert tv.shape == ti.shape == (1, 4) and pts[0][0] == rows[int(ti[0, 0])].tolist()
        assert np.array_equal(tv[0], ehvi(rows)[ti[0]])
    else:
        tv, ti, pts = bogp.sweep_topk_generated([ehvi], space, 700, 4, seed=9)
        drawn = F.decode_rows(cols, engines[0].Xs)
        assert tv.shape == (1, 4) and pts[0] == [drawn[int(i)] for i in ti[0]] and np.array_equal(tv[0], ehvi(drawn)[ti[0]])


# ---- the reference's MOBO under install() -------------------------------------------------------------------------------------------
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
def test_reference_mobo_with_a_forest_under_install(reference, engines, which):
    """`MOBO(model=RandomForest(levels=...))` on the space of the reference's unittest/test_mobo.py::test_recommend with optimizer
    "sweep": three ask / tell steps; the criterion behind `_create_acquisition()` is `bogp.EHVI`; the point returned is the stand-in's
    argmax over the rows of that sweep.  With "MIES" (the default on this space) the criterion stays the reference's EHVI."""
    from bayes_optim import MOBO, BoolSpace, DiscreteSpace, IntegerSpace, RealSpace
    from bayes_optim.multi_objective import EHVI as RefEHVI

    def space():
        return (RealSpace([10, 30], var_name="p1", precision=2) + IntegerSpace([20, 40], var_name="p2")
                + DiscreteSpace([128, 256, 512], var_name="p3") + BoolSpace(var_name="p4"))

    f1 = lambda x: (x[0] - 20) ** 2 + abs(x[1] - 25) + x[2] / 128.0 + 3 * bool(x[3])  # noqa: E731
    f2 = lambda x: (x[0] - 12) ** 2 + abs(x[1] - 38) - x[2] / 64.0 - 2 * bool(x[3])  # noqa: E731

    def model(sp):
        from bayes_optim.surrogate import RandomForest

        return RandomForest(levels=sp.levels) if which == "reference" else bogp.RandomForest(levels=sp.levels)

    undo = bogp.install(reference)
    try:
        np.random.seed(7)
        sp = space()
        opt = MOBO(search_space=sp, obj_fun=(f1, f2), model=model(sp), max_FEs=100, DoE_size=8, eval_type="list", n_job=1, verbose=False,
                   acquisition_optimization={"optimizer": "sweep", "max_FEs": 2000})  # fmt: skip
        assert opt._optimizer == "sweep"
        X = opt.ask()  # the initial design
        opt.tell(X, [(f1(x), f2(x)) for x in X])
        for _ in range(3):
            n0 = len(engines)
            X = opt.ask(1)
            mine = [e for e in engines if "sweep_ehvi" in e.calls]
            assert len(mine) == 1 and mine[0].M == 2000 and mine[0].forest_outputs() == 2
            crit = _criterion_behind(opt._create_acquisition())
            assert isinstance(crit, bogp.EHVI) and crit.model is opt.model and crit.n_obj == 2
            eng = mine[0]
            cols = F.space_columns(sp, F.device_of(opt.model).packed)
            swept = eng.Xs.copy()
            vals = ehvi_ref64.ehvi(*S.moments_multi(S.leaves_multi(eng.forest, swept)), crit.cell_lower_bounds, crit.cell_upper_bounds)
            assert list(X[0]) == F.decode_rows(cols, swept[[int(np.argmax(vals))]])[0]
            assert list(X[0]) in sp
            eng.calls.clear()
            opt.tell(X, [(f1(x), f2(x)) for x in X])
        with pytest.raises(NotImplementedError, match="no fixed variables"):
            opt.ask(1, fixed={"p2": 30})
        # MIES: nothing changes
        sp = space()
        opt = MOBO(search_space=sp, obj_fun=(f1, f2), model=model(sp), max_FEs=100, DoE_size=8, eval_type="list", n_job=1, verbose=False,
                   acquisition_optimization={"max_FEs": 50})  # fmt: skip
        assert opt._optimizer == "MIES"
        X = opt.ask()
        opt.tell(X, [(f1(x), f2(x)) for x in X])
        assert isinstance(_criterion_behind(opt._create_acquisition()), RefEHVI)
        if which == "reference":
            for e in engines:
                e.calls.clear()
            opt.ask(1)
            assert not any("sweep_ehvi" in e.calls for e in engines)
    finally:
        undo()
    from bayes_optim import mobo

    assert mobo.MOBO._create_acquisition.__name__ == "_create_acquisition"
