"""PCA-BO on the host side (no GPU): `bogp.Lift` (the NumPy restatement of the lift and its box penalty) against the golden G41
recorded from the reference, the reference's own `PCABO` under `install()` on the oracle-backed stand-in engine of
tests/support/lift_engine.py -- the surrogate is `bogp.GaussianProcess`, the sweep family is served by the lifted sweep and
returns the row-by-row argmax of the reference's own wrapper --, the refusals, and `uninstall()`."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT, load_golden

import bogp
from bogp import optim

REF = "/root/reference"
has_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
STATES = ("d5_", "d20_")


def _state(prefix):
    g = load_golden("G41_pcabo")
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def _lift(s):
    return bogp.Lift(s["A"], s["mean"], s["center"], s["bounds"][:, 0], s["bounds"][:, 1])


@pytest.mark.parametrize("prefix", STATES)
def test_lift_restatement_against_the_reference(prefix):
    s = _state(prefix)
    lift = _lift(s)
    width = float(np.max(s["bounds"][:, 1] - s["bounds"][:, 0]))
    assert (lift.r, lift.D) == s["A"].shape and lift.r == s["Z"].shape[1]
    np.testing.assert_allclose(lift.to_original(s["Z"][:256]), s["x_orig"], rtol=1e-6, atol=1e-12 * width)
    pen = lift.penalty(s["Z"])
    # a penalty is a sum of differences that goes to zero at the boundary: rtol 1e-6 with atol = 1e-12 max(hi - lo) (README ledger T12)
    np.testing.assert_allclose(pen, s["penalty"], rtol=1e-6, atol=1e-12 * width)
    assert np.array_equal(lift.feasible(s["Z"]), s["penalty"] == 0)
    assert np.array_equal(pen == 0, s["penalty"] == 0) and int((pen == 0).sum()) >= 100
    np.testing.assert_allclose(np.array(lift.reduced_bounds()), s["reduced_bounds"], rtol=1e-6)


def test_lift_construction_and_edges():
    class Pca:
        components_ = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
        mean_ = np.array([0.5, 0.0, 0.0])
        center = np.array([0.0, 0.0, 1.0])

    lift = bogp.Lift.from_pca(Pca(), [(-1, 1), (-1, 1), (0, 2)])
    assert (lift.r, lift.D) == (2, 3)
    Z = np.array([[0.5, 1.0], [0.5 + 2.0**-40, 1.0], [-2.0, -3.0], [0.0, 0.0]])
    X = lift.to_original(Z)
    assert X[0].tolist() == [1.0, 1.0, 1.0]
    pen = lift.penalty(Z)
    assert pen[0] == 0 and pen[3] == 0  # exactly ON a bound is feasible
    assert pen[1] == -(2.0**-40)  # the smallest step outside is not
    assert pen[2] == -(0.5 + 2.0)  # lower violations add up
    assert lift.feasible(Z).tolist() == [True, False, False, True]
    assert lift.penalty(np.array([[np.nan, 0.0]]))[0] == 0  # a NaN coordinate violates nothing (:66-67): the criterion decides
    rb = lift.reduced_bounds()
    assert len(rb) == 2 and np.isclose(rb[0][1] - rb[0][0], 2 * np.sqrt(3.0))
    with pytest.raises(ValueError, match="not fitted"):
        bogp.Lift.from_pca(object(), [(-1, 1)])
    with pytest.raises(ValueError, match="lo <= hi"):
        bogp.Lift(np.eye(2), [0, 0], None, [0, 1], [1, 0])
    with pytest.raises(ValueError, match="finite"):
        bogp.Lift(np.array([[np.inf, 0.0]]), [0, 0], None, [0, 0], [1, 1])
    with pytest.raises(ValueError, match="D = 2 entries"):
        bogp.Lift(np.eye(2), [0, 0, 0], None, [0, 0], [1, 1])
    assert np.array_equal(bogp.Lift(np.eye(2), [0, 0], None, [0, 0], [1, 1]).center, np.zeros(2))


# ----------------------------------------------------------------------------------------------------------------------
# the stand-in engine's lifted sweep against the golden (the contract of bogp_lift_sweep_topk, on the CPU oracle)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", STATES)
def test_stand_in_lifted_sweep_equals_the_references_wrapper(prefix):
    from bogp import _lib
    from support.lift_engine import LiftOracleEngine

    s = _state(prefix)
    eng = LiftOracleEngine()
    eng.set_train(s["X"], s["y"])
    eng.commit(int(s["kernel"]), int(s["mode"]), s["par"], float(s["noise_var"]), bool(s["estimate_trend"]), 0.0)
    eng.upload_candidates(s["Z"])
    eng.set_lift(s["A"], s["mean"], s["center"], s["bounds"][:, 0], s["bounds"][:, 1])
    best, idx, nf, vals = eng.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], float(s["plugin"]), True, k=16, return_values=True)
    feas = s["penalty"] == 0
    assert nf == int(feas.sum())
    np.testing.assert_allclose(vals[0][feas], s["value"][feas], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(vals[0][~feas], s["value"][~feas], rtol=1e-6, atol=1e-12 * 10.0)
    assert int(idx[0, 0]) == int(s["argmax"])
    for rank, (mine, ref) in enumerate(zip(idx[0], s["top16"])):  # exact, or a tie of the reference's own two values (T10)
        assert mine == ref or abs(s["value"][mine] - s["value"][ref]) <= 1e-9 * abs(s["value"][ref]), rank


# ----------------------------------------------------------------------------------------------------------------------
# the reference's PCABO under install()
# ----------------------------------------------------------------------------------------------------------------------
def _ref_modules():
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim
    import bayes_optim.extension  # noqa: F401

    return bayes_optim


@pytest.fixture()
def installed(monkeypatch):
    if not os.path.isdir(os.path.join(REF, "bayes_optim")):
        pytest.skip("reference tree not present")
    bayes_optim = _ref_modules()
    from support.lift_engine import LiftOracleEngine

    created = []

    def engine(device=0):
        created.append(LiftOracleEngine(device))
        return created[-1]

    monkeypatch.setattr(bogp._lib, "Engine", engine)
    undo = bogp.install(bayes_optim)
    yield bayes_optim, created
    undo()


DIM = 5


def _fitness(x):
    return float(np.sum((np.arange(1, DIM + 1) * np.asarray(x)) ** 2))


def _pcabo(bayes_optim, acquisition_optimization, max_FEs=13, seed=11):
    from bayes_optim.extension import PCABO, RealSpace

    np.random.seed(seed)
    kw = {} if acquisition_optimization is None else {"acquisition_optimization": acquisition_optimization}
    return PCABO(search_space=RealSpace([-5, 5]) * DIM, obj_fun=_fitness, DoE_size=8, max_FEs=max_FEs, verbose=False, n_point=1,
                 n_components=0.95, **kw)  # fmt: skip


def _is_device_gp(model):
    return type(model) is bogp.GaussianProcess


@pytest.mark.timeout(900)
@pytest.mark.parametrize("optimizer", ["sweep", "sweep-device"])
def test_pcabo_with_a_sweep_optimiser_runs_the_lifted_sweep(installed, optimizer):
    """Fails on the parent commit with `TypeError: optimizer='sweep' needs one of this package's criteria ...`."""
    bayes_optim, created = installed
    budget = 20000
    opt = _pcabo(bayes_optim, {"optimizer": optimizer, "max_FEs": budget})
    models, checked = [], 0
    while opt.eval_count < opt.max_FEs:
        X = opt.ask()
        if opt.model is not None and opt.model.is_fitted:
            eng = opt.model.engine
            Z, vals, winners = eng.lifted_sweeps[-1]
            assert eng.lift is None  # taken off the engine again
            assert Z.shape == (budget, opt._search_space.dim) and vals.shape == (1, budget)
            if checked == 0:  # one ask() against the reference's OWN wrapper, row by row
                wrapper = opt._create_acquisition(par={}, return_dx=False)
                assert isinstance(wrapper, functools.partial) and wrapper.func is bayes_optim.extension.penalized_acquisition
                ref = np.array([float(np.ravel(wrapper(z))[0]) for z in Z])
                j = int(np.argmax(ref))
                assert j == int(winners[0])
                np.testing.assert_allclose(vals[0], ref, rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(np.asarray(X[0], dtype=float), np.asarray(opt._pca.inverse_transform(Z[j]), dtype=float), rtol=0, atol=1e-12)
                assert 0 < int((bogp.Lift.from_pca(opt._pca, [(-5, 5)] * DIM).penalty(Z) == 0).sum()) < budget
                checked += 1
        opt.tell(X, [_fitness(x) for x in X])
        models.append(opt.model)
    assert opt.eval_count == opt.max_FEs and checked == 1
    assert len(models) >= 5 and all(_is_device_gp(m) for m in models)
    assert sum(len(e.__dict__.get("lifted_sweeps", [])) for e in created) == len(models) - 1  # one lifted sweep per model-based ask


@pytest.mark.timeout(900)
def test_pcabo_with_bfgs_fits_on_the_device_class(installed):
    """On the parent commit the models are the reference's CPU class (extension.py:17 bound the name at import time)."""
    bayes_optim, created = installed
    opt = _pcabo(bayes_optim, {"optimizer": "BFGS"}, max_FEs=11)  # (as the reference's example/example_PCABO.py)
    models = []
    while opt.eval_count < opt.max_FEs:
        X = opt.ask()
        opt.tell(X, [_fitness(x) for x in X])
        models.append(opt.model)
    assert len(models) >= 3 and all(_is_device_gp(m) for m in models)
    assert all(not e.__dict__.get("lifted_sweeps") for e in created)  # the reference's own loop and penalized_acquisition ran


@has_ref
def test_uninstall_restores_the_extension_module():
    bayes_optim = _ref_modules()
    ext = bayes_optim.extension
    before = ext.GaussianProcess
    undo = bogp.install(bayes_optim)
    try:
        assert ext.GaussianProcess is not before and ext.GaussianProcess is bayes_optim.surrogate.GaussianProcess
    finally:
        undo()
    assert ext.GaussianProcess is before
    undo = bogp.install(bayes_optim, surrogate=False)
    try:
        assert ext.GaussianProcess is before
    finally:
        undo()
    assert ext.GaussianProcess is before


# ----------------------------------------------------------------------------------------------------------------------
# refusals, and the lift never leaking into a later plain sweep
# ----------------------------------------------------------------------------------------------------------------------
def _penalized(x, acquisition_func, bounds, pca, return_dx):  # the shape of PCA-BO's wrapper (extension.py:62, 127-133)
    raise AssertionError("the sweep family never calls the wrapper")


class _Pca:
    components_ = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    mean_ = np.zeros(3)
    center = np.zeros(3)


def _fitted_model():
    from bogp import _lib
    from support.lift_engine import LiftOracleEngine

    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, size=(12, 2))
    eng = LiftOracleEngine()
    eng.set_train(X, np.sum(X**2, axis=1).reshape(-1, 1))
    eng.commit(_lib.KERNEL_MATERN32, _lib.MODE_NOISY, np.array([1.0, 1.0, 0.5]), 1e-6, True, 0.0)

    class Model:
        _committed_par = np.ones(3)
        engine = eng

        def _check_X(self, X):
            return np.asarray(X, float)

    return Model(), eng


def _ei(model):
    ei = bogp.acquisition.EI.__new__(bogp.acquisition.EI)
    ei._model, ei.minimize, ei._plugin = model, True, 0.0
    return ei


def _wrap(inner, return_dx=False):
    return functools.partial(_penalized, acquisition_func=inner, bounds=[(-0.5, 0.5)] * 3, pca=_Pca(), return_dx=return_dx)


def test_unwrap_lift_recognises_the_wrapper():
    model, _ = _fitted_model()
    ei = _ei(model)
    crit, lift = optim.unwrap_lift(_wrap(functools.partial(ei, return_dx=False)))
    assert crit is ei and isinstance(lift, bogp.Lift) and (lift.r, lift.D) == (2, 3) and lift.hi.tolist() == [0.5] * 3
    assert optim.unwrap_lift(ei) == (None, None) and optim.unwrap_lift(functools.partial(ei, return_dx=False)) == (None, None)
    assert optim.unwrap_lift(_wrap(lambda x: 0.0))[0] is None  # the wrapper around a foreign criterion
    assert optim.unwrap_criterion(_wrap(ei)) == (None, None, None)  # unwrap_criterion keeps stopping at the plain function


def test_lifted_sweep_through_argmax_restart_and_no_leak():
    model, eng = _fitted_model()
    ei = _ei(model)
    box = optim.Box([(-1, 1), (-1, 1)], random_seed=2)
    x, f = optim.argmax_restart(_wrap(functools.partial(ei, return_dx=False)), box, eval_budget=500, optimizer="sweep")
    Z, vals, winners = eng.lifted_sweeps[-1]
    assert len(Z) == 500 and x == Z[int(winners[0])].tolist() and f == vals[0, int(winners[0])]
    assert np.all(np.abs(np.asarray(x)) <= 0.5)  # a feasible row wins: EI >= 0 > any penalty
    assert eng.lift is None
    pen = bogp.Lift.from_pca(_Pca(), [(-0.5, 0.5)] * 3).penalty(Z)
    assert 0 < int((pen == 0).sum()) < 500 and np.array_equal(vals[0][pen != 0], pen[pen != 0])
    # a plain sweep right after it sees no lift: every row gets its criterion value
    best, idx, xb = optim.sweep_argmax([ei], Z)
    plain = eng.sweep([(ei.acq_id, ei.acq_par())], ei.effective_plugin(), True, return_values=True)[2][0]
    assert np.all(plain >= 0) and best[0] == plain.max()
    np.testing.assert_allclose(plain[pen == 0], vals[0][pen == 0], rtol=1e-9)  # (the stand-in's BLAS rounds a subset of rows differently)
    # top-k flavours, host and generated candidates
    tv, ti, tx = optim.sweep_topk([ei], Z, 4, lift=bogp.Lift.from_pca(_Pca(), [(-0.5, 0.5)] * 3))
    assert tv.shape == (1, 4) and ti[0, 0] == winners[0] and np.array_equal(tx[0], Z[ti[0]]) and eng.lift is None
    gv, gi, gx = optim.sweep_topk_generated([ei], box, 300, 3, seed=9, lift=bogp.Lift.from_pca(_Pca(), [(-0.5, 0.5)] * 3))
    assert gv.shape == (1, 3) and np.array_equal(gx[0], eng.Xs[gi[0]]) and len(eng.Xs) == 300
    bv, bi, bx = optim.sweep_generated([ei], box, 300, seed=9, lift=bogp.Lift.from_pca(_Pca(), [(-0.5, 0.5)] * 3))
    assert bv[0] == gv[0, 0] and bi[0] == gi[0, 0] and np.array_equal(bx[0], gx[0, 0])
    # the lift comes off the engine when the sweep raises, too
    eng.lift_sweep_topk = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        optim.sweep_argmax([ei], Z, lift=bogp.Lift.from_pca(_Pca(), [(-0.5, 0.5)] * 3))
    assert eng.lift is None


def test_refusals_name_the_limitation(monkeypatch):
    model, eng = _fitted_model()
    ei = _ei(model)
    box = optim.Box([(-1, 1), (-1, 1)], random_seed=2)
    w = _wrap(functools.partial(ei, return_dx=False))
    for name in ("sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="no device polish"):
            optim.argmax_restart(w, box, eval_budget=50, optimizer=name)
    with pytest.raises(NotImplementedError, match="no constraints"):
        optim.argmax_restart(w, box, h=lambda x: 0.0, eval_budget=50, optimizer="sweep")
    with pytest.raises(NotImplementedError, match="no constraints"):
        optim.argmax_restart(w, box, g=lambda x: -1.0, eval_budget=50, optimizer="sweep-device")
    with pytest.raises(TypeError, match="behind PCA-BO's wrapper"):
        optim.argmax_restart(_wrap(lambda x: 0.0), box, eval_budget=50, optimizer="sweep")

    def fixed_wrapper():  # what partial_argument builds for ask(fixed=...) (utils.py:184-213): `masks` / `values` in a closure
        masks, values = np.array([True, False]), [0.25]

        @functools.wraps(ei)
        def inner(x):
            return masks, values

        inner.__wrapped__ = functools.partial(ei, return_dx=False)
        return inner

    with pytest.raises(NotImplementedError, match="no fixed variables"):
        optim.argmax_restart(_wrap(fixed_wrapper()), box, eval_budget=50, optimizer="sweep")
    lift = bogp.Lift.from_pca(_Pca(), [(-0.5, 0.5)] * 3)
    ehvi = bogp.EHVI(model=model, ref_point=[0, 0], cells=(np.zeros((1, 2)), np.full((1, 2), np.inf)))
    with pytest.raises(NotImplementedError, match="not EHVI"):
        optim.sweep_argmax([ehvi], np.zeros((4, 2)), lift=lift)
    with pytest.raises(ValueError, match="reduced dimensions"):
        optim.sweep_argmax([ei], np.zeros((4, 2)), lift=bogp.Lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3)))
    monkeypatch.setattr(type(eng), "comm_world", 2, raising=False)
    monkeypatch.setattr(type(eng), "comm_rank", 0, raising=False)
    for call in (lambda: optim.argmax_restart(w, box, eval_budget=50, optimizer="sweep"),
                 lambda: optim.sweep_argmax([ei], np.zeros((4, 2)), lift=lift),
                 lambda: optim.sweep_topk([ei], np.zeros((4, 2)), 2, lift=lift),
                 lambda: optim.sweep_generated([ei], box, 10, seed=1, rank=0, world=2, lift=lift),
                 lambda: optim.sweep_topk_generated([ei], box, 10, 2, seed=1, rank=0, world=2, lift=lift)):  # fmt: skip
        with pytest.raises(NotImplementedError, match="one rank"):
            call()
    assert eng.lift is None
