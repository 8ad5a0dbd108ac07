"""EHVI on the host side (no GPU): the float64 restatement (tests/support/ehvi_ref64.py) against the reference's own
`EHVI.forward`, `bogp.pareto`'s cell decomposition against the reference's partitioning, the criterion's argument checks,
the sweep routing's refusals, and the reference's `MOBO` under `install()`: with a sweep optimiser its acquisition is
`bogp.EHVI` (one upload of `max_FEs` candidates per ask, the returned point the restatement's argmax), with the CMA
optimiser it stays the reference's EHVI.  The engine under `bogp.GaussianProcess` is the oracle-backed stand-in of
tests/support/oracle_engine.py, extended here by the EHVI sweep and the device generator."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from support.ehvi_ref64 import ehvi as ehvi_ref

import bogp
from bogp import _lib, pareto

REF = "/root/reference"
has_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")


def _ref_modules():
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import torch
    from bayes_optim.multi_objective import EHVI as RefEHVI
    from bayes_optim.utils.multi_objective.box_decompositions import NondominatedPartitioning

    return torch, RefEHVI, NondominatedPartitioning


def _front(rng, n, m):
    Y = rng.uniform(0, 1, size=(n, m))
    return Y / np.linalg.norm(Y, axis=1, keepdims=True) ** 0.5


class _Fixed:
    """a model whose predict returns given moments (float32-exact: the reference's torch.Tensor casts lose nothing)"""

    def __init__(self, mu, mse):
        self.mu, self.mse = mu, mse

    def predict(self, X, eval_MSE=True):
        return self.mu[: len(X)], self.mse[: len(X)]


@has_ref
@pytest.mark.parametrize("m", [2, 3])
def test_restatement_equals_reference_forward(m):
    torch, RefEHVI, NP = _ref_modules()
    rng = np.random.default_rng(m)
    Y = _front(rng, 12, m)
    ref_point = np.full(m, -0.05)
    part = NP(ref_point=torch.tensor(ref_point, dtype=torch.float64), Y=torch.tensor(Y, dtype=torch.float64))
    lo, hi = (np.asarray(b, dtype=float) for b in part.get_hypercell_bounds())
    crit = None
    vals, refs = [], []
    for i in range(40):  # one row per call, as MOBO's inner optimiser calls it
        mu = np.float32(rng.uniform(-0.2, 1.1, size=(1, m))).astype(np.float64)
        sd = rng.integers(1, 40, size=(1, m)) / 64.0  # sd^2 and its float32 square root are exact
        model = _Fixed(mu, sd**2)
        crit = RefEHVI(model=model, ref_point=ref_point.tolist(), partitioning=part)
        refs.append(float(np.ravel(crit(np.zeros((1, 3))))[0]))
        vals.append(float(ehvi_ref(mu, sd**2, lo, hi)[0]))
    vals, refs = np.array(vals), np.array(refs)
    assert np.abs(vals - refs).max() <= 1e-12 * np.abs(refs).max()


@has_ref
@pytest.mark.parametrize("m", [2, 3, 4])
def test_grid_cells_give_the_reference_cells_ehvi(m):
    torch, _, NP = _ref_modules()
    for seed in range(3):
        rng = np.random.default_rng(10 * m + seed)
        Y = np.vstack([_front(rng, 8 if m < 4 else 5, m), rng.uniform(-0.3, 0.5, size=(6, m))])  # plus dominated rows
        ref_point = np.full(m, -0.1)
        part = NP(ref_point=torch.tensor(ref_point, dtype=torch.float64), Y=torch.tensor(Y, dtype=torch.float64))
        rlo, rhi = (np.asarray(b, dtype=float) for b in part.get_hypercell_bounds())
        lo, hi = pareto.hypercell_bounds(Y, ref_point)
        mu = rng.uniform(-0.2, 1.2, size=(200, m))
        mse = rng.uniform(1e-4, 0.1, size=(200, m))
        a, b = ehvi_ref(mu, mse, lo, hi), ehvi_ref(mu, mse, rlo, rhi)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
        assert np.array_equal(np.sort(pareto.pareto_front(Y, ref_point), axis=0), np.sort(np.asarray(part.pareto_Y), axis=0))


def test_pareto_basics_and_limits():
    Y = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [0.4, 0.4], [1.0, 0.0]])
    assert pareto.is_non_dominated(Y).tolist() == [True, True, True, False, False]
    lo, hi = pareto.hypercell_bounds(Y, [-1.0, -1.0])
    assert len(lo) == 4 and np.all(np.isinf(hi[:, 1]))
    lo1, hi1 = pareto.hypercell_bounds(np.array([[-2.0, 3.0]]), [-1.0, -1.0])  # nothing above the reference point: one cell
    assert lo1.tolist() == [[-1.0, -1.0]] and np.all(np.isinf(hi1))
    big = np.random.default_rng(0).uniform(size=(300, 3))
    big = big / np.linalg.norm(big, axis=1, keepdims=True)
    with pytest.raises(ValueError, match="pass the cells explicitly"):
        pareto.hypercell_bounds(big, np.zeros(3))
    # (P + 1)^(m - 1) past 2^63 (m = 8, 600 distinct coordinates per axis): the count must not wrap round below the limit
    wide = np.random.default_rng(1).uniform(size=(600, 8))
    wide[:, 7] = 8.0 - wide[:, :7].sum(axis=1)  # on a hyperplane: every row non-dominated
    with pytest.raises(ValueError, match="pass the cells explicitly"):
        pareto.hypercell_bounds(wide, np.full(8, -10.0))


class _NoEngineModel:
    _committed_par = None

    def predict(self, X, eval_MSE=True):
        raise AssertionError


def test_criterion_argument_checks():
    model = _NoEngineModel()
    Y = np.array([[1.0, 0.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match="exactly one"):
        bogp.EHVI(model=model, ref_point=[0, 0])
    with pytest.raises(ValueError, match="exactly one"):
        bogp.EHVI(model=model, ref_point=[0, 0], Y=Y, cells=(np.zeros((1, 2)), np.ones((1, 2))))
    # no observed point above the reference point: the whole region is one cell (the reference's partitioning keeps no front)
    c0 = bogp.EHVI(model=model, ref_point=[2.0, 2.0], Y=Y)
    assert c0.cell_lower_bounds.tolist() == [[2.0, 2.0]] and np.all(np.isinf(c0.cell_upper_bounds))
    with pytest.raises(ValueError, match="number of outcomes"):
        bogp.EHVI(model=model, ref_point=[0, 0, 0], Y=Y)
    with pytest.raises(ValueError, match="C x 2"):
        bogp.EHVI(model=model, ref_point=[0, 0], cells=(np.zeros((2, 3)), np.ones((2, 3))))

    class Part:  # the reference's partitioning, duck-typed
        num_outcomes = 2
        pareto_Y = Y

        def get_hypercell_bounds(self):
            return np.stack(pareto.hypercell_bounds(Y, [-0.5, -0.5]))

    with pytest.raises(ValueError, match="better than the reference point"):  # analytic.py:158-160
        bogp.EHVI(model=model, ref_point=[2.0, 2.0], partitioning=Part())
    c = bogp.EHVI(model=model, ref_point=[-0.5, -0.5], partitioning=Part())
    assert c.cell_lower_bounds.shape == (3, 2) and c.n_obj == 2
    with pytest.raises(NotImplementedError):
        c(np.zeros((1, 2)), return_dx=True)
    with pytest.raises(Exception, match="not fitted"):
        c(np.zeros((1, 2)))


class _EhviOracleEngine:
    """mixin over the oracle engine: bogp_sweep_ehvi through the float64 restatement, and a host stand-in for the
    device generator (uniform rows in the drawing box, rounded to the variables' precision)"""

    def sweep_ehvi(self, lower, upper, k=1, return_values=False, return_moments=False):
        from oracle import gp_oracle as O

        mu, mse = O.predict_chunked(self.st, self.Xs, 1024)
        vals = ehvi_ref(mu, mse, lower, upper)
        order = sorted(range(len(vals)), key=lambda j: (-vals[j], j))[:k]
        idx = np.array(order + [-1] * (k - len(order)), dtype=np.int64)
        best = np.array([vals[j] if j >= 0 else -np.inf for j in idx])
        self.__dict__.setdefault("ehvi_winners", []).append(self.Xs[idx[0]].copy())
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_moments:
            out += (mu, mse)
        return out

    def set_candidate_transform(self, scale, precision, lo, hi):
        self._prec = None if precision is None else list(precision)

    def generate_candidates(self, lo, hi, M, seed=0, first_row=0, method="uniform", n_total=None, sobol_sv=None, maximin=5):
        X = np.random.default_rng(int(seed) % 2**32).uniform(lo, hi, size=(int(M), len(lo)))
        for j, p in enumerate(getattr(self, "_prec", None) or []):
            if p is not None:
                X[:, j] = np.round(X[:, j], p)
        self.upload_candidates(X)


@pytest.fixture()
def installed(monkeypatch):
    if not os.path.isdir(os.path.join(REF, "bayes_optim")):
        pytest.skip("reference tree not present")
    _ref_modules()
    import bayes_optim
    from support.oracle_engine import OracleEngine

    created = []

    class Recording(_EhviOracleEngine, OracleEngine):
        def upload_candidates(self, Xs, lazy=False):
            self.__dict__.setdefault("uploads", []).append(len(Xs))
            return super().upload_candidates(Xs)

    def engine(device=0):
        created.append(Recording(device))
        return created[-1]

    monkeypatch.setattr(bogp._lib, "Engine", engine)
    undo = bogp.install(bayes_optim)
    yield bayes_optim, created
    undo()


def _mobo(bayes_optim, optimizer, max_FEs, seed=3):
    from bayes_optim import MOBO
    from bayes_optim.search_space import RealSpace

    np.random.seed(seed)
    space = RealSpace([0, 10], var_name="a", precision=2) + RealSpace([0, 10], var_name="b", precision=2) + RealSpace([0, 10], var_name="c", precision=2)
    f1 = lambda x: x[0] ** 2 + x[1] + x[2] ** 2  # noqa: E731  (the objectives of the reference's unittest/test_mobo.py::test_3D)
    f2 = lambda x: x[0] + x[1] ** 2 + x[2] ** 2  # noqa: E731
    f3 = lambda x: x[0] ** 2 + x[1] + x[2]  # noqa: E731
    d = 3
    model = bayes_optim.GaussianProcess(theta0=np.full(d, 0.5), thetaL=np.full(d, 1e-3), thetaU=np.full(d, 1e2), nugget=1e-6,
                                        noise_estim=False, likelihood="concentrated")  # fmt: skip
    opt = MOBO(search_space=space, obj_fun=(f1, f2, f3), model=model, max_FEs=100, DoE_size=5, eval_type="list", n_job=1,
               verbose=False, minimize=True, acquisition_optimization={"optimizer": optimizer, "max_FEs": max_FEs})  # fmt: skip
    return opt, (f1, f2, f3), model


@pytest.mark.timeout(900)
@pytest.mark.parametrize("optimizer", ["sweep", "sweep-device"])
def test_mobo_with_a_sweep_optimiser_runs_on_ehvi(installed, optimizer):
    bayes_optim, created = installed
    opt, fs, model = _mobo(bayes_optim, optimizer, 400)
    assert type(model).__module__.startswith("bogp")
    n_ask = 0
    for _ in range(17):
        X = opt.ask(1)
        eng = model.engine
        n_before = len(eng.__dict__.get("ehvi_winners", []))
        opt.tell(X, [tuple(f(x) for f in fs) for x in X])
        if n_before:
            n_ask += 1
            np.testing.assert_allclose(X[0], eng.ehvi_winners[-1], rtol=0, atol=1e-12)
    assert n_ask >= 15
    eng = model.engine
    assert eng.uploads.count(400) >= 15  # one upload of max_FEs rows per ask, nothing else of that size
    crit = bayes_optim.mobo.MOBO._create_acquisition(opt)
    from bogp.optim import unwrap_criterion

    assert isinstance(unwrap_criterion(crit)[0], bogp.EHVI)
    with pytest.raises(NotImplementedError):
        opt.ask(3)


@pytest.mark.timeout(900)
def test_mobo_with_cma_keeps_the_reference_ehvi(installed):
    bayes_optim, created = installed
    opt, fs, model = _mobo(bayes_optim, "OnePlusOne_Cholesky_CMA", 60)
    for _ in range(7):
        X = opt.ask(1)
        opt.tell(X, [tuple(f(x) for f in fs) for x in X])
    from bayes_optim.multi_objective import EHVI as RefEHVI
    from bogp.optim import unwrap_criterion

    w = bayes_optim.mobo.MOBO._create_acquisition(opt)
    inner = w
    import functools

    for _ in range(8):
        inner = inner.func if isinstance(inner, functools.partial) else getattr(inner, "__wrapped__", inner)
    assert isinstance(inner, RefEHVI) and unwrap_criterion(w)[0] is None


def test_sweep_routing_refusals(monkeypatch):
    from bogp import optim

    class Eng:
        comm_world = 0
        d = 2

    class Model:
        _committed_par = np.ones(2)
        engine = Eng()

        def _check_X(self, X):
            return np.asarray(X, float)

    e = bogp.EHVI(model=Model(), ref_point=[0, 0], cells=(np.zeros((1, 2)), np.full((1, 2), np.inf)))
    ei = bogp.acquisition.EI.__new__(bogp.acquisition.EI)
    ei._model, ei.minimize, ei._plugin = Model(), True, 0.0
    with pytest.raises(ValueError, match="sweeps alone"):
        optim.sweep_argmax([e, ei], np.zeros((4, 2)))
    box = optim.Box([(0, 1), (0, 1)])
    for name in ("sweep-BFGS", "sweep-device-BFGS", "BFGS"):
        with pytest.raises(NotImplementedError, match="input gradient"):
            optim.argmax_restart(e, box, eval_budget=10, optimizer=name)
    monkeypatch.setattr(Eng, "comm_world", 2, raising=False)
    monkeypatch.setattr(Eng, "comm_rank", 0, raising=False)
    with pytest.raises(NotImplementedError, match="one rank"):
        optim.sweep_argmax([e], np.zeros((4, 2)))
    assert optim.unwrap_criterion(e)[0] is e
