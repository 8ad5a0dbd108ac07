"""Thompson batches for multi-objective runs, host twin (no GPU): `thompson.hvi_select_numpy` against the hypervolume computed
directly, on the restatement alone the conditions every case of tests/thompson_ehvi_cases.py is chosen for, and the reference's own
`MOBO` under `install(ehvi_thompson=True)` on a stand-in engine."""
import os
import sys
import warnings

import numpy as np
import pytest

import thompson_constrained_cases as TC
import thompson_ehvi_cases as EC
from bogp import pareto, thompson
from support.thompson_constrained_engine import ThompsonConstrainedOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
EPS = np.finfo(float).eps
FRONT = {2: np.array([[1.0, 4.0], [2.0, 3.0], [3.5, 1.0]]), 3: np.array([[1.0, 4.0, 2.0], [2.0, 3.0, 3.0], [3.5, 1.0, 2.5]])}
# an improving point, a dominated one, one on a cell edge (its first coordinate is a front point's); a column per objective
POINTS = {2: np.array([[2.5, 3.25], [1.5, 2.0], [2.0, 3.75]]), 3: np.array([[2.5, 3.25, 1.0], [1.5, 2.0, 1.5], [2.0, 3.75, 3.5]])}


def free_volume(F, ref, box):
    """The volume between `ref` and `box` that the front of F does not dominate, from its own cells."""
    lo, hi = pareto.hypercell_bounds(F, ref)
    return float(np.sum(np.prod(np.minimum(hi, box) - lo, axis=1)))


@pytest.mark.parametrize("m", [2, 3])
def test_hvi_is_the_hypervolume_the_point_adds(m):
    F, ref, box = FRONT[m], np.zeros(m), np.full(m, 5.0)
    lower, upper = pareto.hypercell_bounds(F, ref)
    sel = thompson.hvi_select_numpy(POINTS[m].T[None], lower, upper, np.ones(m), 1)  # one member, three rows
    before = free_volume(F, ref, box)
    for i, y in enumerate(POINTS[m]):
        want = before - free_volume(np.vstack([F, y]), ref, box)  # HV(F + y) - HV(F): the box's volume cancels
        got = max(sel["A"][0, i], 0.0)
        print("m %d point %d: HVI %.17g direct %.17g" % (m, i, got, want))
        assert abs(got - want) <= 16 * EPS * before  # a few ulp of the larger volume: each side sums at most 16 cells of it
    assert sel["A"][0, 0] > 0 and sel["A"][0, 2] > 0 and sel["B"][0, 0] == 0 and sel["B"][0, 2] == 0
    assert sel["A"][0, 1] == -np.inf and sel["B"][0, 1] == -0.5  # dominated: 0.5 below the cell above (2, 3) in one objective
    np.testing.assert_array_equal(sel["best_idx"][0], [[int(np.argmax(sel["A"][0]))], [0]])


@pytest.mark.parametrize("name", list(EC.CASES))
def test_the_cases_hold_their_conditions(name):
    c = EC.case(name)
    ref = TC.restate(c.st, c.dr, c.Xs)
    assert ref.cond <= 1e8
    sel = thompson.hvi_select_numpy(ref.paths, c.lower, c.upper, c.st.sigma2, 16)
    share = float(np.mean(sel["A"] > -np.inf))
    print("%s: C = %d, cond %.2e, share %.3f" % (name, len(c.lower), ref.cond, share))
    if c.front == "far":
        assert share == 0 and np.all(sel["B"] < 0)
    elif c.front == "empty":
        assert len(c.lower) == 1 and share > 0.9
    else:
        assert 0.005 < share < 0.6
    assert len(c.lower) == {"arc": 33, "stairs": 121, "empty": 1, "far": 2 ** (c.m - 1), "one": 2 ** (c.m - 1)}[c.front]
    assert np.isinf(c.upper).any() and np.all(np.isfinite(c.lower))


def test_install_validates_ehvi_thompson():
    import bogp
    from bogp import integration

    with pytest.raises(ValueError, match="two batch strategies"):
        bogp.install(object(), ehvi_thompson=True, batch_strategy="believer")
    assert not integration._ORIGINAL and "thompson" not in integration._EHVI


class _Engine(ThompsonConstrainedOracleEngine):
    """The stand-in engine with `sweep_thompson_ehvi` served by the restatement."""

    def sweep_thompson_ehvi(self, draw, q, lower, upper, k=1, return_values=False):
        self.calls.append(("sweep_thompson_ehvi", int(q), int(k), len(lower)))
        dst = self.dense_state_multi()
        paths, gt = thompson.paths_multi_numpy(dst, draw, self.Xs)
        sel = thompson.hvi_select_numpy(paths, lower, upper, dst.sigma2, int(k))
        idx = sel["best_idx"]
        bx = np.where((idx >= 0)[..., None], self.Xs[np.clip(idx, 0, len(self.Xs) - 1)], np.nan)
        return dict(best_val=sel["best_val"], best_idx=idx, best_x=bx, coef=gt)


@pytest.mark.timeout(900)
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
def test_mobo_reaches_the_ehvi_thompson_batch(monkeypatch):
    """The reference's unmodified MOBO(n_point=3) with a noiseless device model on the stand-in engine: ONE `sweep_thompson_ehvi` call
    per ask under install(ehvi_thompson=True), three distinct points, none evaluated before; NotImplementedError under install()."""
    import bogp

    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim
    from bayes_optim import MOBO
    from bayes_optim.search_space import RealSpace

    monkeypatch.setattr(bogp._lib, "Engine", lambda device=0: _Engine(device))
    fs = (lambda x: x[0] ** 2 + x[1] + x[2] ** 2, lambda x: x[0] + x[1] ** 2 + x[2] ** 2)

    def driver():
        np.random.seed(3)
        space = RealSpace([0, 10], var_name="a") + RealSpace([0, 10], var_name="b") + RealSpace([0, 10], var_name="c")
        model = bayes_optim.GaussianProcess(theta0=np.full(3, 0.5), thetaL=np.full(3, 1e-3), thetaU=np.full(3, 1e2), nugget=0,
                                            noise_estim=False, likelihood="concentrated")  # fmt: skip
        opt = MOBO(search_space=space, obj_fun=fs, model=model, max_FEs=100, DoE_size=6, n_point=3, eval_type="list", n_job=1,
                   verbose=False, minimize=True, acquisition_optimization={"optimizer": "sweep", "max_FEs": 300})  # fmt: skip
        X = opt.ask()
        opt.tell(X, [tuple(f(x) for f in fs) for x in X])
        return opt, model, X

    undo = bogp.install(bayes_optim, ehvi_thompson=True)
    try:
        opt, model, seen = driver()
        model.engine.calls.clear()
        X = opt.ask()
        assert len(X) == 3 and len({tuple(x) for x in X}) == 3 and not any(tuple(x) in {tuple(s) for s in seen} for x in X)
        calls = [c for c in model.engine.calls if c[0].startswith("sweep")]
        assert len(calls) == 1 and calls[0][:2] == ("sweep_thompson_ehvi", 3), calls
        with pytest.raises(NotImplementedError):  # a fixed variable: the inherited method
            opt.ask(3, fixed={"a": 1.0})
        undo()
        undo = bogp.install(bayes_optim)  # the default: as before
        with pytest.raises(NotImplementedError):
            driver()[0].ask(3)
    finally:
        undo()
