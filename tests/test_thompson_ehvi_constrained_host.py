"""Thompson batches for constrained multi-objective runs, host twin (no GPU): on the restatement alone what every case of
tests/thompson_ehvi_constrained_cases.py is built for, `thompson.hvi_constrained_select_numpy` against its two pieces, `merge_ranks`
over tiers, and the Python routing and refusals on a stand-in engine."""
import os
import sys
import warnings

import numpy as np
import pytest

import bogp
import thompson_constrained_cases as TC
import thompson_ehvi_constrained_cases as CC
from bogp import integration, optim, thompson
from support.constrained_ehvi_engine import ConstrainedEhviOracleEngine
from support.thompson_constrained_engine import ThompsonConstrainedOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
INF = float("inf")


@pytest.mark.parametrize("name", list(CC.CASES))
def test_the_cases_hold_their_conditions(name):
    c = CC.case(name)
    ref = TC.restate(c.st, c.dr, c.Xs)
    assert ref.cond <= 1e8
    lo, hi = CC.bounds_for_share(ref.paths, c.m_obj, c.share)
    sel = thompson.hvi_constrained_select_numpy(ref.paths, c.m_obj, c.lower, c.upper, lo, hi, c.st.sigma2, 16)
    feas, improving = float(np.mean(sel["feas"])), float(np.mean(sel["A"] > -INF))
    print("%s: C = %d, cond %.2e, feasible %.3f, improving %.3f" % (name, len(c.lower), ref.cond, feas, improving))
    assert CC.BAND[c.share][0] <= feas <= CC.BAND[c.share][1]
    assert np.array_equal(sel["B"] > -INF, sel["feas"]) and np.all(sel["V"][sel["feas"]] == 0) and np.all(sel["V"][~sel["feas"]] < 0)
    if c.front == "far":
        assert improving == 0
    elif c.front == "empty":
        assert len(c.lower) == 1 and improving > 0.8 * feas
    elif c.share > 0:
        assert 0 < improving < feas
    if c.share == 1.0:  # infinite bounds: the objective columns alone decide, exactly as `hvi_select_numpy` has them
        obj = thompson.hvi_select_numpy(ref.paths[:, : c.m_obj], c.lower, c.upper, c.st.sigma2[: c.m_obj], 16)
        for key in ("A", "B"):
            np.testing.assert_array_equal(sel[key].view(np.int64), obj[key].view(np.int64))
        np.testing.assert_array_equal(sel["best_idx"][:, :2], obj["best_idx"])
    con = thompson.select_numpy(ref.paths[:, c.m_obj - 1 :], lo, hi, c.st.sigma2[c.m_obj - 1 :], False, 16)  # V is its B on the constraint columns
    np.testing.assert_array_equal(sel["V"].view(np.int64), con["B"].view(np.int64))
    np.testing.assert_array_equal(sel["best_idx"][:, 2], con["best_idx"][:, 1])


def test_a_nan_among_the_values_and_merge_ranks_over_tiers():
    paths = np.array([[[1.0, np.nan, 2.0], [1.0, 1.0, 2.0], [-1.0, -1.0, 3.0]]])  # one member, m = 3, three rows; row 1: a NaN objective
    sel = thompson.hvi_constrained_select_numpy(paths, 2, [[0.0, 0.0]], [[INF, INF]], [-INF], [0.0], np.ones(3), 3)
    np.testing.assert_array_equal(sel["A"][0], [1.0, -INF, -INF])
    np.testing.assert_array_equal(sel["V"][0], [0.0, -INF, -3.0])
    assert thompson.merge_ranks(sel["best_val"][0], sel["best_idx"][0]) == [(0, 0, 0), (2, 2, 1)]
    val, idx = np.array([[3.0, -INF, -INF], [-0.0, -1.0, -2.0]]), np.array([[4, -1, -1], [4, 7, 9]])  # (2, k): as it always was
    assert thompson.merge_ranks(val, idx) == [(4, 0, 0), (7, 1, 1), (9, 1, 2)] and thompson.merge_ranks(val, idx, 2) == [(4, 0, 0), (7, 1, 1)]


def test_install_validates_constrained_mobo_thompson():
    with pytest.raises(ValueError, match="needs constrained_mobo=True"):
        bogp.install(object(), constrained_mobo_thompson=True)
    with pytest.raises(ValueError, match="two batch strategies"):
        bogp.install(object(), expensive_constraints=True, constrained_mobo=True, constrained_mobo_thompson=True, constrained_mobo_batches="believer")
    with pytest.raises(ValueError, match="'topk' or 'believer'"):
        bogp.install(object(), expensive_constraints=True, constrained_mobo=True, constrained_mobo_batches="thompson")
    assert not integration._ORIGINAL and "mobo_batches" not in integration._CONSTRAINTS


class _Engine(ThompsonConstrainedOracleEngine, ConstrainedEhviOracleEngine):
    """The stand-in engine with `sweep_thompson_ehvi_constrained` served by the restatement."""

    def sweep_thompson_ehvi_constrained(self, draw, q, lower, upper, lo, hi, k=1, return_values=False):
        self.calls.append(("sweep_thompson_ehvi_constrained", int(q), int(k), len(lower)))
        dst = self.dense_state_multi()
        paths, gt = thompson.paths_multi_numpy(dst, draw, self.Xs)
        sel = thompson.hvi_constrained_select_numpy(paths, np.shape(lower)[1], lower, upper, lo, hi, dst.sigma2, int(k))
        idx = sel["best_idx"]
        bx = np.where((idx >= 0)[..., None], self.Xs[np.clip(idx, 0, len(self.Xs) - 1)], np.nan)
        return dict(best_val=sel["best_val"], best_idx=idx, best_x=bx, coef=gt)


def _g_true(X):
    return 0.8 - X[:, 0] - X[:, 1] + 0.3 * np.sin(6 * X[:, 0])


@pytest.mark.timeout(900)
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "bayes_optim")), reason="reference tree not present")
def test_mobo_reaches_the_constrained_ehvi_thompson_batch(monkeypatch):
    """The reference's unmodified MOBO(n_point=3) with g_vals and a noiseless device model (length scales bounded so that no fit raises the nugget
    and leaves the noiseless mode, which Thompson sampling refuses) on the stand-in engine: ONE
    `sweep_thompson_ehvi_constrained` call per ask under install(constrained_mobo_thompson=True), three distinct points, none evaluated
    before; the three existing Thompson entries and a foreign criterion are refused in their words; without the switch, as before."""
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim
    from bayes_optim import MOBO
    from bayes_optim.search_space import RealSpace

    monkeypatch.setattr(bogp._lib, "Engine", lambda device=0: _Engine(device))
    fs = (lambda x: x[0] ** 2 + 0.5 * x[1], lambda x: x[1] ** 2 + 0.5 * x[0])

    def driver():
        np.random.seed(4)
        space = RealSpace([0, 1], var_name="a") + RealSpace([0, 1], var_name="b")
        model = bogp.GaussianProcess(corr="matern", thetaL=np.ones(2), thetaU=1e2 * np.ones(2), nugget=0, random_start=2)  # (short length scales: R stays well conditioned, the fit noiseless)
        opt = MOBO(search_space=space, obj_fun=fs, model=model, max_FEs=100, DoE_size=8, n_point=3, eval_type="list", n_job=1,
                   verbose=False, minimize=True, acquisition_optimization={"optimizer": "sweep", "max_FEs": 300})  # fmt: skip
        X = opt.ask(8)
        opt.tell(X, [tuple(f(x) for f in fs) for x in np.asarray(X)], g_vals=_g_true(np.asarray(X, dtype=float)).tolist())
        return opt, model, X

    undo = bogp.install(bayes_optim, expensive_constraints=True, constrained_mobo=True, constrained_mobo_thompson=True)
    try:
        opt, model, seen = driver()
        model.engine.calls.clear()
        X = opt.ask()
        assert len(X) == 3 and len({tuple(x) for x in X}) == 3 and not any(tuple(x) in {tuple(s) for s in seen} for x in X)
        calls = [c for c in model.engine.calls if c[0].startswith("sweep")]
        assert len(calls) == 1 and calls[0][:2] == ("sweep_thompson_ehvi_constrained", 3) and calls[0][3] >= 1, calls
        crit = optim.unwrap_criterion(opt._create_acquisition())[0]
        box = optim.Box([(0, 1)] * 2, random_seed=1)
        for entry, args in ((bogp.constrained_thompson_batch, (crit,)), (bogp.ehvi_thompson_batch, (crit,))):
            with pytest.raises(NotImplementedError, match="has no Thompson batches"):
                entry(*args, box, 100, 2)
        with pytest.raises(NotImplementedError, match="has no Thompson batches"):
            bogp.thompson_batch(model, box, 100, 2, criteria=[crit])
        with pytest.raises(TypeError, match="takes a constrained EHVI"):
            bogp.constrained_ehvi_thompson_batch(bogp.EHVI(model=model, ref_point=np.zeros(3), Y=model.y), box, 100, 2)
        with pytest.raises(NotImplementedError, match="cheap constraints"):
            bogp.constrained_ehvi_thompson_batch(crit, box, 100, 2, h=lambda x: 0.0)
        with pytest.raises(NotImplementedError, match="ConstrainedEHVI"):  # a fixed variable: as before
            opt.ask(3, fixed={"a": 0.5})
        undo()
        undo = bogp.install(bayes_optim, expensive_constraints=True, constrained_mobo=True)  # without the switch: as before
        with pytest.raises(NotImplementedError, match="ConstrainedEHVI"):
            driver()[0].ask()
    finally:
        undo()
