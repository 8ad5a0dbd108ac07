"""The host side of the constrained Thompson polish, without a device: `thompson.feasible_merit_numpy`'s gradient against central
differences (ledger T15's rule: within 10 max|FD(h) - FD(h / 2)| at h = 1e-5 of the box width, away from every kink), `thompson.tighten`'s three cases, the
acceptance rule of `optim._constrained_thompson_polished` on a NumPy stand-in engine, `constrained_thompson_batch` with and without the
polish on the oracle-backed stand-in engine (its merit the restatement's, its polish a projected ascent on it), the install keywords."""
from types import SimpleNamespace

import numpy as np
import pytest

import bogp
import thompson_constrained_cases as TC
from bogp import _lib, integration, optim, thompson
from support.thompson_constrained_engine import ThompsonConstrainedOracleEngine
from test_thompson_constrained_host import _box, _cands, _crit, _model


@pytest.mark.parametrize("n_obj,minimize", [(1, True), (1, False), (3, False)])
def test_the_restated_gradient_against_central_differences(n_obj, minimize):
    m, q, d, Bn = n_obj + 2, 2, 3, 12
    X, Y, theta, Xs = TC.problem(Bn, d, 40, _lib.KERNEL_MATERN52, m)
    st = TC.state(X, Y, theta, _lib.KERNEL_MATERN52)
    dr, members = thompson.draw_multi(st, q, 48, seed=5), np.arange(Bn) % q
    y = thompson.paths_multi_numpy(st, dr, Xs)[0][members, :, np.arange(Bn)]
    lower = np.quantile(y[:, :n_obj], [0.2, 0.5], axis=0) if n_obj > 1 else None  # two cells over the 0.2 and 0.5 quantiles
    upper = None if lower is None else np.vstack([lower[1], np.full(n_obj, np.inf)])
    plo, phi = np.r_[-np.inf, np.quantile(y[:, -1], 0.4)], np.r_[np.quantile(y[:, -2], 0.6), np.inf]
    f = lambda Z, **kw: thompson.feasible_merit_numpy(st, dr, Z, members, n_obj, lower, upper, plo, phi, minimize, 100.0, **kw)  # noqa: E731
    merit, grad, p = f(Xs, parts=True)
    assert np.count_nonzero(p["P"]) >= 3 and np.count_nonzero(p["F"]) >= 3
    h, away, fd, fd2 = 1e-5 * 4.4, np.ones(Bn, dtype=bool), np.empty((Bn, d)), np.empty((Bn, d))
    for k in range(d):
        E = np.zeros(d)
        E[k] = h
        for Z in (Xs + E, Xs - E):  # a point whose step crosses a cell face or a bound sees a kink: left out
            pz = f(Z, parts=True)[2]
            away &= np.all(np.sign(pz["u"]) == np.sign(p["u"]), axis=1) & np.all((pz["W"] == 0) == (p["W"] == 0), axis=1)
        fd[:, k] = (f(Xs + E)[0] - f(Xs - E)[0]) / (2 * h)
        fd2[:, k] = (f(Xs + E / 2)[0] - f(Xs - E / 2)[0]) / h
    assert away.sum() >= Bn // 2
    tol = 10 * np.max(np.abs(fd - fd2)[away])  # T15: a central difference is as good as FD(h) - FD(h / 2) says
    assert tol <= 1e-5 * np.max(np.abs(grad[away])) and np.max(np.abs(grad - fd)[away]) <= tol, (tol, np.max(np.abs(grad - fd)[away]))


def test_tighten():
    plo, phi = thompson.tighten([0.0, 0.0, -np.inf, -np.inf], [10.0, 0.05, 1.0, np.inf], [2.0, 1.0, 1.0, 3.0], 0.05)
    np.testing.assert_array_equal(plo, [0.1, 0.025, -np.inf, -np.inf])  # wide; narrower than 2 tau sd: the midpoint; infinite bounds stay
    np.testing.assert_array_equal(phi, [9.9, 0.025, 0.95, np.inf])


class StandIn:
    """An engine of two candidate rows a member whose polish moves every start by `step` and whose path values are those of `y_of`."""

    d = 1

    def __init__(self, step, y_of):
        self.step, self.y_of, self.polished = step, y_of, 0

    def polish_path_feasible(self, starts, lo, hi, dr, coef, members, *a, **kw):
        self.polished += 1
        return np.clip(starts + self.step, lo, hi), np.zeros(len(starts)), np.ones(len(starts), dtype=np.int32)

    def point_eval_path_feasible(self, X, dr, coef, members, *a, **kw):
        return None, None, np.array([self.y_of(x[0]) for x in X]), None


@pytest.mark.parametrize("case,want", [("higher", [0.75]), ("infeasible", [0.5]), ("lower", [0.5])])
def test_the_acceptance_rule_on_a_stand_in_engine(case, want, monkeypatch):
    """One member, rows x = 0.5 (A rank: feasible, objective -1) and x = 0.1 (B rank).  Minimising y_0 under c <= 0: the polished point
    x + 0.25 is proposed only where it is feasible under the TRUE bound and better; the row stays otherwise."""
    y_of = {"higher": lambda x: [-2.0, -0.5], "infeasible": lambda x: [-9.0, 0.5], "lower": lambda x: [-0.5, -1.0]}[case]
    eng = StandIn(0.25, y_of)
    st = SimpleNamespace(y=np.zeros((4, 2)), sigma2=np.ones(2))
    out = dict(best_idx=np.array([[[0], [1]]]), best_x=np.array([[[[0.5]], [[0.1]]]]), best_val=np.array([[[1.0], [-0.3]]]), coef=None)
    monkeypatch.setattr(thompson, "draw_multi", lambda *a, **k: None)
    monkeypatch.setattr(thompson, "objective_path_at", lambda *a, **k: 0.0)
    xs, fs = optim._constrained_thompson_polished(None, st, eng, optim.Box([(0.0, 1.0)], random_seed=0), 1, 1, 16, 0, None, 1, lambda dr, qb, kk: out,
                                                  [-np.inf], [0.0], None, None, True, 2, 5, 100.0, 0.05)  # fmt: skip
    assert eng.polished == 1 and list(xs[0]) == want and fs[0] == (y_of(0)[0] if case == "higher" else -1.0)


class OracleEngine(ThompsonConstrainedOracleEngine):
    def point_eval_path_feasible(self, X, dr, coef, members, lower, upper, plo, phi, minimize=True, rho=100.0, jacobian=True):
        merit, grad, p = thompson.feasible_merit_numpy(self.dense_state_multi(), dr, X, members, 1, lower, upper, plo, phi, minimize, rho, parts=True)
        return merit, grad, p["y"], p["jac"]

    def polish_path_feasible(self, starts, lo, hi, *ops, max_evals=50, **kw):
        self.calls.append(("polish_path_feasible", len(starts)))
        x, t = np.clip(starts, lo, hi), np.full((len(starts), 1), 0.05)
        for _ in range(max_evals):  # projected ascent, a step halved wherever it does not climb
            f, g = self.point_eval_path_feasible(x, *ops, **kw)[:2]
            z = np.clip(x + t * g, lo, hi)
            up = self.point_eval_path_feasible(z, *ops, **kw)[0] > f
            x, t = np.where(up[:, None], z, x), np.where(up[:, None], t, t / 2)
        return x, self.point_eval_path_feasible(x, *ops, **kw)[0], np.full(len(x), max_evals, dtype=np.int32)


def test_the_batch_with_and_without_the_polish_on_the_oracle_engine():
    gp = _model()
    gp.engine.__class__ = OracleEngine
    crit, Xs, kw = _crit(gp), _cands(), dict(q=3, n_features=64, seed=4)
    st, dr = thompson.state_of_multi(gp), thompson.draw_multi(gp, 3, 64, seed=4)
    rank = lambda j, x: (lambda s: (0, s["A"][0, 0]) if s["feas"][0, 0] else (1, s["B"][0, 0]))(  # noqa: E731  (tier, score) on the TRUE bounds
        thompson.select_numpy(thompson.paths_multi_numpy(gp, dr, np.asarray(x)[None])[0][j : j + 1], crit.lo, crit.hi, st.sigma2, True, 1))
    paths = thompson.paths_multi_numpy(gp, dr, Xs)[0]
    feas = thompson.select_numpy(paths, crit.lo, crit.hi, st.sigma2, True, 1)["feas"]
    xs, fs = bogp.constrained_thompson_batch(crit, _box(), 300, Xs=Xs, polish=False, **kw)  # unchanged: each member's best feasible row, no polish
    assert list(xs) == [Xs[int(np.argmin(np.where(feas[j], paths[j, 0], np.inf)))].tolist() for j in range(3)]
    assert fs == tuple(float(paths[j, 0][feas[j]].min()) for j in range(3)) and not any(c[0] == "polish_path_feasible" for c in gp.engine.calls)
    xp, fp = bogp.constrained_thompson_batch(crit, _box(), 300, Xs=Xs, polish=True, n_starts=4, max_iter=20, **kw)
    assert [c for c in gp.engine.calls if c[0] == "polish_path_feasible"] == [("polish_path_feasible", 12)] and np.all(np.abs(xp) <= 2.2)
    before, after = [rank(j, xs[j]) for j in range(3)], [rank(j, xp[j]) for j in range(3)]
    assert all((a[0], -a[1]) <= (b[0], -b[1]) for a, b in zip(after, before)) and any(a[1] > b[1] for a, b in zip(after, before))
    assert all(a[0] == 0 and abs(f + a[1]) <= 1e-10 for a, f in zip(after, fp))  # feasible; fopt the drawn objective (two float64 sums of O(100) terms of O(1))


@pytest.mark.parametrize("kw", [dict(constraint_thompson_polish=True), dict(constrained_mobo_thompson_polish=True),
                                dict(expensive_constraints=True, constraint_thompson_polish=True)])  # fmt: skip
def test_each_install_keyword_alone_raises(kw):
    with pytest.raises(ValueError, match="refines the members"):
        integration.install(bayes_optim=SimpleNamespace(), **kw)
