"""Input gradient of the feasibility-weighted criterion, the parts that need no GPU: the library's host function
`bogp_feasibility_grad` against the committed exact table tests/golden/G47_feasibility_grad_truth.npz (ledger T21) and on its exact
edge rows, the NumPy restatement (tests/support/constrained_grad_ref.py) against central differences of the value restatement over
the same posterior and against `constrained_ref.constrained` on the same moments, `Constrained(input_gradient=True)` and the routing of
`optim.argmax_restart` / `polish_topk` on the oracle-backed stand-in (tests/support/constrained_grad_engine.py), and the reference's
unmodified `BO` under `install(expensive_constraints=True, constraint_gradient=True)`."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

import criteria_cases as CC
import feasibility_grad_cases as FG
from conftest import ROOT, load_golden
from oracle import gp_oracle as O
from support import constrained_grad_ref as R
from support import constrained_ref as CR
from support.constrained_grad_engine import ConstrainedGradOracleEngine

import bogp
from bogp import _lib, optim

REF = os.environ.get("BOGP_REFERENCE", "/root/reference")
INF = float("inf")
BOX = (-2.0, 2.0)


# ----------------------------------------------------------------------------------------------------------------------
# 1. bogp_feasibility_grad against the exact table (ledger T21)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    g = load_golden("G47_feasibility_grad_truth")
    c = FG.draw()
    assert len(c["mu"]) == 10_000 == len(g["dmu_true"]) == len(g["dsd_true"]) and CC.checksum(c) == float(g["checksum"])
    return c, {n: (g[n + "_true"], g[n + "_rlo"], FG.allowance(n, c)) for n in FG.NAMES}


def test_table_is_smaller_than_the_limit_for_a_committed_file():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "G47_feasibility_grad_truth.npz")) < 1 << 20


@pytest.mark.parametrize("name", FG.NAMES)
def test_reference_expression_stays_within_the_recorded_ratio(table, name):
    c, t = table
    true, rlo, allow = t[name]
    r, cmp = FG.ratios(FG.reference(name, c), true, rlo, allow)
    print("T21 %s reference: worst |value - exact| / allowance = %.4g over %d of %d rows (recorded %.3g, F = %d)"
          % (name, r.max(), cmp.sum(), len(cmp), FG.REFERENCE_RATIO[name], FG.F[name]))  # fmt: skip
    assert cmp.sum() >= 0.95 * len(cmp) and np.all(np.isfinite(allow[cmp])) and np.all(allow[cmp] > 0)
    assert r.max() <= FG.REFERENCE_RATIO[name]  # what F was taken from ...
    assert FG.F[name] == int(np.ceil(4.0 * FG.REFERENCE_RATIO[name])) and r.max() > 0.8 * FG.REFERENCE_RATIO[name]  # ... and not a loose record of it
    assert FG.tiny_rows_ok(FG.reference(name, c), cmp)


def test_host_function_against_the_table(table):
    c, t = table
    out = np.array([_lib.feasibility_grad(m, s, 1.0, a, b) for m, s, a, b in zip(c["mu"], c["mse"], c["lo"], c["hi"])])
    F0 = np.array([_lib.feasibility(m, s, 1.0, a, b) for m, s, a, b in zip(c["mu"], c["mse"], c["lo"], c["hi"])])
    assert np.array_equal(out[:, 0], F0)  # F is bogp_feasibility itself, bit for bit
    for j, name in enumerate(FG.NAMES):
        true, rlo, allow = t[name]
        r, cmp = FG.ratios(out[:, 1 + j], true, rlo, allow)
        print("T21 %s host: worst |value - exact| / allowance = %.4g over %d rows (F = %d)" % (name, r.max(), cmp.sum(), FG.F[name]))
        assert r.max() <= FG.F[name] and FG.tiny_rows_ok(out[:, 1 + j], cmp)
    # the signs of a one-sided constraint: g <= 0 loses feasibility as the mean rises
    one = np.isinf(c["lo"]) & np.isfinite(c["hi"]) & (np.abs(c["zb"]) < 5)
    assert one.sum() > 500 and np.all(out[one, 1] < 0)


def test_generator_reproduces_the_committed_table(table):
    pytest.importorskip("mpmath")
    c, t = table
    rows = np.random.default_rng(47).choice(10_000, size=1000, replace=False)
    ex = FG.exact(c, rows)
    for name in FG.NAMES:
        np.testing.assert_array_equal(ex[name][0], t[name][0][rows])
        np.testing.assert_array_equal(ex[name][1], t[name][1][rows])


def test_edge_rows_are_exact():
    fg = _lib.feasibility_grad
    phi = lambda z: np.exp(-(z * z) / 2.0) / 2.5066282746310002  # noqa: E731  (norm_pdf of csrc/bogp_device.h, operation for operation)
    # the small-variance guard: the indicator, both derivatives exactly 0
    assert fg(0.5, 1e-14, 1.0, 0.0, 1.0) == (1.0, 0.0, 0.0) and fg(1.5, 1e-14, 1.0, 0.0, 1.0) == (0.0, 0.0, 0.0)
    assert fg(0.5, 0.99e-12 * 4.0, 4.0, 0.0, 1.0) == (1.0, 0.0, 0.0)  # (sd / sqrt(sigma2) just below 1e-6)
    assert fg(0.5, 1.01e-12 * 4.0, 4.0, 0.0, 1.0)[0] == 1.0  # just above: the difference of two cdfs, 250 000 sd inside the interval
    # mse == 0
    assert fg(0.3, 0.0, 1.0, -INF, 0.0) == (0.0, 0.0, 0.0) and fg(-0.3, 0.0, 1.0, -INF, 0.0) == (1.0, 0.0, 0.0)
    # each infinite side contributes exactly 0: the other side's term alone, in the kernel's operations
    mu, mse, sd = 0.3, 0.25, 0.5
    zb = (0.0 - mu) / sd
    F, dm, ds = fg(mu, mse, 1.0, -INF, 0.0)
    assert F == _lib.feasibility(mu, mse, 1.0, -INF, 0.0) and dm == (0.0 - phi(zb)) / sd and ds == (0.0 - zb * phi(zb)) / sd
    za = (0.1 - mu) / sd
    F, dm, ds = fg(mu, mse, 1.0, 0.1, INF)
    assert F == _lib.feasibility(mu, mse, 1.0, 0.1, INF) and dm == (phi(za) - 0.0) / sd and ds == (za * phi(za) - 0.0) / sd
    # both infinite, lo == hi
    assert fg(mu, mse, 1.0, -INF, INF) == (1.0, 0.0, 0.0)
    assert fg(mu, mse, 1.0, 0.1, 0.1) == (0.0, 0.0, 0.0) and fg(mu, mse, 1.0, -7.0, -7.0) == (0.0, 0.0, 0.0)
    # the restatement forms the same three numbers to rounding
    for args in ((0.3, 0.25, 1.0, -INF, 0.0), (0.3, 0.25, 1.0, 0.1, INF), (0.3, 0.25, 2.0, -0.2, 0.9), (5.0, 0.25, 1.0, -0.2, 0.9)):
        np.testing.assert_allclose(fg(*args), R.feasibility_grad(*args), rtol=1e-12, atol=0)


# ----------------------------------------------------------------------------------------------------------------------
# 2. / 3. the restatement against central differences, and against constrained_ref on the same moments
# ----------------------------------------------------------------------------------------------------------------------
ACQS = {"EI": (O.ACQ_EI, 0.0), "EpsilonPI": (O.ACQ_EPSILON_PI, 0.05), "MGFI": (O.ACQ_MGFI, 2.0), "NONE": (R.ACQ_NONE, 0.0)}


def _bounds(Y, first=0):
    """Bounds of the constraint columns as quantiles of the training column, the four kinds in rotation: g-type (-inf, median],
    an interval [q40, q60], an upper tail [q90, +inf), an equality [-tol, tol]."""
    lo, hi = [], []
    for k in range(1, Y.shape[1]):
        col = Y[:, k]
        kind = (first + k - 1) % 4
        if kind == 0:
            lo.append(-INF), hi.append(float(np.median(col)))
        elif kind == 1:
            lo.append(float(np.quantile(col, 0.4))), hi.append(float(np.quantile(col, 0.6)))
        elif kind == 2:
            lo.append(float(np.quantile(col, 0.9))), hi.append(INF)
        else:
            tol = 0.3 * float(col.std())
            lo.append(-tol), hi.append(tol)
    return np.array(lo), np.array(hi)


def _state(m, d, kernel, N=30, seed=0, first=0):
    """An m-target oracle state at fixed hyper-parameters (fixed constant trend, as several targets require), bounds and a plugin.
    (d = 2 takes short length scales: with long ones the noise-estimating mode's variance bracket clips to 0 on most rows, which
    leaves P in {0, 1} and nothing to differentiate.)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(*BOX, size=(N, d))
    Y = np.sin(X @ rng.normal(size=(d, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    st = O.make_state(np.r_[np.full(d, 10.0 if d == 2 else 0.6 / d), 0.9], X, Y, kernel, O.MODE_NOISE_ESTIM, 0.0, beta=0.0)
    lo, hi = _bounds(Y, first)
    return st, X, Y, lo, hi, float(np.median(Y[:, 0])), rng


FD_CASES = [  # (kernel, d, m, criterion, minimize, first bound kind): d, m, the four kernels and every criterion id all appear
    (O.KERNEL_SE, 2, 2, "EI", True, 0), (O.KERNEL_MATERN32, 2, 3, "EpsilonPI", True, 1), (O.KERNEL_MATERN52, 2, 8, "MGFI", True, 2),
    (O.KERNEL_ABSEXP, 2, 2, "NONE", True, 3), (O.KERNEL_MATERN52, 12, 2, "EI", False, 1), (O.KERNEL_SE, 12, 3, "MGFI", True, 0),
    (O.KERNEL_MATERN32, 12, 8, "EI", True, 0), (O.KERNEL_ABSEXP, 12, 3, "EpsilonPI", False, 2), (O.KERNEL_MATERN52, 23, 2, "EI", True, 2),
    (O.KERNEL_SE, 23, 3, "NONE", True, 1), (O.KERNEL_MATERN32, 23, 8, "MGFI", False, 3), (O.KERNEL_ABSEXP, 23, 2, "EpsilonPI", True, 0),
]


@pytest.mark.parametrize("case", FD_CASES, ids=lambda c: "k%d-d%d-m%d-%s-%s-b%d" % (c[0], c[1], c[2], c[3], "min" if c[4] else "max", c[5]))
def test_restatement_against_central_differences(case):
    """Tolerance (ledger T15): the difference quotient's own error, estimated per case as max |FD(h) - FD(h / 2)| with h = 1e-5 of the
    box width, times 10.  The same rows: the restatement's values equal `constrained_ref.constrained` on the same moments."""
    kernel, d, m, name, minimize, first = case
    st, X, Y, lo, hi, plugin, rng = _state(m, d, kernel, seed=100 * m + 10 * kernel + d, first=first)
    if not minimize:
        plugin = -plugin
    acq = [ACQS[name]]
    h = 1e-5 * (BOX[1] - BOX[0])

    def value(z):
        mu, mse = O.predict(st, z[None, :])
        return CR.constrained(mu, mse, st.sigma2, lo, hi, acq, plugin, minimize)[0][0, 0]

    def fd(x, step):
        return np.array([(value(x + step * e) - value(x - step * e)) / (2 * step) for e in np.eye(d)])

    err = own = scale = 0.0
    n = tries = 0
    while n < 4:
        tries += 1
        assert tries < 400, "no row with a value to differentiate"
        x = rng.uniform(BOX[0] + 0.1, BOX[1] - 0.1, size=d)  # away from the training set (a continuous draw)
        v, g, P, dP, mu, mse, dmu, dmse = R.constrained_grad(st, x, lo, hi, acq, plugin, minimize)
        if not (v[0] > 1e-30 and np.abs(g[0]).max() > 0):  # (a product of up to 7 probabilities is small but keeps its relative digits;
            continue                                          #  an underflowed one has nothing to differentiate)
        n += 1
        np.testing.assert_allclose(v[0], value(x), rtol=1e-9, atol=0)
        a, b = fd(x, h), fd(x, h / 2)
        err, own, scale = max(err, np.abs(g[0] - a).max()), max(own, np.abs(a - b).max()), max(scale, np.abs(g[0]).max())
    print("%s: |grad - FD| / max|grad| = %.3g, FD's own error estimate %.3g (ratio %.3g of the allowance)"
          % (case, err / scale, own / scale, err / (10.0 * own)))  # fmt: skip
    assert scale > 0 and err <= 10.0 * own


@pytest.mark.parametrize("m,d", [(2, 2), (3, 12), (8, 23)])
def test_restatement_values_equal_constrained_ref_on_the_same_moments(m, d):
    st, X, Y, lo, hi, plugin, rng = _state(m, d, O.KERNEL_MATERN52, seed=7 + m, first=m)
    acq = list(ACQS.values())
    rows = np.vstack([rng.uniform(*BOX, size=(6, d)), X[:2]])
    out = R.batch(st, rows, lo, hi, acq, plugin, True)
    want, P = CR.constrained(out[4], out[5], st.sigma2, lo, hi, acq, plugin, True)
    assert np.array_equal(out[0], want.T) and np.array_equal(out[2], P)
    assert out[1].shape == (8, 4, d) and out[3].shape == (8, d) and out[6].shape == (8, m, d)
    assert np.array_equal(out[1][:, 3], out[3])  # feasibility only: the gradient is dP/dx itself


def test_zero_factors_remove_their_terms():
    """P == 0 and base == 0 give an exactly zero gradient, never 0 x inf or 0 / 0."""
    st, X, Y, lo, hi, plugin, rng = _state(3, 2, O.KERNEL_MATERN52, seed=3)
    x = rng.uniform(*BOX, size=2)
    far = np.array([1e6, -INF]), np.array([INF, 0.0])  # constraint 1 cannot hold: F_1 underflows to 0
    v, g, P, dP = R.constrained_grad(st, x, far[0], far[1], list(ACQS.values()), plugin, True)[:4]
    assert P == 0.0 and np.all(v == 0.0) and np.all(g == 0.0) and np.all(dP == 0.0)
    mu, mse, dmu, dmse = R.ER.moments(st, x)
    v, g, P, dP = R.from_moments(mu, np.r_[0.0, mse[1:]], dmu, dmse, st.sigma2, lo, hi, [ACQS["EI"], ACQS["NONE"]], plugin, True)
    assert v[0] == 0.0 and np.all(g[0] == 0.0) and np.array_equal(g[1], dP) and np.all(np.isfinite(g))


# ----------------------------------------------------------------------------------------------------------------------
# 4. Constrained(input_gradient=True) on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
def _gp(d=2, m=2, N=30, seed=9):
    rng = np.random.default_rng(seed)
    X = rng.uniform(*BOX, size=(N, d))
    Y = np.sin(X @ rng.normal(size=(d, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(d, beta=0.0), corr="matern", thetaL=[1e-3] * d, thetaU=[1e2] * d, nugget=1e-6)
    model._engine = ConstrainedGradOracleEngine()
    model.set_state(np.r_[np.full(d, 0.6 / d), 0.9], X, Y)
    return model, Y


def _box(d=2, seed=None):
    return optim.Box([BOX] * d, random_seed=seed)


def test_return_shapes_and_values():
    model, Y = _gp()
    crit = bogp.Constrained(model=model, fun="EI", input_gradient=True)
    plain = bogp.Constrained(model=model, fun="EI")
    assert crit.input_gradient and not plain.input_gradient and optim.is_constrained(crit)
    X = np.random.default_rng(0).uniform(*BOX, size=(5, 2))
    v1, g1 = crit(X[:1], return_dx=True)
    assert v1.shape == (1,) and g1.shape == (1, 2)  # the single-objective criteria's one-row shapes
    v5, g5 = crit(X, return_dx=True)
    assert v5.shape == (5, 1) and g5.shape == (5, 2)  # ... and their M-row shapes
    assert v5[0, 0] == v1[0] and np.array_equal(g5[0], g1[0])
    eng = model.engine
    eng.calls.clear()
    vals = crit(X)  # at most 64 rows: the same call
    assert vals.shape == (5,) and eng.calls == [("point_eval_constrained", 5, (_lib.ACQ_EI,))]
    np.testing.assert_allclose(vals, plain(X), rtol=1e-10, atol=0)  # (the sweep path of the stand-in: the chunked posterior)
    eng.calls.clear()
    big = np.random.default_rng(1).uniform(*BOX, size=(65, 2))
    assert crit(big).shape == (65,) and eng.calls[-1][0] == "sweep_constrained"
    vr, gr = R.constrained_grad(eng.st, X[0], crit.lo, crit.hi, [(crit.acq_id, crit.acq_par())], crit.plugin, True)[:2]
    assert v1[0] == vr[0] and np.array_equal(g1[0], gr[0])
    # the other criteria and the feasibility-only object take the same route
    for kw in (dict(fun="MGFI", t=2), dict(fun="EpsilonPI", epsilon=0.05), dict(fun="PI"), dict(fun=None), dict(fun="EI", minimize=False)):
        c = bogp.Constrained(model=model, input_gradient=True, **kw)
        v, g = c(X[:1], return_dx=True)
        vr, gr = R.constrained_grad(eng.st, X[0], c.lo, c.hi, [(c.acq_id, c.acq_par())], c.effective_plugin(), c.minimize)[:2]
        assert v[0] == vr[0] and np.array_equal(g[0], gr[0]) and np.all(np.isfinite(g))


@pytest.mark.parametrize("optimizer", ["BFGS", "sweep-BFGS", "sweep-device-BFGS"])
def test_polish_optimisers_reach_at_least_the_sweep_winner(optimizer):
    """The hybrids polish the sweep's own top rows (same candidates under the same seed), so their result is >= the sweep's winner by
    construction.  "BFGS" (10 restarts of L-BFGS-B from uniform starts) is compared with the best of as many uniform rows."""
    model, Y = _gp()
    crit = bogp.Constrained(model=model, fun="EI", input_gradient=True)
    eng = model.engine
    sweep_of = {"BFGS": "sweep", "sweep-BFGS": "sweep", "sweep-device-BFGS": "sweep-device"}[optimizer]
    budget = 10 if optimizer == "BFGS" else 200
    np.random.seed(4)
    xs, fs = optim.argmax_restart(crit, _box(seed=7), eval_budget=budget, optimizer=sweep_of)
    eng.calls.clear()
    np.random.seed(4)
    xp, fp = optim.argmax_restart(crit, _box(seed=7), eval_budget=200, n_restart=10, optimizer=optimizer)
    print("%s: sweep winner %.6g, result %.6g" % (optimizer, fs, fp))
    assert fp >= fs
    assert all(BOX[0] <= v <= BOX[1] for v in xp) and len(xp) == 2
    np.testing.assert_allclose(fp, crit(np.array([xp]))[0], rtol=1e-12)
    sweeps = [c for c in eng.calls if c[0] == "sweep_constrained"]
    if optimizer != "BFGS":
        assert sweeps[0] == ("sweep_constrained", (_lib.ACQ_EI,), 10)  # crit.sweep(k), then the polish (sequential fall-back here)
    else:
        assert not sweeps
    assert any(c == ("point_eval_constrained", 1, (_lib.ACQ_EI,)) for c in eng.calls)
    # the reference's wrapper around the criterion (functools.partial, as BaseBO._create_acquisition binds return_dx)
    if optimizer == "sweep-BFGS":
        np.random.seed(4)
        x2, f2 = optim.argmax_restart(functools.partial(crit, return_dx=False), _box(seed=7), eval_budget=200, n_restart=10, optimizer=optimizer)
        assert x2 == xp and f2 == fp


def test_polish_topk_dispatches_to_the_engine_polish():
    model, Y = _gp()
    crit = bogp.Constrained(model=model, fun="MGFI", t=2, input_gradient=True, lo=[-0.5], hi=[0.25])
    seen = {}

    def polish_constrained(starts, box_lo, box_hi, acq, plugin, minimize, lo, hi, max_evals=50):
        seen.update(starts=np.array(starts), box_lo=np.array(box_lo), box_hi=np.array(box_hi), acq=acq, plugin=plugin, minimize=minimize,
                    lo=lo, hi=hi, max_evals=max_evals)  # fmt: skip
        return np.array(starts) + 0.0, np.arange(len(starts), dtype=float), np.ones(len(starts), dtype=np.int32)

    model.engine.polish_constrained = polish_constrained
    starts = np.array([[0.1, 0.2], [0.3, 0.4], [9.0, 9.0]])
    xs, fs = optim.polish_topk(crit, starts, np.array([BOX, BOX]), max_iter=17)
    assert np.array_equal(xs, starts) and fs.tolist() == [0.0, 1.0, 2.0]
    assert seen["max_evals"] == 17 and seen["box_lo"].tolist() == [-2.0, -2.0] and seen["box_hi"].tolist() == [2.0, 2.0]
    assert seen["acq"] == (_lib.ACQ_MGFI, 2.0) and seen["plugin"] == crit.effective_plugin() and seen["minimize"] is True
    assert seen["lo"] is crit.lo and seen["hi"] is crit.hi


def test_default_object_still_refuses():
    model, Y = _gp()
    plain = bogp.Constrained(model=model, fun="EI")
    with pytest.raises(NotImplementedError, match="no input gradient yet"):
        plain(np.zeros((1, 2)), return_dx=True)
    for name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="input gradient"):
            optim.argmax_restart(plain, _box(), eval_budget=10, optimizer=name)
    model.engine.calls.clear()
    plain(np.zeros((3, 2)))  # the default object never takes the point call
    assert [c[0] for c in model.engine.calls] == ["upload", "sweep_constrained"]


def test_refusals_by_name(monkeypatch):
    model, Y = _gp()
    crit = bogp.Constrained(model=model, fun="EI", input_gradient=True)
    masks, values = np.array([False, True, False]), [0.5]

    @functools.wraps(functools.partial(crit))
    def fixed(X):  # the shape of the reference's partial_argument wrapper (utils.py:184-213): `masks` / `values` in its closure
        full = np.empty((1, len(masks)))
        full[:, ~masks], full[:, masks] = X, values
        return crit(full)

    fixed.__wrapped__ = functools.partial(crit)
    assert optim.unwrap_criterion(fixed)[0] is crit and optim.unwrap_criterion(fixed)[1] is not None
    for name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="fixed variables"):
            optim.argmax_restart(fixed, _box(), eval_budget=20, optimizer=name)
        with pytest.raises(NotImplementedError, match="cheap constraints h / g"):
            optim.argmax_restart(crit, _box(), g=lambda x: -1.0, eval_budget=20, optimizer=name)
        with pytest.raises(NotImplementedError, match="cheap constraints h / g"):
            optim.argmax_restart(crit, _box(), h=lambda x: 0.0, eval_budget=20, optimizer=name)
    for name in ("sweep-BFGS", "sweep-device-BFGS"):
        lifted = functools.partial(lambda x, **kw: 0.0, acquisition_func=functools.partial(crit), bounds=np.array([BOX, BOX]), pca=object())
        with pytest.raises(NotImplementedError, match="lift"):
            optim.argmax_restart(lifted, _box(), eval_budget=20, optimizer=name)
    monkeypatch.setattr(ConstrainedGradOracleEngine, "comm_world", 2, raising=False)
    monkeypatch.setattr(ConstrainedGradOracleEngine, "comm_rank", 0, raising=False)
    for name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="one rank"):
            optim.argmax_restart(crit, _box(), eval_budget=20, optimizer=name)
    monkeypatch.undo()
    # an engine without the point call says so
    model2, _ = _gp()
    from support.constrained_engine import ConstrainedOracleEngine

    model2._engine.__class__ = ConstrainedOracleEngine
    with pytest.raises(NotImplementedError, match="point_eval_constrained"):
        bogp.Constrained(model=model2, fun="EI", input_gradient=True)(np.zeros((1, 2)), return_dx=True)


# ----------------------------------------------------------------------------------------------------------------------
# 5. the reference's BO under install(expensive_constraints=True, constraint_gradient=True)
# ----------------------------------------------------------------------------------------------------------------------
def _g_true(X):
    return 0.8 - X[:, 0] - X[:, 1] + 0.3 * np.sin(6 * X[:, 0])


@pytest.fixture()
def reference(monkeypatch):
    if not os.path.isdir(os.path.join(REF, "bayes_optim")):
        pytest.skip("reference tree not present")
    for p in (REF, os.path.join(ROOT, "oracle", "shims")):
        if p not in sys.path:
            sys.path.insert(0, p)
    warnings.filterwarnings("ignore")
    import bayes_optim

    monkeypatch.setattr(bogp._lib, "Engine", ConstrainedGradOracleEngine)
    yield bayes_optim
    bogp.uninstall()


def _bo(bayes_optim, optimizer):
    from bayes_optim.search_space import RealSpace

    space = RealSpace([0, 1], var_name="a") + RealSpace([0, 1], var_name="b")
    model = bayes_optim.GaussianProcess(theta0=np.full(2, 1.0), thetaL=np.full(2, 1e-2), thetaU=np.full(2, 1e2), nugget=1e-6,
                                        noise_estim=False, likelihood="concentrated")  # fmt: skip
    opt = bayes_optim.BO(search_space=space, obj_fun=lambda x: x[0] + x[1], model=model, max_FEs=100, DoE_size=6, eval_type="list",
                         n_job=1, verbose=False, minimize=True, acquisition_fun="EI",
                         acquisition_optimization={"optimizer": optimizer, "max_FEs": 200, "n_restart": 4})  # fmt: skip
    return opt, model


def _evaluate(X):
    A = np.asarray(X, dtype=float)
    return A.sum(1).tolist(), _g_true(A).tolist()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("optimizer", ["BFGS", "sweep-BFGS"])
def test_the_reference_bo_asks_through_the_new_calls(reference, optimizer):
    bayes_optim = reference
    bogp.install(bayes_optim, expensive_constraints=True, constraint_gradient=True)
    np.random.seed(4)
    opt, model = _bo(bayes_optim, optimizer)
    assert type(model).__module__.startswith("bogp")
    X = opt.ask()  # the DoE
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    for _ in range(2):
        eng = model.engine
        eng.calls.clear()
        X = opt.ask(1)
        eng = model.engine
        assert len(X) == 1 and all(0.0 <= v <= 1.0 for v in X[0])
        assert ("point_eval_constrained", 1, (_lib.ACQ_EI,)) in eng.calls  # the gradient call served the ask ...
        sweeps = [c for c in eng.calls if c[0] == "sweep_constrained"]
        assert (sweeps == [("sweep_constrained", (_lib.ACQ_EI,), 4)]) if optimizer == "sweep-BFGS" else (not sweeps)
        assert not any(c[0] in ("sweep", "sweep_topk") for c in eng.calls)  # ... never a single-target criterion
        f, g = _evaluate(X)
        opt.tell(X, f, g_vals=g)
    crit = optim.unwrap_criterion(opt._create_acquisition(par={}, return_dx=False))[0]
    assert isinstance(crit, bogp.Constrained) and crit.input_gradient and model.y.shape[1] == 2


@pytest.mark.timeout(900)
@pytest.mark.parametrize("optimizer", ["BFGS", "sweep-BFGS"])
def test_without_the_switch_the_driver_raises_as_before(reference, optimizer):
    bayes_optim = reference
    bogp.install(bayes_optim, expensive_constraints=True)
    np.random.seed(4)
    opt, model = _bo(bayes_optim, optimizer)
    X = opt.ask()
    f, g = _evaluate(X)
    opt.tell(X, f, g_vals=g)
    with pytest.raises(NotImplementedError, match="served by the sweep family only"):
        opt.ask(1)


def test_the_switch_alone_is_refused(reference):
    with pytest.raises(ValueError, match="expensive_constraints=True"):
        bogp.install(reference, constraint_gradient=True)
    from bogp import integration

    assert not integration._CONSTRAINTS and not integration._ORIGINAL  # nothing was installed
